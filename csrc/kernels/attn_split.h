// Flash-decoding split arithmetic: the two functions every decode kernel (attention.hip, attn_d256.hip), the fused
// merges and the combine kernels count with. One definition for all units: a disagreement between the kernel that
// writes the partials and the code that merges them is a dropped or a double-counted partial.
#pragma once
#include "common.h"

// Keys per flash-decoding split. chunk > 0: fixed; chunk < 0: balanced over n_split with at least
// -chunk keys; chunk == 0: balanced with at least 64 keys below 1K of context, 128 at 1K-2K and 256 above
// (batch-1 A/B, profiles/attn_split_policy_b1.txt: 64-key splits win on short contexts, where the split's
// dependent K/V fetch chain dominates; 128-256-key splits at 1K-4K, where the merge of many partials does).
// With up to 64 splits at batch 1 (models/llama.py _SPLIT_CAP), 8K-32K contexts get 32-64 splits of
// 256-512 keys: 512 workgroups keep enough K/V in flight to stream the cache at HBM rate.
__device__ __forceinline__ int split_chunk(int chunk, int ctx, int n_split, int bs, int short_min = 64) {
  if (chunk > 0) return chunk;
  const int mn = chunk ? -chunk : (ctx >= 2048 ? 256 : (ctx >= 1024 ? 128 : short_min));
  return max(mn, ((ctx + n_split - 1) / n_split + bs - 1) / bs * bs);
}

// Splits that have keys, of a row whose splits of `chunk` keys cover [first, ctx) (first = lo_al; 0 without a window).
// Both decode kernels (which splits return at once, whose ticket is the last), the fused merge and attn_combine
// count with this one function: a disagreement is a dropped or a double-counted partial.
DEVI int active_splits(int ctx, int first, int chunk, int n_split) {
  return min(n_split, (ctx - first + chunk - 1) / chunk);
}
