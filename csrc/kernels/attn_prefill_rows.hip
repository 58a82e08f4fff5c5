// Causal flash attention for prefill over the paged KV cache for ANY GQA group size G = Hq / Hkv (1 .. 16):
// attn_prefill2's tile loop (attn_prefill.hip) with the query ROWS of a kv head packed into waves, instead of
// "4 query heads x 2 token halves" per workgroup, which needs G % 4 == 0.
//
// Row packing. A 64-token query block (ops.prefill_blocks) and one kv head give R = ntok * G query rows that share
// that head's K/V, numbered token-major: rho = tok * G + g. A wave takes 32 consecutive rows as the 32 columns of
// the 32x32x16 MFMAs; lane l (and l ^ 32, which holds the other half of the row's keys) owns row r0 + (l & 31):
// it gathers that row's Q fragments from q + (t0 + tok) * ldq + (hk * G + g) * D, masks with its own position
// pos0 + tok and scatters its own output row. Token-major keeps a wave's rows within ceil(32 / G) + 1 consecutive
// positions, so a wave computes tiles up to the position of its LAST VALID row and masks only the tiles that
// reach past the position of its FIRST row. Lanes past R repeat row R - 1 and store nothing; a wave whose rows
// are all >= R does no MFMA work but still stages K/V.
//
// Workgroup split. The up to 2 G waves of rows of a (query block, kv head) go to nwg = ceil(2 G / 8) workgroups
// of W = ceil(2 G / nwg) waves (G = 1: 1 x 2, 2: 1 x 4, 3: 1 x 6, 5: 2 x 5, 6: 2 x 6, 7: 2 x 7, 14: 4 x 7). A
// workgroup runs the tiles up to the position of ITS last valid row (the earlier rows' workgroup stops sooner)
// and leaves at once when it has no row. Grid nqb * Hkv * nwg, kv head fastest (one XCD per kv head), the latest
// query blocks and, within one, the latest rows first.
//
// W is a template constant (2, 4 .. 8): the K/V staging is register-staged (issue early, write late), so its
// per-thread chunk count KT * NCH / (64 W) must be a compile-time bound for the chunks to stay in registers; a
// runtime W would size those registers for W = 2 in every launch. Every instantiation compiles without scratch
// (profiles/prefill_any_group.txt); the runtime-W variant was not built, so there is no A/B of the two.
//
// Per tile and wave, as in attn_prefill2: S^T = K Q^T (2 key blocks x D / 16 MFMAs, 32 scores per lane),
// in-register base-2 softmax with the rescale skipped when no row maximum grew, O^T += V^T P^T with V read back
// transposed (ds_read_b64_tr_b16) from the XOR-swizzled tile and P^T straight from the S^T registers; 64-key K / V
// tiles double-buffered in LDS (2 x (K | V) x 64 x 2 D bytes), one barrier per tile.
//
// SWA (attn_window.h), as in attn_prefill2: the tile loop of a workgroup starts at the tile of its first row's first
// key; a wave skips the tiles wholly below its first row's window and masks key <= qpos - window in those that reach
// below its last row's; a tile in which all of a row's keys are masked while its m is still -inf adds exact zeros
// (the rescale and the exponent offset treat m = -inf as "nothing yet"); the head's sink joins the final 1 / l.
//
// This unit is built without the packed-fp32 VALU forms (build.py NO_PK_F32).
#include "attn_window.h"

namespace {

constexpr float LOG2E_R = 1.4426950408889634f;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

template <int D, typename KV, int W, bool SWA = false>
__global__ __launch_bounds__(64 * W, W == 2 ? 1 : 2) void attn_prefill_rows_kernel(
    const __bf16* __restrict__ q, long ldq, const KV* __restrict__ kc, const KV* __restrict__ vc,
    const int* __restrict__ block_tables, int bt_stride, const int* __restrict__ qblocks, int nqb, int Hkv, int G,
    int nwg, int bs_shift, float scale, act_t* __restrict__ out, long ldo, int window,
    const float* __restrict__ sinks) {
  constexpr int KT = 64;                 // keys per tile
  constexpr int NCH = D / 8;             // 16-byte chunks per K / V row
  constexpr int ROWB = D * 2;            // bytes per LDS row
  constexpr int TILEB = KT * ROWB;       // one K (or V) tile
  constexpr int NKS = D / 16;            // k-steps of S^T over the head dim
  constexpr int NDB = D / 32;            // 32-dim blocks of O^T
  constexpr int NT = 64 * W;             // threads
  constexpr int NE = KT * NCH;           // 16-byte chunks of a K (or V) tile
  constexpr int NLD = (NE + NT - 1) / NT;   // staging chunks per thread per tile (the last one guarded)
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * TILEB];   // [buf][K | V]

  const int bi = blockIdx.x;
  const int hk = bi % Hkv;
  const int rest = bi / Hkv;
  const int wg = nwg - 1 - rest % nwg;   // latest rows first
  const int qb = nqb - 1 - rest / nwg;   // heaviest (latest) query blocks first
  const int t0 = qblocks[qb * 4], ntok = qblocks[qb * 4 + 1], seq = qblocks[qb * 4 + 2], pos0 = qblocks[qb * 4 + 3];
  const int R = ntok * G;                // query rows of this (block, kv head)
  const int rw0 = 32 * W * wg;           // the workgroup's first row
  if (rw0 >= R) return;                  // a short block leaves the later workgroups without rows
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, tl = lane & 31;
  const int r0 = rw0 + 32 * wave;        // the wave's first row
  const bool wact = r0 < R;
  const int rho = min(r0 + tl, R - 1);   // this lane's row (rows >= R repeat the last one, never stored)
  const int tok = rho / G;
  const int head = hk * G + rho - tok * G;
  const int qpos = pos0 + tok;
  const int wfirst = pos0 + r0 / G;                      // position of the wave's first row
  const int wlast = pos0 + min(r0 + 31, R - 1) / G;      // and of its last valid row
  const int ntile = (pos0 + (min(rw0 + 32 * W, R) - 1) / G) / KT + 1;   // up to the workgroup's last valid row
  const int nkeys = pos0 + ntok;
  const int* bt = block_tables + (size_t)seq * bt_stride;
  const int bsm = (1 << bs_shift) - 1;
  const float sl2 = scale * LOG2E_R;
  const bool win = SWA && window > 0;
  const int tfirst = win ? max(0, pos0 + rw0 / G - window + 1) / KT : 0;   // the tile of the first row's first key
  const int wlo = win ? qpos - window : -1;              // the row's last key below its window

  // ---- Q^T fragments of the lane's row: dims 16 ks + 8 h .. +7
  bf16x8 qf[NKS];
  {
    const __bf16* qrow = q + (size_t)(t0 + tok) * ldq + (size_t)head * D;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * h);
  }

  // ---- staging: thread tid moves chunks e = tid + NT i < NE (key e / NCH, chunk e % NCH) of K and of V
  typename KVRaw<KV>::raw kr[NLD], vr[NLD];
  auto load_tile = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = tid + NT * i, key = e / NCH, ch = e % NCH;
      const int p = t * KT + key;
      if (e < NE && p < nkeys) {
        const size_t off = ((size_t)(bt[p >> bs_shift] << bs_shift | (p & bsm)) * Hkv + hk) * D + ch * 8;
        kr[i] = KVRaw<KV>::ld(kc + off);
        vr[i] = KVRaw<KV>::ld(vc + off);
      } else {
        kr[i] = typename KVRaw<KV>::raw{};
        vr[i] = typename KVRaw<KV>::raw{};
      }
    }
  };
  auto store_tile = [&](int buf) __attribute__((always_inline)) {
    uint8_t* kb = lds + buf * 2 * TILEB;
    uint8_t* vb = kb + TILEB;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = tid + NT * i, key = e / NCH, ch = e % NCH;
      if (NE % NT == 0 || e < NE) {
        *reinterpret_cast<u32x4*>(kb + key * ROWB + ((ch ^ (key & (NCH - 1) & 15)) << 4)) = KVRaw<KV>::bf16(kr[i]);
        *reinterpret_cast<u32x4*>(vb + key * ROWB + ((ch ^ (((key & 3) << 2) & (NCH - 1))) << 4)) = KVRaw<KV>::bf16(vr[i]);
      }
    }
  };

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  float m = -INFINITY, l = 0.f;

  load_tile(tfirst);
  store_tile(tfirst & 1);
  __syncthreads();
  // V^T fragment read: lane (group of 16: q = (l & 15) >> 2 row, p = l & 3 column quad) supplies row
  // kbase + q (and + 8), dims 32 db + 16 ((l >> 4) & 1) + 4 p
  const int vq = (lane & 15) >> 2, vp = lane & 3, vhalf = (lane >> 4) & 1;
  for (int t = tfirst; t < ntile; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntile) load_tile(t + 1);      // issue early: lands while this tile computes
    const int k0 = t * KT;
    if (wact && k0 <= wlast && (!win || k0 + KT - 1 > wfirst - window)) {
      const uint8_t* kb = lds + cur * 2 * TILEB;
      const uint8_t* vb = kb + TILEB;
      // ---- S^T = K Q^T
      f32x16 s[2];
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
        s[kb2] = f32x16{};
        const int key = 32 * kb2 + tl;
        const uint8_t* krow = kb + key * ROWB;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const int ch = 2 * ks + h;
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(krow + ((ch ^ (key & (NCH - 1) & 15)) << 4));
          s[kb2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[ks], s[kb2], 0, 0, 0);
        }
      }
      // ---- causal mask (only tiles that reach past the wave's first row; SWA: or below its last row's window)
      // + row max
      float mx = -INFINITY;
      if (k0 + KT - 1 > wfirst || (win && k0 <= wlast - window)) {
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * kb2 + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v = key <= qpos && (!SWA || key > wlo) ? s[kb2][r] : -INFINITY;
            s[kb2][r] = v;
            mx = fmaxf(mx, v);
          }
      } else {
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb2][r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx);
      if (!__all(mn == m)) {                 // some row's max grew: rescale (rare after the first tiles)
        const float alpha = (mn == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f((m - mn) * sl2);
        l *= alpha;
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] *= alpha;
        m = mn;
      }
      const float nb = (m == -INFINITY) ? 0.f : -m * sl2;
      // ---- P = exp2((s - m) * scale log2e), row partial sums, and O^T += V^T P^T per 16-key step
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int kb2 = ks >> 1, rr = 8 * (ks & 1);
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[kb2][rr + j], sl2, nb));
          l += p;
          pb[j] = (__bf16)p;
        }
        // keys of this step in the fragment's k order: 32 kb2 + 16 (ks & 1) + 4 h + {0..3, 8..11}
        const int kbase = 32 * kb2 + 16 * (ks & 1) + 4 * h;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const int ch = 4 * db + 2 * vhalf + (vp >> 1);
          const int k1 = kbase + vq, k2 = kbase + 8 + vq;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(vb + k1 * ROWB + ((ch ^ (((k1 & 3) << 2) & (NCH - 1))) << 4) + 8 * (vp & 1)));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(vb + k2 * ROWB + ((ch ^ (((k2 & 3) << 2) & (NCH - 1))) << 4) + 8 * (vp & 1)));
          const s16x8 a8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a8), pb, o[db], 0, 0, 0);
        }
      }
    }
    if (t + 1 < ntile) store_tile(cur ^ 1);   // write late: the other buffer was last read in tile t - 1
    __syncthreads();
  }
  // ---- normalise and scatter the lane's row: O[row][32 db + 8 g + 4 h + 0..3] in o[db][4 g .. 4 g + 3]
  l += __shfl_xor(l, 32, 64);
  if (wact && r0 + tl < R) {
    if constexpr (SWA) l = sink_denom(m * sl2, l, sinks, head);
    const float inv = l > 0.f ? 1.f / l : 0.f;
    act_t* orow = out + (size_t)(t0 + tok) * ldo + (size_t)head * D;
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<h4*>(orow + 32 * db + 8 * g + 4 * h) =
            h4{(act_t)(o[db][4 * g] * inv), (act_t)(o[db][4 * g + 1] * inv), (act_t)(o[db][4 * g + 2] * inv),
               (act_t)(o[db][4 * g + 3] * inv)};
  }
}

template <int D, typename KV, int W>
void launch_w(dim3 grid, hipStream_t st, const void* q, long ldq, const void* kc, const void* vc, const int* block_tables,
              int bt_stride, const int* qblocks, int nqb, int Hkv, int G, int nwg, int bs_shift, float scale, void* out,
              long ldo, int window, const float* sinks) {
#define ROWS_K(SW)                                                                                                 \
  hipLaunchKernelGGL((attn_prefill_rows_kernel<D, KV, W, SW>), grid, dim3(64 * W), 0, st, (const __bf16*)q, ldq,    \
                     (const KV*)kc, (const KV*)vc, block_tables, bt_stride, qblocks, nqb, Hkv, G, nwg, bs_shift, scale, \
                     (act_t*)out, ldo, window, sinks)
  if (window > 0 || sinks) ROWS_K(true); else ROWS_K(false);
#undef ROWS_K
}

template <int D, typename KV>
int launch_d(int W, dim3 grid, hipStream_t st, const void* q, long ldq, const void* kc, const void* vc,
             const int* block_tables, int bt_stride, const int* qblocks, int nqb, int Hkv, int G, int nwg, int bs_shift,
             float scale, void* out, long ldo, int window, const float* sinks) {
#define ROWS_W(w)                                                                                                  \
  case w:                                                                                                          \
    launch_w<D, KV, w>(grid, st, q, ldq, kc, vc, block_tables, bt_stride, qblocks, nqb, Hkv, G, nwg, bs_shift, scale, \
                       out, ldo, window, sinks);                                                                   \
    break;
  switch (W) {
    ROWS_W(2) ROWS_W(4) ROWS_W(5) ROWS_W(6) ROWS_W(7) ROWS_W(8)
    default: return -1;
  }
#undef ROWS_W
  return (int)hipGetLastError();
}

}  // namespace

// attn_d256.hip: head size 256, the token-major rows form is quad = false
int attn_prefill_d256_launch(bool quad, bool kv8, const void* q, long ldq, const void* kc, const void* vc,
                             const int* block_tables, int bt_stride, const int* qblocks, int nqb, int Hkv, int G,
                             int block_size, float scale, void* out, long ldo, void* stream, int window,
                             const float* sinks);

// The launcher behind nls_attn_prefill / nls_attn_prefill8 (attn_prefill.hip) for group sizes attn_prefill2 does not
// take: 1 <= G <= 16, D in {64, 128} (256: attn_d256.hip), a power-of-two block size. No allocation, no sync (graph-capturable).
template <typename KV>
int attn_prefill_rows_impl(const void* q, long ldq, const void* kc, const void* vc, const int* block_tables,
                           int bt_stride, const int* qblocks, int nqb, int Hq, int Hkv, int D, int block_size, float scale,
                           void* out, long ldo, void* stream, int window, const float* sinks) {
  if (Hkv < 1 || Hq % Hkv || Hq / Hkv < 1 || Hq / Hkv > 16 || (D != 64 && D != 128 && D != 256) || nqb < 1 ||
      block_size < 1 || (block_size & (block_size - 1)) || window < 0)
    return -1;
  const int G = Hq / Hkv;
  if (D == 256)
    return attn_prefill_d256_launch(false, sizeof(KV) == 1, q, ldq, kc, vc, block_tables, bt_stride, qblocks, nqb, Hkv, G,
                                    block_size, scale, out, ldo, stream, window, sinks);
  const int nwg = (2 * G + 7) / 8;               // workgroups per (query block, kv head)
  const int W = (2 * G + nwg - 1) / nwg;         // waves of 32 rows per workgroup
  const int bs_shift = __builtin_ctz(block_size);
  dim3 grid(nqb * Hkv * nwg);
  hipStream_t st = (hipStream_t)stream;
  if (D == 128)
    return launch_d<128, KV>(W, grid, st, q, ldq, kc, vc, block_tables, bt_stride, qblocks, nqb, Hkv, G, nwg, bs_shift,
                             scale, out, ldo, window, sinks);
  return launch_d<64, KV>(W, grid, st, q, ldq, kc, vc, block_tables, bt_stride, qblocks, nqb, Hkv, G, nwg, bs_shift,
                          scale, out, ldo, window, sinks);
}

template int attn_prefill_rows_impl<__bf16>(const void*, long, const void*, const void*, const int*, int, const int*,
                                            int, int, int, int, int, float, void*, long, void*, int, const float*);
template int attn_prefill_rows_impl<uint8_t>(const void*, long, const void*, const void*, const int*, int, const int*,
                                             int, int, int, int, int, float, void*, long, void*, int, const float*);
