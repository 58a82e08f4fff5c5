// Sliding-window and sink attention: the two definitions the decode kernels (attention.hip) and the prefill kernels
// (attn_prefill.hip, attn_prefill_rows.hip) share. Both enter a kernel only in its SWA instantiation (a template
// constant); the instantiations without a window and without sinks keep the code they were measured with.
//
// Window W > 0: the query at position p uses key j iff p - W < j <= p (llama.cpp: masked when p - j >= n_swa).
// W = 0: no window. Sinks: one raw logit per query head (natural-log units, not multiplied by the softmax scale) that
// joins the softmax denominator and contributes no value: out = sum_k p_k v_k / (sum_k p_k + exp(sink - m)).
#pragma once
#include "common.h"

// First key of a row with ctx = p + 1 keys: its keys are [window_lo, ctx).
DEVI int window_lo(int ctx, int window) { return window > 0 ? max(0, ctx - window) : 0; }

// The denominator of a row's FINAL normalisation from its merged (m, l) in base 2 (m2 = the maximum of the used
// scores times log2 e, l = sum_k 2^(s_k - m2)): l plus the sink's term. It enters once per (token, head) -- never per
// split or per tile. A row without keys (l = 0) stays 0, so it is still written as zeros; sinks == nullptr and a
// sink of -inf add nothing; a sink so large that exp2 overflows gives inf, and O / inf is the zero row the
// mathematical result rounds to.
DEVI float sink_denom(float m2, float l, const float* __restrict__ sinks, int head) {
  if (!sinks || !(l > 0.f)) return l;
  return l + exp2f(sinks[head] * 1.4426950408889634f - m2);
}
