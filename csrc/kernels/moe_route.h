// MoE top-k route of one token (shared by the route kernels in ops.hip and the o-projection GEMV that
// folds the FFN norm + router + route into its last workgroup, qgemv_impl.h).
#pragma once
#include "common.h"

// logits [T][E] f32; outputs: topw [T][k], counts [E] (must be zeroed), rows [E][T*k]
// (segment-local x row = token t, y row = t*k + j).
// One wave per token, lane e holds expert e (E <= 64): softmax and the k arg-max rounds are wave
// reductions, so nothing is indexed at run time (no scratch). NaN / inf logits: a NaN never wins a
// comparison, ties and NaNs resolve to the lowest unused expert, so k distinct valid experts are
// always chosen.
// One wave routes token t from its E logits `lt` (global or LDS).
DEVI void route_one(const float* __restrict__ lt, int t, int lane, int E, int k, int renorm, float* __restrict__ topw,
                    int* __restrict__ counts, int* __restrict__ xrows, int* __restrict__ yrows, int cap,
                    int* __restrict__ sel) {
  const bool live = lane < E;
  const float l = live ? lt[lane] : -INFINITY;
  float mx = l;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float p = live ? __expf(l - mx) : 0.f;
  float sum = p;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  bool used = !live;
  float wsum = 0.f, myw = 0.f;
  int myj = -1;
  for (int j = 0; j < k; ++j) {
    // arg-max over unused experts: key = (value ordered, lowest index wins ties); NaN -> lowest key
    const float v = used ? -INFINITY : p;
    uint32_t u = __float_as_uint(v);
    u = (v != v) ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    unsigned long long key = used ? 0ull : (((unsigned long long)u << 32) | (uint32_t)(63 - lane) | (1ull << 31));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(key, o, 64);
      key = ok > key ? ok : key;
    }
    const int be = 63 - (int)(key & 63);
    const float bv = __shfl(p, be, 64);
    const float w = bv / sum;
    wsum += w;
    if (lane == be) {
      used = true;
      myw = w;
      myj = j;
    }
  }
  if (myj >= 0) {
    if (sel) sel[t * k + myj] = lane;           // routed expert of (token, slot): device-selected launches
    topw[t * k + myj] = renorm ? myw / wsum : myw;
    const int pos = atomicAdd(counts + lane, 1);
    xrows[lane * cap + pos] = t;
    yrows[lane * cap + pos] = t * k + myj;
  }
}

// 64 < E <= 128: lane l holds experts l and l + 64. The contract of route_one: softmax over all E logits, k <= 8
// arg-max rounds as wave reductions over (value, lowest index) keys -- the key's index field is 7 bits wide, so an
// equal value in the low half (expert l) beats the one in the high half (expert l + 64) -- NaNs lose every
// comparison, k distinct valid experts always. Both halves live in named registers: nothing indexed at run time.
DEVI unsigned long long route_key(float p, bool used, int e) {
  uint32_t u = __float_as_uint(p);
  u = (p != p) ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
  return used ? 0ull : (((unsigned long long)u << 32) | (uint32_t)(127 - e) | (1ull << 31));
}

DEVI void route_wide(const float* __restrict__ lt, int t, int lane, int E, int k, int renorm, float* __restrict__ topw,
                     int* __restrict__ counts, int* __restrict__ xrows, int* __restrict__ yrows, int cap,
                     int* __restrict__ sel) {
  const bool live1 = lane + 64 < E;            // the low half (expert `lane` < 64 < E) is always live
  const float l0 = lt[lane];
  const float l1 = live1 ? lt[lane + 64] : -INFINITY;
  float mx = fmaxf(l0, l1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float p0 = __expf(l0 - mx);
  const float p1 = live1 ? __expf(l1 - mx) : 0.f;
  float sum = p0 + p1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  bool used0 = false, used1 = !live1;
  float wsum = 0.f, w0 = 0.f, w1 = 0.f;
  int j0 = -1, j1 = -1;
  for (int j = 0; j < k; ++j) {
    const unsigned long long k0 = route_key(p0, used0, lane), k1 = route_key(p1, used1, lane + 64);
    unsigned long long key = k1 > k0 ? k1 : k0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(key, o, 64);
      key = ok > key ? ok : key;
    }
    const int be = 127 - (int)(key & 127);
    const float b0 = __shfl(p0, be & 63, 64), b1 = __shfl(p1, be & 63, 64);
    const float w = (be < 64 ? b0 : b1) / sum;
    wsum += w;
    if (lane == (be & 63)) {
      if (be < 64) {
        used0 = true;
        w0 = w;
        j0 = j;
      } else {
        used1 = true;
        w1 = w;
        j1 = j;
      }
    }
  }
  if (j0 >= 0) {
    if (sel) sel[t * k + j0] = lane;
    topw[t * k + j0] = renorm ? w0 / wsum : w0;
    const int pos = atomicAdd(counts + lane, 1);
    xrows[lane * cap + pos] = t;
    yrows[lane * cap + pos] = t * k + j0;
  }
  if (j1 >= 0) {
    const int e = lane + 64;
    if (sel) sel[t * k + j1] = e;
    topw[t * k + j1] = renorm ? w1 / wsum : w1;
    const int pos = atomicAdd(counts + e, 1);
    xrows[e * cap + pos] = t;
    yrows[e * cap + pos] = t * k + j1;
  }
}
