// Batched token sampling on the GPU: repetition / presence / frequency penalties,
// temperature, top-k, min-p, top-p and the final draw -- one workgroup per row, one launch
// for every sampled request of a step (SURVEY.md §2F sample_topk_topp).
//
// No sort over the vocabulary: top-k and top-p become VALUE thresholds found by two histogram
// passes over block-wide counts / masses (k-th largest logit; the logit above which the kept
// probability mass reaches top_p), and the draw is an inverse-CDF walk in INDEX order over
// the kept tokens (same distribution as sampling in sorted order). The uniform variate comes
// from the host (per-request seeded generator), so seeded requests stay reproducible.
#include "common.h"

namespace {

struct SampleParams {
  float temperature, top_p, min_p, repeat_penalty, presence_penalty, frequency_penalty, u;
  int top_k, n_hist, n_bias;                          // n_bias: entries of the row's logit_bias table (0: none)
};

constexpr int NT = 1024;

DEVI float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) s += red[i];
  return s;
}

DEVI float block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float s = -INFINITY;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) s = fmaxf(s, red[i]);
  return s;
}

// order-preserving uint32 key of a float (larger float <=> larger key) and its inverse
DEVI uint32_t okey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEVI float okey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// Keep-threshold by two histogram passes (instead of ~32 bisection scans of the vocabulary): bins
// over [a, b] (bin 0 = highest logits) accumulate the weight w of each kept logit (count: 1; mass:
// exp((l - mx) * it)); the bin where the running weight from the top reaches `target` is refined by a
// second histogram over that bin alone. Returns t: keeping l >= t reaches `target` (sub-bin ties are
// kept, resolution (b - a) / NB^2).
// t is never a computed bin edge: the second pass takes exactly the logits the first one counted into the
// crossing bin (the same bin expression, not a comparison with edges that round differently), records the
// smallest logit of each sub-bin, and t is the smallest logit counted toward the target -- the bin index is
// monotone in the logit, so l >= t keeps the counted logits and nothing else. A search that finds no
// crossing (target above the weight of the whole range) returns a: the whole range is kept.
constexpr int NB = 1024;

// wave 0: the bin where above + (running weight from bin 0) reaches target -> s_bin (-1: no crossing) and the
// weight before it -> s_before; one wave scans the bins, 16 per lane
DEVI void hist_cross(const float* hbin, float above, float target, int* s_bin, float* s_before) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    float mine = 0.f;
#pragma unroll
    for (int j = 0; j < NB / 64; ++j) mine += hbin[lane * (NB / 64) + j];
    float incl = mine;                              // inclusive prefix over lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    const float excl = incl - mine;
    const bool cross = above + incl >= target && above + excl < target;
    const unsigned long long m = __ballot(cross);
    if (!m) {
      if (lane == 0) {
        *s_bin = -1;
        *s_before = above;
      }
    } else if (lane == __ffsll((long long)m) - 1) {
      float acc = above + excl;
      int bin = lane * (NB / 64) + NB / 64 - 1;
      for (int j = 0; j < NB / 64; ++j) {
        const float w = hbin[lane * (NB / 64) + j];
        if (acc + w >= target) { bin = lane * (NB / 64) + j; break; }
        acc += w;
      }
      *s_bin = bin;
      *s_before = acc;
    }
  }
}

DEVI float hist_threshold(const float* __restrict__ l, int V, float a, float b, float keep_lo, bool count, float mx,
                          float it, float target, float* hbin, float* red) {
  __shared__ uint32_t hmin[NB];
  __shared__ int s_bin;
  __shared__ float s_before;
  __shared__ uint32_t s_key;
  if (!(b > a)) return a;
  const float scale = (float)NB / (b - a);
  for (int i = threadIdx.x; i < NB; i += NT) hbin[i] = 0.f;
  __syncthreads();
  for (int i = threadIdx.x; i < V; i += NT) {
    const float v = l[i];
    if (v >= a && v <= b && v >= keep_lo && v > -INFINITY) {     // NaN / -inf never binned
      const int bin = min(NB - 1, (int)((b - v) * scale));
      atomicAdd(&hbin[bin], count ? 1.f : __expf((v - mx) * it));
    }
  }
  __syncthreads();
  hist_cross(hbin, 0.f, target, &s_bin, &s_before);
  __syncthreads();
  const int bin0 = s_bin;
  const float above = s_before;
  __syncthreads();
  if (bin0 < 0) return a;
  // second pass over the logits of bin0, re-binned over its (approximate) edges [na, nb]
  const float nb = b - (float)bin0 / scale, na = b - (float)(bin0 + 1) / scale;
  const float scale1 = nb - na > 1e-30f ? (float)NB / (nb - na) : 0.f;
  for (int i = threadIdx.x; i < NB; i += NT) {
    hbin[i] = 0.f;
    hmin[i] = 0xFFFFFFFFu;
  }
  __syncthreads();
  // (glo, ghi: the edges widened far beyond what their rounding and the bin expression's can differ by, 16 * 2^-23
  // of the largest logit -- most of the row is turned away by two comparisons; the bin expression decides)
  const float guard = 1.9e-6f * fmaxf(fabsf(a), fabsf(b));
  const float glo = fmaxf(fmaxf(a, keep_lo), na - guard), ghi = fminf(b, nb + guard);
  for (int i = threadIdx.x; i < V; i += NT) {
    const float v = l[i];
    if (v >= glo && v <= ghi && v > -INFINITY && min(NB - 1, (int)((b - v) * scale)) == bin0) {
      const int bin = max(0, min(NB - 1, (int)((nb - v) * scale1)));
      atomicAdd(&hbin[bin], count ? 1.f : __expf((v - mx) * it));
      atomicMin(&hmin[bin], okey(v));
    }
  }
  __syncthreads();
  hist_cross(hbin, above, target, &s_bin, &s_before);
  __syncthreads();
  // the smallest logit of sub-bins [0, s_bin] (of every sub-bin when rounding of the mass sums hid the crossing)
  if (threadIdx.x < 64) {
    const int last = s_bin < 0 ? NB - 1 : s_bin;
    uint32_t k = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < NB / 64; ++j) {
      const int at = threadIdx.x * (NB / 64) + j;
      if (at <= last) k = min(k, hmin[at]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k = min(k, (uint32_t)__shfl_xor((int)k, o, 64));
    if (threadIdx.x == 0) s_key = k;
  }
  __syncthreads();
  const uint32_t key = s_key;
  __syncthreads();
  return key != 0xFFFFFFFFu ? okey_inv(key) : na;
}

// Max and sum exp((l - max) * it) of a row in ONE pass (online rescaling), non-finite entries skipped.
DEVI void block_max_z(const float* __restrict__ l, int V, float it, float& mx, float& z, float* red) {
  float m = -INFINITY, s = 0.f;
#pragma unroll 8
  for (int i = threadIdx.x; i < V; i += NT) {
    const float v = l[i];
    if (!(v > -INFINITY)) continue;                  // -inf and NaN
    if (v > m) {
      s = s * __expf((m - v) * it) + 1.f;
      m = v;
    } else {
      s += __expf((v - m) * it);
    }
  }
  mx = block_max(m, red);
  z = block_sum(m > -INFINITY ? s * __expf((m - mx) * it) : 0.f, red);
}

// The draw: inverse CDF in index order over the kept logits (l >= lo), u in [0, 1). Weights are summed
// per 64-token tile (a wave per tile, coalesced), the tile sums are scanned block-wide, and one wave scans
// the tile that holds the target -- no serial walk over chunks or tokens. Returns the token in every thread.
constexpr int MAXT = 4096;                            // 64-token tiles: V <= 262144
DEVI int draw_index_order(const float* __restrict__ l, int V, float lo, float mx, float it, float u, float* tile,
                          float* red, int* s_tok) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nt = (V + 63) >> 6;
#pragma unroll 4
  for (int t = w; t < nt; t += NT / 64) {
    const int i = (t << 6) + lane;
    float x = 0.f;
    if (i < V) {
      const float v = l[i];
      if (v >= lo && v > -INFINITY) x = __expf((v - mx) * it);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane == 0) tile[t] = x;
  }
  __shared__ int s_tile;
  __shared__ float s_before;
  if (threadIdx.x == 0) s_tile = -1;
  __syncthreads();
  // exclusive scan of per-thread tile runs [per * tid, per * tid + per)
  const int per = (nt + NT - 1) / NT;
  const int t0 = threadIdx.x * per;
  float loc = 0.f;
  for (int j = 0; j < per; ++j)
    if (t0 + j < nt) loc += tile[t0 + j];
  float incl = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) red[w] = incl;
  __syncthreads();
  float off = 0.f, Z = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const float r = red[i];
    off += i < w ? r : 0.f;
    Z += r;
  }
  const float target = u * Z;
  const float excl = off + incl - loc;
  if (loc > 0.f && excl <= target && target < excl + loc) {
    float acc = excl;
    for (int j = 0; j < per && t0 + j < nt; ++j) {
      const float x = tile[t0 + j];
      if (x > 0.f && acc + x > target) {
        s_tile = t0 + j;
        s_before = acc;
        break;
      }
      acc += x;
    }
  }
  __syncthreads();
  int t = s_tile;
  float before = s_before;
  bool last = false;
  if (t < 0) {                                        // rounding at the very end: the last kept token
    int mine = -1;
    for (int j = per - 1; j >= 0; --j)
      if (t0 + j < nt && tile[t0 + j] > 0.f) { mine = t0 + j; break; }
    t = (int)block_max((float)mine, red);             // exact for tile ids < 2^24
    last = true;
  }
  if (w == 0) {
    int tok = -1;
    if (t >= 0) {
      const int i = (t << 6) + lane;
      float x = 0.f;
      if (i < V) {
        const float v = l[i];
        if (v >= lo && v > -INFINITY) x = __expf((v - mx) * it);
      }
      const unsigned long long kept = __ballot(x > 0.f);
      if (!last) {
        float c = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const float y = __shfl_up(c, o, 64);
          if (lane >= o) c += y;
        }
        const unsigned long long hit = __ballot(x > 0.f && before + c > target);
        if (hit) tok = (t << 6) + __ffsll((long long)hit) - 1;
      }
      if (tok < 0 && kept) tok = (t << 6) + 63 - __clzll((long long)kept);
    }
    if (lane == 0) *s_tok = tok < 0 ? 0 : tok;       // nothing kept: a non-finite row -> a valid id anyway
  }
  __syncthreads();
  return *s_tok;
}

// ---- top-k fast path (0 < top_k <= KFAST, the usual chat payload: top_k 40): after the top-k threshold
// (two histogram passes) every kept logit is compacted into LDS in ONE more pass, and min-p, top-p and the
// draw run on those <= CCAP entries -- 4 passes over the vocabulary instead of 8. The k-th largest value is
// taken exactly from the sorted candidates (the binned threshold keeps its sub-bin ties), so the kept set,
// the top-p cut and the index-order draw are those of the CPU twin (engine/sampling.py sample_rows).
constexpr int KFAST = 256;
constexpr int CCAP = 512;

// block bitonic sort of CCAP (key, idx) pairs in LDS: by value, descending (ties: lower index first), or by
// index, ascending. Padding entries carry (-inf, INT_MAX) and end up last either way.
DEVI void bitonic_pairs(float* key, int* idx, bool byval) {
  for (int k = 2; k <= CCAP; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < CCAP; i += NT) {
        const int l = i ^ j;
        if (l > i) {
          const float ka = key[i], kb = key[l];
          const int ia = idx[i], ib = idx[l];
          const bool a_first = byval ? (ka > kb || (ka == kb && ia < ib)) : ia < ib;
          if (((i & k) == 0) != a_first) {
            key[i] = kb;
            key[l] = ka;
            idx[i] = ib;
            idx[l] = ia;
          }
        }
      }
    }
  __syncthreads();
}

// inclusive block scan of one value per thread (NT threads)
DEVI float block_incl_scan(float v, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  __syncthreads();
  if (lane == 63) red[w] = incl;
  __syncthreads();
  float off = 0.f;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) off += i < w ? red[i] : 0.f;
  return off + incl;
}

// Returns the token (every thread), or -1 (every thread) when the compacted set overflows CCAP (a row with
// massive ties at the threshold): the caller then takes the general path.
DEVI int sample_topk_fast(const float* __restrict__ l, int V, const SampleParams& p, float u, float mx, float mn,
                          float it, float* red, float* sk, int* sidx, float* hbin) {
  __shared__ int s_n, s_pick, s_last;
  __shared__ float s_tot, s_thr, s_z;
  const float t = hist_threshold(l, V, mn, mx, -INFINITY, true, mx, it, (float)p.top_k, hbin, red);
  if (threadIdx.x == 0) {
    s_n = 0;
    s_pick = 0x7FFFFFFF;
    s_last = -1;
    s_thr = 0.f;              // (no crossing found through rounding: keep the whole top-k set)
  }
  __syncthreads();
  for (int i = threadIdx.x; i < V; i += NT) {
    const float v = l[i];
    if (v >= t && v > -INFINITY) {
      const int at = atomicAdd(&s_n, 1);
      if (at < CCAP) {
        sk[at] = v;
        sidx[at] = i;
      }
    }
  }
  __syncthreads();
  const int n = s_n;
  if (n > CCAP || n < 1) return -1;
  for (int i = n + threadIdx.x; i < CCAP; i += NT) {
    sk[i] = -INFINITY;
    sidx[i] = 0x7FFFFFFF;
  }
  bitonic_pairs(sk, sidx, true);
  // exact k-th largest (ties kept), then min-p
  float lo = sk[min(p.top_k, n) - 1];
  if (p.min_p > 0.f) lo = fmaxf(lo, mx + p.temperature * __logf(p.min_p));
  const int j = threadIdx.x;
  const bool in = j < n && sk[j] >= lo;
  float w = in ? __expf((sk[j] - mx) * it) : 0.f;
  if (p.top_p < 1.f) {
    // smallest top set (by value) whose mass reaches top_p of the kept mass; ties of its last weight kept
    const float cum = block_incl_scan(w, red);
    if (j == NT - 1) s_tot = cum;
    __syncthreads();
    const float target = p.top_p * s_tot;
    if (in && cum >= target && cum - w < target) s_thr = w;
    __syncthreads();
    if (w < s_thr) w = 0.f;
  }
  // the draw: inverse CDF in INDEX order over the kept entries
  __syncthreads();
  if (j < CCAP) sk[j] = w;
  // by index (weights ride along as keys)
  for (int k = 2; k <= CCAP; k <<= 1)
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < CCAP; i += NT) {
        const int o = i ^ jj;
        if (o > i && (((i & k) == 0) != (sidx[i] < sidx[o]))) {
          const float kt = sk[i];
          sk[i] = sk[o];
          sk[o] = kt;
          const int it2 = sidx[i];
          sidx[i] = sidx[o];
          sidx[o] = it2;
        }
      }
    }
  __syncthreads();
  const float wj = j < CCAP ? sk[j] : 0.f;
  const float cdf = block_incl_scan(wj, red);
  if (j == NT - 1) s_z = cdf;
  __syncthreads();
  const float target = u * s_z;
  if (wj > 0.f && cdf > target) atomicMin(&s_pick, j);
  if (wj > 0.f) atomicMax(&s_last, j);
  __syncthreads();
  const int at = s_pick != 0x7FFFFFFF ? s_pick : s_last;
  return at >= 0 ? sidx[at] : 0;
}

// One row: penalties over the history window h[0, n_hist) (any order), then greedy / temperature /
// top-k / min-p / top-p and the draw with uniform u. The token is returned in EVERY thread.
DEVI int sample_one(float* __restrict__ l, int V, const SampleParams& p, float u, const int* __restrict__ h,
                    int n_hist, float* red, float* s_chunk, int* s_tok, float* hbin) {
  // 1) penalties on the distinct ids of the history window (llama.cpp-style semantics)
  if (n_hist > 0 && (p.repeat_penalty != 1.f || p.presence_penalty != 0.f || p.frequency_penalty != 0.f)) {
    const int j = threadIdx.x;
    if (j < n_hist) {
      const int id = h[j];
      bool first = true;
      int cnt = 0;
      for (int i = 0; i < n_hist; ++i) {
        if (h[i] == id) {
          ++cnt;
          if (i < j) first = false;
        }
      }
      if (first && id >= 0 && id < V) {
        float v = l[id];
        if (p.repeat_penalty != 1.f) v = v > 0.f ? v / p.repeat_penalty : v * p.repeat_penalty;
        v -= p.presence_penalty + p.frequency_penalty * (float)cnt;
        l[id] = v;
      }
    }
    __syncthreads();
  }
  // 2) greedy: plain arg-max (lowest index on ties)
  const bool trunc = (p.top_k > 0 && p.top_k < V) || p.min_p > 0.f;
  const float it = p.temperature > 0.f ? 1.f / p.temperature : 0.f;
  if (p.temperature > 0.f && p.top_k > 0 && p.top_k <= KFAST && p.top_k < V && s_chunk != nullptr) {
    float m = -INFINITY, mnv = INFINITY;
    for (int i = threadIdx.x; i < V; i += NT) {
      const float v = l[i];
      if (v > -INFINITY) {
        m = fmaxf(m, v);
        mnv = fminf(mnv, v);
      }
    }
    const float fmx = block_max(m, red), fmn = -block_max(-mnv, red);
    if (fmx > -INFINITY) {
      const int tok = sample_topk_fast(l, V, p, u, fmx, fmn, it, red, s_chunk,
                                       reinterpret_cast<int*>(s_chunk + CCAP), hbin);
      if (tok >= 0) return tok;
    }
  }
  float mx = -INFINITY, Z = 0.f;
  if (p.temperature > 0.f && !trunc) {
    block_max_z(l, V, it, mx, Z, red);               // max and the untruncated mass in one pass
  } else {
    for (int i = threadIdx.x; i < V; i += NT) mx = fmaxf(mx, l[i]);
    mx = block_max(mx, red);
  }
  if (p.temperature <= 0.f) {
    int best = 0x7FFFFFFF;
    for (int i = threadIdx.x; i < V; i += NT)
      if (l[i] == mx) best = min(best, i);
    float b = (float)best;   // exact for V < 2^24
    b = -block_max(-b, red);
    // no logit equals the max only when the row is all NaN: never hand an out-of-range id to the
    // next step's embedding gather (chained decode feeds next_ids straight back on the device)
    return b < (float)V ? (int)b : 0;
  }
  // 3) keep-threshold on the logit scale: top-k (k-th largest) and min-p (p >= min_p * p_max)
  float lo = -INFINITY;
  if (p.top_k > 0 && p.top_k < V) {
    // lower search bound over FINITE logits only: a masked (-inf) entry would make the bin scale 0
    // and its bin index NaN, and the threshold -inf would keep the whole vocabulary
    float mn = INFINITY;
    for (int i = threadIdx.x; i < V; i += NT) {
      const float v = l[i];
      if (v > -INFINITY) mn = fminf(mn, v);
    }
    mn = -block_max(-mn, red);
    lo = hist_threshold(l, V, mn, mx, -INFINITY, true, mx, it, (float)p.top_k, hbin, red);
  }
  if (p.min_p > 0.f) lo = fmaxf(lo, mx + p.temperature * __logf(p.min_p));
  // 4) top-p: logit threshold above which the kept mass reaches top_p of the kept total
  if (p.top_p < 1.f) {
    if (trunc) {
      Z = 0.f;
      for (int i = threadIdx.x; i < V; i += NT)
        if (l[i] >= lo) Z += __expf((l[i] - mx) * it);
      Z = block_sum(Z, red);
    }
    // tokens more than 30 temperatures below the max carry < e^-30 of the mass each: search above them
    const float a = fmaxf(lo, mx - 30.f * p.temperature);
    lo = fmaxf(lo, hist_threshold(l, V, a, mx, lo, false, mx, it, p.top_p * Z, hbin, red));
  }
  // 5) inverse CDF in index order over the kept tokens
  return draw_index_order(l, V, lo, mx, it, u, s_chunk, red, s_tok);
}

// logit_bias (stage 0, in front of the penalties): the row's table of nb <= NT (id, value) entries is ADDED to the
// raw fp32 logits, the row is sampled as any other, and the raw words are written back once the token is known -- on
// every exit of sample_one, since this wraps it -- so the row keeps no trace of its bias (the logprob kernels around
// the sampler read raw logits). Thread j owns entry j and keeps its raw word in a register. The ids of a row are
// DISTINCT (the host guarantees it: SamplingParams.logit_bias comes from the keys of a JSON object); two entries
// with one id would race here. An id outside [0, V) is skipped. -inf and NaN logits stay what they are (x + b).
// sample_one returns behind a barrier that follows its last read of the row, so the write-back needs none.
//
// Allowed-token mask (stage -1, in front of the bias): `mask` is the row's ceil(V/32) words, bit (t & 31) of word
// (t >> 5) set: token t is allowed; null: the row has no mask. A disallowed t < V gets -inf, which bias and penalties
// leave -inf and no later stage keeps; bits at t >= V are ignored and nothing at or beyond l + V is written. Unlike
// the bias the -inf words STAY in the row (callers sample copies of the rows they still need raw). A bias entry on a
// disallowed id reads -inf behind the barrier, adds to it and writes -inf back.
DEVI int sample_one_biased(float* __restrict__ l, int V, const SampleParams& p, float u, const int* __restrict__ h,
                           int n_hist, const int* __restrict__ bid, const float* __restrict__ bval, int nb,
                           const unsigned* __restrict__ mask, float* red, float* s_chunk, int* s_tok, float* hbin) {
  if (mask != nullptr) {
    // one logit per lane: 32 neighbouring lanes share a mask word (one broadcast load), the -inf stores coalesce
    for (int t = threadIdx.x; t < V; t += NT)
      if (!((mask[t >> 5] >> (t & 31)) & 1u)) l[t] = -INFINITY;
    __syncthreads();
  }
  int id = -1;
  float raw = 0.f;                                    // (a float load and store move the word as it is, NaN included)
  if (nb > 0) {
    if ((int)threadIdx.x < nb) {
      const int t = bid[threadIdx.x];
      if (t >= 0 && t < V) {
        id = t;
        raw = l[t];
        l[t] = raw + bval[threadIdx.x];
      }
    }
    __syncthreads();
  }
  const int tok = sample_one(l, V, p, u, h, n_hist, red, s_chunk, s_tok, hbin);
  if (id >= 0) l[id] = raw;
  return tok;
}

__global__ __launch_bounds__(NT) void sample_kernel(float* __restrict__ logits, long ld, int V,
                                                    const SampleParams* __restrict__ params,
                                                    const int* __restrict__ hist, int hist_stride,
                                                    const int* __restrict__ bias_ids,
                                                    const float* __restrict__ bias_val, int bias_stride,
                                                    const unsigned* __restrict__ mask, int mask_stride,
                                                    const int* __restrict__ mask_rows, int n_masks,
                                                    int* __restrict__ out) {
  __shared__ float red[NT / 64];
  __shared__ float s_chunk[MAXT];
  __shared__ int s_tok;
  __shared__ float hbin[NB];
  const int row = blockIdx.x;
  const SampleParams p = params[row];
  const int nb = bias_ids != nullptr ? min(p.n_bias, bias_stride) : 0;
  // -1: no mask. The host guarantees mr < n_masks (engine/sampling.py mask_tables numbers the rows of the table it
  // stacks); the check only keeps a broken caller from reading past the table -- such a row is sampled unmasked
  const int mr = mask_rows != nullptr ? mask_rows[row] : -1;
  const unsigned* m = mr >= 0 && mr < n_masks ? mask + (size_t)mr * mask_stride : nullptr;
  const int tok = sample_one_biased(logits + (size_t)row * ld, V, p, p.u, hist + (size_t)row * hist_stride, p.n_hist,
                                    bias_ids + (size_t)row * bias_stride, bias_val + (size_t)row * bias_stride, nb, m,
                                    red, s_chunk, &s_tok, hbin);
  if (threadIdx.x == 0) out[row] = tok;
}

// counter-based uniform in [0, 1): splitmix64 of (seed, position) -- reproducible per seeded request
DEVI float uniform01(unsigned long long seed, int pos) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(pos + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.f / 16777216.f);
}

// In-graph sampling of a decode step: rows whose params ask for sampling replace the fused arg-max
// token in next_ids with a draw; the uniform comes from (seed, position), the penalty window is a
// per-row ring of the last HIST tokens indexed by absolute position (the host fills it when the row
// is assigned, every sampled step appends its token), so sampled rows stay on the chained
// asynchronous decode path (no host round trip, no logits copy).
__global__ __launch_bounds__(NT) void sample_decode_kernel(float* __restrict__ logits, long ld, int V,
                                                           const SampleParams* __restrict__ params,
                                                           const unsigned long long* __restrict__ seeds,
                                                           const int* __restrict__ pos, const int* __restrict__ ctx_len,
                                                           int* __restrict__ hist, int hist_stride,
                                                           const int* __restrict__ bias_ids,
                                                           const float* __restrict__ bias_val, int bias_stride,
                                                           int* __restrict__ next_ids) {
  __shared__ float red[NT / 64];
  __shared__ float s_chunk[MAXT];
  __shared__ int s_tok;
  __shared__ float hbin[NB];
  const int row = blockIdx.x;
  const SampleParams p = params[row];
  const bool penal = p.repeat_penalty != 1.f || p.presence_penalty != 0.f || p.frequency_penalty != 0.f;
  const int nb = bias_ids != nullptr ? min(p.n_bias, bias_stride) : 0;
  // padding / greedy row (a temperature-0 row with a bias table is no greedy row: its arg-max is the biased one)
  if (ctx_len[row] <= 0 || (p.temperature <= 0.f && !penal && nb <= 0)) return;
  const int ps = pos[row];
  int* h = hist + (size_t)row * hist_stride;
  const int n_hist = min(hist_stride, ps + 1);
  const int tok = sample_one_biased(logits + (size_t)row * ld, V, p, uniform01(seeds[row], ps), h, n_hist,
                                    bias_ids + (size_t)row * bias_stride, bias_val + (size_t)row * bias_stride, nb,
                                    nullptr, red, s_chunk, &s_tok, hbin);
  if (threadIdx.x == 0) {
    next_ids[row] = tok;
    h[(ps + 1) % hist_stride] = tok;
  }
}

// Tensor-parallel variant: the row is the gathered candidate list of every rank (values `cand` [n, M] in
// vocabulary order, global ids `ids`, (-inf, -1) padding) instead of the full vocabulary. The history ring
// (token ids) is mapped to candidate positions first -- a history token outside the candidates cannot
// reach the kept set (the engine only takes this path when penalties can only LOWER logits and top-k fits
// the candidates: Engine._cand_ok) -- then the same sampler draws a position, whose id is the token.
constexpr int MAXC = 1024;
__global__ __launch_bounds__(NT) void sample_decode_cand_kernel(float* __restrict__ cand, long ld, int M,
                                                                const int* __restrict__ ids, long ldi,
                                                                const SampleParams* __restrict__ params,
                                                                const unsigned long long* __restrict__ seeds,
                                                                const int* __restrict__ pos,
                                                                const int* __restrict__ ctx_len,
                                                                int* __restrict__ hist, int hist_stride,
                                                                int* __restrict__ next_ids) {
  __shared__ float red[NT / 64];
  __shared__ float s_chunk[MAXT];
  __shared__ int s_tok;
  __shared__ float hbin[NB];
  __shared__ int s_ids[MAXC];
  __shared__ int s_hpos[NT];
  const int row = blockIdx.x;
  const SampleParams p = params[row];
  const bool penal = p.repeat_penalty != 1.f || p.presence_penalty != 0.f || p.frequency_penalty != 0.f;
  if (ctx_len[row] <= 0 || (p.temperature <= 0.f && !penal)) return;     // padding / greedy row
  const int* idr = ids + (size_t)row * ldi;
  for (int i = threadIdx.x; i < M; i += NT) s_ids[i] = idr[i];
  const int ps = pos[row];
  int* h = hist + (size_t)row * hist_stride;
  const int n_hist = min(hist_stride, ps + 1);
  __syncthreads();
  if (threadIdx.x < n_hist) {
    const int id = h[threadIdx.x];
    int at = -1;
    if (id >= 0)
      for (int i = 0; i < M; ++i)
        if (s_ids[i] == id) {
          at = i;
          break;
        }
    s_hpos[threadIdx.x] = at;
  }
  __syncthreads();
  const int j = sample_one(cand + (size_t)row * ld, M, p, uniform01(seeds[row], ps), s_hpos, n_hist, red, s_chunk,
                           &s_tok, hbin);
  if (threadIdx.x == 0) {
    const int tok = (j >= 0 && j < M && s_ids[j] >= 0) ? s_ids[j] : 0;
    next_ids[row] = tok;
    h[(ps + 1) % hist_stride] = tok;
  }
}


// ---------------------------------------------------------------------------------------------------------------
// Tensor-parallel sampling: per row, the C largest logits of this rank's vocab shard in VOCABULARY order, written as
// (f32 value bits, global token id) straight into the [2][n][C] int32 source buffer of the candidate all-gather
// (parallel/comm.py gather_candidates) -- the round-5 graph ran PyTorch's radix top-k + sort + gather + fill + stack
// here (profiles/tp_graph_nodes_r05.txt). One 256-thread workgroup per row:
//   * radix select of the k-th largest order-preserving key (k = min(C, valid)): four 8-bit histogram passes over
//     the row (L2-resident after the first), each bin found by a wave-0 suffix scan; T = that key, need_eq = how many
//     keys equal to T belong to the top k (the lowest indices first: deterministic, ties never exceed k);
//   * compaction in index order: each thread owns a contiguous chunk, counts its keys > T and == T, a block
//     exclusive scan gives every thread its output offset, and it writes its selected entries in order.
// Shards with fewer than C tokens pad with (-inf, -1), as the host reference does.
constexpr int TCT = 256;

// exclusive prefix sums over the workgroup of two per-thread counts (TCT threads); returns via refs
DEVI void block_excl2(int a, int b, int& ea, int& eb, int* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int ia = a, ib = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ta = __shfl_up(ia, o, 64), tb = __shfl_up(ib, o, 64);
    if (lane >= o) {
      ia += ta;
      ib += tb;
    }
  }
  if (lane == 63) {
    red[w] = ia;
    red[4 + w] = ib;
  }
  __syncthreads();
  int oa = 0, ob = 0;
#pragma unroll
  for (int i = 0; i < TCT / 64; ++i)
    if (i < w) {
      oa += red[i];
      ob += red[4 + i];
    }
  ea = oa + ia - a;
  eb = ob + ib - b;
}

// the selection key: -0.0 and +0.0 are one value (a tie, lowest indices first), as in logprob_kernel
DEVI uint32_t tkey(float f) { return okey(f == 0.f ? 0.f : f); }

__global__ __launch_bounds__(TCT) void topc_kernel(const float* __restrict__ logits, long ld, int valid, int C,
                                                   int vocab_lo, int* __restrict__ out, long plane) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_bin, s_above;
  __shared__ int red[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (size_t)row * ld;
  int* ov = out + (size_t)row * C;
  int* oi = out + plane + (size_t)row * C;
  const int k = min(C, max(valid, 0));
  for (int j = k + tid; j < C; j += TCT) {          // padding of a short shard
    ov[j] = (int)0xFF800000u;
    oi[j] = -1;
  }
  if (k <= 0) return;
  uint32_t prefix = 0u, mask = 0u;
  int need = k;                                       // keys still to take at the current prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < valid; i += TCT) {
      const uint32_t key = tkey(x[i]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {                                   // wave 0: lane l holds bins 4l..4l+3; suffix sums over lanes
      const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
      const uint32_t ls = h0 + h1 + h2 + h3;
      uint32_t sfx = ls;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_down(sfx, o, 64);
        if (tid + o < 64) sfx += t;
      }
      uint32_t above = sfx - ls;                      // keys in bins above this lane's four
      const uint32_t hh[4] = {h0, h1, h2, h3};
#pragma unroll
      for (int e = 3; e >= 0; --e) {
        const uint32_t c = above + hh[e];
        if (above < (uint32_t)need && c >= (uint32_t)need) {
          s_bin = 4u * tid + e;
          s_above = above;
        }
        above = c;
      }
    }
    __syncthreads();
    prefix |= s_bin << shift;
    mask |= 255u << shift;
    need -= (int)s_above;
    __syncthreads();                                  // s_bin / hist reused by the next pass
  }
  // keys > prefix: k - need of them, all taken; keys == prefix: the first `need` in index order
  const int chunk = (valid + TCT - 1) / TCT;
  const int c0 = min(valid, tid * chunk), c1 = min(valid, c0 + chunk);
  int ngt = 0, neq = 0;
  for (int i = c0; i < c1; ++i) {
    const uint32_t key = tkey(x[i]);
    ngt += key > prefix;
    neq += key == prefix;
  }
  int gt, eq;
  block_excl2(ngt, neq, gt, eq, red);
  for (int i = c0; i < c1; ++i) {
    const float v = x[i];
    const uint32_t key = tkey(v);
    int pos = -1;
    if (key > prefix) {
      pos = gt + min(eq, need);
      ++gt;
    } else if (key == prefix) {
      if (eq < need) pos = gt + eq;
      ++eq;
    }
    if (pos >= 0) {
      ov[pos] = __float_as_int(v);
      oi[pos] = vocab_lo + i;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Per-token log-probabilities of the model's own distribution: log_softmax of the RAW fp32 logits over [0, V) at
// temperature 1 -- before penalties and truncation, non-finite entries skipped -- for the chosen token and the n_top
// (<= LP_TOP) most likely tokens, ordered by descending logit, ties by lower id (at the cut too). Two launches around
// the sampler, which rewrites the logits of penalised history tokens in place and recycles a history-ring slot:
//   logprob_kernel (before it; one workgroup per row, two read passes over the row):
//     1) online max / sum exp in one pass, every thread keeping the largest logit it saw. The k-th largest of the NT
//        thread maxima (k rounds of a block-wide max over (value, thread) keys) is a lower bound tau of the row's
//        k-th largest logit: those are k distinct entries >= tau;
//     2) the entries >= tau -- about k of them unless the large logits crowd into few threads' strides -- are
//        compacted into LDS and ranked by counting (value descending, id ascending): ids are exact by construction.
//        More than LP_CAP survivors (massive ties, or every large logit in one thread's stride): k exact rounds of
//        "the next entry in (value, id) order" over the row instead -- slow, degenerate rows only.
//     It writes the top-n entries, leaves (max, log sum) in record words 0 / 1 for the pick, and stashes (id, raw
//     logit) of a penalised row's history window.
//   logprob_pick_kernel (after it; one thread per row): raw logit of next_ids[row] from the stash if the id is there,
//     else from the row; record words 0 / 1 become (id, (raw - max) - log sum).
// Record (LP_REC int32 words, 176 B): chosen id | chosen logprob bits | LP_TOP logprob bits | LP_TOP ids | 2 pad;
// entries past the row's finite count are (-1, -inf). Rows with n_top < 0 (and padding rows, ctx_len <= 0) are left
// untouched by both kernels.
constexpr int LP_TOP = 20;
constexpr int LP_REC = 2 + 2 * LP_TOP + 2;
constexpr int LP_CAP = 2048;

DEVI unsigned long long block_max_u64(unsigned long long v, unsigned long long* red64) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red64[w] = v;
  __syncthreads();
  unsigned long long s = 0ull;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) s = red64[i] > s ? red64[i] : s;
  return s;
}

// SHARD (tensor parallelism, one launch per rank): the row is the rank's vocab shard, V (>= 0) real columns holding
// the ids [vocab_lo, vocab_lo + V). The same two passes; the output is a shard partial of LP_REC words for
// logprob_merge_kernel instead of a record: max bits (-inf: no finite entry) | sum exp(l - max) (the sum, not its
// log; 0: no finite entry) | LP_TOP RAW logits | LP_TOP GLOBAL ids | raw logit of next_ids[row] if the shard owns the
// id (bit for bit) | 1 if it does, else 0. No stash: the TP sampler works on gathered copies of the candidates.
template <bool SHARD>
__global__ __launch_bounds__(NT) void logprob_kernel(const float* __restrict__ logits, long ld, int V,
                                                     const int* __restrict__ n_top, const int* __restrict__ ctx_len,
                                                     const SampleParams* __restrict__ params,
                                                     const int* __restrict__ pos, const int* __restrict__ hist,
                                                     int hist_stride, int* __restrict__ rec, int* __restrict__ stash,
                                                     int vocab_lo, const int* __restrict__ next_ids) {
  __shared__ float red[NT / 64];
  __shared__ unsigned long long red64[NT / 64];
  __shared__ float s_val[LP_CAP];
  __shared__ int s_idx[LP_CAP];
  __shared__ int s_n;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int nt = min(n_top[row], LP_TOP);
  if (nt < 0 || (ctx_len != nullptr && ctx_len[row] <= 0)) return;
  const float* l = logits + (size_t)row * ld;
  int* r = rec + (size_t)row * LP_REC;
  // the penalised row's history window with its raw logits, before the sampler rewrites them
  if (!SHARD && stash != nullptr) {
    int* st = stash + (size_t)row * (1 + 2 * hist_stride);
    int nh = 0;
    if (params != nullptr) {
      const SampleParams p = params[row];
      if (p.repeat_penalty != 1.f || p.presence_penalty != 0.f || p.frequency_penalty != 0.f)
        nh = min(hist_stride, pos[row] + 1);
    }
    if (tid < nh) {
      const int id = hist[(size_t)row * hist_stride + tid];
      st[1 + tid] = id;
      st[1 + hist_stride + tid] = __float_as_int(id >= 0 && id < V ? l[id] : 0.f);
    }
    if (tid == 0) st[0] = nh;
  }
  // 1) max, sum exp(l - max), finite count; m stays this thread's largest logit
  float m = -INFINITY, s = 0.f, c = 0.f;
#pragma unroll 8
  for (int i = tid; i < V; i += NT) {
    const float v = l[i];
    if (!(v > -INFINITY)) continue;                  // -inf and NaN
    c += 1.f;
    if (v > m) {
      s = s * __expf(m - v) + 1.f;
      m = v;
    } else {
      s += __expf(v - m);
    }
  }
  const float mx = block_max(m, red);
  const float z = block_sum(m > -INFINITY ? s * __expf(m - mx) : 0.f, red);
  const int nfin = (int)block_sum(c, red);            // exact: V < 2^24
  if (SHARD) {
    if (tid == 0) {
      const int id = next_ids[row] - vocab_lo;        // (an id below vocab_lo, -1 included: negative)
      const bool own = id >= 0 && id < V;
      r[0] = __float_as_int(nfin > 0 ? mx : -INFINITY);
      r[1] = __float_as_int(nfin > 0 ? z : 0.f);
      r[2 + 2 * LP_TOP] = own ? __float_as_int(l[id]) : 0;
      r[3 + 2 * LP_TOP] = own ? 1 : 0;
    }
  } else if (tid == 0) {                              // (a row with no finite entry: the pick reports the raw logit)
    r[0] = __float_as_int(nfin > 0 ? mx : 0.f);
    r[1] = __float_as_int(nfin > 0 ? logf(z) : 0.f);
  }
  const int k = min(nt, nfin);
  for (int j = k + tid; j < LP_TOP; j += NT) {
    r[2 + j] = (int)0xFF800000u;
    r[2 + LP_TOP + j] = -1;
  }
  if (k <= 0) return;
  const float logz = logf(z);
  // lower bound of the k-th largest logit: the k-th largest thread maximum
  unsigned long long mine = m > -INFINITY ? ((unsigned long long)okey(m) << 32) | (unsigned)(NT - 1 - tid) : 0ull;
  unsigned long long kth = 0ull;
  for (int j = 0; j < k; ++j) {
    kth = block_max_u64(mine, red64);
    if (mine == kth) mine = 0ull;
  }
  const float tau = kth ? okey_inv((uint32_t)(kth >> 32)) : -INFINITY;   // fewer than k threads hold finite entries
  // 2) survivors into LDS
  if (tid == 0) s_n = 0;
  __syncthreads();
#pragma unroll 8
  for (int i = tid; i < V; i += NT) {
    const float v = l[i];
    if (v > -INFINITY && v >= tau) {
      const int at = atomicAdd(&s_n, 1);
      if (at < LP_CAP) {
        s_val[at] = v;
        s_idx[at] = i;
      }
    }
  }
  __syncthreads();
  const int n = s_n;
  if (n <= LP_CAP) {
    for (int j = tid; j < n; j += NT) {
      const float vj = s_val[j];
      const int ij = s_idx[j];
      int rank = 0;
      for (int q = 0; q < n; ++q) {
        const float vq = s_val[q];
        rank += (vq > vj || (vq == vj && s_idx[q] < ij)) ? 1 : 0;
      }
      if (rank < k) {
        r[2 + rank] = __float_as_int(SHARD ? vj : (vj - mx) - logz);
        r[2 + LP_TOP + rank] = SHARD ? vocab_lo + ij : ij;
      }
    }
    return;
  }
  // degenerate row: the next entry in (value descending, id ascending) order, k times
  unsigned long long prev = ~0ull;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = 0ull;
    for (int i = tid; i < V; i += NT) {
      const float v = l[i];
      if (!(v > -INFINITY)) continue;
      const unsigned long long key = ((unsigned long long)okey(v == 0.f ? 0.f : v) << 32) | (0xFFFFFFFFu - (unsigned)i);
      if (key < prev && key > best) best = key;
    }
    prev = block_max_u64(best, red64);
    if (prev == 0ull) break;                          // (cannot happen: k <= finite entries)
    if (tid == 0) {
      const int id = (int)(0xFFFFFFFFu - (unsigned)(prev & 0xFFFFFFFFull));
      r[2 + j] = __float_as_int(SHARD ? l[id] : (l[id] - mx) - logz);
      r[2 + LP_TOP + j] = SHARD ? vocab_lo + id : id;
    }
  }
}

// Tensor parallelism, after the all-gather of the shard partials: parts[row] = W partials (rank p at words
// [LP_REC p, LP_REC p + LP_REC)) -> the ordinary record. One wave per row. M = max m_r over the shards with z_r > 0,
// Z = sum z_r exp(m_r - M); an entry's logprob is (v - M) - log Z, the expression of logprob_kernel. The top n_top are
// ranked by counting over the <= LP_TOP * W gathered candidates (value descending, global id ascending; ids < 0 are
// absent): the global top-n lies in the union of the shards' top-n under the same order, so ties at the cut are exact.
// The chosen token's raw logit comes from the shard that owns it; none does (-1, an id past the vocabulary): -inf. A
// row with no finite entry anywhere: M = log Z = 0, as logprob_kernel / logprob_pick_kernel leave it.
constexpr int LP_MERGE_RANKS = 8;                     // AR_MAX_RANKS of allreduce.hip

__global__ __launch_bounds__(64) void logprob_merge_kernel(const int* __restrict__ parts, int W,
                                                           const int* __restrict__ n_top,
                                                           const int* __restrict__ ctx_len,
                                                           const int* __restrict__ next_ids, int* __restrict__ rec) {
  __shared__ float s_val[LP_TOP * LP_MERGE_RANKS];
  __shared__ int s_idx[LP_TOP * LP_MERGE_RANKS];
  const int row = blockIdx.x, lane = threadIdx.x;
  const int nt = min(n_top[row], LP_TOP);
  if (nt < 0 || (ctx_len != nullptr && ctx_len[row] <= 0)) return;
  const int* p = parts + (size_t)row * W * LP_REC;
  int* r = rec + (size_t)row * LP_REC;
  // every lane: the W (max, sum) pairs and the owner's raw logit -- uniform, W <= 8
  float M = -INFINITY;
  for (int q = 0; q < W; ++q) {
    const float mq = __int_as_float(p[q * LP_REC]), zq = __int_as_float(p[q * LP_REC + 1]);
    if (zq > 0.f) M = fmaxf(M, mq);
  }
  float Z = 0.f, raw = -INFINITY;
  for (int q = 0; q < W; ++q) {
    const float mq = __int_as_float(p[q * LP_REC]), zq = __int_as_float(p[q * LP_REC + 1]);
    if (zq > 0.f) Z += zq * expf(mq - M);
    if (p[q * LP_REC + 3 + 2 * LP_TOP] == 1) raw = __int_as_float(p[q * LP_REC + 2 + 2 * LP_TOP]);
  }
  const bool any = Z > 0.f;
  const float mx = any ? M : 0.f, logz = any ? logf(Z) : 0.f;
  const int nc = W * LP_TOP;
  int mine = 0;
  for (int j = lane; j < nc; j += 64) {
    const int q = j / LP_TOP, e = j - q * LP_TOP;
    const int id = p[q * LP_REC + 2 + LP_TOP + e];
    s_val[j] = __int_as_float(p[q * LP_REC + 2 + e]);
    s_idx[j] = id;
    mine += id >= 0 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  __syncthreads();
  const int k = min(nt, mine);
  for (int j = lane; j < nc; j += 64) {
    const float vj = s_val[j];
    const int ij = s_idx[j];
    if (ij < 0) continue;
    int rank = 0;
    for (int q = 0; q < nc; ++q) {
      const float vq = s_val[q];
      const int iq = s_idx[q];
      rank += (iq >= 0 && (vq > vj || (vq == vj && iq < ij))) ? 1 : 0;
    }
    if (rank < k) {
      r[2 + rank] = __float_as_int((vj - mx) - logz);
      r[2 + LP_TOP + rank] = ij;
    }
  }
  for (int j = k + lane; j < LP_TOP; j += 64) {
    r[2 + j] = (int)0xFF800000u;
    r[2 + LP_TOP + j] = -1;
  }
  if (lane == 0) {
    r[0] = next_ids[row];
    r[1] = __float_as_int((raw - mx) - logz);
  }
}

__global__ __launch_bounds__(256) void logprob_pick_kernel(const float* __restrict__ logits, long ld, int V, int n,
                                                           const int* __restrict__ n_top,
                                                           const int* __restrict__ ctx_len,
                                                           const int* __restrict__ next_ids,
                                                           const int* __restrict__ stash, int hist_stride,
                                                           int* __restrict__ rec) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n || n_top[row] < 0 || (ctx_len != nullptr && ctx_len[row] <= 0)) return;
  int* r = rec + (size_t)row * LP_REC;
  const int id = next_ids[row];
  float raw = id >= 0 && id < V ? logits[(size_t)row * ld + id] : -INFINITY;
  if (stash != nullptr) {
    const int* st = stash + (size_t)row * (1 + 2 * hist_stride);
    const int nh = min(st[0], hist_stride);
    for (int j = 0; j < nh; ++j)
      if (st[1 + j] == id) {
        raw = __int_as_float(st[1 + hist_stride + j]);
        break;
      }
  }
  const float mx = __int_as_float(r[0]), logz = __int_as_float(r[1]);
  r[0] = id;
  r[1] = __float_as_int((raw - mx) - logz);
}

}  // namespace

// per-token log-probabilities of rows [0, n): records of LP_REC int32 words (see logprob_kernel). n_top[row] < 0
// skips the row; ctx_len / params / stash may be null (no padding rows / no penalised rows). stash: n rows of
// 1 + 2 * hist_stride int32 words.
extern "C" int nls_logprobs(const float* logits, long ld, int n, int V, const int* n_top, const int* ctx_len,
                            const void* params, const int* pos, const int* hist, int hist_stride, int* rec,
                            int* stash, void* stream) {
  if (n < 1 || V < 1 || V > 64 * MAXT || ld < V) return -1;
  if (stash != nullptr && (hist_stride < 1 || hist_stride > NT || (params != nullptr && (!pos || !hist)))) return -1;
  if (stash == nullptr && params != nullptr) return -1;
  hipLaunchKernelGGL(logprob_kernel<false>, dim3(n), dim3(NT), 0, (hipStream_t)stream, logits, ld, V, n_top, ctx_len,
                     (const SampleParams*)params, pos, hist, hist_stride, rec, stash, 0, (const int*)nullptr);
  return (int)hipGetLastError();
}

// tensor parallelism: the shard partials of rows [0, n) of one rank's logits (columns [0, valid) real, valid may be
// 0: an empty tail shard still writes its empty partials) into part [n, LP_REC]; see logprob_kernel<true>
extern "C" int nls_logprobs_shard(const float* logits, long ld, int n, int valid, int vocab_lo, const int* n_top,
                                  const int* ctx_len, const int* next_ids, int* part, void* stream) {
  if (n < 1 || valid < 0 || valid > 64 * MAXT || ld < valid || vocab_lo < 0) return -1;
  if (!logits || !n_top || !next_ids || !part) return -1;
  hipLaunchKernelGGL(logprob_kernel<true>, dim3(n), dim3(NT), 0, (hipStream_t)stream, logits, ld, valid, n_top,
                     ctx_len, (const SampleParams*)nullptr, (const int*)nullptr, (const int*)nullptr, 0, part,
                     (int*)nullptr, vocab_lo, next_ids);
  return (int)hipGetLastError();
}

// the gathered partials parts [n, world * LP_REC] -> the records rec [n, LP_REC]; see logprob_merge_kernel
extern "C" int nls_logprobs_merge(const int* parts, int n, int world, const int* n_top, const int* ctx_len,
                                  const int* next_ids, int* rec, void* stream) {
  if (n < 1 || world < 1 || world > LP_MERGE_RANKS) return -1;
  if (!parts || !n_top || !next_ids || !rec) return -1;
  hipLaunchKernelGGL(logprob_merge_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, parts, world, n_top, ctx_len,
                     next_ids, rec);
  return (int)hipGetLastError();
}

// after the sampler: the chosen token (next_ids[row]) and its logprob into record words 0 / 1
extern "C" int nls_logprobs_pick(const float* logits, long ld, int n, int V, const int* n_top, const int* ctx_len,
                                 const int* next_ids, const int* stash, int hist_stride, int* rec, void* stream) {
  if (n < 1 || V < 1 || V > 64 * MAXT || ld < V) return -1;
  if (stash != nullptr && (hist_stride < 1 || hist_stride > NT)) return -1;
  hipLaunchKernelGGL(logprob_pick_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, ld, V, n,
                     n_top, ctx_len, next_ids, stash, hist_stride, rec);
  return (int)hipGetLastError();
}

extern "C" int nls_logprobs_rec_words() { return LP_REC; }

// per row r < n: the C largest of logits[r][0, valid) in vocabulary order -> out[0][r][:] (f32 bits), out[1][r][:]
// (vocab_lo + index); plane = n * C (the offset of the id plane)
extern "C" int nls_topc(const float* logits, long ld, int n, int valid, int C, int vocab_lo, int* out, void* stream) {
  if (n < 1 || C < 1 || C > (1 << 16)) return -1;
  hipLaunchKernelGGL(topc_kernel, dim3(n), dim3(TCT), 0, (hipStream_t)stream, logits, ld, valid, C, vocab_lo, out,
                     (long)n * C);
  return (int)hipGetLastError();
}

extern "C" int nls_sample_decode_cand(void* cand, long ld, int n, int M, const int* ids, long ldi, const void* params,
                                      const void* seeds, const int* pos, const int* ctx_len, int* hist, int hist_stride,
                                      int* next_ids, void* stream) {
  if (n < 1 || M < 1 || M > MAXC || hist_stride < 1 || hist_stride > NT) return -1;
  hipLaunchKernelGGL(sample_decode_cand_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, (float*)cand, ld, M, ids,
                     ldi, (const SampleParams*)params, (const unsigned long long*)seeds, pos, ctx_len, hist,
                     hist_stride, next_ids);
  return (int)hipGetLastError();
}

// bias_ids / bias_val: the rows' logit_bias tables (bias_stride entries per row, SampleParams.n_bias of them used), or
// both null: no row is biased, whatever its n_bias says (the kernels then never look at it)
// mask / mask_rows: the allowed-token table (n_masks rows of mask_stride words) and each logits row's table row (-1:
// none), or both null: no row is masked
static int launch_sample(void* logits, long ld, int n, int V, const void* params, const int* hist, int hist_stride,
                         const int* bias_ids, const float* bias_val, int bias_stride, const unsigned* mask,
                         int mask_stride, const int* mask_rows, int n_masks, int* out, void* stream) {
  if (n < 1 || V < 1 || V > 64 * MAXT) return -1;
  hipLaunchKernelGGL(sample_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, (float*)logits, ld, V,
                     (const SampleParams*)params, hist, hist_stride, bias_ids, bias_val, bias_stride, mask,
                     mask_stride, mask_rows, n_masks, out);
  return (int)hipGetLastError();
}

extern "C" int nls_sample(void* logits, long ld, int n, int V, const void* params, const int* hist, int hist_stride,
                          int* out, void* stream) {
  return launch_sample(logits, ld, n, V, params, hist, hist_stride, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, out,
                       stream);
}

// nls_sample with logit_bias tables. The rows' n_bias live in device memory, so the entry cannot tell a biased row
// from here: it refuses null tables outright (-1, nothing launched) instead of sampling such a row without its bias.
extern "C" int nls_sample_bias(void* logits, long ld, int n, int V, const void* params, const int* hist,
                               int hist_stride, const int* bias_ids, const float* bias_val, int bias_stride, int* out,
                               void* stream) {
  if (!bias_ids || !bias_val || bias_stride < 1 || bias_stride > NT) return -1;
  return launch_sample(logits, ld, n, V, params, hist, hist_stride, bias_ids, bias_val, bias_stride, nullptr, 0,
                       nullptr, 0, out, stream);
}

// nls_sample_bias with an allowed-token mask stage in front (sample_one_biased): `mask` uint32 [n_masks, mask_stride],
// `mask_rows` int32 [n]: the table row of logits row r, or -1. The bias tables may both be null (no row has entries);
// one of them alone, a null mask under non-null mask_rows (or the reverse), mask_stride < ceil(V/32) or n_masks < 1:
// -1, nothing launched. Masked-out logits are left -inf.
extern "C" int nls_sample_mask(void* logits, long ld, int n, int V, const void* params, const int* hist,
                               int hist_stride, const int* bias_ids, const float* bias_val, int bias_stride,
                               const unsigned* mask, int mask_stride, const int* mask_rows, int n_masks, int* out,
                               void* stream) {
  if ((bias_ids == nullptr) != (bias_val == nullptr)) return -1;
  if (bias_ids && (bias_stride < 1 || bias_stride > NT)) return -1;
  if (!mask || !mask_rows || V < 1 || mask_stride < (V + 31) / 32 || n_masks < 1) return -1;
  return launch_sample(logits, ld, n, V, params, hist, hist_stride, bias_ids, bias_val, bias_ids ? bias_stride : 0,
                       mask, mask_stride, mask_rows, n_masks, out, stream);
}

extern "C" int nls_sample_params_size() { return (int)sizeof(SampleParams); }

static int launch_sample_decode(void* logits, long ld, int n, int V, const void* params, const void* seeds,
                                const int* pos, const int* ctx_len, int* hist, int hist_stride, const int* bias_ids,
                                const float* bias_val, int bias_stride, int* next_ids, void* stream) {
  if (n < 1 || V < 1 || V > 64 * MAXT || hist_stride < 1 || hist_stride > NT) return -1;
  hipLaunchKernelGGL(sample_decode_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, (float*)logits, ld, V,
                     (const SampleParams*)params, (const unsigned long long*)seeds, pos, ctx_len, hist, hist_stride,
                     bias_ids, bias_val, bias_stride, next_ids);
  return (int)hipGetLastError();
}

extern "C" int nls_sample_decode(void* logits, long ld, int n, int V, const void* params, const void* seeds,
                                 const int* pos, const int* ctx_len, int* hist, int hist_stride, int* next_ids,
                                 void* stream) {
  return launch_sample_decode(logits, ld, n, V, params, seeds, pos, ctx_len, hist, hist_stride, nullptr, nullptr, 0,
                              next_ids, stream);
}

// nls_sample_decode with logit_bias tables (null tables: -1, as nls_sample_bias)
extern "C" int nls_sample_decode_bias(void* logits, long ld, int n, int V, const void* params, const void* seeds,
                                      const int* pos, const int* ctx_len, int* hist, int hist_stride,
                                      const int* bias_ids, const float* bias_val, int bias_stride, int* next_ids,
                                      void* stream) {
  if (!bias_ids || !bias_val || bias_stride < 1 || bias_stride > NT) return -1;
  return launch_sample_decode(logits, ld, n, V, params, seeds, pos, ctx_len, hist, hist_stride, bias_ids, bias_val,
                              bias_stride, next_ids, stream);
}
