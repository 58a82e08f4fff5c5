// Attention at head size 256 (Gemma 2 / 3, Qwen3-Next) for gfx950: paged flash-decoding and causal flash-prefill
// over the cache layout of attention.hip / attn_prefill.hip, reached through their host entries (D == 256). The
// D = 64 / 128 kernels cannot be instantiated at 256 -- attn_prefill2 would need 64 + 128 + 32 + 32 registers of
// fragments alone in a 256-register budget, the 8-wave decode form 288 in 192 -- so the work is split differently:
//
// Decode (attn_decode_d256_kernel). The MFMA shapes of attn_decode_mfma_kernel: the G <= 16 query heads of a kv head
// are the 16 columns of v_mfma_f32_16x16x32_bf16; S^T = K Q^T with K rows straight from HBM (8 k-steps of 32 dims),
// O^T += V^T P^T with V^T read back transposed (ds_read_b64_tr_b16) from a 32-key tile in LDS and P^T straight from
// the S^T accumulators; 16 dim tiles of O^T per lane, the softmax state of head r in lane column r.
//   * 32 keys per group (the MFMA's k), so P^T needs no repacking; a 16-key group would halve the staging registers
//     but need the 16x16x16 shape for P.V and twice the softmax passes per key.
//   * Forms: ONE wave per workgroup (grids of >= 1K workgroups) and FOUR waves that take the 32-key groups of the
//     workgroup's range round-robin (smaller grids). Both run one wave per SIMD with up to 512 registers; there is
//     no 8-wave form: two waves per SIMD leave 256 registers, below the ~290 the loop holds.
//   * In flight per wave: the next group's K (16 x 16 B per lane, 16 KiB per wave at bf16) and V (the same) while
//     this group computes: qf 32 + O^T 64 + K 64 + next K 64 + next V 64 registers.
//   * V tile: 32 rows of 512 bytes per wave, one buffer (a wave's LDS operations run in order). 16-byte chunk ch of
//     row `row` lies at chunk ch ^ 2 u(row), u = (row & 3) | (((row >> 2) ^ (row >> 3)) & 1) << 2: a row write is
//     32 lanes x 16 B over 32 distinct chunks (any XOR keeps that conflict-free); a transposed read takes 32 B of
//     each of rows 4g .. 4g + 3 per 16-lane group g, and u sends the 8 rows of lanes 0-31 (rows 0-7), of lanes 32-63
//     (8-15) and of the lane groups {0, 2} (rows 0-3, 8-11) and {1, 3} to 8 distinct 32-byte bank groups of the 256.
//   Splits, the `cnt` ticket, the window and the sinks follow attention.hip (attn_split.h, attn_window.h).
//
// Prefill (attn_prefill_d256_kernel). attn_prefill2's pipeline (32x32x16 MFMAs, a lane owns one query row,
// in-register base-2 softmax with the rescale skipped when no row maximum grew, V^T by transposed reads, the next
// tile loaded into registers while this one computes and written to the other buffer after it, one barrier per
// tile) with FOUR waves at one wave per SIMD (512 registers: qf 64, O^T 128 accumulators, S^T 16, staging 32) and
// 32-key tiles: 2 buffers x (K | V) x 32 x 512 B = 64 KiB of LDS. A workgroup is 128 query rows of one (query
// block, kv head):
//   quad form (G % 4 == 0): wave w = query head 4 hq4 + w over the 32 tokens of one half of the 64-token block, so
//     four heads share every staged tile;
//   rows form (any other G <= 16): the block's token-major (token, head) rows rho = tok * G + g, 32 to a wave,
//     ceil(G / 2) workgroups per (block, kv head).
// Both are one kernel body; the forms differ only in which (token, head) a lane owns. Per 32-key tile a wave issues
// 16 + 16 MFMAs and about 150 vector instructions of softmax (16 scores per lane): ~5 VALU per MFMA, half the D = 128
// kernels' ratio, but with one wave per SIMD nothing but the wave's own MFMA queue overlaps them.
// Tile skips, m = -inf as "nothing yet" and the sink at the final 1 / l: as attn_prefill2.
//
// Built without the packed-fp32 VALU forms (build.py NO_PK_F32), as every unit added since that list began.
#include "attn_split.h"
#include "attn_window.h"

namespace {

constexpr float LOG2E_W = 1.4426950408889634f;
constexpr int D = 256;
constexpr int NCH = D / 8;             // 16-byte chunks per K / V row
constexpr int ROWB = D * 2;            // bytes per LDS row

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

DEVI s16x4 ld_tr(const uint8_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// ------------------------------------------------------------------------------------------------------- decode

// Merge of the na (<= 64) partials of (token t, kv head kh) by the last split to finish. One wave per head reduces
// the splits' (m, l) across its lanes into weights f_s = 2^(m_s - M) / L (LDS); then a head's 256 dims are exactly
// one wave of 4-dim items, so thread (wave w, lane) sums f_s * O_s for dims 4 lane .. + 3 of heads w, w + WAVES, ...
// over all the splits (independent 16-byte loads). smem: 16 * 64 floats.
template <int WAVES, bool SWA>
DEVI void merge_splits_d256(const float* __restrict__ part_o, const float* __restrict__ part_ml, int t, int kh, int G,
                            int Hq, int n_split, int na, act_t* __restrict__ out, long ldo, float* f,
                            const float* __restrict__ sinks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int h = wave; h < G; h += WAVES) {
    const size_t pb = ((size_t)t * Hq + kh * G + h) * n_split;
    const float ms = lane < na ? part_ml[2 * (pb + lane)] : -INFINITY;
    const float ls = lane < na ? part_ml[2 * (pb + lane) + 1] : 0.f;
    float M = ms;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    const float w = ms == -INFINITY ? 0.f : exp2f(ms - M);
    float L = w * ls;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) L += __shfl_xor(L, o, 64);
    if constexpr (SWA) L = sink_denom(M, L, sinks, kh * G + h);
    f[h * 64 + lane] = L > 0.f ? w / L : 0.f;
  }
  __syncthreads();
  for (int h = wave; h < G; h += WAVES) {
    const size_t pb = ((size_t)t * Hq + kh * G + h) * n_split;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s2 = 0; s2 < na; ++s2)
      acc += f[h * 64 + s2] * *reinterpret_cast<const f32x4*>(part_o + (pb + s2) * D + 4 * lane);
    *reinterpret_cast<h4*>(out + (size_t)t * ldo + (size_t)(kh * G + h) * D + 4 * lane) =
        h4{(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
  }
}

template <typename KV, int WAVES, bool SWA>
__global__ __launch_bounds__(64 * WAVES) void attn_decode_d256_kernel(
    const __bf16* __restrict__ q, long ldq, const KV* __restrict__ kc, const KV* __restrict__ vc,
    const int* __restrict__ block_tables, int bt_stride, const int* __restrict__ tok_seq,
    const int* __restrict__ ctx_len, int Hkv, int G, int bs, float scale, int chunk, int n_split,
    act_t* __restrict__ out, long ldo, float* __restrict__ part_o, float* __restrict__ part_ml,
    int* __restrict__ cnt, int window, const float* __restrict__ sinks) {
  static_assert(WAVES == 1 || WAVES == 4, "one wave per SIMD");
  constexpr int NKK = D / 32, NDT = D / 16, KG = 32;
  constexpr int NVL = KG / 2;          // V: 32 lanes per row, 2 rows per load, 16 loads per 32 keys
  typedef KVRaw<KV> R;
  // per wave one 32-key V tile (16 KiB); the space is reused for the cross-wave merge and the split merge
  constexpr int VB = WAVES * KG * ROWB, MB = WAVES > 1 ? (2 * WAVES * 16 + WAVES * 16 * D) * 4 : 0, CB = 16 * 64 * 4;
  constexpr int SMEM = VB > MB ? (VB > CB ? VB : CB) : (MB > CB ? MB : CB);
  __shared__ __attribute__((aligned(16))) uint8_t Vsm[SMEM];
  const int t = blockIdx.x, kh = blockIdx.y, split = blockIdx.z;
  const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
  const int wave = WAVES == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t* Vs = Vsm + wave * KG * ROWB;
  const int Hq = Hkv * G;
  const int ctx = ctx_len[t];
  // short contexts: at least one 32-key group per wave of the workgroup per split (>= 64 keys)
  const int lo = SWA ? window_lo(ctx, window) : 0, lo_al = lo / bs * bs;   // keys [lo, ctx), splits over [lo_al, ctx)
  chunk = split_chunk(chunk, ctx - lo_al, n_split, bs, KG * WAVES > 64 ? KG * WAVES : 64);
  const int start = lo_al + split * chunk;
  if (n_split > 1 && start >= ctx && ctx > 0) return;       // inactive split: the merge skips it
  const int end = min(ctx, start + chunk);
  // active splits: with ONE (short context) the split writes the output itself -- no partials, no ticket
  const int na = ctx > 0 ? active_splits(ctx, lo_al, chunk, n_split) : n_split;
  const bool direct = n_split == 1 || (na == 1 && cnt);
  const int* bt = block_tables + (size_t)tok_seq[t] * bt_stride;
  const float sl2 = scale * LOG2E_W;

  bf16x8 qf[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) {
    qf[kk] = bf16x8{};
    if (r < G) qf[kk] = *reinterpret_cast<const bf16x8*>(q + (size_t)t * ldq + (size_t)(kh * G + r) * D + kk * 32 + 8 * g);
  }
  f32x4 o[NDT];
#pragma unroll
  for (int c = 0; c < NDT; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  // Block-table entries from a register window (lane i holds entry b0 + 64 * win + i, refreshed once per 64
  // blocks), broadcast per 32-key group as wave-uniform values. A group touches at most NGB blocks (bs >= 16).
  constexpr int NGB = 4;
  const int b0 = start / bs;
  int btw = -1, btreg = 0;
  int gblk[NGB] = {0, 0, 0, 0};
  auto group_blocks = [&](int base) __attribute__((always_inline)) {
    const int bi0 = base / bs - b0;
    const int nbg = (min(base + KG, end) - 1) / bs - base / bs + 1;     // blocks this group touches
    const int win = bi0 >> 6;
    if (win != btw) {
      btw = win;
      const int e = b0 + win * 64 + lane;
      btreg = e * bs < end ? bt[e] : 0;
    }
#pragma unroll
    for (int i = 0; i < NGB; ++i) {
      const int bi = bi0 + i;
      if (i < nbg) gblk[i] = (bi >> 6) == win ? __builtin_amdgcn_readlane(btreg, bi & 63) : bt[b0 + bi];
    }
  };
  auto kv_row = [&](int p, int base) -> size_t {       // element offset of key p's row (keys past the end: the last)
    const int pc = min(p, end - 1);
    const int lb = pc / bs - base / bs;                // 0 .. NGB - 1
    const int blk = lb == 0 ? gblk[0] : (lb == 1 ? gblk[1] : (lb == 2 ? gblk[2] : gblk[3]));
    return ((size_t)((long)blk * bs + pc % bs) * Hkv + kh) * D;
  };
  auto voff = [](int row, int ch) {                    // swizzled byte offset of chunk ch of V row `row` (see top)
    return row * ROWB + 16 * (ch ^ (((row & 3) | ((((row >> 2) ^ (row >> 3)) & 1) << 2)) << 1));
  };
  // K of 32 keys: [n-tile][k-step]; V of 32 keys: row 2 i + lane / 32, chunk lane % 32
  typename R::raw kr[2][NKK];
  auto load = [&](int base, typename R::raw (&K)[2][NKK], typename R::raw (&V)[NVL]) __attribute__((always_inline)) {
    group_blocks(base);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const size_t o0 = kv_row(base + 16 * nt + r, base);
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) K[nt][kk] = R::ld(kc + o0 + kk * 32 + 8 * g);
    }
#pragma unroll
    for (int i = 0; i < NVL; ++i) V[i] = R::ld(vc + kv_row(base + 2 * i + (lane >> 5), base) + 8 * (lane & 31));
  };
  auto store_v = [&](typename R::raw (&V)[NVL]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NVL; ++i) *reinterpret_cast<u32x4*>(Vs + voff(2 * i + (lane >> 5), lane & 31)) = R::bf16(V[i]);
  };
  // wave w takes the 32-key groups w, w + WAVES, ... of the workgroup's range
  const int ngrp_all = end > start ? (end - start + KG - 1) / KG : 0;
  const int ngrp = ngrp_all > wave ? (ngrp_all - wave + WAVES - 1) / WAVES : 0;
  if (ngrp > 0) {
    typename R::raw v0[NVL];
    load(start + wave * KG, kr, v0);
    store_v(v0);
  }
  for (int j = 0; j < ngrp; ++j) {
    const int base = start + (j * WAVES + wave) * KG;
    typename R::raw kn[2][NKK], vn[NVL];
    const bool more = j + 1 < ngrp;
    if (more) load(base + WAVES * KG, kn, vn);
    // ---- S^T = K Q^T: s[nt][i] = S[head r][key base + 16 nt + 4 g + i]
    f32x4 s[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk)
        s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, R::bf16(kr[nt][kk])), qf[kk],
                                                        s[nt], 0, 0, 0);
    }
    // ---- online softmax of head r (base 2), keys past `end` (SWA: and below lo, in the first split) masked
    float mx = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kp = base + 16 * nt + 4 * g + i;
        const float v = kp < end && (!SWA || kp >= lo) ? s[nt][i] * sl2 : -INFINITY;
        s[nt][i] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float alpha = m == -INFINITY ? 0.f : exp2f(m - mn);
    float ps = 0.f;
    bf16x8 pb;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = s[nt][i] == -INFINITY ? 0.f : exp2f(s[nt][i] - mn);
        ps += pv;
        pb[4 * nt + i] = (__bf16)pv;
      }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
    // ---- O^T = O^T * alpha + V^T P^T over the 32 keys; V^T fragment of dim tile c: transposed reads of rows
    // {4g + qq} and {16 + 4g + qq}, columns 16c + 4pp .. + 3 (lane 4qq + pp of the group supplies the address)
    const int qq = r >> 2, pp = r & 3;
#pragma unroll
    for (int c = 0; c < NDT; ++c) {
      const int ch = 2 * c + (pp >> 1);
      const s16x4 lo4 = ld_tr(Vs + voff(4 * g + qq, ch) + 8 * (pp & 1));
      const s16x4 hi4 = ld_tr(Vs + voff(16 + 4 * g + qq, ch) + 8 * (pp & 1));
      const s16x8 a8 = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
      o[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a8), pb, o[c] * alpha, 0, 0, 0);
    }
    if (more) {
      store_v(vn);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) kr[nt][kk] = kn[nt][kk];
    }
  }

  // ---- output. Four waves: merge the waves' partial (m, l, O) of each head through LDS (the V tiles' space);
  // one wave: lane (g, r) holds dims 16c + 4g + i of head r in registers
  if constexpr (WAVES > 1) {
    float* mb = reinterpret_cast<float*>(Vsm);                      // [WAVES][16] m, [WAVES][16] l
    float* ob = mb + 2 * WAVES * 16;                                  // [WAVES][16 heads][D]
    __syncthreads();                                                  // every wave is done with its V tile
    if (g == 0) {
      mb[wave * 16 + r] = m;
      mb[(WAVES + wave) * 16 + r] = l;
    }
#pragma unroll
    for (int c = 0; c < NDT; ++c)
      *reinterpret_cast<f32x4*>(ob + ((size_t)wave * 16 + r) * D + 16 * c + 4 * g) = o[c];
    __syncthreads();
    for (int e = threadIdx.x; e < G * D; e += 64 * WAVES) {
      const int h = e / D, d = e - h * D;
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) M = fmaxf(M, mb[w * 16 + h]);
      float L = 0.f, O = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        const float mw = mb[w * 16 + h];
        const float f = mw == -INFINITY ? 0.f : exp2f(mw - M);
        L += mb[(WAVES + w) * 16 + h] * f;
        O += ob[((size_t)w * 16 + h) * D + d] * f;
      }
      const int qh2 = kh * G + h;
      if (direct) {
        if constexpr (SWA) L = sink_denom(M, L, sinks, qh2);
        out[(size_t)t * ldo + (size_t)qh2 * D + d] = (act_t)(L > 0.f ? O / L : 0.f);
      } else {
        const size_t pi = ((size_t)t * Hq + qh2) * n_split + split;
        part_o[pi * D + d] = O;
        if (d == 0) {
          part_ml[2 * pi] = M;
          part_ml[2 * pi + 1] = L;
        }
      }
    }
    if (direct) return;
  } else {
    const int qh = kh * G + r;
    if (direct) {
      if (r < G) {
        if constexpr (SWA) l = sink_denom(m, l, sinks, qh);
        const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
        for (int c = 0; c < NDT; ++c)
          *reinterpret_cast<h4*>(out + (size_t)t * ldo + (size_t)qh * D + 16 * c + 4 * g) =
              h4{(_Float16)(o[c][0] * inv), (_Float16)(o[c][1] * inv), (_Float16)(o[c][2] * inv),
                 (_Float16)(o[c][3] * inv)};
      }
      return;
    }
    if (r < G) {
      const size_t pi = ((size_t)t * Hq + qh) * n_split + split;
#pragma unroll
      for (int c = 0; c < NDT; ++c) *reinterpret_cast<f32x4*>(part_o + pi * D + 16 * c + 4 * g) = o[c];
      if (g == 0) {
        part_ml[2 * pi] = m;
        part_ml[2 * pi + 1] = l;
      }
    }
  }
  if (!cnt) return;
  // fused combine: the last active split of (token, kv head) to arrive merges them (the ticket of attention.hip)
  __shared__ int last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    int* cp = cnt + (size_t)t * Hkv + kh;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(cp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == na - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(cp, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  merge_splits_d256<WAVES, SWA>(part_o, part_ml, t, kh, G, Hq, n_split, na, out, ldo, reinterpret_cast<float*>(Vsm),
                                sinks);
}

// attn_combine at D = 256 (no counters): one thread per dim, with the short-context split size of the form that
// wrote the partials
template <bool SWA>
__global__ __launch_bounds__(D) void attn_combine_d256_kernel(const float* __restrict__ part_o,
                                                              const float* __restrict__ part_ml,
                                                              const int* __restrict__ ctx_len, int Hq, int n_split,
                                                              int chunk, int bs, act_t* __restrict__ out, long ldo,
                                                              int short_min, int window,
                                                              const float* __restrict__ sinks) {
  const int t = blockIdx.x, h = blockIdx.y, d = threadIdx.x;
  const int ctx = ctx_len[t];
  const int lo_al = SWA ? window_lo(ctx, window) / bs * bs : 0;
  chunk = split_chunk(chunk, ctx - lo_al, n_split, bs, short_min);
  const int na = active_splits(ctx, lo_al, chunk, n_split);   // (the others never wrote)
  const size_t pb = ((size_t)t * Hq + h) * n_split;
  float M = -INFINITY;
  for (int s = 0; s < na; ++s) M = fmaxf(M, part_ml[2 * (pb + s)]);
  float L = 0.f, O = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < na; ++s) {
      const float ms = part_ml[2 * (pb + s)];
      if (ms == -INFINITY) continue;
      const float f = exp2f(ms - M);
      L += part_ml[2 * (pb + s) + 1] * f;
      O += part_o[(pb + s) * D + d] * f;
    }
  }
  if constexpr (SWA) L = sink_denom(M, L, sinks, h);
  out[(size_t)t * ldo + (size_t)h * D + d] = (act_t)(L > 0.f ? O / L : 0.f);
}

// ------------------------------------------------------------------------------------------------------ prefill

template <typename KV, bool QUAD, bool SWA>
__global__ __launch_bounds__(256, 1) void attn_prefill_d256_kernel(
    const __bf16* __restrict__ q, long ldq, const KV* __restrict__ kc, const KV* __restrict__ vc,
    const int* __restrict__ block_tables, int bt_stride, const int* __restrict__ qblocks, int nqb, int Hkv, int G,
    int nwg, int bs_shift, float scale, act_t* __restrict__ out, long ldo, int window,
    const float* __restrict__ sinks) {
  constexpr int KT = 32;                 // keys per tile: one 32-key block of S^T
  constexpr int TILEB = KT * ROWB;       // one K (or V) tile: 16 KiB
  constexpr int NKS = D / 16;            // k-steps of S^T over the head dim
  constexpr int NDB = D / 32;            // 32-dim blocks of O^T
  constexpr int NLD = KT * NCH / 256;    // staging chunks per thread per K (and per V) tile
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * TILEB];   // [buf][K | V]

  const int bi = blockIdx.x;
  const int hk = bi % Hkv;
  const int rest = bi / Hkv;
  const int wg = nwg - 1 - rest % nwg;   // latest rows first
  const int qb = nqb - 1 - rest / nwg;   // heaviest (latest) query blocks first
  const int t0 = qblocks[qb * 4], ntok = qblocks[qb * 4 + 1], seq = qblocks[qb * 4 + 2], pos0 = qblocks[qb * 4 + 3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, tl = lane & 31;
  // ---- the lane's query row (tok, head), whether it exists, and the positions that bound the wave's and the
  // workgroup's tiles: wfirst / wlast = the wave's first row and last valid row, gfirst / glast = the workgroup's
  int tok, head, wfirst, wlast, gfirst, glast;
  bool wact, mine;
  if constexpr (QUAD) {                  // wg = (token half, quad of heads); wave = head of the quad
    const int nq4 = G / 4, tw0 = 32 * (wg / nq4);
    if (tw0 >= ntok) return;             // a short block has no second half
    tok = min(tw0 + tl, ntok - 1);
    head = hk * G + 4 * (wg % nq4) + wave;
    wact = true;
    mine = tw0 + tl < ntok;
    wfirst = gfirst = pos0 + tw0;
    wlast = glast = pos0 + min(tw0 + 31, ntok - 1);
  } else {                               // wg = 128 token-major rows; wave = 32 of them
    const int R = ntok * G, rw0 = 128 * wg, r0 = rw0 + 32 * wave;
    if (rw0 >= R) return;                // a short block leaves the later workgroups without rows
    const int rho = min(r0 + tl, R - 1); // (rows >= R repeat the last one, never stored)
    tok = rho / G;
    head = hk * G + rho - tok * G;
    wact = r0 < R;
    mine = r0 + tl < R;
    wfirst = pos0 + r0 / G;
    wlast = pos0 + min(r0 + 31, R - 1) / G;
    gfirst = pos0 + rw0 / G;
    glast = pos0 + (min(rw0 + 128, R) - 1) / G;
  }
  const int qpos = pos0 + tok;
  const int nkeys = pos0 + ntok;
  const int ntile = glast / KT + 1;      // up to the workgroup's last valid row
  const int* bt = block_tables + (size_t)seq * bt_stride;
  const int bsm = (1 << bs_shift) - 1;
  const float sl2 = scale * LOG2E_W;
  const bool win = SWA && window > 0;
  const int tfirst = win ? max(0, gfirst - window + 1) / KT : 0;   // the tile of the first row's first key
  const int wlo = win ? qpos - window : -1;                        // the row's last key below its window

  // ---- Q^T fragments of the lane's row: dims 16 ks + 8 h .. +7
  bf16x8 qf[NKS];
  {
    const __bf16* qrow = q + (size_t)(t0 + tok) * ldq + (size_t)head * D;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * h);
  }

  // ---- staging: thread tid moves chunk tid % 32 of keys tid / 32 + 8 i of K and of V. K rows are swizzled by
  // key & 15 (conflict-free ds_read_b128 down 16 rows); V rows by 4 (key & 3) ^ 2 ((key >> 2) & 1): a transposed
  // read takes 64 B of each of 4 consecutive rows per half wave, which land in 4 distinct 64-byte bank groups,
  // and rows key + 4 sit 32 B apart from rows key, should lane groups {0, 2} be served together
  auto kswz = [](int key, int ch) { return key * ROWB + ((ch ^ (key & 15)) << 4); };
  auto vswz = [](int key, int ch) { return key * ROWB + ((ch ^ ((key & 3) << 2) ^ (((key >> 2) & 1) << 1)) << 4); };
  typename KVRaw<KV>::raw kr[NLD], vr[NLD];
  auto load_tile = [&](int t) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int p = t * KT + (tid >> 5) + 8 * i;
      if (p < nkeys) {
        const size_t off = ((size_t)(bt[p >> bs_shift] << bs_shift | (p & bsm)) * Hkv + hk) * D + (tid & 31) * 8;
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
      const int key = (tid >> 5) + 8 * i, ch = tid & 31;
      *reinterpret_cast<u32x4*>(kb + kswz(key, ch)) = KVRaw<KV>::bf16(kr[i]);
      *reinterpret_cast<u32x4*>(vb + vswz(key, ch)) = KVRaw<KV>::bf16(vr[i]);
    }
  };

  f32x16 o[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) o[i] = f32x16{};
  float m = -INFINITY, l = 0.f;

  load_tile(tfirst);
  store_tile(tfirst & 1);
  __syncthreads();
  // V^T fragment read: lane (group of 16: vq = (l & 15) >> 2 row, vp = l & 3 column quad) supplies row kbase + vq
  // (and + 8), dims 32 db + 16 ((l >> 4) & 1) + 4 vp
  const int vq = (lane & 15) >> 2, vp = lane & 3, vhalf = (lane >> 4) & 1;
  for (int t = tfirst; t < ntile; ++t) {
    const int cur = t & 1;
    if (t + 1 < ntile) load_tile(t + 1);      // issue early: lands while this tile computes
    const int k0 = t * KT;
    if (wact && k0 <= wlast && (!win || k0 + KT - 1 > wfirst - window)) {
      const uint8_t* kb = lds + cur * 2 * TILEB;
      const uint8_t* vb = kb + TILEB;
      // ---- S^T = K Q^T: s[r] = S[row][key k0 + (r & 3) + 8 (r >> 2) + 4 h]
      f32x16 s = f32x16{};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(kb + kswz(tl, 2 * ks + h)), qf[ks],
                                                    s, 0, 0, 0);
      // ---- causal mask (only tiles that reach past the wave's first row; SWA: or below its last row's window)
      // + row max
      float mx = -INFINITY;
      if (k0 + KT - 1 > wfirst || (win && k0 <= wlast - window)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * h;
          const float v = key <= qpos && (!SWA || key > wlo) ? s[r] : -INFINITY;
          s[r] = v;
          mx = fmaxf(mx, v);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
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
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[8 * ks + j], sl2, nb));
          l += p;
          pb[j] = (__bf16)p;
        }
        // keys of this step in the fragment's k order: 16 ks + 4 h + {0..3, 8..11}
        const int k1 = 16 * ks + 4 * h + vq, k2 = k1 + 8;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const int ch = 4 * db + 2 * vhalf + (vp >> 1);
          const s16x4 lo4 = ld_tr(vb + vswz(k1, ch) + 8 * (vp & 1));
          const s16x4 hi4 = ld_tr(vb + vswz(k2, ch) + 8 * (vp & 1));
          const s16x8 a8 = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a8), pb, o[db], 0, 0, 0);
        }
      }
    }
    if (t + 1 < ntile) store_tile(cur ^ 1);   // write late: the other buffer was last read in tile t - 1
    __syncthreads();
  }
  // ---- normalise and scatter the lane's row: O[row][32 db + 8 g + 4 h + 0..3] in o[db][4 g .. 4 g + 3]
  l += __shfl_xor(l, 32, 64);
  if (wact && mine) {
    if constexpr (SWA) l = sink_denom(m * sl2, l, sinks, head);
    const float inv = l > 0.f ? 1.f / l : 0.f;
    act_t* orow = out + (size_t)(t0 + tok) * ldo + (size_t)head * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<h4*>(orow + 32 * db + 8 * g + 4 * h) =
            h4{(act_t)(o[db][4 * g] * inv), (act_t)(o[db][4 * g + 1] * inv), (act_t)(o[db][4 * g + 2] * inv),
               (act_t)(o[db][4 * g + 3] * inv)};
  }
}

}  // namespace

// The launchers behind attn_decode_impl / launch_combine (attention.hip), attn_prefill2_impl (attn_prefill.hip) and
// attn_prefill_rows_impl (attn_prefill_rows.hip) at D == 256; the callers have checked the shapes. No allocation,
// no sync (graph-capturable).
int attn_decode_d256_launch(int waves, const void* q, long ldq, const void* kc, const void* vc, const int* block_tables,
                            int bt_stride, const int* tok_seq, const int* ctx_len, int T, int Hkv, int G, int block_size,
                            float scale, int chunk, int n_split, void* out, long ldo, float* part_o, float* part_ml,
                            int* cnt, void* stream, bool kv8, int window, const float* sinks) {
  if ((waves != 1 && waves != 4) || G < 1 || G > 16 || block_size < 16 || n_split < 1 || n_split > 64) return -1;
  const dim3 grid(T, Hkv, n_split);
  hipStream_t st = (hipStream_t)stream;
#define D256_DEC(KVT, W, SW)                                                                                      \
  hipLaunchKernelGGL((attn_decode_d256_kernel<KVT, W, SW>), grid, dim3(64 * W), 0, st, (const __bf16*)q, ldq,       \
                     (const KVT*)kc, (const KVT*)vc, block_tables, bt_stride, tok_seq, ctx_len, Hkv, G, block_size, \
                     scale, chunk, n_split, (act_t*)out, ldo, part_o, part_ml, cnt, window, sinks)
#define D256_DEC_W(KVT, SW) \
  if (waves == 1) D256_DEC(KVT, 1, SW); else D256_DEC(KVT, 4, SW)
  const bool swa = window > 0 || sinks;
  if (kv8) {
    if (swa) { D256_DEC_W(uint8_t, true); } else { D256_DEC_W(uint8_t, false); }
  } else {
    if (swa) { D256_DEC_W(__bf16, true); } else { D256_DEC_W(__bf16, false); }
  }
#undef D256_DEC_W
#undef D256_DEC
  return (int)hipGetLastError();
}

void attn_combine_d256_launch(bool swa, int T, int Hq, void* stream, const float* part_o, const float* part_ml,
                              const int* ctx_len, int n_split, int chunk, int bs, void* out, long ldo, int short_min,
                              int window, const float* sinks) {
#define D256_COMB(SW)                                                                                             \
  hipLaunchKernelGGL((attn_combine_d256_kernel<SW>), dim3(T, Hq), dim3(D), 0, (hipStream_t)stream, part_o, part_ml, \
                     ctx_len, Hq, n_split, chunk, bs, (act_t*)out, ldo, short_min, window, sinks)
  if (swa) D256_COMB(true); else D256_COMB(false);
#undef D256_COMB
}

int attn_prefill_d256_launch(bool quad, bool kv8, const void* q, long ldq, const void* kc, const void* vc,
                             const int* block_tables, int bt_stride, const int* qblocks, int nqb, int Hkv, int G,
                             int block_size, float scale, void* out, long ldo, void* stream, int window,
                             const float* sinks) {
  if (Hkv < 1 || G < 1 || (quad ? G % 4 != 0 : G > 16) || nqb < 1 || block_size < 1 ||
      (block_size & (block_size - 1)) || window < 0)
    return -1;
  // workgroups of 128 rows per (query block, kv head): 2 token halves x G / 4 quads, or ceil(64 G / 128)
  const int nwg = quad ? 2 * (G / 4) : (G + 1) / 2;
  const int bs_shift = __builtin_ctz(block_size);
  const dim3 grid(nqb * Hkv * nwg);
  hipStream_t st = (hipStream_t)stream;
#define D256_PRE(KVT, QD, SW)                                                                                     \
  hipLaunchKernelGGL((attn_prefill_d256_kernel<KVT, QD, SW>), grid, dim3(256), 0, st, (const __bf16*)q, ldq,        \
                     (const KVT*)kc, (const KVT*)vc, block_tables, bt_stride, qblocks, nqb, Hkv, G, nwg, bs_shift,  \
                     scale, (act_t*)out, ldo, window, sinks)
#define D256_PRE_Q(KVT, SW) \
  if (quad) D256_PRE(KVT, true, SW); else D256_PRE(KVT, false, SW)
  const bool swa = window > 0 || sinks;
  if (kv8) {
    if (swa) { D256_PRE_Q(uint8_t, true); } else { D256_PRE_Q(uint8_t, false); }
  } else {
    if (swa) { D256_PRE_Q(__bf16, true); } else { D256_PRE_Q(__bf16, false); }
  }
#undef D256_PRE_Q
#undef D256_PRE
  return (int)hipGetLastError();
}
