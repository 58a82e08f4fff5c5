// Per-head Q/K RMSNorm + RoPE + paged KV append (gfx950) for the families that normalise every Q and K head
// over head_dim before the rotation (Qwen3: blk.N.attn_q_norm / attn_k_norm, f32 [D], shared by the heads of a
// layer). A stand-alone launch after the Q|K|V projection; rope_kv_kernel (ops.hip) and the GEMV / GEMM RoPE
// epilogues of the other families are not involved.
//
// qkv row: [Hq*D | Hkv*D | Hkv*D] f32 (row stride ldqkv), or `ks` split-K partial slabs of it at stride `slab`
// floats, summed here in the fixed order 0..ks-1. cs: [max_pos][D/2][2] (cos, sin) f32. Per (token t, head h):
//   x  = sum_k slab_k[t][h*D .. h*D+D)                                          (fp32)
//   Q and K heads:  y = x * rsqrtf(sum(x^2) / D + eps) * w   (w = qw or kw), then rotated with pos[t]:
//                   adjacent pairs (2i, 2i+1) for neox = 0, pairs (i, i + D/2) for neox = 1
//   Q -> q_out[t] (bf16), K -> kc[slot[t]] (kv_st4), V (un-normalised, un-rotated) -> vc[slot[t]] (kv_st4)
//   slot[t] < 0: the row writes its Q and no K/V.
//
// Mapping (chosen over one wave per head with two values per lane so that every access is a vector one and
// K / V go through kv_st4, which takes 4 consecutive values): D/4 lanes per head, each lane owning columns
// 4l .. 4l+3 -- one 16-byte load per slab, one 8-byte bf16 (4-byte fp8) store. A head is half a wave for D = 128
// and a quarter for D = 64, so the sum of squares is log2(D/4) xor-shuffle steps that never leave the head's
// aligned lane group. neox = 0: a lane holds two whole pairs. neox = 1: the partner column i + D/2 sits in lane
// l ^ (D/8) of the same group -- one shuffle per value, no LDS. The norm weights and the (cos, sin) entries are
// loaded with the slabs, ahead of the reduction. 256 threads (4 waves) per workgroup = 1024 / D heads, grid
// (T, ceil((Hq + 2*Hkv) * D / 1024)): a batch-1 step of 32 + 2*8 heads of 128 spreads over 6 workgroups.
// All stores are plain vector stores; lanes past the last head (and K/V lanes of a slot -1 row) load nothing and
// store nothing but stay in the shuffles.
#include "common.h"

#ifndef NLS_SLAB_RUNTIME
#define NLS_SLAB_RUNTIME 0   // 1: always the runtime-ks kernels (A/B build tag, as in ops.hip)
#endif

namespace {

// KS > 0: the slab count as a constant (all slab loads issued before the first add); KS = 0: run-time loop
template <typename KV, int D, int KS>
__global__ __launch_bounds__(256) void qknorm_rope_kv_kernel(const float* __restrict__ qkv, long ldqkv, int ks,
                                                             long slab, const float* __restrict__ qw,
                                                             const float* __restrict__ kw, float eps,
                                                             const int* __restrict__ pos,
                                                             const int* __restrict__ slot,
                                                             const float* __restrict__ cs,
                                                             __bf16* __restrict__ q_out, long ldq,
                                                             KV* __restrict__ kc, KV* __restrict__ vc, int Hq,
                                                             int Hkv, int neox) {
  constexpr int LPH = D / 4;          // lanes per head
  constexpr int HPB = 256 / LPH;      // heads per workgroup
  constexpr int HALF = D / 2;
  const int t = blockIdx.x;
  const int l = threadIdx.x % LPH;
  const int h = blockIdx.y * HPB + threadIdx.x / LPH;
  const int col = 4 * l;
  const long s = slot[t];             // int32 slot index, widened
  const bool isq = h < Hq, isv = h >= Hq + Hkv;
  const bool live = h < Hq + 2 * Hkv && (isq || s >= 0);
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f), w = make_float4(1.f, 1.f, 1.f, 1.f);
  float4 c0 = make_float4(1.f, 0.f, 1.f, 0.f), c1 = c0;
  if (live) {
    const float* src = qkv + (size_t)t * ldqkv + (size_t)h * D + col;
    if constexpr (KS > 0) {
      float4 u[KS];
#pragma unroll
      for (int k = 0; k < KS; ++k) u[k] = *reinterpret_cast<const float4*>(src + (size_t)k * slab);
      x = u[0];
#pragma unroll
      for (int k = 1; k < KS; ++k) {
        x.x += u[k].x; x.y += u[k].y; x.z += u[k].z; x.w += u[k].w;
      }
    } else {
      x = *reinterpret_cast<const float4*>(src);
      for (int k = 1; k < ks; ++k) {
        const float4 u = *reinterpret_cast<const float4*>(src + (size_t)k * slab);
        x.x += u.x; x.y += u.y; x.z += u.z; x.w += u.w;
      }
    }
    if (!isv) {
      w = *reinterpret_cast<const float4*>((isq ? qw : kw) + col);
      const float* c = cs + (size_t)pos[t] * D;      // [D/2][2] (cos, sin)
      if (neox) {                                    // pairs (i, i + D/2), i = col % (D/2) .. + 3
        const int i = col & (HALF - 1);
        c0 = *reinterpret_cast<const float4*>(c + 2 * i);
        c1 = *reinterpret_cast<const float4*>(c + 2 * i + 4);
      } else {                                       // pairs col/2, col/2 + 1
        c0 = *reinterpret_cast<const float4*>(c + col);
      }
    }
  }
  float ss = x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
#pragma unroll
  for (int o = LPH / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float inv = rsqrtf(ss / (float)D + eps);
  const float4 y = make_float4(x.x * inv * w.x, x.y * inv * w.y, x.z * inv * w.z, x.w * inv * w.w);
  float4 r;
  if (neox) {       // uniform branch: every lane of the wave takes the shuffles
    const float4 p = make_float4(__shfl_xor(y.x, LPH / 2, 64), __shfl_xor(y.y, LPH / 2, 64),
                                 __shfl_xor(y.z, LPH / 2, 64), __shfl_xor(y.w, LPH / 2, 64));
    if (l < LPH / 2)   // first half: y0 = x0 * cos - x1 * sin
      r = make_float4(y.x * c0.x - p.x * c0.y, y.y * c0.z - p.y * c0.w, y.z * c1.x - p.z * c1.y,
                      y.w * c1.z - p.w * c1.w);
    else               // second half: y1 = x0 * sin + x1 * cos
      r = make_float4(p.x * c0.y + y.x * c0.x, p.y * c0.w + y.y * c0.z, p.z * c1.y + y.z * c1.x,
                      p.w * c1.w + y.w * c1.z);
  } else {
    r = make_float4(y.x * c0.x - y.y * c0.y, y.x * c0.y + y.y * c0.x, y.z * c0.z - y.w * c0.w,
                    y.z * c0.w + y.w * c0.z);
  }
  if (!live) return;
  if (isq) {
    typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<bf4*>(q_out + (size_t)t * ldq + (size_t)h * D + col) =
        bf4{(__bf16)r.x, (__bf16)r.y, (__bf16)r.z, (__bf16)r.w};
  } else if (!isv) {
    kv_st4(kc + ((size_t)s * Hkv + (h - Hq)) * D + col, r.x, r.y, r.z, r.w);
  } else {
    kv_st4(vc + ((size_t)s * Hkv + (h - Hq - Hkv)) * D + col, x.x, x.y, x.z, x.w);
  }
}

template <typename KV, int D>
int launch_d(int nk, dim3 grid, hipStream_t st, const float* qkv, long ldqkv, int ks, long slab, const float* qw,
             const float* kw, float eps, const int* pos, const int* slot, const float* cs, __bf16* q_out, long ldq,
             KV* kc, KV* vc, int Hq, int Hkv, int neox) {
  auto k = nk == 1 ? qknorm_rope_kv_kernel<KV, D, 1> : nk == 2 ? qknorm_rope_kv_kernel<KV, D, 2>
         : nk == 3 ? qknorm_rope_kv_kernel<KV, D, 3> : nk == 4 ? qknorm_rope_kv_kernel<KV, D, 4>
                                                               : qknorm_rope_kv_kernel<KV, D, 0>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, st, qkv, ldqkv, ks, slab, qw, kw, eps, pos, slot, cs, q_out, ldq, kc, vc,
                     Hq, Hkv, neox);
  return (int)hipGetLastError();
}

template <typename KV>
int launch(const float* qkv, long ldqkv, int ks, long slab, const float* qw, const float* kw, float eps,
           const int* pos, const int* slot, const float* cs, void* q_out, long ldq, void* kc, void* vc, int T, int Hq,
           int Hkv, int D, int neox, void* stream) {
  // 16-byte slab loads and 8-byte q stores: rows and slabs must keep the 4-float / 4-bf16 alignment
  if (ks < 1 || (D != 128 && D != 64) || T < 1 || Hq < 1 || Hkv < 1 || ldqkv % 4 || ldq % 4 ||
      (ks > 1 && slab % 4) || !qw || !kw || ((uintptr_t)qkv & 15) || ((uintptr_t)q_out & 7))
    return -1;
  const int nk = (NLS_SLAB_RUNTIME || ks > 4) ? 0 : ks;
  const int nh = Hq + 2 * Hkv, hpb = 1024 / D;
  const dim3 grid(T, (nh + hpb - 1) / hpb);
  hipStream_t st = (hipStream_t)stream;
  if (D == 128)
    return launch_d<KV, 128>(nk, grid, st, qkv, ldqkv, ks, slab, qw, kw, eps, pos, slot, cs, (__bf16*)q_out, ldq,
                             (KV*)kc, (KV*)vc, Hq, Hkv, neox);
  return launch_d<KV, 64>(nk, grid, st, qkv, ldqkv, ks, slab, qw, kw, eps, pos, slot, cs, (__bf16*)q_out, ldq,
                          (KV*)kc, (KV*)vc, Hq, Hkv, neox);
}

}  // namespace

extern "C" {

// qw / kw: f32 [D] per-head norm weights (this layer); the other arguments as nls_rope_kv (no bias)
int nls_qknorm_rope_kv(const float* qkv, long ldqkv, int ks, long slab, const float* qw, const float* kw, float eps,
                       const int* pos, const int* slot, const float* cs, void* q_out, long ldq, void* kc, void* vc,
                       int T, int Hq, int Hkv, int D, int neox, void* stream) {
  return launch<__bf16>(qkv, ldqkv, ks, slab, qw, kw, eps, pos, slot, cs, q_out, ldq, kc, vc, T, Hq, Hkv, D, neox,
                        stream);
}

// the same with an fp8 (OCP e4m3) K/V cache
int nls_qknorm_rope_kv8(const float* qkv, long ldqkv, int ks, long slab, const float* qw, const float* kw, float eps,
                        const int* pos, const int* slot, const float* cs, void* q_out, long ldq, void* kc, void* vc,
                        int T, int Hq, int Hkv, int D, int neox, void* stream) {
  return launch<uint8_t>(qkv, ldqkv, ks, slab, qw, kw, eps, pos, slot, cs, q_out, ldq, kc, vc, T, Hq, Hkv, D, neox,
                         stream);
}

}  // extern "C"
