// What every GEMV / GEMM kernel of the dispatcher (qgemv.hip) is launched with, gfx950: the epilogue kinds, the
// segment list and the argument block, the kernel type-sets and their one dispatch helper, and the small device
// helpers that the shared block code (gemm_block.h) and paths A / B (qgemv_impl.h) both need. No kernel lives here.
#pragma once
#include <utility>
#include "common.h"

namespace nls_gemv {

// EPI_SLABS: split-K partial slabs only (the caller fuses the reduce, e.g. with RMSNorm);
// EPI_ARGMAX: fused arg-max keys only, no logits stored (greedy decode)
// EPI_ROPE: the Q|K|V projection's rows leave the tile rotated (adjacent-pair RoPE, + optional bias)
//           straight into q (bf16) and the paged K/V cache: no fp32 qkv round trip, no RoPE launch
enum Epi : int { EPI_F32 = 0, EPI_ACT = 1, EPI_ADD_F32 = 2, EPI_SWIGLU = 3, EPI_SLABS = 4, EPI_ARGMAX = 5,
                 EPI_ROPE = 6 };

struct Seg {
  const uint8_t* w;
  const int* xmap;     // optional: segment-local batch row -> x row (-1: none)
  const int* ymap;     // optional: segment-local batch row -> y row
  const int* mcount;   // optional: device count of valid rows (tiles skip when 0)
  int type, rows, K, tile_begin, ycol, tile_begin_col;
};
struct SegList { Seg s[8]; int nseg; int pad[3]; };

struct GemvArgs {
  const act_t* x; long ldx;
  void* y; long ldy;
  int M;               // rows of x / y (or max rows per segment when mapped)
  int epi;
  float alpha;
  int pad;            // path B split-K: total raw output columns
  unsigned long long* argmax;   // optional [M] packed (ordered value << 32 | ~idx)
  int m0, mtot;       // large-M split-K: first activation row of this block, total rows (slab index)
  // optional fused input RMSNorm (path A, staged rows): x = f16(rmsnorm(xf[m]) * nw), xf f32
  const float* xf; long ldxf;
  const float* nw; float eps;
  // EPI_ROPE operands (see rope_kv_kernel in ops.hip for the cache layout)
  const int* pos; const int* slot; const float* cs; const float* bias;
  __bf16* q_out; long ldq; __bf16* kc; __bf16* vc; int Hq, Hkv, D;
  // EPI_ADD_F32 + onw: after the residual update the LAST workgroup to finish (agent-scope ticket
  // `cnt`, zero between launches) normalises the updated rows: hout = f16(rmsnorm(y) * onw)
  act_t* hout; long ldh; const float* onw; int* cnt;
  // RMSNorm split across a producer / consumer pair (no norm launch, no full-row reduction pass):
  // an EPI_ADD_F32 path-A launch writes, per token m, its workgroup's share of sum(x^2) over the
  // rows it updated to ssq_out[m * ldss + blockIdx.x]; a consumer with xf / nw sums the nss_in
  // shares of ssq_in (fixed order: deterministic) to get the row's inverse RMS.
  float* ssq_out; const float* ssq_in; int ldss, nss_in;
  // device-selected segments (MoE decode, few tokens): workgroup i serves segment sel[i / sel_tiles] -
  // sel_base (out of range or a repeat of an earlier slot: exit), tile i % sel_tiles of it -- only the
  // routed experts' tiles are launched instead of every expert's (most of which would exit at once)
  const int* sel; int sel_tiles, sel_base, pad1;
  // MoE decode (with onw): after the residual update + FFN RMSNorm the last workgroup also computes the router
  // logits hout . wr[e] (wr: the router's f16 copy [E][D]) and the top-k route (route_one) -- the separate
  // norm + router + route launch folded away. counts [E] are zeroed here first.
  const act_t* wr; int E, topk, renorm, rcap;
  float* rlogits; float* topw; int* counts; int* xrows; int* yrows; int* rsel;
  // expert table (MoE with more than 8 local experts; paths A / B and the LDS-dequant GEMM): ONE segment carries the
  // type / rows / K all experts share and the row-map and count bases of expert 0; expert e's weights are tab[e],
  // its maps lie e * tab_cap ints on, its count e ints on, its sel_tiles tiles start at tile e * sel_tiles
  // (table_seg). The grid is tab_n * sel_tiles workgroups, or the selected slots' as without a table.
  const uint8_t* const* tab; int tab_n, tab_cap;
};

// ---- kernel type-sets: the weight formats one kernel instantiation holds. Splitting the format switch keeps the
// register budget of the quantised kernels small (a switch case's VGPR demand is paid by every case). A launch runs
// on the lowest-numbered set that holds every segment's type (type_set, qgemv.hip; ops.kernel_set in Python):
//   0: the Q4_K_M mix; 1: the Q5_K / Q8_0 mixes; 2: plain floats (tiled); 3: Q5_1 as Q51; 4: the IQ4_NL / IQ4_XS mixes.
struct KSet { int n; int t[4]; };
constexpr int NKSET = 5;
constexpr KSet KSETS[NKSET] = {{2, {QT_Q4_K, QT_Q6_K}},
                               {3, {QT_Q5_K, QT_Q6_K, QT_Q8_0}},
                               {3, {QT_F16, QT_BF16, QT_F32}},
                               {3, {QT_Q51, QT_Q6_K, QT_Q8_0}},
                               {4, {QT_IQ4, QT_Q5_K, QT_Q6_K, QT_Q8_0}}};

template <int... Ts> struct TypeList {};
template <int T> struct TypeC { static constexpr int v = T; };
template <int KSET, int... I>
constexpr auto kset_list(std::integer_sequence<int, I...>) { return TypeList<KSETS[KSET].t[I]...>{}; }
// the types of set KSET as a TypeList
template <int KSET> using KSetTypes = decltype(kset_list<KSET>(std::make_integer_sequence<int, KSETS[KSET].n>{}));

// f(TypeC<T>{}) for the T of the list that equals `type` (a segment's: scalar, so a uniform branch per candidate),
// nothing for a type outside the list (the plan lets none through)
template <int... Ts, class F>
DEVI void with_type(TypeList<Ts...>, int type, F f) {
  (void)((type == Ts ? (f(TypeC<Ts>{}), true) : false) || ...);
}

// segment of expert e of an expert table (GemvArgs::tab): uniform, scalar registers only
DEVI void table_seg(Seg& S, const GemvArgs& a, int e) {
  S.w = a.tab[e];
  if (S.xmap) S.xmap += (size_t)e * a.tab_cap;
  if (S.ymap) S.ymap += (size_t)e * a.tab_cap;
  if (S.mcount) S.mcount += e;
  S.tile_begin = e * a.sel_tiles;
}

// inv[m] = 1 / rms of rows m < M from producer partial sums of squares (see GemvArgs::ssq_in); one
// wave per row, lanes sum the shares in a fixed order; ends with a workgroup barrier
template <int NT>
DEVI void ssq_inv(const float* ssq, int ldss, int n, int M, int K, float eps, float* inv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int m = wave; m < M; m += NT / 64) {
    float s = 0.f;
    for (int j = lane; j < n; j += 64) s += ssq[(size_t)m * ldss + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) inv[m] = rsqrtf(s / (float)K + eps);
  }
  __syncthreads();
}

// Workgroup ticket: true in exactly one workgroup, the last of `n` to arrive, after which every
// global store of the others is visible to it (cdna_hip_programming.md Guideline 16: each wave drains
// its stores, barrier, one lane releases at agent scope then bumps the counter; the last arriver
// acquires). The last arriver re-arms the counter for the next launch. `flag`: one LDS int.
DEVI bool last_arriver(int* cnt, int n, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == n - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

// rows [0, M) of y (f32, width D, stride ldy) -> hout = f16(rmsnorm(row) * w); one workgroup of NT threads
template <int NT>
DEVI void rows_rmsnorm(const float* y, long ldy, int M, int D, const float* w, float eps, act_t* hout, long ldh,
                       float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  typedef act_t act4 __attribute__((ext_vector_type(4)));
  for (int m = 0; m < M; ++m) {
    const float* yr = y + (size_t)m * ldy;
    float ss = 0.f;
    for (int i = threadIdx.x * 4; i < D; i += NT * 4) {
      const float4 v = *reinterpret_cast<const float4*>(yr + i);
      ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) tot += red[i];
    __syncthreads();
    const float inv = rsqrtf(tot / (float)D + eps);
    for (int i = threadIdx.x * 4; i < D; i += NT * 4) {
      const float4 v = *reinterpret_cast<const float4*>(yr + i);
      const float4 g = *reinterpret_cast<const float4*>(w + i);
      *reinterpret_cast<act4*>(hout + (size_t)m * ldh + i) =
          act4{(act_t)(v.x * inv * g.x), (act_t)(v.y * inv * g.y), (act_t)(v.z * inv * g.z), (act_t)(v.w * inv * g.w)};
    }
  }
}

// EPI_ROPE of the dense GEMMs (modes 4/5/10, split-K 1): Q|K|V column `col` of activation row `b` (global
// row) with value v and the value p of its RoPE partner column col ^ 1 (adjacent pairs, as path A): add the
// bias, rotate q / k, store bf16 into q or the paged K / V cache (slot < 0: padding row, no cache write)
DEVI void rope_store1(const GemvArgs& a, int col, int b, float v, float p) {
  const bool odd = col & 1;
  float x0 = odd ? p : v, x1 = odd ? v : p;
  if (a.bias) {
    x0 += a.bias[col & ~1];
    x1 += a.bias[col | 1];
  }
  const int h = col / a.D, dd = col - h * a.D;
  const long s = a.slot[b];
  float y = odd ? x1 : x0;
  __bf16* d = nullptr;
  if (h < a.Hq + a.Hkv) {
    const float2 c = reinterpret_cast<const float2*>(a.cs + (size_t)a.pos[b] * a.D)[dd >> 1];
    y = odd ? x0 * c.y + x1 * c.x : x0 * c.x - x1 * c.y;
    if (h < a.Hq) d = a.q_out + (size_t)b * a.ldq + col;
    else if (s >= 0) d = a.kc + ((size_t)s * a.Hkv + (h - a.Hq)) * a.D + dd;
  } else if (s >= 0) {
    d = a.vc + ((size_t)s * a.Hkv + (h - a.Hq - a.Hkv)) * a.D + dd;
  }
  if (d) *d = (__bf16)y;
}

DEVI unsigned long long argmax_key(float v, int idx) {
  uint32_t u = __builtin_bit_cast(uint32_t, v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (0xFFFFFFFFu - (uint32_t)idx);
}

// x * sigmoid(x) with the hardware reciprocal (1 ulp; an IEEE divide is ~10 instructions per value in
// the GEMM epilogues). exp(-g) = inf for g << 0 gives g * 0 = -0.
DEVI float silu(float g) { return g * __builtin_amdgcn_rcpf(1.f + __expf(-g)); }

}  // namespace nls_gemv
