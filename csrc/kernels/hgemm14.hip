// Dense f16 GEMM, "mode 14" of the qgemv dispatcher (gfx950): 128 activation rows x 96 weight rows per workgroup on
// mode 10's schedule (hgemm10.hip: counted vmcnt, raw barriers, two wave groups staggered by one barrier) with mode 4's
// operands, LDS image and summation order (hgemm.hip), so every output is bit-identical to mode 4's.
//
//   y[m, n] (epilogue) alpha * sum_k x[m, k] * W[n, k]      x f16 [M, K], W f16 [N, K] row-major
//
// Why 96 weight rows (profiles/hgemm14_qkv_o.txt): mode 4's K loop already fetches at 60 GB/s per CU, near what
// LDS-DMA delivers from L2, and a launch costs about 10 us on top of its K loop; the staggered schedule at 128 x 128
// ran level with mode 4. What mode 4 leaves on the table at Llama-3-8B's Q|K|V (6144 rows, M = 512) is a quarter of
// the chip: 48 tiles x 4 activation blocks = 192 workgroups for 256 CUs. 96-row tiles give 64 x 4 = 256 workgroups
// that each fetch 7/8 of the bytes per K step.
// Structure:
//   * 8 waves = 2 groups (wr: 48 weight rows each) x 4 (wc: 32 activation rows each); a wave owns 32 x 48 outputs,
//     2 x 3 accumulator tiles of v_mfma_f32_16x16x32_f16, activations as the A operand (mode 4's roles: a lane ends
//     with activation rows 4g + e of weight row r);
//   * K advances in "pairs": a pair is a 64-column step of both operands, two units x[128][64] (16 KiB) | W[96][64]
//     (12 KiB) in mode 4's image (128-B rows, 16-B chunk c of row r at c ^ (r & 7), permuted on the DMA source:
//     conflict-free ds_read_b128). Pair s is read in two phases of one 32-deep slice each, 2s (even) and 2s + 1 (odd):
//     [load section] 5 ds_read_b128, on odd phases the DMA issue of one pair (global_load_lds_dwordx4: 4 per lane in
//     group 0, 3 in group 1) -> barrier -> lgkmcnt(0), 6 MFMAs at raised priority -> on even phases a counted vmcnt
//     -> barrier. Group 1 runs ONE barrier behind group 0, so on every SIMD (one wave of each group) one wave's MFMAs
//     overlap the other wave's LDS reads and DMA issue;
//   * the pairs live in a ring of R = 4 slots of 32 KiB (128 KiB of LDS, one workgroup per CU; 5 slots measured the
//     same). With a staggered group a ds_read of phase p is complete for both groups only from phase p + 2, so the
//     slot of pair s is restaged in the odd phase of pair s + 1, with pair s + R; and a unit read in phase p must be
//     retired by every wave's wait of phase p - 2 (group 0 reads before group 1 has passed the wait of p - 1): the wait
//     of pair s's even phase retires pair s + 1 and leaves the R - 3 pairs issued after it in flight.
// K is summed ascending in 32-deep slices from the slice's first column into zeroed accumulators, alpha in the
// epilogue: per output the MFMA sequence of mode 4. Slices are mode 4's 64-column steps ((K / 64 * kslice) / ks);
// the dispatcher's plan takes launches whose slices are whole 128-column K-tiles. Grid: dense_grid_pos with the
// default map; workgroup prologue, epilogue (epi_rows) and launcher: gemm_block.h. Epilogues: f32 / residual add / f16 /
// RoPE + KV append / split-K slabs (no SwiGLU, no arg-max: plan refuses them).
#include "qgemm_dma.h"

namespace nls_hg14 {
using namespace nls_gemv;
using nls_dma::glds16;
using nls_dma::lds_addr;

constexpr int BM = 128, BN = 96;         // activation / weight rows per workgroup
constexpr int UB = 128 * 128;            // one unit: up to 128 rows x 64 k of one operand
constexpr int SLOT = 2 * UB;             // a pair: x unit, W unit
constexpr int R = 4;                     // ring slots (128 KiB of LDS, one workgroup per CU)
constexpr int MTW = 2, NTW = BN / 32;     // 16-row activation / weight tiles per wave

template <int N>
DEVI void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// ---- EPI_ROPE: rope_store1's arithmetic (qgemv_impl.h: bias, rotation, bf16 store into q or the paged K / V cache;
// the same expressions, so the same bits), with what depends on the lane's 3 weight rows alone (head, offset in the
// head, bias pair: one integer division per row, not per element) and on its 8 activation rows alone (slot, position)
// read once, and the 12 cos/sin pairs of an accumulator row-tile requested together ahead of their stores. Per
// element rope_store1 divides, reloads slot and position and waits for its table load: 8 us of the 52 us Q|K|V
// launch at M = 512 (profiles/hgemm14_qkv_o.txt).
DEVI void h14_rope(const f32x4 (&acc)[MTW][NTW], const Seg& S, int rbase, int mbase, const GemvArgs& a) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int M = a.M, D = a.D;
  const bool odd = r & 1;                  // (rbase, ycol and 16 j are even: the column's parity is the lane's)
  int col[NTW], hd[NTW], dd[NTW];
  float b0[NTW], b1[NTW];
  bool okr[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int row = rbase + 16 * j + r;
    okr[j] = row < S.rows;
    col[j] = S.ycol + row;
    hd[j] = col[j] / D;
    dd[j] = col[j] - hd[j] * D;
    b0[j] = a.bias && okr[j] ? a.bias[col[j] & ~1] : 0.f;
    b1[j] = a.bias && okr[j] ? a.bias[col[j] | 1] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    long slot[4];
    const float* csr[4];
    bool okb[4];
    float2 c[4][NTW];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = mbase + 16 * i + 4 * g + e;
      okb[e] = b < M;
      const int bg = a.m0 + (okb[e] ? b : 0);
      slot[e] = a.slot[bg];
      csr[e] = a.cs + (size_t)a.pos[bg] * D;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < NTW; ++j)
        c[e][j] = hd[j] < a.Hq + a.Hkv ? reinterpret_cast<const float2*>(csr[e])[dd[j] >> 1] : float2{1.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = a.m0 + mbase + 16 * i + 4 * g + e;
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        const float v = acc[i][j][e] * a.alpha;
        const float p = __shfl_xor(v, 1, 64);
        float x0 = odd ? p : v, x1 = odd ? v : p;
        if (a.bias) {
          x0 += b0[j];
          x1 += b1[j];
        }
        const int h = hd[j];
        const long s = slot[e];
        float y = odd ? x1 : x0;
        __bf16* d = nullptr;
        if (h < a.Hq + a.Hkv) {
          const float2 cc = c[e][j];
          y = odd ? x0 * cc.y + x1 * cc.x : x0 * cc.x - x1 * cc.y;
          if (h < a.Hq) d = a.q_out + (size_t)b * a.ldq + col[j];
          else if (s >= 0) d = a.kc + ((size_t)s * a.Hkv + (h - a.Hq)) * D + dd[j];
        } else if (s >= 0) {
          d = a.vc + ((size_t)s * a.Hkv + (h - a.Hq - a.Hkv)) * D + dd[j];
        }
        if (d && okb[e] && okr[j]) *d = (__bf16)y;
      }
    }
  }
}

DEVI void h14_tile(const Seg& S, int row0, int kslice, int ks, const GemvArgs& a, float* ws, uint8_t* lds) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int r = lane & 15, g = lane >> 4;
  const int nk64 = S.K >> 6;
  const int p0 = (nk64 * kslice) / ks;                             // slice in 64-column pairs
  const int np = (nk64 * (kslice + 1)) / ks - p0;
  const int M = a.M;

  // ---- DMA: a unit is up to 16 groups of 8 rows (1 KiB, one wave-instruction each). x: this wave issues groups
  // 2 * wave + i. W (12 groups): waves 0-3 groups 2 * wave + i, waves 4-7 group 8 + (wave & 3). Lane -> row
  // group_row + (lane >> 3), physical chunk lane & 7 <- logical chunk (lane & 7) ^ (lane >> 3)
  const int c = (lane & 7) ^ (lane >> 3);
  const bool wone = wr == 1;                                       // this wave issues one W instruction per unit
  const int wg0 = wone ? 8 + (wave & 3) : 2 * wave;
  const act_t* Wd = reinterpret_cast<const act_t*>(S.w);
  const act_t* xsrc[2];
  const act_t* wsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int xr = 8 * (2 * wave + i) + (lane >> 3);
    xsrc[i] = a.x + (size_t)min(xr, M - 1) * a.ldx + p0 * 64 + c * 8;        // rows >= M: clamped, never stored
    const int wrow = min(8 * (wg0 + i) + (lane >> 3), BN - 1);
    wsrc[i] = Wd + (size_t)min(row0 + wrow, S.rows - 1) * S.K + p0 * 64 + c * 8;
  }
  const uint32_t base = __builtin_amdgcn_readfirstlane(lds_addr(lds));
  const uint32_t xdst = base + (uint32_t)(2 * wave) * 1024u, wdst = base + UB + (uint32_t)wg0 * 1024u;
  // pair q -> ring slot `slot`; past the end: the last pair again (same bytes, into a slot nobody reads any more)
  auto dma = [&](int q, int slot) __attribute__((always_inline)) {
    const int koff = min(q, np - 1) * 64;
    const uint32_t so = (uint32_t)slot * SLOT;
    glds16(xsrc[0] + koff, xdst + so);
    glds16(xsrc[1] + koff, xdst + so + 1024);
    glds16(wsrc[0] + koff, wdst + so);
    if (!wone) glds16(wsrc[1] + koff, wdst + so + 1024);
  };
  // n pairs of this wave's DMA instructions stay in flight
  auto wait_pairs = [&](auto n) __attribute__((always_inline)) {
    constexpr int N = decltype(n)::value;
    if (wone) wait_vm<3 * N>();
    else wait_vm<4 * N>();
  };

  // ---- fragments of half t (32 columns) of the pair in `slot`, mode 4's addressing
  f16x8 A[MTW], B[NTW];
  const int xo = (wc * 32 + r) * 128, wo = UB + (wr * (BN / 2) + r) * 128;
  auto rd = [&](int slot, int t) __attribute__((always_inline)) {
    const uint8_t* sb = lds + slot * SLOT;
    const int co = ((4 * t + g) ^ (r & 7)) << 4;
#pragma unroll
    for (int i = 0; i < MTW; ++i) A[i] = *reinterpret_cast<const f16x8*>(sb + xo + i * 2048 + co);
#pragma unroll
    for (int j = 0; j < NTW; ++j) B[j] = *reinterpret_cast<const f16x8*>(sb + wo + j * 2048 + co);
  };
  f32x4 acc[MTW][NTW];
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mma = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MTW; ++i)
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc[i][j] = mfma16(A[i], B[j], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
  };
  auto bar = []() __attribute__((always_inline)) {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  if (np > 0) {
    // prologue: what the steady state would have issued before phase 0: pairs 0 .. R - 2; pair 0 landed, then one
    // barrier for all and group 1's stagger
#pragma unroll
    for (int q = 0; q < R - 1; ++q) dma(q, q);
    wait_pairs(std::integral_constant<int, R - 2>{});
    bar();
    if (wr == 1) bar();
    int slot = 0, prev = R - 1;                 // slots of pairs s and s - 1
    for (int s = 0; s < np; ++s) {
      // ---- even phase: columns 0-31 of pair s
      rd(slot, 0);
      bar();
      mma();
      wait_pairs(std::integral_constant<int, R - 3>{});   // pair s + 1 landed
      bar();
      // ---- odd phase: columns 32-63; pair s + R - 1 into the slot of pair s - 1 (last read two phases ago)
      rd(slot, 1);
      dma(s + R - 1, prev);
      bar();
      mma();
      bar();
      prev = slot;
      slot = slot + 1 == R ? 0 : slot + 1;
    }
    if (wr == 0) bar();                         // barrier counts even again
  }
  wait_vm<0>();                                 // drain the clamped tail DMAs (nothing reads LDS after the loop)

  // ---- epilogue (mode 4's lane mapping): lane holds weight rows rbase + 16j + r, activation rows mbase + 16i + 4g + e;
  // plain rows. RoPE (never with split-K: the plan) is this kernel's own, hoisted form
  const int rbase = row0 + wr * (BN / 2), mbase = wc * 32;
  if (ks <= 1 && a.epi == EPI_ROPE) {      // RoPE pair (row, row ^ 1) = lanes r, r ^ 1 (same activation row)
    h14_rope(acc, S, rbase, mbase, a);
    return;
  }
  epi_rows<0, MTW, NTW, 4, 16, 512, BM>(
      [&](int i, int j, int e) __attribute__((always_inline)) { return acc[i][j][e]; },
      [&](int j) __attribute__((always_inline)) { return rbase + 16 * j + r; },
      [&](int i, int e) __attribute__((always_inline)) { return mbase + 16 * i + 4 * g + e; }, S, kslice, ks, a, ws,
      lds, nullptr);
}

__global__ __launch_bounds__(512, 1) void hgemm14_kernel(SegList segs, GemvArgs a, int ks, float* ws, int ntiles,
                                                          int nmb) {
  extern __shared__ __attribute__((aligned(16))) uint8_t h14lds[];
  Block B;
  if (!block_prologue<BM, BN, false>(segs, a, dense_grid_pos(blockIdx.x, ks, nmb, 0), ntiles, B))
    return;
  h14_tile(B.S, B.row0, B.kslice, ks, a, ws, h14lds);
}

int launch_dense14(const SegList& sl, int ntiles, int ks, float* ws, const GemvArgs& a, hipStream_t st) {
  constexpr int LDS = R * SLOT;
  const int nmb = (a.M + BM - 1) / BM;
  return launch_lds<hgemm14_kernel>(dense_grid(ntiles, nmb, ks, 0), 512, LDS, st, sl, a, ks, ws, ntiles, nmb);
}

}  // namespace nls_hg14
