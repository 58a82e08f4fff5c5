// Dispatcher of the quantised GEMV / GEMM (kernels: qgemv_impl.h, instantiated per type-set in
// qgemv_k{0,1,2,3,4}.hip; arguments and type-sets: gemv_args.h). One launch entry, nls_qgemv, in two steps: `plan` decides from the arguments alone --
// no HIP call, no device pointer dereferenced -- whether this library runs the launch (-1: it does not, nothing is
// launched) and what the launch looks like (NlsPlan, SegList, GemvArgs); `run` launches a plan and answers 0 or
// a hipError_t, never -1. nls_qgemv_plan exports the first step alone.
#include "qgemv_impl.h"
#include "qgemm_impl.h"
#include "qgemm_dma.h"

using namespace nls_gemv;

namespace nls_hgemm {
int launch_dense(int wm, int bn, int waves, int nst, const SegList& sl, int ntiles, int ks, float* ws,
                 const GemvArgs& a, hipStream_t st);
}
namespace nls_hg10 {
int launch_dense10(int bn, const SegList& sl, int ntiles, int ks, float* ws, const GemvArgs& a, hipStream_t st);
}
namespace nls_hg14 {
int launch_dense14(const SegList& sl, int ntiles, int ks, float* ws, const GemvArgs& a, hipStream_t st);
}
namespace nls_q9 {
int launch_q9(int kset, int waves, int rt, const SegList& sl, int ntiles, int ks, float* ws, const GemvArgs& a,
              hipStream_t st, int bm);
}


extern "C" {

// Host-side segment descriptor (plain C layout for ctypes).
struct NlsSeg {
  const void* w;
  const int* xmap;
  const int* ymap;
  const int* mcount;
  int type, rows, K, ycol;
};

// Optional fused operands of a launch (plain C layout for ctypes; every pointer may be null).
struct NlsFuse {
  const float* xf; long ldxf; const float* nw; float eps;                    // input RMSNorm (paths A / B, staged)
  const int* pos; const int* slot; const float* cs; const float* bias;      // EPI_ROPE
  void* q_out; long ldq; void* kc; void* vc; int Hq, Hkv, D, pad0;
  void* hout; long ldh; const float* onw; int* cnt;                          // residual add + RMSNorm
  float* ssq_out; const float* ssq_in; int ldss, nss_in;                     // split RMSNorm (GemvArgs)
  const int* sel; int sel_slots, sel_base, pad1;                             // device-selected segments
  const void* wr; int E, topk, renorm, rcap;                                 // MoE route after the norm (onw)
  float* rlogits; float* topw; int* counts; int* xrows; int* yrows; int* rsel;
  const void* tab; int tab_n, tab_cap;                                       // expert table (GemvArgs::tab)
};

// What `plan` decided about an accepted launch (plain C layout for ctypes).
struct NlsPlan {
  int kset;            // kernel type-set that covers every segment
  int tile_rows;       // weight rows per workgroup tile
  int tiles;           // the grid's tile count (after tab_n / sel_slots)
  int cols;            // output rows over all segments
  int slab_width;      // floats per row of a split-K slab
  int mapped_splitk;   // slabs indexed by the y row, one shared output segment
  int reduce;          // a splitk_reduce_kernel follows the launch
  int pad;
  long ws_floats;      // floats the launch writes into `ws` (0 without split-K)
};

}  // extern "C"

namespace {

inline bool mapped(const NlsSeg& s) { return s.xmap || s.ymap || s.mcount; }

// Input RMSNorm fused into the activation staging (xf, nw; ssq_in: the partial sums of squares a split-RMSNorm
// producer left): a few rows on path A, or on path B with the partial sums.
bool norm_in_ok(const NlsFuse& f, int M, int mode) {
  if (f.xf && (M > 16 || !f.nw || (mode != 0 && !(mode == 1 && f.ssq_in)))) return false;
  if (f.ssq_in && (!f.xf || f.nss_in < 1 || f.nss_in > f.ldss)) return false;
  return true;
}

// Producer of a split RMSNorm (ssq_out): path A residual add, whole tiles of tokens.
bool norm_producer_ok(const NlsFuse& f, const NlsSeg* segs, int nseg, int M, int epi, const void* argmax, int waves,
                      int rt, int mode) {
  if (!f.ssq_out) return true;
  const int ncols = ((M + 15) / 16) * 16;
  return !(mode != 0 || epi != EPI_ADD_F32 || nseg != 1 || mapped(segs[0]) || argmax || f.onw || M > 32 ||
           (waves * 64) % ncols || f.ldss < (segs[0].rows + 16 * rt - 1) / (16 * rt));
}

// Fused RoPE / KV append (EPI_ROPE): path A or a dense GEMM without split-K; plain rows, contiguous Q|K|V segments.
bool rope_ok(const NlsFuse& f, const NlsSeg* segs, int nseg, int epi, const void* argmax, int mode, int ks) {
  if (epi != EPI_ROPE) return true;
  const bool dense = mode == 4 || mode == 5 || mode == 10 || mode == 14;
  if (!(mode == 0 || (dense && ks <= 1)) || argmax || !f.pos || !f.slot || !f.cs || !f.q_out || !f.kc || !f.vc ||
      f.D < 2 || f.D % 2 || f.Hq < 1 || f.Hkv < 1)
    return false;
  int c = 0;
  for (int i = 0; i < nseg; ++i) {
    if (mapped(segs[i]) || segs[i].rows % 16 || segs[i].ycol != c) return false;
    c += segs[i].rows;
  }
  return c == (f.Hq + 2 * f.Hkv) * f.D;
}

// Residual add + output RMSNorm in the last workgroup (onw), and the MoE route after it (wr).
bool add_norm_ok(const NlsFuse& f, const NlsSeg* segs, int nseg, int M, int epi, const void* argmax, int mode) {
  if (f.onw && (mode != 0 || epi != EPI_ADD_F32 || nseg != 1 || segs[0].ycol || mapped(segs[0]) || !f.cnt ||
                !f.hout || segs[0].rows % 4 || argmax))
    return false;
  if (f.wr && (!f.onw || M > 4 || f.E < 1 || f.E > 64 || f.topk < 1 || f.topk > f.E || f.topk > 8 || !f.rlogits ||
               !f.topw || !f.counts || !f.xrows || !f.yrows || segs[0].rows % 4))
    return false;
  return true;
}

// Device-selected segments (sel): path A over routed experts only, identical segment shapes.
bool selected_ok(const NlsFuse& f, const NlsSeg* segs, int nseg, const void* argmax, int mode) {
  if (!f.sel) return true;
  if (mode != 0 || f.sel_slots < 1 || f.sel_slots > 256 || argmax) return false;
  for (int i = 1; i < nseg; ++i)
    if (segs[i].rows != segs[0].rows || segs[i].K != segs[0].K) return false;
  return true;
}

// Expert table (tab): one segment = the experts' shared shape + expert 0's maps and count; paths A / B and the
// LDS-dequant GEMM, no split-K, no fused operands.
bool table_ok(const NlsFuse& f, const NlsSeg* segs, int nseg, int epi, const void* argmax, int mode, int ks) {
  if (!f.tab) return true;
  return !(nseg != 1 || mode < 0 || mode > 2 || ks > 1 || f.tab_n < 1 || f.tab_cap < 1 || !segs[0].mcount ||
           argmax || f.xf || f.onw || f.ssq_out || epi == EPI_ROPE || epi == EPI_SLABS);
}

// The (waves, rt) instances, operand alignment and segment kinds each mode runs.
bool mode_shape_ok(const NlsFuse& f, const NlsSeg* segs, int nseg, long ldx, long ldy, int M, int epi, int waves,
                   int rt, int mode) {
  if (waves != 4 && waves != 8 && !(waves == 16 && mode >= 4) && !(waves == 7 && mode == 1 && rt == 1 && M == 1))
    return false;
  if (mode < 0 || (mode > 10 && mode != 14) || mode == 7 || mode == 8 || (mode == 6 && (waves != 8 || rt != 2)))
    return false;
  const bool unaligned_y = (epi == EPI_F32 || epi == EPI_ADD_F32 || epi == EPI_ACT) && ldy % 4;
  if (mode == 14) {            // 128 x 96 tiles, 8 waves; rt 2 as mode 4's: 128-row activation blocks
    if (waves != 8 || rt != 2 || f.xf || f.onw || ldx % 8 || unaligned_y) return false;
    if (epi == EPI_SWIGLU || epi == EPI_ARGMAX) return false;
    for (int i = 0; i < nseg; ++i)
      if (segs[i].type != QT_F16 || mapped(segs[i]) || segs[i].ycol % 4) return false;
  } else if (mode == 10) {     // rt 1: 256-row weight tiles, rt 2: 128-row
    if (waves != 8 || (rt != 1 && rt != 2) || f.xf || f.onw || ldx % 8 || unaligned_y) return false;
    // (rows % 4: epi_cols4 stores four output columns -- and four slab floats -- at a time behind one row check)
    for (int i = 0; i < nseg; ++i)
      if (segs[i].type != QT_F16 || mapped(segs[i]) || segs[i].ycol % 4 || segs[i].rows % 4) return false;
  } else if (mode == 9) {
    if (!((waves == 4 && rt == 2) || (waves == 8 && (rt == 2 || rt == 1))) || f.xf || f.onw || epi == EPI_ROPE ||
        ldx % 8 || unaligned_y)
      return false;
    for (int i = 0; i < nseg; ++i)
      if (mapped(segs[i]) || segs[i].ycol % 4 || segs[i].rows % 4) return false;   // (as mode 10)
  } else if (mode >= 4) {
    if ((waves != 8 && waves != 16) || (rt != 2 && rt != 4) || f.xf || f.onw || (epi == EPI_ROPE && mode == 6))
      return false;
    for (int i = 0; i < nseg; ++i)
      if (segs[i].type != QT_F16) return false;
  } else if (mode == 3) {
    if (waves != 4 || (rt != 4 && rt != 6 && rt != 8 && rt != 16)) return false;
    for (int i = 0; i < nseg; ++i)
      if (segs[i].type == QT_Q8_0) return false;   // raw Q8_0 tiles do not fit the DMA LDS budget
  } else if (mode == 2 ? (waves != 8 || (rt != 1 && rt != 2 && rt != 4)) : (rt != 1 && rt != 2)) {
    return false;
  }
  return !(M > 64 && mode == 0);   // large M: path B / LDS GEMM
}

// The kernel type-set that covers every segment: the lowest-numbered set of KSETS (gemv_args.h) that holds every
// segment's type, -1 if no single set does.
int type_set(const NlsSeg* segs, int nseg) {
  for (int k = 0; k < NKSET; ++k) {
    bool all = true;
    for (int i = 0; i < nseg && all; ++i) {
      bool held = false;
      for (int j = 0; j < KSETS[k].n; ++j) held |= KSETS[k].t[j] == segs[i].type;
      all = held;
    }
    if (all) return k;
  }
  return -1;
}

// Split-K reduction + epilogue. ws: [ks][M][ntot] fp32 (ntot = raw output rows over all segments)
struct RedSeg { int col0, rows, ycol, pad; };
struct RedList { RedSeg s[8]; int nseg, pad[3]; };

__global__ void splitk_reduce_kernel(const float* __restrict__ ws, int ks, int M, int ntot, RedList rl, GemvArgs a) {
  const int b = blockIdx.y;
  const bool swiglu = a.epi == EPI_SWIGLU;
  const int nout = swiglu ? ntot / 2 : ntot;
  unsigned long long best = 0ull;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < nout; j += gridDim.x * blockDim.x) {
    int col = swiglu ? (j >> 3) * 16 + (j & 7) : j;
    RedSeg S = rl.s[0];
    for (int i = 1; i < rl.nseg; ++i)
      if (col >= rl.s[i].col0) S = rl.s[i];
    float v = 0.f, u = 0.f;
    for (int k = 0; k < ks; ++k) {
      v += ws[((size_t)k * M + b) * ntot + col];
      if (swiglu) u += ws[((size_t)k * M + b) * ntot + col + 8];
    }
    v *= a.alpha;
    u *= a.alpha;
    const int row = col - S.col0;
    if (swiglu) {
      const int n = S.ycol + (row >> 4) * 8 + (row & 7);
      reinterpret_cast<act_t*>(a.y)[(size_t)b * a.ldy + n] = (act_t)(silu(v) * u);
      continue;
    }
    const size_t off = (size_t)b * a.ldy + S.ycol + row;
    if (a.epi == EPI_F32) reinterpret_cast<float*>(a.y)[off] = v;
    else if (a.epi == EPI_ADD_F32) reinterpret_cast<float*>(a.y)[off] += v;
    else if (a.epi == EPI_ACT) reinterpret_cast<act_t*>(a.y)[off] = (act_t)v;
    if (a.argmax) {
      const unsigned long long k = argmax_key(v, S.ycol + row);
      best = k > best ? k : best;
    }
  }
  if (a.argmax) {
    // one atomic per workgroup and row (a per-element atomicMax on the one key of a row serialises
    // ~128K updates for an lm_head: 27 us of a 2.2 ms batch-1 step)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(best, o, 64);
      best = ok > best ? ok : best;
    }
    __shared__ unsigned long long red[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < (int)(blockDim.x >> 6); ++w) best = red[w] > best ? red[w] : best;
      if (best) atomicMax(a.argmax + b, best);
    }
  }
}

inline int mtiles(int M) { return M > 64 ? 8 : (M + 15) / 16; }      // 16-row activation tiles per block (A / B)
inline int mblocks(int M) { return M > 64 ? (M + 127) / 128 : 1; }   // 128-row activation blocks (path B)

// mode 0: path A (waves split K, LDS reduce; mapped rows / MoE capable)
// mode 1: path B (waves split rows, LDS-staged activations, optional split-K `ks` with workspace
//         `ws` of ks*M*sum(rows) floats); grid maps and workgroup prologue from gemm_block.h.
// mode 2: large-M LDS-dequant GEMM (qgemm_impl.h; K-quant types only): 8 waves, `rt` = WM (4: 256-row
//         activation blocks, 2: 128-row), optional split-K as mode 1.
// mode 3: large-M LDS-DMA GEMM (qgemm_dma.h; Q4_K/Q5_K/Q6_K only): 4 waves, `rt` = activation
//         tiles per block (16: 256 rows, 8: 128 rows; 6 / 4: 96 / 64 rows at two workgroups per CU, the MoE
//         expert blocks), mapped rows, optional split-K as mode 1.
// mode 4: large-M dense f16 GEMM (hgemm.hip): every segment is type F16 with `w` = a ROW-MAJOR
//         [rows][K] f16 matrix (not the tiled layout); 8 waves, `rt` = WM (4: 256-row activation
//         blocks, 2: 128-row), optional split-K as mode 1.
// mode 5: mode 4 with 256-row weight tiles (twice the MFMA work per fetched activation byte).
// mode 6: mode 4 at 128-row activation blocks (rt 2) with 2-deep rings: two workgroups per CU.
// mode 10: dense f16 GEMM, 256 x 256 tiles, 4 phases per 64-deep K-tile with the two wave groups staggered
//         by one barrier (hgemm10.hip); weights as the MFMA A operand and mode 9's epilogues (epi_cols4,
//         gemm_block.h) plus RoPE, optional split-K.
// mode 14: dense f16 GEMM, 128 activation rows x 96 weight rows per workgroup on mode 10's staggered schedule with
//         mode 4's operands and summation order (hgemm14.hip; bit-identical to mode 4): 8 waves, rt 2, K slices of
//         whole 128-column K-tiles; f32 / add / f16 / RoPE epilogues and split-K, no SwiGLU, no arg-max. A third
//         more workgroups where 128-row weight tiles leave CUs idle (Llama-3-8B Q|K|V at M = 512: 256, not 192).
// (Modes 7, 8 and 11-13 are not in the build: 7 was the library GEMM, 8 a dense twin of mode 9 that mode 10
//  superseded; 11-13 -- mode 10 on raw K-quant tiles, mode 9 at 64-row blocks, stream-K -- lost every measured shape
//  in round 5; profiles/streamk_r05.txt, profiles/qgemm11_r05.txt. `plan` refuses them.)
// The large-M kernels (modes 2 - 14) share their grid maps, workgroup prologue, epilogues and launcher, path B the
// first two: gemm_block.h, over the argument block, kernel type-sets (KSETS) and type dispatch of gemv_args.h.
// mode 9: quantised GEMM on the raw tile-blocks (qgemm9.hip; Q4_K/Q5_K/Q6_K/Q8_0/Q51/IQ4): 256-row activation
//         blocks x 16*waves*rt weight rows ((waves, rt) = (4, 2) | (8, 2) | (8, 1)), the four-rows-per-lane
//         epilogues (epi_cols4, gemm_block.h), optional split-K.
// 0 and `p`, `sl`, `a` filled, or -1: these arguments are not a launch this library runs.
int plan(const NlsSeg* segs, int nseg, const void* x, long ldx, void* y, long ldy, int M, float alpha, int epi,
         void* argmax, int waves, int rt, int mode, int ks, const void* ws, long ws_floats, const NlsFuse& f,
         NlsPlan& p, SegList& sl, GemvArgs& a) {
  if (nseg < 1 || nseg > 8 || M < 1) return -1;
  if (!mode_shape_ok(f, segs, nseg, ldx, ldy, M, epi, waves, rt, mode) || !norm_in_ok(f, M, mode) ||
      !norm_producer_ok(f, segs, nseg, M, epi, argmax, waves, rt, mode) ||
      !rope_ok(f, segs, nseg, epi, argmax, mode, ks) || !add_norm_ok(f, segs, nseg, M, epi, argmax, mode) ||
      !selected_ok(f, segs, nseg, argmax, mode) || !table_ok(f, segs, nseg, epi, argmax, mode, ks))
    return -1;
  if (mode != 0 && ks > 1 && !ws) return -1;
  if (mode == 14 && argmax) return -1;
  if (epi == EPI_SLABS && (mode == 0 || ks < 2)) return -1;   // slabs exist only with split-K
  // mapped split-K (MoE down projection at many tokens): slabs indexed by the y row, one reduce
  bool mks = (mode >= 1 && mode <= 5) && ks > 1 && epi == EPI_F32 && !argmax;
  for (int i = 0; i < nseg && mks; ++i)
    mks = segs[i].ymap && segs[i].ycol == 0 && segs[i].rows == segs[0].rows;
  sl = SegList{};
  int tiles = 0, cols = 0;
  const int tile_rows = mode == 14 ? 96 : mode == 10 ? 256 / rt : mode == 9 ? 16 * waves * rt
                        : (mode == 5 ? 256 : (mode >= 2 ? 128 : (mode == 1 ? waves : 1) * rt * 16));
  for (int i = 0; i < nseg; ++i) {
    if (segs[i].K % 256 || segs[i].rows < 1) return -1;
    if (epi == EPI_SWIGLU && segs[i].rows % 16) return -1;
    for (int s = 1; mode == 14 && s < ks; ++s)
      if (((segs[i].K / 64) * s / ks) % 2) return -1;   // a slice boundary inside a 128-column K-tile
    // mapped rows (MoE): path A, or path B / the LDS-dequant / LDS-DMA / dense GEMMs (modes 1-5) without
    // arg-max; split-K only as "mapped split-K" (every segment an expert writing the same output
    // columns of its own y rows, f32 store)
    if (mapped(segs[i]) && mode != 0 &&
        (!(mode >= 1 && mode <= 5) || argmax || epi == EPI_SLABS || (ks > 1 && !mks)))
      return -1;
    sl.s[i] = Seg{(const uint8_t*)segs[i].w, segs[i].xmap, segs[i].ymap, segs[i].mcount, segs[i].type, segs[i].rows,
                  segs[i].K, /*tile_begin*/ tiles, segs[i].ycol, /*tile_begin_col*/ cols};
    tiles += (segs[i].rows + tile_rows - 1) / tile_rows;
    cols += segs[i].rows;
  }
  sl.nseg = nseg;
  if (f.tab) tiles *= f.tab_n;      // every expert's tiles, expert-major (table_seg)
  const int sel_tiles = (segs[0].rows + tile_rows - 1) / tile_rows;
  if (f.sel) tiles = f.sel_slots * sel_tiles;
  const int kset = type_set(segs, nseg);
  if (kset < 0) return -1;
  if (mode >= 2 && mode <= 3 && kset >= 2) return -1;   // tiled float / Q51 / IQ4 weights: paths A and B only
  if (mode == 9 && kset == 2) return -1;   // mode 9: quantised formats only
  const int nks = mode != 0 && ks > 1 ? ks : 1;
  // fused input norm needs the staged (MT = 1, unmapped, fitting) path; the 7-wave instance exists for the staged
  // batch-1 path only
  if (mode == 0 && f.xf && !staged_lds_a(sl, waves, rt, mtiles(M), M)) return -1;
  if (mode == 1 && (f.xf || waves == 7) && !staged_lds_b(sl, mtiles(M), M, nks, mblocks(M), f.xf)) return -1;
  p = NlsPlan{};
  p.kset = kset;
  p.tile_rows = tile_rows;
  p.tiles = tiles;
  p.cols = cols;
  p.slab_width = mks ? segs[0].rows : cols;
  p.mapped_splitk = mks;
  p.reduce = nks > 1 && epi != EPI_SLABS;
  p.ws_floats = nks > 1 ? (long)nks * M * p.slab_width : 0;
  if (ws_floats < p.ws_floats) return -1;   // the slabs would run past the workspace
  // (one line per group of GemvArgs, in its declaration's order; with xf the kernels read no x)
  a = GemvArgs{(const act_t*)(f.xf ? (const void*)f.xf : x), ldx, y, ldy, M, epi, alpha, /*pad*/ p.slab_width,
               (unsigned long long*)argmax, /*m0*/ 0, /*mtot*/ M,
               f.xf, f.ldxf, f.nw, f.eps,
               f.pos, f.slot, f.cs, f.bias, (__bf16*)f.q_out, f.ldq, (__bf16*)f.kc, (__bf16*)f.vc, f.Hq, f.Hkv, f.D,
               (act_t*)f.hout, f.ldh, f.onw, f.cnt,
               f.ssq_out, f.ssq_in, f.ldss, f.nss_in,
               f.sel, sel_tiles, f.sel_base, /*pad1*/ 0,
               (const act_t*)f.wr, f.E, f.topk, f.renorm, f.rcap,
               f.rlogits, f.topw, f.counts, f.xrows, f.yrows, f.rsel,
               (const uint8_t* const*)f.tab, f.tab_n, f.tab_cap};
  return 0;
}

// Launch a plan: the mode's kernel, then the split-K reduce where the plan has one. 0 or a hipError_t.
int run(const NlsPlan& p, const SegList& sl, const GemvArgs& a, int waves, int rt, int mode, int ks, float* ws,
        hipStream_t st) {
  const int M = a.M, mt = mtiles(M);
  auto launch = p.kset == 0 ? launch_k0
                            : p.kset == 1 ? launch_k1 : p.kset == 2 ? launch_k2 : p.kset == 3 ? launch_k3 : launch_k4;
  if (mode == 0) return launch(0, waves, rt, mt, sl, p.tiles, 1, nullptr, a, st, 1);
  if (ks < 1) ks = 1;
  int rc;
  if (mode == 14)
    rc = nls_hg14::launch_dense14(sl, p.tiles, ks, ws, a, st);
  else if (mode == 10)
    rc = nls_hg10::launch_dense10(256 / rt, sl, p.tiles, ks, ws, a, st);
  else if (mode == 9)
    rc = nls_q9::launch_q9(p.kset, waves, rt, sl, p.tiles, ks, ws, a, st, 256);
  else if (mode >= 4)
    rc = nls_hgemm::launch_dense(rt, mode == 5 ? 256 : 128, waves, mode == 6 ? 2 : 3, sl, p.tiles, ks, ws, a, st);
  else if (mode == 3)
    rc = (p.kset == 0 ? nls_dma::launch_dma_k0 : nls_dma::launch_dma_k1)(rt, sl, p.tiles, ks, ws, a, st);
  else if (mode == 2)
    rc = (p.kset == 0 ? nls_gemm::launch_lds_k0 : nls_gemm::launch_lds_k1)(rt, sl, p.tiles, ks, ws, a, st);
  else
    rc = launch(1, waves, rt, mt, sl, p.tiles, ks, ws, a, st, mblocks(M));
  if (rc || !p.reduce) return rc;
  RedList rl{};
  if (p.mapped_splitk) {   // slabs [ks][M y rows][rows]: one shared output segment
    rl.s[0] = RedSeg{0, p.slab_width, 0, 0};
    rl.nseg = 1;
  } else {
    for (int i = 0; i < sl.nseg; ++i) rl.s[i] = RedSeg{sl.s[i].tile_begin_col, sl.s[i].rows, sl.s[i].ycol, 0};
    rl.nseg = sl.nseg;
  }
  const int nout = a.epi == EPI_SWIGLU ? p.slab_width / 2 : p.slab_width;
  dim3 grid((nout + 255) / 256, M);
  hipLaunchKernelGGL(splitk_reduce_kernel, grid, dim3(256), 0, st, (const float*)ws, ks, M, p.slab_width, rl, a);
  return (int)hipGetLastError();
}

const NlsFuse kNoFuse{};

}  // namespace

extern "C" {

// The launch entry. `fz` may be null; with fz->xf the kernels read their activations from it and `x` is ignored.
// `ws_floats`: the size of `ws` in floats. Returns 0, a hipError_t, or -1 where `plan` refuses (nothing launched).
int nls_qgemv(const NlsSeg* segs, int nseg, const void* x, long ldx, void* y, long ldy, int M, float alpha, int epi,
              void* argmax, int waves, int rt, int mode, int ks, void* ws, long ws_floats, void* stream,
              const NlsFuse* fz) {
  NlsPlan p;
  SegList sl;
  GemvArgs a;
  if (plan(segs, nseg, x, ldx, y, ldy, M, alpha, epi, argmax, waves, rt, mode, ks, ws, ws_floats, fz ? *fz : kNoFuse,
           p, sl, a))
    return -1;
  return run(p, sl, a, waves, rt, mode, ks, (float*)ws, (hipStream_t)stream);
}

// `plan` alone: -1, or 0 with what the launch would be in `out`. Launches nothing, dereferences no device pointer.
int nls_qgemv_plan(const NlsSeg* segs, int nseg, const void* x, long ldx, void* y, long ldy, int M, float alpha,
                   int epi, void* argmax, int waves, int rt, int mode, int ks, void* ws, long ws_floats, void* stream,
                   const NlsFuse* fz, NlsPlan* out) {
  SegList sl;
  GemvArgs a;
  (void)stream;
  return plan(segs, nseg, x, ldx, y, ldy, M, alpha, epi, argmax, waves, rt, mode, ks, ws, ws_floats,
              fz ? *fz : kNoFuse, *out, sl, a);
}

int nls_fuse_size() { return (int)sizeof(NlsFuse); }
int nls_plan_size() { return (int)sizeof(NlsPlan); }

}  // extern "C"
