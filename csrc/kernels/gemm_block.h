// What the GEMM kernels share around their K loops (modes 2 qgemm_impl.h, 3 qgemm_dma.h, 4/5/6 hgemm.hip, 9 qgemm9.hip,
// 10 hgemm10.hip, 14 hgemm14.hip; of path B = mode 1, qgemv_impl.h, the grid maps and the prologue), gfx950: the grid
// maps, the workgroup prologue, the two epilogues (one per accumulator lane mapping) and the launcher. The K loops,
// LDS layouts and tile shapes stay with each kernel; the launch arguments, type-sets and small helpers used here are
// gemv_args.h's, the only include.
#pragma once
#include "gemv_args.h"

namespace nls_gemv {

// ---- grid: workgroup -> (weight tile, m-block, k-slice).
// Workgroup i is taken to run on XCD i & 7 (a speed assumption only: no result depends on it).
//   * default map: every m-block and k-slice of a weight tile on one XCD (tile = 8 * (j / ks / nmb) + xcd), so a
//     weight tile leaves HBM once; every XCD's L2 then pulls the WHOLE activation matrix through the fabric;
//   * slice-per-XCD map (mode 10 under split-K with ks in {2, 4, 8}, plain rows): XCD x runs k-slice x % ks of the
//     tiles of group x / ks (G = 8 / ks groups), all m-blocks. An XCD reads only its slice of the activations (fabric
//     reads of X fall from 8 X to G X), every weight byte is still fetched by one XCD and the m-blocks of a weight
//     tile still share it in that XCD's L2. Slices, slab layout and slab sums are the default map's: same bits.
//     Measured (profiles/splitk_xcd_map_r10.txt): the down projection at M = 512 reads 147 MB instead of 235 MB
//     from the fabric and runs 2-3 us (3-4 %) faster; hgemm.hip keeps the default map (no gain, one loss).
struct GridPos { int tile, mb, kslice; };

// k-slices per XCD group when the launch takes the slice-per-XCD map, else 0. MoE launches (mapped rows, device
// row counts) keep the default map.
inline int splitk_xcd(const SegList& sl, int ks) {
  if (ks != 2 && ks != 4 && ks != 8) return 0;
  for (int i = 0; i < sl.nseg; ++i)
    if (sl.s[i].xmap || sl.s[i].ymap || sl.s[i].mcount) return 0;
  return ks;
}
// workgroups of a launch (xk = splitk_xcd(), 0: default map); those past the last tile exit at once
inline int dense_grid(int ntiles, int nmb, int ks, int xk) {
  if (xk) return 8 * nmb * ((ntiles + 8 / xk - 1) / (8 / xk));
  return ((ntiles + 7) / 8) * 8 * nmb * ks;
}
DEVI GridPos dense_grid_pos(int i, int ks, int nmb, int xk) {
  const int xcd = i & 7, j = i >> 3;
  if (xk) return GridPos{(j / nmb) * (8 / xk) + xcd / xk, j % nmb, xcd % xk};
  return GridPos{(j / ks / nmb) * 8 + xcd, (j / ks) % nmb, j % ks};
}
// path B at one m-block (decode): ntiles * ks workgroups, none padding, a tile's k-slices on neighbouring XCDs
// (the placement its decode configurations were tuned on; the default map would put them on one XCD)
DEVI GridPos flat_grid_pos(int i, int ks) { return GridPos{i / ks, 0, i % ks}; }

// ---- workgroup prologue: from its grid position gp, this workgroup's segment, k-slice, first weight row and
// activation block. BM activation rows per m-block, TILE weight rows per tile. False: the workgroup has nothing to do (a tile past the last, or an
// m-block past the rows an expert was given). Else `a` is rebased to the m-block (x, y, argmax, m0, M = its rows).
//   MAPPED: the segments may carry MoE row maps and a device-side row count (the grid is sized for the worst case,
//     every routed row on one expert; m-blocks past the count exit before reading any weights): xm / ym = the block's
//     slice of the maps (x / y stay un-rebased under a map). Kernels whose plan refuses mapped rows load neither;
//   TABLE: the segment may be one expert of an expert table (GemvArgs::tab).
struct Block { Seg S; int kslice, row0; const int* xm; const int* ym; };

template <int BM, int TILE, bool MAPPED, bool TABLE = false>
DEVI bool block_prologue(const SegList& segs, GemvArgs& a, const GridPos gp, int ntiles, Block& B) {
  if (gp.tile >= ntiles) return false;
  const int m0 = gp.mb * BM;
  Seg& S = B.S;
  S = segs.s[0];
  if (TABLE && a.tab) {
    table_seg(S, a, gp.tile / a.sel_tiles);
  } else {
    // (an exit at the first s >= nseg, not a condition per s: a launch of one or two segments, i.e. nearly every
    // launch, then loads no other segment's tile_begin before it starts -- as a condition the compiler loaded and
    // waited for all eight, 0.4 us on the o projection's launches)
#pragma unroll
    for (int s = 1; s < 8; ++s) {
      if (s >= segs.nseg) break;
      if (gp.tile >= segs.s[s].tile_begin) S = segs.s[s];
    }
  }
  const int mrows = (MAPPED && S.mcount) ? min(*S.mcount, a.M) : a.M;
  if (MAPPED && m0 >= mrows) return false;
  B.xm = (MAPPED && S.xmap) ? S.xmap + m0 : nullptr;
  B.ym = (MAPPED && S.ymap) ? S.ymap + m0 : nullptr;
  a.m0 = m0;
  if (!B.xm) a.x += (size_t)m0 * a.ldx;
  const size_t esz = (a.epi == EPI_F32 || a.epi == EPI_ADD_F32 || a.epi == EPI_ARGMAX) ? 4 : 2;
  if (!B.ym) a.y = (char*)a.y + (size_t)m0 * a.ldy * esz;
  if (a.argmax) a.argmax += m0;
  a.M = min(BM, mrows - m0);
  B.kslice = gp.kslice;
  B.row0 = (gp.tile - S.tile_begin) * TILE;
  return true;
}

// ---- epilogues. A kernel compiles in the optional ones its plan (qgemv.hip) lets through; the split-K slab store and
// the f32 / add / f16 stores are always there.
constexpr unsigned ADMIT_SWIGLU = 1u << EPI_SWIGLU, ADMIT_ARGMAX = 1u << EPI_ARGMAX, ADMIT_ROPE = 1u << EPI_ROPE;
struct NoRope { DEVI void operator()(int, int, float) const {} };

// Row-per-lane mapping (activations as the MFMA A operand; modes 2, 3, 4/5/6, 14; path B keeps a copy, see there): of its NI x NJ accumulator tiles
// the lane holds weight row wrow(j) and the NE activation rows arow(i, e), as accv(i, j, e); RED lanes share an
// activation row (16; 32 with 32x32 tiles). NT threads, BM activation rows per workgroup. ym: the block's y-row map
// or null. `rope(row, b, v)` is the kernel's EPI_ROPE store of one element (mode 4: rope_store1; mode 14 runs its
// hoisted RoPE over the whole tile itself and admits none here). `lds` (free after the K loop, BM * 8 bytes) carries
// the arg-max reduction.
template <unsigned ADMIT, int NI, int NJ, int NE, int RED, int NT, int BM, class Acc, class WRow, class ARow,
          class Rope = NoRope>
DEVI void epi_rows(Acc accv, WRow wrow, ARow arow, const Seg& S, int kslice, int ks, const GemvArgs& a, float* ws,
                   void* lds, const int* ym, Rope rope = Rope{}) {
  const int lane = threadIdx.x & 63;
  const int M = a.M;
  if (ks > 1) {   // (also every EPI_SLABS launch: the plan admits it only with ks >= 2)
    const int ntot = a.pad;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int row = wrow(j);
      if (row >= S.rows) continue;
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const int b = arow(i, e);
          if (b >= M) continue;
          if (ym)        // mapped split-K: slab row = the token's y row, columns shared by every expert
            ws[((size_t)kslice * a.mtot + ym[b]) * ntot + S.ycol + row] = accv(i, j, e);
          else
            ws[((size_t)kslice * a.mtot + a.m0 + b) * ntot + S.tile_begin_col + row] = accv(i, j, e);
        }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int row = wrow(j);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int b = arow(i, e);
        const float v = accv(i, j, e) * a.alpha;
        if constexpr ((ADMIT & ADMIT_ROPE) != 0) {
          if (a.epi == EPI_ROPE) {
            rope(row, b, v);
            continue;
          }
        }
        if constexpr ((ADMIT & ADMIT_SWIGLU) != 0) {
          if (a.epi == EPI_SWIGLU) {
            // interleaved [g0..g7, u0..u7] per 16 weight rows: the partner row is lane ^ 8 (same b). A lane's rows
            // are a multiple of 16 plus r = lane & 15 (or & 31), so (row & 8) == 0 is r < 8 (a gate row) and
            // ((row & ~15) >> 1) + (row & 7) is (first row of the 16-row tile >> 1) + r
            const float u = __shfl_xor(v, 8, 64);
            if ((row & 8) == 0 && b < M && row < S.rows) {
              const int n = S.ycol + ((row & ~15) >> 1) + (row & 7);
              reinterpret_cast<act_t*>(a.y)[(size_t)(ym ? ym[b] : b) * a.ldy + n] = (act_t)(silu(v) * u);
            }
            continue;
          }
        }
        if (b < M && row < S.rows) {
          const size_t off = (size_t)(ym ? ym[b] : b) * a.ldy + S.ycol + row;
          if (a.epi == EPI_F32) reinterpret_cast<float*>(a.y)[off] = v;
          else if (a.epi == EPI_ADD_F32) reinterpret_cast<float*>(a.y)[off] += v;
          else if (a.epi == EPI_ACT) reinterpret_cast<act_t*>(a.y)[off] = (act_t)v;
        }
      }
    }
  }
  if constexpr ((ADMIT & ADMIT_ARGMAX) != 0) {
    if (a.argmax) {
      // greedy arg-max: max over the lane's weight rows, then the lanes sharing an activation row, then the
      // workgroup's waves through LDS -> ONE global atomic per activation row per workgroup (vs one per 16 rows: 1M
      // contended 64-bit atomics on the 128K-row lm_head otherwise)
      unsigned long long* red = reinterpret_cast<unsigned long long*>(lds);
      __syncthreads();   // every wave is done with the K loop's LDS
      for (int idx = threadIdx.x; idx < BM; idx += NT) red[idx] = 0ull;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          unsigned long long k = 0ull;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int row = wrow(j);
            const unsigned long long kj = (row < S.rows) ? argmax_key(accv(i, j, e) * a.alpha, S.ycol + row) : 0ull;
            k = kj > k ? kj : k;
          }
#pragma unroll
          for (int o = 1; o < RED; o <<= 1) {
            const unsigned long long ok = __shfl_xor(k, o, 64);
            k = ok > k ? ok : k;
          }
          if ((lane & (RED - 1)) == 0) atomicMax(red + arow(i, e), k);
        }
      __syncthreads();
      for (int idx = threadIdx.x; idx < M; idx += NT) atomicMax(a.argmax + idx, red[idx]);
    }
  }
}

// Four-rows-per-lane mapping (weights as the MFMA A operand; modes 9 and 10): of the wave's NI x NJ accumulator tiles
// lane l holds weight rows nb + 16i + 4(l >> 4) + e (e = 0..3: four consecutive output columns, so 16-byte stores, and
// RoPE pairs (e, e + 1) inside the lane) and activation row mb + 16j + (l & 15). SwiGLU's interleaved [g0..g7 | u0..u7]
// per 16 weight rows puts the gate rows in lanes 0-31 and their up partners in lane ^ 32. ym: the block's y-row map
// or null (mapped split-K slabs are indexed by the y row, one shared segment column range).
template <unsigned ADMIT, int NI, int NJ>
DEVI void epi_cols4(const f32x4 (&acc)[NI][NJ], const Seg& S, int nb, int mb, int kslice, int ks, const GemvArgs& a,
                    float* ws, const int* ym) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const int M = a.M;
  const int g4 = 4 * (lane >> 4), r16 = lane & 15;
  auto yrow = [&](int m) __attribute__((always_inline)) { return ym ? ym[m] : m; };
  if (ks > 1 || a.epi == EPI_SLABS) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = nb + 16 * i + g4;
      if (n >= S.rows) continue;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int m = mb + 16 * j + r16;
        if (m >= M) continue;
        const size_t srow = ym ? (size_t)ym[m] : (size_t)(a.m0 + m);
        const int scol = ym ? n : S.tile_begin_col + n;
        *reinterpret_cast<f32x4*>(ws + ((size_t)kslice * a.mtot + srow) * a.pad + scol) = acc[i][j];
      }
    }
    return;
  }
  const float al = a.alpha;
  if constexpr ((ADMIT & ADMIT_ROPE) != 0) {
    if (a.epi == EPI_ROPE) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int n = nb + 16 * i + g4;
        if (n >= S.rows) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int m = mb + 16 * j + r16;
          if (m >= M) continue;
          const f32x4 v = acc[i][j] * al;
          rope_store1(a, S.ycol + n, a.m0 + m, v[0], v[1]);
          rope_store1(a, S.ycol + n + 1, a.m0 + m, v[1], v[0]);
          rope_store1(a, S.ycol + n + 2, a.m0 + m, v[2], v[3]);
          rope_store1(a, S.ycol + n + 3, a.m0 + m, v[3], v[2]);
        }
      }
      return;
    }
  }
  if (a.epi == EPI_SWIGLU) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        f32x4 u;
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = __shfl_xor(acc[i][j][e] * al, 32, 64);
        const int n16 = nb + 16 * i, m = mb + 16 * j + r16;
        if (lane < 32 && m < M && n16 < S.rows) {
          h4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (_Float16)(silu(acc[i][j][e] * al) * u[e]);
          *reinterpret_cast<h4*>(reinterpret_cast<act_t*>(a.y) + (size_t)yrow(m) * a.ldy + S.ycol + (n16 >> 1) + g4) = o;
        }
      }
    }
    return;
  }
  if (a.epi != EPI_ARGMAX) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = nb + 16 * i + g4;
      if (n >= S.rows) continue;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int m = mb + 16 * j + r16;
        if (m >= M) continue;
        const f32x4 v = acc[i][j] * al;
        if (a.epi == EPI_ACT) {
          *reinterpret_cast<h4*>(reinterpret_cast<act_t*>(a.y) + (size_t)yrow(m) * a.ldy + S.ycol + n) =
              h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        } else {
          f32x4* p = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.y) + (size_t)yrow(m) * a.ldy + S.ycol + n);
          *p = a.epi == EPI_ADD_F32 ? *p + v : v;
        }
      }
    }
  }
  if (a.argmax) {
    // per activation row: max over the lane's rows, then the 4 lanes of the row (l ^ 16, l ^ 32)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      unsigned long long k = 0ull;
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int n = nb + 16 * i + g4 + e;
          const unsigned long long kk = n < S.rows ? argmax_key(acc[i][j][e] * al, S.ycol + n) : 0ull;
          k = kk > k ? kk : k;
        }
      unsigned long long o = __shfl_xor(k, 16, 64);
      k = o > k ? o : k;
      o = __shfl_xor(k, 32, 64);
      k = o > k ? o : k;
      const int m = mb + 16 * j + r16;
      if (lane < 16 && m < M) atomicMax(a.argmax + m, k);
    }
  }
}

// ---- launcher of a kernel with dynamic LDS. More than 64 KiB must be opted into, once per kernel instantiation.
template <auto Kernel, class... Args>
int launch_lds(int grid, int threads, size_t lds_bytes, hipStream_t st, const Args&... args) {
  static bool attr = false;
  if (!attr) {
    const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    attr = true;
  }
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds_bytes, st, args...);
  return (int)hipGetLastError();
}

}  // namespace nls_gemv
