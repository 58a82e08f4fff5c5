"""The GEMV/GEMM dispatcher's refusal rules and the Python-side twins of what it decides, on the CPU.

Everything here goes through `nls_qgemv_plan`, the first half of the launch entry: it decides from the arguments
alone, makes no HIP call and dereferences no pointer, so the pointers below are dummy non-null integers and nothing
is launched on any machine. THIS MODULE MUST NEVER CALL `nls_qgemv`: with these pointers a real launch would fault
the device. (The one place that exercises `ops._launch` swaps the library for a shim whose `nls_qgemv` is the planner.)

The library is loaded with `_lib.lib()`: where it was not built the tests fail, they do not skip.
"""
import ctypes
import itertools
import types

import pytest

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.ops import _lib, transcode

P = 0x10000          # a non-null pointer that is never dereferenced
F32, F16, Q4_0, Q8_0, Q4_K, Q5_K, Q6_K, BF16 = 0, 1, 2, 8, 12, 13, 14, 30
Q51, IQ4 = transcode.QT_Q51, transcode.QT_IQ4
TYPES = (F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K, Q51, IQ4, Q4_0)    # the nine device types + one with no kernel


def S(type=Q4_K, rows=64, K=256, ycol=0, xmap=None, ymap=None, mcount=None):
    return _lib.NlsSeg(P, xmap, ymap, mcount, type, rows, K, ycol)


def plan(segs, M=1, epi="f32", cfg=(0, 4, 1, 1), ldx=None, ldy=4096, argmax=None, ws=None, ws_floats=0, fz=None):
    """(accepted, NlsPlan) of one launch's arguments."""
    arr = (_lib.NlsSeg * max(len(segs), 1))(*segs)
    mode, waves, rt, ks = cfg
    out = _lib.NlsPlan()
    ldx = ldx if ldx is not None else (segs[0].K if segs else 256)
    rc = _lib.lib().nls_qgemv_plan(arr, len(segs), P, ldx, P, ldy, M, 1.0, ops.EPI[epi], argmax, waves, rt, mode, ks, ws,
                                   ws_floats, None,
                                   None if fz is None else ctypes.byref(fz), ctypes.byref(out))
    assert rc in (0, -1), rc
    return rc == 0, out


def F(**kw):
    return _lib.NlsFuse(**kw)


# ---- the fused-operand groups: the accepted operands of each, to deviate from ---------------------------------------
NORM = dict(xf=P, ldxf=256, nw=P, eps=1e-5)
SSQ_IN = dict(NORM, ssq_in=P, ldss=4, nss_in=4)
SSQ_OUT = dict(ssq_out=P, ldss=4)                                  # rows 64, rt 1: 4 tiles
ROPE = dict(pos=P, slot=P, cs=P, q_out=P, ldq=64, kc=P, vc=P, Hq=2, Hkv=1, D=32)
QKV = lambda t=Q4_K: [S(t, 64, ycol=0), S(t, 32, ycol=64), S(t, 32, ycol=96)]    # (Hq + 2 Hkv) D = 128 rows
ADDNORM = dict(hout=P, ldh=64, onw=P, cnt=P, eps=1e-5)
ROUTE = dict(ADDNORM, wr=P, E=64, topk=8, rlogits=P, topw=P, counts=P, xrows=P, yrows=P)
SEL = dict(sel=P, sel_slots=256, sel_base=0)
TAB = dict(tab=P, tab_n=16, tab_cap=4)
EXPERT = lambda **kw: S(xmap=P, ymap=P, mcount=P, **kw)

# (name, segments, plan() keywords, expected): expected None = refused, else the NlsPlan fields to find
CASES = [
    # ---- every mode: segment list and row count
    ("nseg 0", [], dict(), None),
    ("nseg 8", [S(ycol=64 * i) for i in range(8)], dict(), dict(tiles=32, cols=512)),
    ("nseg 9", [S(ycol=64 * i) for i in range(9)], dict(), None),
    ("M 0", [S()], dict(M=0), None),
    ("K 100", [S(K=100)], dict(), None),
    ("rows 0", [S(rows=0)], dict(), None),
    ("type without a kernel", [S(Q4_0)], dict(), None),
    ("two type-sets", [S(Q4_K), S(Q5_K, ycol=64)], dict(), None),
    ("mode -1", [S()], dict(cfg=(-1, 4, 1, 1)), None),
    ("mode 7", [S()], dict(cfg=(7, 8, 2, 1), M=256), None),
    ("mode 8", [S()], dict(cfg=(8, 8, 2, 1), M=256), None),
    ("mode 11", [S()], dict(cfg=(11, 8, 2, 1), M=256), None),
    # ---- mode 0: path A
    ("A decode", [S()], dict(), dict(kset=0, tile_rows=16, tiles=4, cols=64, ws_floats=0, reduce=0)),
    ("A 8 waves 2 tiles, M 64, 3 segs", QKV(Q6_K), dict(M=64, cfg=(0, 8, 2, 1)), dict(tile_rows=32, tiles=4, cols=128)),
    ("A rows 250, 20", [S(rows=250), S(rows=20, ycol=250)], dict(M=5), dict(tiles=18, cols=270)),
    ("A mapped rows", [EXPERT()], dict(M=33), dict(tiles=4)),
    ("A M 65", [S()], dict(M=65), None),
    ("A 16 waves", [S()], dict(cfg=(0, 16, 1, 1)), None),
    ("A 7 waves", [S()], dict(cfg=(0, 7, 1, 1)), None),
    ("A rt 3", [S()], dict(cfg=(0, 4, 3, 1)), None),
    ("A slabs", [S()], dict(epi="slabs", cfg=(0, 4, 1, 2), ws=P, ws_floats=1 << 20), None),
    ("swiglu rows 16", [S(rows=16)], dict(epi="swiglu"), dict(tiles=1)),
    ("swiglu rows 20", [S(rows=20)], dict(epi="swiglu"), None),
    # ---- mode 1: path B
    ("B 4x2, M 17", [S()], dict(M=17, cfg=(1, 4, 2, 1)), dict(tile_rows=128, tiles=1, ws_floats=0, reduce=0)),
    ("B M 256", [S(rows=250)], dict(M=256, cfg=(1, 8, 1, 1)), dict(tile_rows=128, tiles=2)),
    ("B split-K", [S(), S(Q6_K, ycol=64)], dict(M=4, cfg=(1, 8, 1, 2), ws=P, ws_floats=1024),
     dict(tiles=2, slab_width=128, ws_floats=1024, reduce=1, mapped_splitk=0)),
    ("B split-K slabs", [S()], dict(M=4, epi="slabs", cfg=(1, 8, 1, 2), ws=P, ws_floats=512),
     dict(ws_floats=512, reduce=0)),
    ("B split-K, workspace one float short", [S(), S(Q6_K, ycol=64)], dict(M=4, cfg=(1, 8, 1, 2), ws=P, ws_floats=1023),
     None),
    ("B split-K without a workspace", [S()], dict(M=4, cfg=(1, 8, 1, 2), ws_floats=1 << 20), None),
    ("B slabs without split-K", [S()], dict(M=4, epi="slabs", cfg=(1, 8, 1, 1)), None),
    ("B rt 3", [S()], dict(cfg=(1, 4, 3, 1)), None),
    ("B 16 waves", [S()], dict(cfg=(1, 16, 1, 1)), None),
    ("B mapped rows", [EXPERT()], dict(M=33, cfg=(1, 4, 2, 1)), dict(tiles=1)),
    ("B mapped rows + argmax", [EXPERT()], dict(M=33, cfg=(1, 4, 2, 1), argmax=P), None),
    ("B mapped split-K", [EXPERT(), EXPERT()], dict(M=33, cfg=(1, 4, 2, 2), ws=P, ws_floats=2 * 33 * 64),
     dict(mapped_splitk=1, slab_width=64, cols=128, ws_floats=2 * 33 * 64, reduce=1)),
    ("B mapped split-K, other store", [EXPERT(), EXPERT()], dict(M=33, epi="act", cfg=(1, 4, 2, 2), ws=P, ws_floats=1 << 20),
     None),
    ("B mapped split-K, own columns", [EXPERT(), EXPERT(ycol=64)], dict(M=33, cfg=(1, 4, 2, 2), ws=P, ws_floats=1 << 20),
     None),
    ("B 7 waves", [S(K=24576)], dict(cfg=(1, 7, 1, 1)), dict(tile_rows=112, tiles=1)),
    ("B 7 waves, M 4", [S()], dict(M=4, cfg=(1, 7, 1, 1)), None),
    ("B 7 waves, rt 2", [S()], dict(cfg=(1, 7, 2, 1)), None),
    ("B 7 waves, row too long to stage", [S(K=24832)], dict(cfg=(1, 7, 1, 1)), None),
    ("B 7 waves, row staged per K-slice", [S(K=24832)], dict(cfg=(1, 7, 1, 2), ws=P, ws_floats=128), dict(tiles=1)),
    ("B 7 waves, mapped rows", [S(mcount=P)], dict(cfg=(1, 7, 1, 1)), None),
    # ---- mode 2: LDS-dequant GEMM
    ("LDS 256-row blocks", [S(Q5_K), S(Q8_0, ycol=64)], dict(M=256, cfg=(2, 8, 4, 1)), dict(kset=1, tile_rows=128, tiles=2)),
    ("LDS 64-row blocks, experts", [EXPERT()], dict(M=65, cfg=(2, 8, 1, 1)), dict(tiles=1)),
    ("LDS 4 waves", [S()], dict(M=256, cfg=(2, 4, 4, 1)), None),
    ("LDS rt 3", [S()], dict(M=256, cfg=(2, 8, 3, 1)), None),
    ("LDS f16 tiles", [S(F16)], dict(M=256, cfg=(2, 8, 4, 1)), None),
    ("LDS Q51", [S(Q51)], dict(M=256, cfg=(2, 8, 4, 1)), None),
    ("LDS IQ4", [S(IQ4)], dict(M=256, cfg=(2, 8, 4, 1)), None),
    # ---- mode 3: LDS-DMA GEMM
    ("DMA 256-row blocks", [S(), S(Q6_K, rows=250, ycol=64)], dict(M=256, cfg=(3, 4, 16, 1)), dict(kset=0, tiles=3)),
    ("DMA 96-row blocks, experts", [EXPERT(type=Q5_K)], dict(M=65, cfg=(3, 4, 6, 1)), dict(kset=1, tiles=1)),
    ("DMA 8 waves", [S()], dict(M=256, cfg=(3, 8, 16, 1)), None),
    ("DMA rt 2", [S()], dict(M=256, cfg=(3, 4, 2, 1)), None),
    ("DMA Q8_0", [S(Q5_K), S(Q8_0, ycol=64)], dict(M=256, cfg=(3, 4, 16, 1)), None),
    ("DMA bf16 tiles", [S(BF16)], dict(M=256, cfg=(3, 4, 16, 1)), None),
    ("DMA IQ4", [S(IQ4)], dict(M=256, cfg=(3, 4, 16, 1)), None),
    # ---- modes 4 / 5 / 6: dense f16 GEMM
    ("dense 128-row tiles", [S(F16, rows=250)], dict(M=256, cfg=(4, 8, 4, 1)), dict(kset=2, tile_rows=128, tiles=2)),
    ("dense 16 waves, split-K", [S(F16)], dict(M=256, cfg=(4, 16, 2, 2), ws=P, ws_floats=2 * 256 * 64),
     dict(ws_floats=2 * 256 * 64, reduce=1)),
    ("dense mapped rows", [EXPERT(type=F16)], dict(M=65, cfg=(4, 8, 2, 1)), dict(tiles=1)),
    ("dense 4 waves", [S(F16)], dict(M=256, cfg=(4, 4, 4, 1)), None),
    ("dense rt 1", [S(F16)], dict(M=256, cfg=(4, 8, 1, 1)), None),
    ("dense Q4_K", [S()], dict(M=256, cfg=(4, 8, 4, 1)), None),
    ("dense 256-row tiles", [S(F16, rows=250), S(F16, rows=20, ycol=250)], dict(M=256, cfg=(5, 8, 2, 1)),
     dict(tile_rows=256, tiles=2)),
    ("dense 256-row tiles, rt 3", [S(F16)], dict(M=256, cfg=(5, 8, 3, 1)), None),
    ("dense 256-row tiles, bf16", [S(BF16)], dict(M=256, cfg=(5, 8, 4, 1)), None),
    ("dense 2-deep rings", [S(F16)], dict(M=256, cfg=(6, 8, 2, 1)), dict(tile_rows=128, tiles=1)),
    ("dense 2-deep rings, 16 waves", [S(F16)], dict(M=256, cfg=(6, 16, 2, 1)), None),
    ("dense 2-deep rings, rt 4", [S(F16)], dict(M=256, cfg=(6, 8, 4, 1)), None),
    # ---- mode 9: quantised GEMM on raw tile-blocks
    ("q9 4x2", [S(), S(Q6_K, rows=252, ycol=64)], dict(M=256, cfg=(9, 4, 2, 1)), dict(kset=0, tile_rows=128, tiles=3)),
    ("q9 8x1, Q8_0", [S(Q8_0)], dict(M=256, cfg=(9, 8, 1, 1)), dict(kset=1, tile_rows=128)),
    ("q9 8x2, IQ4 split-K", [S(IQ4)], dict(M=65, cfg=(9, 8, 2, 2), ws=P, ws_floats=2 * 65 * 64),
     dict(kset=4, tile_rows=256, reduce=1)),
    ("q9 Q51", [S(Q51)], dict(M=256, cfg=(9, 8, 2, 1)), dict(kset=3)),
    ("q9 4x1", [S()], dict(M=256, cfg=(9, 4, 1, 1)), None),
    ("q9 8x4", [S()], dict(M=256, cfg=(9, 8, 4, 1)), None),
    ("q9 f16 tiles", [S(F16)], dict(M=256, cfg=(9, 8, 2, 1)), None),
    ("q9 mapped rows", [EXPERT()], dict(M=256, cfg=(9, 8, 2, 1)), None),
    ("q9 ldx % 8", [S()], dict(M=256, cfg=(9, 8, 2, 1), ldx=260), None),
    ("q9 ldy % 4", [S()], dict(M=256, cfg=(9, 8, 2, 1), ldy=250), None),
    ("q9 ldy % 4, swiglu", [S()], dict(M=256, epi="swiglu", cfg=(9, 8, 2, 1), ldy=250), dict(tiles=1)),
    ("q9 ycol % 4", [S(ycol=2)], dict(M=256, cfg=(9, 8, 2, 1)), None),
    # (epi_cols4 stores four output columns, and four slab floats, behind one row check)
    ("q9 rows % 4", [S(), S(Q6_K, rows=250, ycol=64)], dict(M=256, cfg=(9, 4, 2, 1)), None),
    ("q9 rows % 4, split-K", [S(rows=37)], dict(M=65, cfg=(9, 8, 2, 2), ws=P, ws_floats=2 * 65 * 37), None),
    # ---- mode 10: dense f16 GEMM, 256 x 256 tiles
    ("d10 256-row tiles", [S(F16, rows=252), S(F16, rows=20, ycol=252)], dict(M=256, cfg=(10, 8, 1, 1)),
     dict(kset=2, tile_rows=256, tiles=2)),
    ("d10 128-row tiles, split-K", [S(F16, rows=252)], dict(M=33, cfg=(10, 8, 2, 2), ws=P, ws_floats=2 * 33 * 252),
     dict(tile_rows=128, tiles=2, ws_floats=2 * 33 * 252, reduce=1)),
    ("d10 rows % 4", [S(F16, rows=250)], dict(M=256, cfg=(10, 8, 1, 1)), None),
    ("d10 rows % 4, second segment", [S(F16, rows=252), S(F16, rows=37, ycol=252)], dict(M=256, cfg=(10, 8, 2, 1)),
     None),
    ("d10 rows % 4, split-K", [S(F16, rows=293)], dict(M=33, cfg=(10, 8, 2, 2), ws=P, ws_floats=2 * 33 * 293), None),
    ("d10 ldx % 8", [S(F16)], dict(M=256, cfg=(10, 8, 1, 1), ldx=260), None),
    ("d10 ldy % 4", [S(F16)], dict(M=256, cfg=(10, 8, 1, 1), ldy=250), None),
    ("d10 Q4_K", [S()], dict(M=256, cfg=(10, 8, 1, 1)), None),
    ("d10 bf16", [S(BF16)], dict(M=256, cfg=(10, 8, 1, 1)), None),
    ("d10 rt 3", [S(F16)], dict(M=256, cfg=(10, 8, 3, 1)), None),
    ("d10 4 waves", [S(F16)], dict(M=256, cfg=(10, 4, 1, 1)), None),
    ("d10 16 waves", [S(F16)], dict(M=256, cfg=(10, 16, 1, 1)), None),
    ("d10 mapped rows", [EXPERT(type=F16)], dict(M=256, cfg=(10, 8, 1, 1)), None),
    ("d10 ycol % 4", [S(F16, ycol=2)], dict(M=256, cfg=(10, 8, 1, 1)), None),
    # ---- input RMSNorm
    ("norm", [S()], dict(M=16, fz=F(**NORM)), dict(tiles=4)),
    ("norm M 17", [S()], dict(M=17, fz=F(**NORM)), None),
    ("norm without weights", [S()], dict(M=16, fz=F(**dict(NORM, nw=None))), None),
    ("norm rows fill the LDS", [S(K=1792)], dict(M=16, fz=F(**NORM)), dict(tiles=4)),
    ("norm rows past the LDS", [S(K=2048)], dict(M=16, fz=F(**NORM)), None),
    ("norm mapped rows", [S(mcount=P)], dict(M=16, fz=F(**NORM)), None),
    ("norm path B", [S()], dict(M=16, cfg=(1, 4, 2, 1), fz=F(**NORM)), None),
    ("norm LDS GEMM", [S()], dict(M=16, cfg=(2, 8, 4, 1), fz=F(**SSQ_IN)), None),
    ("norm dense GEMM", [S(F16)], dict(M=16, cfg=(4, 8, 4, 1), fz=F(**NORM)), None),
    ("norm q9", [S()], dict(M=16, cfg=(9, 8, 2, 1), fz=F(**NORM)), None),
    ("norm d10", [S(F16)], dict(M=16, cfg=(10, 8, 1, 1), fz=F(**NORM)), None),
    ("norm partial sums", [S()], dict(M=16, fz=F(**SSQ_IN)), dict(tiles=4)),
    ("norm partial sums path B", [S(K=1536)], dict(M=16, cfg=(1, 4, 2, 1), fz=F(**SSQ_IN)), dict(tiles=1)),
    ("norm partial sums path B, slice past the LDS", [S(K=1792)], dict(M=16, cfg=(1, 4, 2, 1), fz=F(**SSQ_IN)), None),
    ("norm partial sums path B, M 17", [S()], dict(M=17, cfg=(1, 4, 2, 1), fz=F(**SSQ_IN)), None),
    ("partial sums without norm rows", [S()], dict(M=16, fz=F(ssq_in=P, ldss=4, nss_in=4)), None),
    ("partial sums: none", [S()], dict(M=16, fz=F(**dict(SSQ_IN, nss_in=0))), None),
    ("partial sums: more than a row holds", [S()], dict(M=16, fz=F(**dict(SSQ_IN, nss_in=5))), None),
    # ---- split-RMSNorm producer
    ("ssq_out", [S()], dict(M=32, epi="add", fz=F(**SSQ_OUT)), dict(tiles=4)),
    ("ssq_out M 33", [S()], dict(M=33, epi="add", fz=F(**SSQ_OUT)), None),
    ("ssq_out ldss one short", [S()], dict(M=32, epi="add", fz=F(**dict(SSQ_OUT, ldss=3))), None),
    ("ssq_out 2 tiles per workgroup", [S()], dict(M=32, epi="add", cfg=(0, 4, 2, 1), fz=F(**dict(SSQ_OUT, ldss=2))),
     dict(tiles=2)),
    ("ssq_out path B", [S()], dict(M=32, epi="add", cfg=(1, 4, 1, 1), fz=F(**SSQ_OUT)), None),
    ("ssq_out plain store", [S()], dict(M=32, fz=F(**SSQ_OUT)), None),
    ("ssq_out 2 segs", [S(rows=16), S(rows=16, ycol=16)], dict(M=32, epi="add", fz=F(**SSQ_OUT)), None),
    ("ssq_out mapped rows", [S(ymap=P)], dict(M=32, epi="add", fz=F(**SSQ_OUT)), None),
    ("ssq_out argmax", [S()], dict(M=32, epi="add", argmax=P, fz=F(**SSQ_OUT)), None),
    ("ssq_out + output norm", [S()], dict(M=32, epi="add", fz=F(**dict(SSQ_OUT, **ADDNORM))), None),
    # ---- RoPE epilogue
    ("rope path A", QKV(), dict(M=5, epi="rope", fz=F(**ROPE)), dict(tiles=8, cols=128)),
    ("rope + norm", QKV(), dict(M=5, epi="rope", fz=F(**dict(ROPE, **NORM))), dict(tiles=8)),
    ("rope dense", QKV(F16), dict(M=256, epi="rope", cfg=(4, 8, 4, 1), fz=F(**ROPE)), dict(tiles=3)),
    ("rope dense 256-row tiles", QKV(F16), dict(M=256, epi="rope", cfg=(5, 8, 4, 1), fz=F(**ROPE)), dict(tiles=3)),
    ("rope d10", QKV(F16), dict(M=256, epi="rope", cfg=(10, 8, 1, 1), fz=F(**ROPE)), dict(tiles=3)),
    ("rope dense split-K", QKV(F16), dict(M=256, epi="rope", cfg=(4, 8, 4, 2), ws=P, ws_floats=1 << 20, fz=F(**ROPE)), None),
    ("rope dense 2-deep rings", QKV(F16), dict(M=256, epi="rope", cfg=(6, 8, 2, 1), fz=F(**ROPE)), None),
    ("rope path B", QKV(), dict(M=5, epi="rope", cfg=(1, 4, 2, 1), fz=F(**ROPE)), None),
    ("rope q9", QKV(), dict(M=256, epi="rope", cfg=(9, 8, 2, 1), fz=F(**ROPE)), None),
    ("rope segments not contiguous", [S(rows=64), S(rows=32, ycol=96), S(rows=32, ycol=64)],
     dict(M=5, epi="rope", fz=F(**ROPE)), None),
    ("rope heads != rows", QKV(), dict(M=5, epi="rope", fz=F(**dict(ROPE, Hq=3))), None),
    ("rope rows 20", [S(rows=64), S(rows=20, ycol=64), S(rows=44, ycol=84)], dict(M=5, epi="rope", fz=F(**ROPE)), None),
    ("rope mapped rows", [S(rows=128, ymap=P)], dict(M=5, epi="rope", fz=F(**ROPE)), None),
    ("rope argmax", QKV(), dict(M=5, epi="rope", argmax=P, fz=F(**ROPE)), None),
    ("rope odd D", QKV(), dict(M=5, epi="rope", fz=F(**dict(ROPE, Hq=126, D=1))), None),
    ("rope no heads", QKV(), dict(M=5, epi="rope", fz=F(**dict(ROPE, Hq=0, Hkv=2))), None),
    *[(f"rope without {k}", QKV(), dict(M=5, epi="rope", fz=F(**dict(ROPE, **{k: None}))), None)
      for k in ("pos", "slot", "cs", "q_out", "kc", "vc")],
    ("rope without operands", QKV(), dict(M=5, epi="rope"), None),
    # ---- residual add + output norm (+ MoE route)
    ("add+norm", [S()], dict(M=5, epi="add", fz=F(**ADDNORM)), dict(tiles=4)),
    ("add+norm path B", [S()], dict(M=5, epi="add", cfg=(1, 4, 1, 1), fz=F(**ADDNORM)), None),
    ("add+norm plain store", [S()], dict(M=5, fz=F(**ADDNORM)), None),
    ("add+norm 2 segs", [S(rows=16), S(rows=16, ycol=16)], dict(M=5, epi="add", fz=F(**ADDNORM)), None),
    ("add+norm ycol", [S(ycol=4)], dict(M=5, epi="add", fz=F(**ADDNORM)), None),
    ("add+norm mapped rows", [S(xmap=P)], dict(M=5, epi="add", fz=F(**ADDNORM)), None),
    ("add+norm rows 250", [S(rows=250)], dict(M=5, epi="add", fz=F(**ADDNORM)), None),
    ("add+norm argmax", [S()], dict(M=5, epi="add", argmax=P, fz=F(**ADDNORM)), None),
    ("add+norm without counter", [S()], dict(M=5, epi="add", fz=F(**dict(ADDNORM, cnt=None))), None),
    ("add+norm without output", [S()], dict(M=5, epi="add", fz=F(**dict(ADDNORM, hout=None))), None),
    ("route", [S()], dict(M=4, epi="add", fz=F(**ROUTE)), dict(tiles=4)),
    ("route M 5", [S()], dict(M=5, epi="add", fz=F(**ROUTE)), None),
    ("route E 65", [S()], dict(M=4, epi="add", fz=F(**dict(ROUTE, E=65))), None),
    ("route E 0", [S()], dict(M=4, epi="add", fz=F(**dict(ROUTE, E=0))), None),
    ("route topk 9", [S()], dict(M=4, epi="add", fz=F(**dict(ROUTE, topk=9))), None),
    ("route topk 0", [S()], dict(M=4, epi="add", fz=F(**dict(ROUTE, topk=0))), None),
    ("route topk > E", [S()], dict(M=4, epi="add", fz=F(**dict(ROUTE, E=4, topk=5))), None),
    ("route without norm", [S()], dict(M=4, epi="add", fz=F(**dict(ROUTE, onw=None))), None),
    *[(f"route without {k}", [S()], dict(M=4, epi="add", fz=F(**dict(ROUTE, **{k: None}))), None)
      for k in ("rlogits", "topw", "counts", "xrows", "yrows")],
    # ---- device-selected segments
    ("sel", [EXPERT(), EXPERT(), EXPERT()], dict(M=4, fz=F(**SEL)), dict(tiles=256 * 4)),
    ("sel 257 slots", [EXPERT(), EXPERT(), EXPERT()], dict(M=4, fz=F(**dict(SEL, sel_slots=257))), None),
    ("sel 0 slots", [EXPERT(), EXPERT(), EXPERT()], dict(M=4, fz=F(**dict(SEL, sel_slots=0))), None),
    ("sel path B", [EXPERT(), EXPERT(), EXPERT()], dict(M=4, cfg=(1, 4, 1, 1), fz=F(**SEL)), None),
    ("sel argmax", [EXPERT(), EXPERT(), EXPERT()], dict(M=4, argmax=P, fz=F(**SEL)), None),
    ("sel other rows", [EXPERT(), EXPERT(rows=16), EXPERT()], dict(M=4, fz=F(**SEL)), None),
    ("sel other K", [EXPERT(), EXPERT(), EXPERT(K=512)], dict(M=4, fz=F(**SEL)), None),
    # ---- expert table
    ("table path A", [EXPERT()], dict(M=4, fz=F(**TAB)), dict(tiles=16 * 4)),
    ("table path B", [EXPERT()], dict(M=4, cfg=(1, 4, 2, 1), fz=F(**TAB)), dict(tiles=16)),
    ("table LDS GEMM", [EXPERT(rows=250)], dict(M=65, cfg=(2, 8, 1, 1), fz=F(**TAB)), dict(tiles=32)),
    ("table + sel", [EXPERT()], dict(M=4, fz=F(**dict(TAB, **dict(SEL, sel_slots=8)))), dict(tiles=8 * 4)),
    ("table ks 2", [EXPERT()], dict(M=4, cfg=(1, 4, 2, 2), ws=P, ws_floats=1 << 20, fz=F(**TAB)), None),
    ("table argmax", [EXPERT()], dict(M=4, argmax=P, fz=F(**TAB)), None),
    ("table 2 segs", [EXPERT(), EXPERT()], dict(M=4, fz=F(**TAB)), None),
    ("table DMA GEMM", [EXPERT()], dict(M=65, cfg=(3, 4, 4, 1), fz=F(**TAB)), None),
    ("table no experts", [EXPERT()], dict(M=4, fz=F(**dict(TAB, tab_n=0))), None),
    ("table no cap", [EXPERT()], dict(M=4, fz=F(**dict(TAB, tab_cap=0))), None),
    ("table without counts", [S(xmap=P, ymap=P)], dict(M=4, fz=F(**TAB)), None),
    ("table + norm", [S(mcount=P)], dict(M=4, fz=F(**dict(TAB, **NORM))), None),
    ("table + output norm", [S(mcount=P)], dict(M=4, epi="add", fz=F(**dict(TAB, **ADDNORM))), None),
    ("table + ssq_out", [S(mcount=P)], dict(M=4, epi="add", fz=F(**dict(TAB, **SSQ_OUT))), None),
    ("table slabs", [EXPERT()], dict(M=4, epi="slabs", cfg=(1, 4, 2, 2), ws=P, ws_floats=1 << 20, fz=F(**TAB)), None),
]


@pytest.mark.parametrize("name,segs,kw,want", CASES, ids=[c[0] for c in CASES])
def test_plan_case(name, segs, kw, want):
    ok, p = plan(segs, **kw)
    assert ok == (want is not None), name
    for k, v in (want or {}).items():
        assert getattr(p, k) == v, (name, k, getattr(p, k), v)


def test_cases_cover_every_mode():
    modes = {}
    for _, _, kw, want in CASES:
        modes.setdefault(kw.get("cfg", (0,))[0], set()).add(want is not None)
    assert all(modes.get(m) == {True, False} for m in (0, 1, 2, 3, 4, 5, 6, 9, 10)), modes


def test_kernel_set_is_the_plans():
    """ops.kernel_set agrees with the planner for every multiset of up to 3 of the device types (+ one type without
    a kernel): the same set, and None exactly where the planner refuses."""
    n = 0
    for k in (1, 2, 3):
        for ts in itertools.combinations_with_replacement(TYPES, k):
            ok, p = plan([S(t, ycol=64 * i) for i, t in enumerate(ts)])
            assert ops.kernel_set(ts) == (p.kset if ok else None), ts
            n += 1
    assert n == 285


class _T:
    """The few tensor attributes a launch reads, for a tensor that does not exist."""
    is_cuda, device, dtype = True, "gpu", ops.ACT_DTYPE

    def __init__(self, rows=0, cols=0):
        self.shape = (rows, cols)

    def data_ptr(self):
        return P

    def stride(self, i):
        return max(self.shape[1], 8)

    def numel(self):
        return self.shape[0] * self.shape[1]


@pytest.fixture
def planner(monkeypatch):
    """ops._launch with the library's launch entry replaced by the planner: every launch the ops module issues is
    planned, never run. Yields the list of (ws_floats passed, accepted, NlsPlan) per launch."""
    seen, real = [], _lib.lib()

    def entry(*a):
        out = _lib.NlsPlan()
        rc = real.nls_qgemv_plan(*a, ctypes.byref(out))
        seen.append((a[15], rc == 0, out))
        return rc

    shim = types.SimpleNamespace(nls_qgemv=entry, nls_qgemv_plan=real.nls_qgemv_plan)
    monkeypatch.setattr(ops._lib, "lib", lambda: shim)
    monkeypatch.setattr(ops, "_workspace", lambda dev, n: _T())
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: None)
    return seen


def _w(rows, K=256, type=Q4_K):
    return types.SimpleNamespace(rows=rows, K=K, type=type, data=_T(), d16=None, name="w")


@pytest.mark.parametrize("rows", [16, 20, 1024, 4096])
@pytest.mark.parametrize("rt", [1, 2])
def test_add_ssq_shares_are_the_plans_tiles(planner, rows, rt):
    parts = ops.qgemv_add_ssq(ops.Seg(_w(rows)), _T(32, 256), _T(32, rows), 32, 1.0, _T(), 4096 // 16,
                              cfg=(0, 4, rt, 1))
    (_, ok, p), = planner
    assert ok and parts == p.tiles


WS_CASES = [
    ("plain", [ops.Seg(_w(64)), ops.Seg(_w(250, type=Q6_K), ycol=64)], 17, "f32", (1, 8, 1, 2)),
    ("swiglu", [ops.Seg(_w(64)), ops.Seg(_w(16), ycol=32)], 5, "swiglu", (1, 4, 2, 4)),
    ("slabs", [ops.Seg(_w(252))], 65, "slabs", (9, 8, 2, 2)),
    ("mapped", [ops.Seg(_w(64), 0, _T(), _T(), _T()), ops.Seg(_w(64), 0, _T(), _T(), _T())], 33, "f32", (3, 4, 4, 2)),
    ("no split-K", [ops.Seg(_w(64))], 17, "f32", (1, 8, 1, 1)),
    ("path A", [ops.Seg(_w(64))], 17, "f32", (0, 8, 1, 2)),
]


@pytest.mark.parametrize("name,segs,M,epi,cfg", WS_CASES, ids=[c[0] for c in WS_CASES])
def test_launcher_passes_the_plans_workspace_size(planner, name, segs, M, epi, cfg):
    assert ops._launch(segs, _T(M, 256), _T(M, 4096), M, 1.0, epi, cfg, soft=True)
    (passed, ok, p), = planner
    assert ok and passed == p.ws_floats == ops._ws_floats(segs, M, cfg[0], cfg[3])
    if passed:      # one float less: refused (the slabs would run past the workspace)
        arr = ops._seg_arr(segs, cfg[0])
        assert not plan(list(arr), M=M, epi=epi, cfg=cfg, ws=P, ws_floats=passed - 1)[0]
        assert plan(list(arr), M=M, epi=epi, cfg=cfg, ws=P, ws_floats=passed)[0]
