"""Mode 14 (hgemm14.hip: the staggered dense f16 GEMM, 128 activation x 96 weight rows per workgroup) in the
dispatcher's plan, on the CPU.

Through `nls_qgemv_plan` alone, as tests/test_gemv_plan.py: dummy non-null pointers, nothing launched. THIS MODULE MUST
NEVER CALL `nls_qgemv`.
"""
import ctypes
import types

import pytest

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.ops import _lib

P = 0x10000          # a non-null pointer that is never dereferenced
F16, Q4_K, Q6_K, BF16 = 1, 12, 14, 30


def S(type=F16, rows=256, K=768, ycol=0, xmap=None, ymap=None, mcount=None):
    return _lib.NlsSeg(P, xmap, ymap, mcount, type, rows, K, ycol)


def plan(segs, M=256, epi="f32", cfg=(14, 8, 2, 1), ldx=None, ldy=4096, argmax=None, ws=None, ws_floats=0, fz=None):
    arr = (_lib.NlsSeg * len(segs))(*segs)
    mode, waves, rt, ks = cfg
    out = _lib.NlsPlan()
    rc = _lib.lib().nls_qgemv_plan(arr, len(segs), P, ldx if ldx is not None else segs[0].K, P, ldy, M, 1.0,
                                   ops.EPI[epi], argmax, waves, rt, mode, ks, ws, ws_floats, None,
                                   None if fz is None else ctypes.byref(fz), ctypes.byref(out))
    assert rc in (0, -1), rc
    return rc == 0, out


ROPE = dict(pos=P, slot=P, cs=P, q_out=P, ldq=64, kc=P, vc=P, Hq=2, Hkv=1, D=32)
QKV = [S(rows=64, ycol=0), S(rows=32, ycol=64), S(rows=32, ycol=96)]
WS = dict(ws=P, ws_floats=1 << 22)

ACCEPTED = [
    ("ks 1", [S(rows=264)], dict(), dict(kset=2, tile_rows=96, tiles=3, cols=264, ws_floats=0, reduce=0)),
    ("Q|K|V of Llama-3-8B: 64 whole tiles", [S(rows=6144, K=4096)], dict(M=512), dict(tiles=64)),
    ("ks 2", [S(rows=264, K=1024)], dict(cfg=(14, 8, 2, 2), ws=P, ws_floats=2 * 256 * 264),
     dict(tiles=3, ws_floats=2 * 256 * 264, reduce=1)),
    ("ks 3 of 6 K-tiles", [S()], dict(cfg=(14, 8, 2, 3), **WS), dict(reduce=1)),
    ("K 768, ks 2: 384-column slices, 3 whole K-tiles", [S()], dict(cfg=(14, 8, 2, 2), **WS), dict(reduce=1)),
    ("M 1", [S()], dict(M=1), dict(tiles=3)),
    ("two segments", [S(rows=250), S(rows=20, ycol=252)], dict(), dict(tiles=4, cols=270)),
    ("add", [S()], dict(epi="add"), dict(tiles=3)),
    ("act", [S()], dict(epi="act"), dict(tiles=3)),
    ("slabs", [S(K=1024)], dict(epi="slabs", cfg=(14, 8, 2, 2), **WS), dict(reduce=0, ws_floats=2 * 256 * 256)),
    ("rope", QKV, dict(epi="rope", fz=_lib.NlsFuse(**ROPE)), dict(tiles=3, cols=128)),
]

REFUSED = [
    ("Q4_K segment", [S(Q4_K)], dict()),
    ("Q6_K segment", [S(Q6_K)], dict()),
    ("bf16 segment", [S(BF16)], dict()),
    ("one quantised segment of two", [S(rows=128), S(Q4_K, rows=128, ycol=128)], dict()),
    ("mapped rows: xmap", [S(xmap=P)], dict()),
    ("mapped rows: ymap", [S(ymap=P)], dict()),
    ("mapped rows: count", [S(mcount=P)], dict()),
    ("4 waves", [S()], dict(cfg=(14, 4, 2, 1))),
    ("16 waves", [S()], dict(cfg=(14, 16, 2, 1))),
    ("rt 1", [S()], dict(cfg=(14, 8, 1, 1))),
    ("rt 4", [S()], dict(cfg=(14, 8, 4, 1))),
    ("K 768, ks 4: 192-column slices", [S()], dict(cfg=(14, 8, 2, 4), **WS)),
    ("K 1280, ks 4: 320-column slices", [S(K=1280)], dict(cfg=(14, 8, 2, 4), **WS)),
    ("K 256, ks 4: 64-column slices", [S(K=256)], dict(cfg=(14, 8, 2, 4), **WS)),
    ("rope with ks 3", QKV, dict(epi="rope", cfg=(14, 8, 2, 3), fz=_lib.NlsFuse(**ROPE), **WS)),
    ("rope with ks 2, K 1024", [S(rows=64, K=1024), S(rows=32, K=1024, ycol=64), S(rows=32, K=1024, ycol=96)],
     dict(epi="rope", cfg=(14, 8, 2, 2), fz=_lib.NlsFuse(**ROPE), **WS)),
    ("swiglu", [S()], dict(epi="swiglu")),
    ("swiglu split-K", [S(K=1024)], dict(epi="swiglu", cfg=(14, 8, 2, 2), **WS)),
    ("argmax epilogue", [S()], dict(epi="argmax", argmax=P)),
    ("argmax keys next to a store", [S()], dict(argmax=P)),
    ("input norm", [S()], dict(M=16, fz=_lib.NlsFuse(xf=P, ldxf=768, nw=P, eps=1e-5))),
    ("output norm", [S()], dict(M=5, epi="add", fz=_lib.NlsFuse(hout=P, ldh=64, onw=P, cnt=P, eps=1e-5))),
    ("ldx % 8", [S()], dict(ldx=772)),
    ("ldy % 4", [S()], dict(ldy=250)),
    ("ycol % 4", [S(ycol=2)], dict()),
    ("split-K without a workspace", [S(K=1024)], dict(cfg=(14, 8, 2, 2), ws_floats=1 << 22)),
    ("workspace one float short", [S(rows=264, K=1024)], dict(cfg=(14, 8, 2, 2), ws=P, ws_floats=2 * 256 * 264 - 1)),
    ("slabs without split-K", [S()], dict(epi="slabs")),
    ("modes 12 and 13 stay unused", [S()], dict(cfg=(12, 8, 2, 1))),
    ("mode 13", [S()], dict(cfg=(13, 8, 2, 1))),
    ("mode 15", [S()], dict(cfg=(15, 8, 2, 1))),
]


@pytest.mark.parametrize("name,segs,kw,want", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_mode14_accepted(name, segs, kw, want):
    ok, p = plan(segs, **kw)
    assert ok, name
    for k, v in want.items():
        assert getattr(p, k) == v, (name, k, getattr(p, k), v)


@pytest.mark.parametrize("name,segs,kw", REFUSED, ids=[c[0] for c in REFUSED])
def test_mode14_refused(name, segs, kw):
    assert not plan(segs, **kw)[0], name


def test_refusals_are_mode14s_own():
    """Each refused case differs from an accepted launch in the named property alone: the same arguments with the
    property put right are accepted (so no case is refused for an unrelated reason)."""
    assert plan([S()], cfg=(14, 8, 2, 3), **WS)[0]                       # K 768 in 3 slices of 2 K-tiles
    assert plan([S(K=1024)], cfg=(14, 8, 2, 4), **WS)[0]                 # K 1024 in 4 slices of 2 K-tiles
    assert plan([S(K=256)], cfg=(14, 8, 2, 2), **WS)[0]                  # 1 K-tile per slice
    assert plan([S()], cfg=(4, 8, 2, 4), **WS)[0]                        # mode 4 takes the 64-column boundary
    assert plan([S()], epi="swiglu", cfg=(4, 8, 2, 1))[0]                # ... SwiGLU and arg-max
    assert plan([S()], argmax=P, cfg=(4, 8, 2, 1))[0]
    assert plan([S(mcount=P)], cfg=(4, 8, 2, 1))[0]                      # ... and mapped rows


def test_python_side_knows_the_mode():
    assert 14 in ops.DENSE_MODES


class _D16:
    """The one attribute of an f16 copy that the launcher's segment merge reads."""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def _qkv(ptrs):
    rows = (4096, 1024, 1024)
    ws = [types.SimpleNamespace(rows=r, K=4096, d16=_D16(p), name="w") for r, p in zip(rows, ptrs)]
    return [ops.Seg(w, sum(rows[:i])) for i, w in enumerate(ws)]


@pytest.mark.parametrize("M,ks", [(512, 1), (256, 2)])
def test_table_runs_mode14_on_the_merged_copies_only(M, ks):
    """Llama-3-8B's Q|K|V entries: mode 14 where the three f16 copies are consecutive rows of one buffer (one launch
    segment, 64 whole 96-row tiles); with per-matrix copies (65 tiles) the launch keeps mode 4 at the same ks."""
    base = 0x100000
    merged = _qkv([base, base + 4096 * 4096 * 2, base + 5120 * 4096 * 2])
    apart = _qkv([base, base + (1 << 30), base + (2 << 30)])
    assert len(ops._merge_dense(merged)) == 1 and len(ops._merge_dense(apart)) == 3
    assert ops.gemv_config(merged, M) == (14, 8, 2, ks)
    assert ops.gemv_config(apart, M) == (4, 16, 2, ks)
