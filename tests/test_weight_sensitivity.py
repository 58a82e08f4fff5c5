"""GEMV / GEMM kernels against an fp64 product with the numpy decode of the ORIGINAL block bytes, with weights and a
metric that notice ONE misplaced scale, block or weight.

Weights. Every other kernel test takes its quantised weights from gguf.quants.random_blocks: one d (and dmin) per
tensor, scales in a narrow positive band -- a kernel that reads d from the wrong row of the 16-row tile, from the
wrong super-block or slab, or a Q6_K scale as unsigned, computes bit-identical outputs on them
(test_random_blocks_cannot_see_scale_faults). tests/qblocks.py writes the families used here: full (every field
over its whole range, different in every block, d of both signs), tiny_d (d / dmin below the f16 normal range) and
integer (every dequantised value exact in f16, activations in {-1, 0, 1}, every partial sum exact in fp32). The
integer family keeps d and dmin to powers of two, 0.5 / 1 / 2 where sub-block scales exist (NEIGHBOURING cells differ:
the next row of the 16-row tile and the next super-block along K; three values cannot make all 16 rows of a tile
differ, which the full family does) and 2^-3 .. 2^4 for the 32-value block formats, so that a block's eight (d, m)
pairs differ. The dequant kernel's integer test runs on these same weights, units of 0.5 and 2^-3 included, not on d
in {1, 2} alone: every value is still exact in f16 (pinned on the CPU by test_families_use_every_field) and equality
is asserted. Q4_K / Q5_K scales are cut only in the cells with d = 2 (or 1) over dmin = 0.5, where the full 6-bit
range would outgrow 11 bits.

Metric. Every output element is judged against its own dot-product size: |y - ref| / B with B = sum_k |x_k| mag_k,
mag_k = |d sc q_k| + |dmin m| in the terms of the DEVICE format (qblocks.decode), so cancellation between the scale
and the min term does not inflate it. The tolerance comes from the reference side only: EMU[family] is the largest
ratio of a CPU emulation of the kernels' arithmetic (qblocks.emulate: d*sc and dmin*m rounded to f16, one f16
rounding of the value, the load-time roundings of IQ4_XS and Q2_K; f16 x, fp32 sum) over the inputs of this module,
pinned by test_emulated_noise_bounds_tol: EMU = 1.7e-4 (full; Q4_K the largest, Q4_0 / Q5_0 0.2e-4) and 1.15e-4
(tiny_d). TOL = 4 * EMU = 6.8e-4 / 4.6e-4 covers the summation order, the split-K slab order and the MFMA's internal
accumulation. The integer family has NO tolerance: the f32 store, and the residual add with alpha = 1/2 onto an
integer base, must EQUAL the reference. Single elements (the dequant kernel, ops.embed, the one-hot columns) are
within ELEM_REL * mag + ELEM_ABS, the f16 roundings of the element's own terms, and equal on the integer family.
f16 epilogues, full family: SwiGLU is judged on its output with B propagated through the derivative of
silu(g) * u (test_swiglu_epilogue_full); the fused-norm GEMV is judged like every other
path, against the product of the fp64-normed, f16-rounded activations (test_fused_norm_gemv_full).

Largest ratio measured on the MI355X by the GPU tests below, in units of 1e-4 (TOL 6.8 full / 4.6 tiny_d), as
full / tiny_d; A = mode 0 and B = mode 1 over the five CFGS at M = 1 .. 64 (200 rows), BL = mode 1 at M = 65 / 300
(264 rows, as modes 2, 3, 9, 10), moe = mapped MoE down projection on path A | mode 1 | mode 3:

  type     A          B          BL         mode 2     mode 3     mode 9     mode 10    moe
  Q4_K     1.20/1.04  1.20/1.04  1.22/1.14  1.22/1.14  1.22/1.14  1.22/1.14  1.22/1.13  1.12|1.38|1.38 / 1.15|1.39|1.39
  Q5_K     1.04/0.98  1.04/0.98  1.12/1.15  1.12/1.15  1.12/1.15  1.12/1.15  -          1.32|1.40|1.40 / 1.22|1.75|1.75
  Q6_K     1.09/1.10  1.09/1.10  1.20/0.99  1.20/0.99  1.20/0.99  1.20/0.99  1.20/0.99  -
  Q8_0     0.83/0.58  0.83/0.58  0.93/0.65  0.93/0.65  -          0.93/0.65  -          -
  F16      0.00       0.00       -          -          -          -          -          -
  BF16     0.00       0.00       -          -          -          -          -          -
  F32      1.04       1.04       -          -          -          -          -          -
  Q4_0     0.22       0.22       -          -          -          0.23       -          -
  Q4_1     0.76       0.76       -          -          -          -          -          -
  Q5_0     0.20       0.20       -          -          -          -          -          -
  Q5_1     0.73       0.73       -          -          -          0.84       -          -
  Q3_K     1.06/0.81  1.06/0.81  -          -          -          1.26/1.07  -          -
  Q2_K     0.72/0.49  0.72/0.49  -          -          -          -          -          -
  IQ4_NL   0.99       0.99       -          -          -          1.16       -          -
  IQ4_XS   1.29       1.29       -          -          -          1.46       -          1.42|1.67|- (full)
  mixed launches (full): type-set 3 (Q4_0 + Q6_K + Q5_1 + Q8_0) 1.00, type-set 4 (IQ4_XS + Q6_K + Q5_K + Q8_0 + IQ4_NL) 1.06

  SwiGLU (full; Q4_K, Q6_K, Q5_1, IQ4_XS over the five CFGS): at most 0.13 of the propagated bound; fused-norm GEMV
  (full; Q4_K, Q6_K, Q8_0): 1.07
  SwiGLU, integer family on modes 2 / 3 / 9 (Q4_K, Q5_K, Q6_K; M 65 / 300, mode 9 also 256; test_swiglu_epilogue_integer): g and u
  exact, every output within 0.992 of half an f16 ulp plus 4 x the emulated silu error (tests/dense_ref.py)

Every correct kernel stays within 0.4 TOL, at the emulated noise itself. The integer family was bit-exact on EVERY
path of the table (f32 store and residual add; paths A and B, modes 2, 3, 9, 10, the mapped MoE launches): the MFMA
adds exactly representable fp32 integers exactly, in every split-K order. The dequant kernel's output is moreover
bit-identical to qblocks.emulate on every (type, family) -- the emulation IS the kernels' dequantisation, and
test_dequant_kernel_families asserts the identity, next to the wider element bound. No kernel
or transcode.py fault was found: the Q3_K -> Q6_K and the legacy -> Q51 re-encodings are right with negative scales
and negative d.

Mode 2 takes 8 waves only: of the (waves, rt, ks) triples (8, 1, 1), (4, 2, 1), (8, 1, 3) the first and the last run
on mode 2 (rt = 1: 64-row activation blocks), next to the (wm, ks) of test_qgemm_lds; (4, 2, 1), which the dispatcher
refuses there, runs where test_qgemm_large_m runs all three, on path B at large M (test_path_b_large_m_families).

Fault models (test_fault_models_are_rejected: applied to the reference decode at M = 1, each is rejected by >= 10x
its tolerance by full or tiny_d -- the weakest: 11x, one 8-value fragment of Q5_0 -- and changes integer outputs).
Localised ones sit in super-block 1, K-step 3, lane group 2:
  W1 d (and dmin) of the neighbouring row of the tile      W2 d / dmin of the neighbouring super-block
  W3 two sub-block (scale, min) pairs swapped              W4 top two bits of the 6-bit scales / mins of sub-blocks
  W5 int8 scale read unsigned; sign of d dropped              4..7 dropped or exchanged; Q3_K / IQ4_XS high bits dropped
  W6 one 8-value fragment dropped, doubled, or of the      W7 high-bit plane shifted by one K-step
     adjacent K-step                                       W8 a super-block in two split-K slabs, or in none
  W9 an output row from the next weight row; the zero tail rows of the last tile in place of its real rows
Pairs at which the fault cannot change the result, hence not in EXPECTED_FAULTS: W1 - W5 and W7 on F16 / BF16 / F32
(no scales, no planes: only W6, W8 and W9, the placement of fragments, slabs and rows); W4 without split scale fields (Q6_K,
Q8_0, Q2_K, the 32-value block formats, IQ4_NL); W5 where d is never negative and the scales are unsigned (Q4_K, Q5_K,
Q2_K, Q4_1, Q5_1); W7 without a high-bit plane, or with an all-zero one (Q4_K, Q8_0, Q2_K, IQ4, Q4_0 / Q4_1 as Q51).
"""
import functools

import numpy as np
import pytest
import torch

import dense_ref as DR
import qblocks as QB
from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType as T

ROWS, K = 200, 768              # 12 full tiles + an 8-row tail; 3 super-blocks: ks = 2 uneven, ks = 3 one per slab
ROWS_L = 264                    # the large-M paths' rows (a partial last 128 / 256-row weight tile)
XROWS = 320
ALL = list(QB.ALL_TYPES)
ONE_D = [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0, T.Q3_K, T.Q2_K, T.IQ4_XS]      # random_blocks: ONE d per tensor
EMU = {"full": 1.7e-4, "tiny_d": 1.15e-4}      # largest emulated ratios (test_emulated_noise_bounds_tol)
TOL = {f: 4 * v for f, v in EMU.items()}
# one element against the reference decode: the f16 roundings of a = d*sc and of c = dmin*m, 2^-12 of each term,
# and of the value, 2^-12 of at most |a*q| + |c| (half an ulp each); below the normal range half an ulp is 2^-25
ELEM_REL, ELEM_ABS = 2.0 ** -10, 3 * 2.0 ** -25
CFGS = [(0, 8, 1, 1), (0, 4, 2, 1), (1, 8, 1, 1), (1, 4, 2, 2), (1, 8, 1, 4)]      # test_qgemv_types
Q9_TYPES = [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0, T.Q4_0, T.Q5_1, T.Q3_K]


def _seed(t, fam, rows):
    return 1000 * int(t) + 10 * QB.FAMILIES.index(fam) + rows


@functools.lru_cache(maxsize=None)
def _acts(fam, k=K, seed=1):
    """f16 activations [XROWS, k] (shared, read-only): the suite's Gaussian rows, or {-1, 0, 1} for integer."""
    g = torch.Generator().manual_seed(seed)
    if fam == "integer":
        return (torch.randint(0, 3, (XROWS, k), generator=g) - 1).to(ops.ACT_DTYPE)
    return torch.randn(XROWS, k, generator=g).to(ops.ACT_DTYPE)


def _case(t, fam, rows=ROWS, k=K, seed=None):
    return _case_of(t, fam, rows, k, seed)      # one cache key per case, however it is asked for


@functools.lru_cache(maxsize=None)
def _case_of(t, fam, rows, k, seed):
    """Weights of one (type, family) with everything the reference side needs (shared, read-only): raw bytes,
    fields, W = the numpy decode of the ORIGINAL bytes, mag, x, ref = x @ W^T in fp64 and B = |x| @ mag^T."""
    rng = np.random.default_rng(_seed(t, fam, rows) if seed is None else seed)
    raw = QB.structured_blocks(t, rows, k, fam, rng)
    return _ref_case(t, fam, raw, rows, k)


def _ref_case(t, fam, raw, rows, k):
    f = QB.fields(t, raw, rows, k)
    W = Q.dequantize(raw, t, (rows, k)).astype(np.float64)
    Wf, mag = QB.decode(f)
    x = _acts(fam, k)
    xd = x.double().numpy()
    return dict(t=t, fam=fam, raw=raw, f=f, W=W, Wf=Wf, mag=mag, x=x, ref=xd @ W.T, B=np.abs(xd) @ mag.T, rows=rows,
                K=k)


def _ratio(y, c, M, rows=slice(None)):
    """|y - ref| / B per output element: every output against its own dot-product size."""
    y = np.asarray(y, np.float64)
    r = np.abs(y - c["ref"][:M, rows]) / c["B"][:M, rows]
    return np.where(np.isfinite(r), r, np.inf)


# ------------------------------------------------------------------------------------------------------ CPU tests

@pytest.mark.parametrize("t", ALL, ids=lambda t: t.name)
def test_families_use_every_field(t):
    """The generator's contract: the field-level decode is the numpy codec's; full covers every legal value of
    every scale field and both signs of d; tiny_d is below the f16 normal range; integer is exact in f16 (the
    emulated kernel arithmetic IS the reference), its partial sums exact in fp32, neighbouring cells differ."""
    for fam in QB.families_of(t):
        c = _case(t, fam)
        f = c["f"]
        assert np.abs(c["Wf"] - c["W"]).max() <= 2.0 ** -22 * c["mag"].max(), fam
        assert (np.abs(c["Wf"] - c["W"]) <= 2.0 ** -22 * c["mag"]).all(), fam
        d = np.abs(f["d"])
        if t in QB.FLOATS:          # no fields: the values themselves, integer ones exact in f16
            assert fam == "full" or (QB.emulate(f) == c["W"]).all()
        elif fam == "full":
            lim = {T.Q4_K: (0, 63), T.Q5_K: (0, 63), T.Q6_K: (-128, 127), T.Q3_K: (-32, 31), T.Q2_K: (0, 15),
                   T.IQ4_XS: (-32, 31)}
            if t in lim:
                assert set(np.unique(f["sc"])) == set(range(lim[t][0], lim[t][1] + 1))
            if t in QB.K4 or t == T.Q2_K:
                assert set(np.unique(f["m"])) == set(range(0, 64 if t in QB.K4 else 16))
            assert d.min() >= 2.0 ** -14.01 and d.max() <= 2.0 ** -4.99 and d.max() / d.min() > 256
            assert ((f["d"] < 0).any() and (f["d"] > 0).any()) == (t in QB.SIGNED_D)
            assert len(np.unique(f["d"])) > f["d"].size // 4
            if t in (T.Q4_1, T.Q5_1):
                assert abs(np.corrcoef(np.log2(d).ravel(), np.log2(np.abs(f["dmin"])).ravel())[0, 1]) < 0.1
                assert (f["dmin"] < 0).any() and (f["dmin"] > 0).any()
        elif fam == "tiny_d":
            assert d.max() < 2.0 ** -14 and d.min() >= 2.0 ** -20.01
        else:
            assert (QB.emulate(f) == c["W"]).all()
            assert float((np.abs(c["x"].double().numpy()) @ np.abs(c["W"]).T).max()) * 8 < 2.0 ** 24      # unit 2^-3
            a, cc = QB.scale_terms(f)
            key = a + 1j * cc                                   # the (scale, min) pair of a sub-block
            for u, v in ((key[0::2], key[1::2]), (key[:, :-1], key[:, 1:])):      # tile neighbour, K neighbour
                assert (u != v).any(axis=2).all()
            if f["d"].shape[2] == 1:
                assert (f["d"][0::2] != f["d"][1::2]).all() and (f["d"][:, :-1] != f["d"][:, 1:]).all()
                if f["dmin"] is not None:
                    assert (f["dmin"][0::2] != f["dmin"][1::2]).all() and (f["dmin"][:, :-1] != f["dmin"][:, 1:]).all()
            assert all(len(np.unique(p)) == p.size for p in key.reshape(-1, key.shape[2]))


def _emulated_ratio(t, fam):
    c = _case(t, fam)
    y = c["x"].float().numpy() @ QB.emulate(c["f"]).astype(np.float32).T          # f16 operands, fp32 sum
    return float(_ratio(y, c, XROWS).max())


def test_emulated_noise_bounds_tol():
    """EMU[family] is the largest ratio of the emulated kernel arithmetic (f16 d*sc and dmin*m, one f16 rounding of
    the value, f16 x, fp32 sum; the load-time roundings of IQ4_XS / Q2_K) over this module's inputs, within a factor
    2 below the constant: it is the measurement, not a guess."""
    for fam in EMU:
        per = {t.name: _emulated_ratio(t, fam) for t in ALL if fam in QB.families_of(t)}
        print(f"emulated noise {fam}: " + " ".join(f"{k}={v:.2e}" for k, v in per.items()))
        worst = max(per.values())
        assert EMU[fam] / 2 <= worst <= EMU[fam], (fam, worst)


# fragment of the localised faults: super-block 1, K-step 3, lane group 2 (csrc/kernels/common.h: k = 32t + 8g)
F_SB, F_T, F_G = 1, 3, 2
F_K0 = 256 * F_SB + 32 * F_T + 8 * F_G


def _hi_plane(f):
    """(unsigned quant values, bits below the high-bit plane) of the device formats that keep one, else None."""
    t = f["t"]
    if t in (T.Q5_K, T.Q5_0, T.Q5_1):
        return f["q"], 4, 0
    if t in (T.Q6_K, T.Q3_K):              # Q3_K runs as Q6_K with q6 = q3 + 28
        return f["q"] + 32, 4, 32
    return None


def _faults(f):
    """(name, faulty W) for every fault model that can change the result of this format (module docstring)."""
    t = f["t"]
    W = QB.decode(f)[0]
    R, nb = f["q"].shape[:2]
    dec = lambda **kw: QB.decode({**f, **kw})[0]
    both = lambda fn: {k: fn(f[k]) for k in ("d", "dmin") if f[k] is not None}
    nbr = np.arange(R) ^ 1
    if t in QB.FLOATS:          # no scales: only the placement of fragments, slabs and rows can go wrong
        yield from _placement_faults(W, R)
        return
    yield "W1 d/dmin of the neighbouring row of the tile", dec(**both(lambda v: v[nbr]))
    yield "W2 d/dmin of the neighbouring super-block", dec(**both(lambda v: np.roll(v, -1, axis=1)))
    per_sub = ("d", "dmin") if f["d"].shape[2] > 1 else ("sc", "m")       # what a sub-block's (scale, min) pair is
    S = f["sc"].shape[2]
    i, j = (1, 6) if S == 8 else (2, 13)
    sw = {}
    for k in per_sub:
        if f[k] is not None:
            sw[k] = f[k].copy()
            sw[k][:, F_SB, [i, j]] = f[k][:, F_SB, [j, i]]
    yield f"W3 (scale, min) pairs of sub-blocks {i} and {j} swapped", dec(**sw)
    if t in QB.K4:
        sc, m = f["sc"].copy(), f["m"].copy()
        sc[:, F_SB, 4:], m[:, F_SB, 4:] = sc[:, F_SB, 4:] & 15, m[:, F_SB, 4:] & 15
        yield "W4 top bits of scales / mins 4..7 dropped", dec(sc=sc, m=m)
        sc, m = f["sc"].copy(), f["m"].copy()
        sc[:, F_SB, 4:] = (f["sc"][:, F_SB, 4:] & 15) | (f["m"][:, F_SB, 4:] & 48)
        m[:, F_SB, 4:] = (f["m"][:, F_SB, 4:] & 15) | (f["sc"][:, F_SB, 4:] & 48)
        yield "W4 top bits of scales and mins 4..7 exchanged", dec(sc=sc, m=m)
    if t in (T.Q3_K, T.IQ4_XS):
        sc = f["sc"].copy()
        sc[:, F_SB] = ((sc[:, F_SB] + 32) & 15) - 32
        yield "W4 high scale bits dropped", dec(sc=sc)
    if t in (T.Q6_K, T.Q3_K):
        yield "W5 int8 scale read unsigned", dec(sc=f["sc"] & 255)
    if t in QB.SIGNED_D:
        yield "W5 sign of d dropped", dec(d=np.abs(f["d"]))
    hp = _hi_plane(f)
    if hp is not None:
        u, bits, off = hp
        u = u.astype(np.int64)
        hi = (u >> bits).reshape(R, nb, 8, 32)
        hi[:, F_SB] = np.roll(hi[:, F_SB], -1, axis=1)
        yield "W7 high-bit plane shifted by one K-step", dec(q=((u & 15) | (hi.reshape(R, nb, 256) << bits)) - float(off))
    yield from _placement_faults(W, R)


def _placement_faults(W, R):
    for name, frag in (("dropped", 0 * W[:, F_K0:F_K0 + 8]), ("doubled", 2 * W[:, F_K0:F_K0 + 8]),
                       ("of the next K-step", W[:, F_K0 + 32:F_K0 + 40])):
        Wf = W.copy()
        Wf[:, F_K0:F_K0 + 8] = frag
        yield f"W6 8-value fragment {name}", Wf
    for name, fac in (("in two split-K slabs", 2.0), ("in no split-K slab", 0.0)):
        Wf = W.copy()
        Wf[:, 256 * F_SB:256 * F_SB + 256] *= fac
        yield f"W8 super-block {name}", Wf
    yield "W9 output row from the next weight row", np.roll(W, -1, axis=0)
    Wf = W.copy()
    Wf[R // 16 * 16:] = 0.0
    yield "W9 zero tail rows of the last tile in place of its real rows", Wf


EXPECTED_FAULTS = {      # fault models per format; the pairs left out cannot change the result (module docstring)
    T.Q4_K: "W1 W2 W3 W4 W6 W8 W9", T.Q5_K: "W1 W2 W3 W4 W6 W7 W8 W9", T.Q6_K: "W1 W2 W3 W5 W6 W7 W8 W9",
    T.Q8_0: "W1 W2 W3 W5 W6 W8 W9", T.Q4_0: "W1 W2 W3 W5 W6 W8 W9", T.Q4_1: "W1 W2 W3 W6 W8 W9",
    T.Q5_0: "W1 W2 W3 W5 W6 W7 W8 W9", T.Q5_1: "W1 W2 W3 W6 W7 W8 W9", T.Q3_K: "W1 W2 W3 W4 W5 W6 W7 W8 W9",
    T.Q2_K: "W1 W2 W3 W6 W8 W9", T.F16: "W6 W8 W9", T.BF16: "W6 W8 W9", T.F32: "W6 W8 W9", T.IQ4_NL: "W1 W2 W3 W5 W6 W8 W9", T.IQ4_XS: "W1 W2 W3 W4 W5 W6 W8 W9"}


@pytest.mark.parametrize("t", ALL, ids=lambda t: t.name)
def test_fault_models_are_rejected(t):
    """Every fault model, applied to the reference decode, at M = 1: at least one of full / tiny_d exceeds its
    tolerance by >= 10x, and the integer family's output differs -- using the reference alone."""
    res = {}
    for fam in QB.families_of(t):
        c = _case(t, fam)
        x0 = c["x"][:1].double().numpy()
        for name, Wf in _faults(c["f"]):
            y = x0 @ Wf.T
            res.setdefault(name, {})[fam] = (float((y != c["ref"][:1]).sum()) if fam == "integer"
                                             else float(_ratio(y, c, 1).max()) / TOL[fam])
    assert sorted({n[:2] for n in res}) == EXPECTED_FAULTS[t].split()
    for name, by in res.items():
        worst = max(v for k, v in by.items() if k != "integer")
        print(f"{t.name} {name}: rejected by {worst:.0f}x tolerance; integer outputs that differ: {by['integer']:.0f}")
        assert worst >= 10.0, (name, by)
        assert by["integer"] > 0, name


@pytest.mark.parametrize("t", ONE_D, ids=lambda t: t.name)
def test_random_blocks_cannot_see_scale_faults(t):
    """The gap the families close: on gguf.quants.random_blocks weights (one d per tensor, positive scales) W1,
    W2 and W5 leave every weight bit-identical, so no test on them can notice these faults."""
    raw = Q.random_blocks(t, ROWS * K, 0.05, np.random.default_rng(0))
    f = QB.fields(t, raw, ROWS, K)
    W = QB.decode(f)[0]
    assert len(np.unique(f["d"])) == 1
    seen = 0
    for name, Wf in _faults(f):
        if name[:2] in ("W1", "W2", "W5"):
            assert (Wf == W).all(), name
            seen += 1
    assert seen >= 2


# ------------------------------------------------------------------------------------------------------ GPU tests

class _Bank:
    """Device copies of the shared cases (weights as QWeight, activations), made once per module."""

    def __init__(self, dev):
        self.dev, self._w, self._x = dev, {}, {}

    def w(self, c, layout="tiled"):
        key = (id(c), layout)
        if key not in self._w:
            self._w[key] = ops.QWeight(c["raw"], c["t"], c["rows"], c["K"], self.dev, layout=layout)
        return self._w[key]

    def x(self, fam, k=K):
        if (fam, k) not in self._x:
            self._x[fam, k] = _acts(fam, k).to(self.dev)
        return self._x[fam, k]


@pytest.fixture(scope="module")
def bank(gpu):
    return _Bank(gpu)


def _where(c, m, n):
    return f"token {m}, weight row {n} (tile {n // 16}, row {n % 16} of it)"


def _check(tag, y, ref, B, fam, tname, what=lambda m, n: f"token {m}, output {n}"):
    """Outputs y against ref: the integer family must be EQUAL, the others within TOL of their own dot-product
    size B; prints the figure of the module docstring's table."""
    y = y.double().cpu().numpy()
    if fam == "integer":
        bad = np.argwhere(y != ref)
        print(f"WQ_RATIO {tag} {tname} integer exact={len(bad) == 0}")
        assert len(bad) == 0, (tag, tname, f"{len(bad)} outputs differ from the exact result",
                               [(what(m, n), y[m, n], ref[m, n]) for m, n in bad[:4]])
        return
    r = np.abs(y - ref) / B
    r = np.where(np.isfinite(r), r, np.inf)
    m, n = np.unravel_index(np.argmax(r), r.shape)
    print(f"WQ_RATIO {tag} {tname} {fam} {r[m, n]:.3e}")
    assert r[m, n] <= TOL[fam], (tag, tname, fam, f"ratio {r[m, n]:.3e} > {TOL[fam]:.1e} at " + what(m, n))


def _run_plain(bank, tag, t, rows, Ms, **cfg):
    """Every family of type t through one launch config at each M: f32 store, and for the integer family the
    residual add with alpha = 1/2 onto an integer base (exact as well)."""
    for fam in QB.families_of(t):
        c = _case(t, fam, rows)
        w, x = bank.w(c), bank.x(fam)
        for M in Ms:
            y = torch.full((XROWS, rows), 3.0, device=bank.dev)
            ops.qgemv([ops.Seg(w)], x, y, M, **cfg)
            _check(f"{tag} M={M}", y[:M], c["ref"][:M], c["B"][:M], fam, t.name, lambda m, n: _where(c, m, n))
            assert float(y[M:].min()) == 3.0 and float(y[M:].max()) == 3.0, "rows past M were written"
            if fam == "integer":
                base = torch.randint(-1000, 1001, (XROWS, rows), generator=torch.Generator().manual_seed(M)).float()
                y = base.to(bank.dev)
                ops.qgemv([ops.Seg(w)], x, y, M, alpha=0.5, epi="add", **cfg)
                _check(f"{tag} add M={M}", y[:M], base[:M].double().numpy() + 0.5 * c["ref"][:M], None, fam, t.name,
                       lambda m, n: _where(c, m, n))


@pytest.mark.gpu
@pytest.mark.parametrize("t", ALL, ids=lambda t: t.name)
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "m%dw%dr%dk%d" % c)
def test_gemv_families(gpu, bank, t, cfg):
    """Path A (mode 0) and path B (mode 1), every format: 12 tiles + an 8-row tail, split-K 2 (uneven) and 4."""
    mode, waves, rt, ks = cfg
    _run_plain(bank, "m%d/w%d/rt%d/ks%d" % cfg, t, ROWS, [1, 7, 16, 33, 64], mode=mode, waves=waves, rt=rt, ks=ks)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0], ids=lambda t: t.name)
@pytest.mark.parametrize("wr", [(8, 1, 1), (4, 2, 1), (8, 1, 3)], ids=lambda c: "w%dr%dk%d" % c)
def test_path_b_large_m_families(gpu, bank, t, wr):
    """Path B at prefill sizes with the (waves, rt, ks) of test_qgemm_large_m: where (4, 2, 1) runs, which mode 2
    refuses (8 waves only); (8, 1, 1) and (8, 1, 3) run on mode 2 as well (test_lds_gemm_families)."""
    _run_plain(bank, "m1L/w%d/rt%d/ks%d" % wr, t, ROWS_L, [65, 300], mode=1, waves=wr[0], rt=wr[1], ks=wr[2])


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0], ids=lambda t: t.name)
@pytest.mark.parametrize("wm,ks", [(1, 1), (1, 3), (4, 1), (2, 1), (4, 3)])
def test_lds_gemm_families(gpu, bank, t, wm, ks):
    """Mode 2 (LDS dequant; 8 waves, rt = wm waves along M): the triples (8, 1, 1) and (8, 1, 3) -- 64-row
    activation blocks, ks = 3 one super-block per slab -- and the (wm, ks) of test_qgemm_lds."""
    _run_plain(bank, f"m2/rt{wm}/ks{ks}", t, ROWS_L, [65, 300], mode=2, waves=8, rt=wm, ks=ks)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q4_K, T.Q5_K, T.Q6_K], ids=lambda t: t.name)
@pytest.mark.parametrize("mt,ks", [(16, 1), (8, 2), (6, 1), (4, 3)])
def test_dma_gemm_families(gpu, bank, t, mt, ks):
    """Mode 3 (LDS-DMA of the raw tile-blocks): ks = 2 is the uneven split of 3 super-blocks."""
    _run_plain(bank, f"m3/rt{mt}/ks{ks}", t, ROWS_L, [65, 300], mode=3, waves=4, rt=mt, ks=ks)


@pytest.mark.gpu
@pytest.mark.parametrize("t", Q9_TYPES + [T.IQ4_NL, T.IQ4_XS], ids=lambda t: t.name)
@pytest.mark.parametrize("cfg", [(8, 2, 1), (8, 1, 2)], ids=lambda c: "w%dr%dk%d" % c)
def test_q9_gemm_families(gpu, bank, t, cfg):
    """Mode 9 (raw tile-blocks DMA'd per super-block, weights as the MFMA A operand)."""
    _run_plain(bank, "m9/w%d/rt%d/ks%d" % cfg, t, ROWS_L, [256, 300], mode=9, waves=cfg[0], rt=cfg[1], ks=cfg[2])


def _elem_check(tag, v, c, rows, cols, what):
    """Dequantised elements v [len(rows), len(cols)] against the reference decode: integer EQUAL, else within the
    f16 roundings of the element's own terms (ELEM_REL * mag + ELEM_ABS)."""
    v = np.asarray(v, np.float64)
    W, mag = c["W"][np.ix_(rows, cols)], c["mag"][np.ix_(rows, cols)]
    err = np.abs(v - W)
    lim = np.zeros_like(mag) if c["fam"] == "integer" else ELEM_REL * mag + ELEM_ABS
    over = np.where(np.isfinite(err), err, np.inf) - lim
    i, j = np.unravel_index(np.argmax(over), over.shape)
    print(f"WQ_ELEM {tag} {c['t'].name} {c['fam']} worst err/mag {float((err / np.maximum(mag, 1e-30)).max()):.3e}")
    assert over[i, j] <= 0, (tag, c["t"].name, c["fam"], what(rows[i], cols[j]), v[i, j], W[i, j])


def _kpos(k):
    return f"super-block {k // 256}, K-step {k % 256 // 32}, lane group {k % 32 // 8}, element {k % 8}"


@pytest.mark.gpu
@pytest.mark.parametrize("t", ALL, ids=lambda t: t.name)
def test_dequant_kernel_families(gpu, bank, t):
    """w.dense(), the root of the production oracle and of every f16 copy, element by element."""
    for fam in QB.families_of(t):
        c = _case(t, fam)
        d = bank.w(c).dense().cpu().numpy()
        emu = QB.emulate(c["f"])
        bad = np.argwhere(d != emu)
        print(f"WQ_DEQ {t.name} {fam} bit-identical to the emulation: {len(bad) == 0}")
        assert len(bad) == 0, (t.name, fam, f"{len(bad)} elements differ from the emulated f16 value",
                               [(f"row {n}, {_kpos(k)}", d[n, k], emu[n, k]) for n, k in bad[:4]])
        _elem_check("dequant", d, c, np.arange(ROWS), np.arange(K), lambda n, k: f"row {n}, {_kpos(k)}")


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q4_K, T.Q6_K], ids=lambda t: t.name)
def test_dense_copy_families(gpu, t):
    """Mode 10 on the f16 copy (the dequant kernel's output)."""
    for fam in QB.families_of(t):
        c = _case(t, fam, ROWS_L)
        w = ops.QWeight(c["raw"], t, ROWS_L, K, gpu)
        w.expand_dense()
        y = torch.zeros(XROWS, ROWS_L, device=gpu)
        ops.qgemv([ops.Seg(w)], _acts(fam).to(gpu), y, 300, mode=10, waves=8, rt=1, ks=1)
        _check("m10/rt1/ks1 M=300", y[:300], c["ref"][:300], c["B"][:300], fam, t.name, lambda m, n: _where(c, m, n))


@pytest.mark.gpu
@pytest.mark.parametrize("t", ALL, ids=lambda t: t.name)
def test_embed_families(gpu, bank, t):
    """ops.embed (the scalar decode of the "rows" layout): the first row, the last one and a row of the tail tile,
    scaled by 2 (exact)."""
    rows = [0, ROWS - 1, ROWS - 5]
    for fam in QB.families_of(t):
        c = _case(t, fam)
        qw = bank.w(c, "rows")
        e = torch.zeros(3, K, device=gpu)
        ops.embed(torch.tensor(rows, dtype=torch.int32, device=gpu), qw, e, 3, 2.0)
        _elem_check("embed", e.cpu().numpy() / 2.0, c, np.array(rows), np.arange(K), lambda n, k: f"row {n}, {_kpos(k)}")


@pytest.mark.gpu
@pytest.mark.parametrize("t", ALL, ids=lambda t: t.name)
@pytest.mark.parametrize("cfg", [CFGS[0], CFGS[2]], ids=lambda c: "m%dw%dr%dk%d" % c)
def test_one_hot_columns(gpu, bank, t, cfg):
    """Row m of x is 1 at column k_m and 0 elsewhere, the k_m walking all 256 positions of each super-block over
    12 launches: the output IS the dequantised column, which localises a fault to its (K-step, lane group)."""
    mode, waves, rt, ks = cfg
    eye = torch.eye(K, dtype=ops.ACT_DTYPE, device=gpu)
    for fam in QB.families_of(t):
        c = _case(t, fam)
        w = bank.w(c)
        y = torch.zeros(K, ROWS, device=gpu)
        for k0 in range(0, K, 64):
            ops.qgemv([ops.Seg(w)], eye[k0:k0 + 64], y[k0:k0 + 64], 64, mode=mode, waves=waves, rt=rt, ks=ks)
        _elem_check(f"one-hot m{mode}", y.cpu().numpy().T, c, np.arange(ROWS), np.arange(K),
                    lambda n, k: f"row {n} (row {n % 16} of its tile), {_kpos(k)}")


def _mixed(gpu, bank, layout, kset):
    Kx = 512
    for M in (3, 40):
        cs = [_case(t, "full", r, Kx, seed=50 + i) for i, (t, r) in enumerate(layout)]
        ws = [bank.w(c) for c in cs]
        assert ops.kernel_set([w.type for w in ws]) == kset
        cols = np.cumsum([0] + [r for _, r in layout])
        y = torch.zeros(64, int(cols[-1]), device=gpu)
        ops.qgemv([ops.Seg(w, int(c0)) for w, c0 in zip(ws, cols)], bank.x("full", Kx), y, M)
        names = [f"{t.name}[{r}]" for t, r in layout]
        _check(f"mixed set {kset} M={M}", y[:M], np.concatenate([c["ref"][:M] for c in cs], axis=1),
               np.concatenate([c["B"][:M] for c in cs], axis=1), "full", "+".join(names),
               lambda m, n: f"token {m}, output {n} (segment {names[int(np.searchsorted(cols, n, 'right')) - 1]})")


@pytest.mark.gpu
def test_mixed_q51_segments_full(gpu, bank):
    """The layout of test_q51_mixed_with_q6k_q8_segments (kernel type-set 3) on the full family."""
    _mixed(gpu, bank, [(T.Q4_0, 64), (T.Q6_K, 48), (T.Q5_1, 32), (T.Q8_0, 16)], 3)


@pytest.mark.gpu
def test_mixed_iq4_segments_full(gpu, bank):
    """The layout of test_iq4_mixed_segments (kernel type-set 4) on the full family."""
    _mixed(gpu, bank, [(T.IQ4_XS, 64), (T.Q6_K, 48), (T.Q5_K, 32), (T.Q8_0, 16), (T.IQ4_NL, 32)], 4)


@pytest.mark.gpu
@pytest.mark.parametrize("qt,Tn,mode,waves,rt", [(qt, *c) for qt in (T.Q4_K, T.Q5_K, T.IQ4_XS)
                                                 for c in ((10, 0, 4, 2), (40, 1, 8, 2), (40, 3, 4, 4))
                                                 if not (qt == T.IQ4_XS and c[1] == 3)],      # IQ4: paths A and B only
                         ids=lambda v: v.name if isinstance(v, T) else str(v))
def test_mapped_moe_down_families(gpu, bank, qt, Tn, mode, waves, rt):
    """Mapped MoE rows, the down projection (f32 store) of test_qgemm_mapped_moe: one path-A, one mode-1 and one
    mode-3 launch over 4 experts, each expert its own weights, every routed row against its expert."""
    E, k, Kd, F = 4, 2, 512, 256
    logits = torch.randn(Tn, E, generator=torch.Generator().manual_seed(Tn)).to(gpu)
    topw = torch.zeros(Tn * k, device=gpu)
    counts = torch.zeros(E, dtype=torch.int32, device=gpu)
    xrows = torch.zeros(E * Tn, dtype=torch.int32, device=gpu)
    yrows = torch.zeros(E * Tn, dtype=torch.int32, device=gpu)
    ops.moe_route(logits, Tn, k, topw, counts, xrows, yrows, Tn)
    cnt, yr = counts.cpu(), yrows.cpu()
    assert int(cnt.sum()) == Tn * k
    for fam in QB.families_of(qt):
        cs = [_case(qt, fam, Kd, F, seed=70 + e) for e in range(E)]
        segs = [ops.Seg(bank.w(cs[e]), 0, yrows[e * Tn:], yrows[e * Tn:], counts[e:e + 1]) for e in range(E)]
        y = torch.full((Tn * k, Kd), 5.0, device=gpu)
        ops.qgemv(segs, bank.x(fam, F), y, Tn, epi="f32", mode=mode, waves=waves, rt=rt, ks=1)
        for e in range(E):
            yi = yr[e * Tn:e * Tn + int(cnt[e])].long().numpy()
            _check(f"moe m{mode}/w{waves}/rt{rt} T={Tn}", y[yi], cs[e]["ref"][yi], cs[e]["B"][yi], fam, qt.name,
                   lambda m, n: f"expert {e}, routed row {yi[m]}, weight row {n}")


SWIGLU_ALPHA = 2.0 ** -6        # keeps silu(g) * u of the full family inside f16 (exact scaling of both products)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q4_K, T.Q6_K, T.Q5_1, T.IQ4_XS], ids=lambda t: t.name)
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "m%dw%dr%dk%d" % c)
def test_swiglu_epilogue_full(gpu, bank, t, cfg):
    """The f16 SwiGLU epilogue on the full family, B propagated through the epilogue's derivative: with the gate
    and up products g, u each within TOL * B of their reference, silu(g) * u is within
    TOL * (|silu'(g)| |u| B_g + |silu(g)| B_u) + TOL^2 B_g B_u / 2 of silu(g) u (silu'' <= 1/2), plus the f16
    rounding of the output, 2^-11 of it. 400 interleaved rows: gate rows 16i .. 16i + 7 of a tile, up rows the other 8."""
    mode, waves, rt, ks = cfg
    c = _case(t, "full", 400)
    gi = (np.arange(200) // 8) * 16 + np.arange(200) % 8
    for M in (1, 33):
        y = torch.zeros(64, 200, dtype=ops.ACT_DTYPE, device=gpu)
        ops.qgemv([ops.Seg(bank.w(c))], bank.x("full"), y, M, alpha=SWIGLU_ALPHA, epi="swiglu", mode=mode, waves=waves,
                  rt=rt, ks=ks)
        g, u = SWIGLU_ALPHA * c["ref"][:M, gi], SWIGLU_ALPHA * c["ref"][:M, gi + 8]
        Bg, Bu = SWIGLU_ALPHA * c["B"][:M, gi], SWIGLU_ALPHA * c["B"][:M, gi + 8]
        sg = 1.0 / (1.0 + np.exp(-g))
        ref = g * sg * u
        assert np.abs(ref).max() < 60000
        tol = TOL["full"]
        lim = tol * (np.abs(sg * (1 + g * (1 - sg)) * u) * Bg + np.abs(g * sg) * Bu) + tol * tol * Bg * Bu / 2 \
            + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
        r = np.abs(y[:M].double().cpu().numpy() - ref) / lim
        r = np.where(np.isfinite(r), r, np.inf)
        print(f"WQ_SWIGLU m{mode}/w{waves}/rt{rt}/ks{ks} M={M} {t.name} full {r.max():.3f} of the propagated bound")
        assert r.max() <= 1.0, (t.name, cfg, M, np.unravel_index(np.argmax(r), r.shape))


ROWS_S = 304                    # SwiGLU on the large-M paths: two 128-row tiles and a partial one of three 16-row groups
# (mode, waves, rt, ks): mode 2 at 64- and 256-row activation blocks, mode 3 at 16 and 8 tiles, mode 9's two 8-wave
# instances; ks > 1 runs the epilogue in the split-K reduce
SWIGLU_L = [(2, 8, 1, 1), (2, 8, 4, 3), (3, 4, 16, 1), (3, 4, 8, 2), (9, 8, 2, 1), (9, 8, 1, 2)]


@functools.lru_cache(maxsize=None)
def _swiglu_int(t):
    """The integer family behind the SwiGLU epilogue: (case, activations as float64, alpha). Rows are read as
    interleaved [g0..g7, u0..u7]; alpha is the power of two that keeps every |g|, |u| <= 16, from the reference."""
    c = _case(t, "integer", ROWS_S)
    return c, c["x"].double().numpy(), 2.0 ** np.floor(np.log2(16.0 / np.abs(c["ref"]).max()))


def test_swiglu_integer_inputs():
    """The judgement of test_swiglu_epilogue_integer rests on exact g and u (integer family: |alpha ref| <= 16, a
    power-of-two alpha) and on the emulated fp32 silu error dense_ref.SILU_EMU, which these inputs stay under."""
    gi = DR.interleaved(ROWS_S)
    for t in (T.Q4_K, T.Q5_K, T.Q6_K):
        c, _, alpha = _swiglu_int(t)
        v = alpha * c["ref"]
        assert np.abs(v).max() <= 16 and (v.astype(np.float32) == v).all()
        g, u = v[:, gi], v[:, gi + 8]
        ref, emu = DR.silu64(g) * u, (DR.silu32(g) * u.astype(np.float32)).astype(np.float64)
        worst = float((np.abs(emu - ref)[ref != 0] / np.abs(ref)[ref != 0]).max())
        print(f"emulated silu(g) u, {t.name} integer: {worst:.2e}")
        assert worst <= DR.SILU_EMU


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q4_K, T.Q5_K, T.Q6_K], ids=lambda t: t.name)
@pytest.mark.parametrize("cfg", SWIGLU_L, ids=lambda c: "m%dw%dr%dk%d" % c)
def test_swiglu_epilogue_integer(gpu, bank, t, cfg):
    """The f16 SwiGLU epilogue of modes 2 / 3 (epi_rows) and 9 (epi_cols4) -- the two epilogues the dense GEMMs
    share -- on the integer family at M 65 / 300 (mode 9 also 256, one whole activation block; at 65 most of its
    block lies past M): g and u are exact, so every output is within half an f16 ulp plus
    4 x the emulated silu error of the fp64 silu(g) u (tests/dense_ref.py, as test_dense_gemm_sensitivity.test_swiglu);
    rows past M and columns past the last output keep the sentinel."""
    mode, waves, rt, ks = cfg
    c, xd, alpha = _swiglu_int(t)
    w, x = bank.w(c), bank.x("integer")
    segs = [(c["W"], 0)]
    for M in (65, 256, 300) if mode == 9 else (65, 300):
        y = torch.full((M + 3, DR.ld_of(segs, "swiglu")), DR.SENT, dtype=ops.ACT_DTYPE, device=gpu)
        ops.qgemv([ops.Seg(w)], x, y, M, alpha=alpha, epi="swiglu", mode=mode, waves=waves, rt=rt, ks=ks)
        ref = DR.run(xd, segs, M, "swiglu", alpha=alpha, nrows=M + 3, silu_tol=DR.SILU_TOL)
        r, i, n = DR.judge(y.cpu().double().numpy(), ref)
        print(f"WQ_SWIGLU_INT m{mode}/w{waves}/rt{rt}/ks{ks} M={M} {t.name} {r:.3f} of the bound")
        assert r <= 1.0, (t.name, cfg, M, f"{n} outputs outside their bound, worst at {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("t", [T.Q4_K, T.Q6_K, T.Q8_0], ids=lambda t: t.name)
def test_fused_norm_gemv_full(gpu, bank, t):
    """Path A with the RMSNorm folded into its activation staging, against the product of the fp64-normed,
    f16-rounded input with the reference decode: the same ratio metric and the same TOL as every other path."""
    c = _case(t, "full")
    g = torch.Generator().manual_seed(5)
    xf = torch.randn(16, K, generator=g) * 3
    nw = 1 + 0.1 * torch.randn(K, generator=g)
    xd = xf.double()
    xn = (xd * torch.rsqrt(xd.pow(2).mean(dim=1, keepdim=True) + 1e-5) * nw.double()).to(ops.ACT_DTYPE).double().numpy()
    for M in (1, 6, 16):
        y = torch.zeros(16, ROWS, device=gpu)
        ops.qgemv([ops.Seg(bank.w(c))], torch.zeros(16, K, dtype=ops.ACT_DTYPE, device=gpu), y, M,
                  norm=(xf.to(gpu), nw.to(gpu), 1e-5), waves=4, rt=2)
        r = np.abs(y[:M].double().cpu().numpy() - xn[:M] @ c["W"].T) / (np.abs(xn[:M]) @ c["mag"].T)
        r = np.where(np.isfinite(r), r, np.inf)
        print(f"WQ_NORM M={M} {t.name} full {r.max():.3e}")
        assert r.max() <= TOL["full"], (t.name, M, np.unravel_index(np.argmax(r), r.shape))


def _fitted_blocks(gt, n, std, rng):
    """Block producer for write_synthetic_gguf: real fits (Q.quantize of Gaussian weights: another d in every
    block, a negative d for about half of the Q4_0 / Q5_0 blocks). The fit of Q6_K only writes scales >= 0, so
    every other Q6_K block gets -sc with -d: the same values with negative int8 scales."""
    raw = Q.quantize(rng.standard_normal(n, dtype=np.float32) * np.float32(std), gt)
    if gt == T.Q6_K:
        b = raw.reshape(-1, 210)
        b[1::2, 192:208] = (-b[1::2, 192:208].view(np.int8)).view(np.uint8)
        b[1::2, 209] ^= 0x80
    return raw


MODEL_CASES = [("tiny-llama", "Q4_K_M"), ("tiny-llama", "Q4_0"), ("tiny-mixtral", "Q4_K_M"), ("tiny-mixtral", "Q4_0")]


@pytest.fixture(scope="module")
def fitted_models(tmp_path_factory):
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    d = tmp_path_factory.mktemp("fitted")
    return {(n, ft): write_synthetic_gguf(str(d / f"{n}-{ft}.gguf"), n, ft, seed=0, blocks=_fitted_blocks)
            for n, ft in MODEL_CASES}


def test_fitted_blocks_have_what_random_blocks_lack():
    rng = np.random.default_rng(0)
    raw6 = _fitted_blocks(T.Q6_K, 64 * 512, 0.02, np.random.default_rng(5))
    f6 = QB.fields(T.Q6_K, raw6, 64, 512)
    assert (f6["sc"] < 0).any() and (f6["sc"] > 0).any() and len(np.unique(f6["d"])) > 64
    x = np.random.default_rng(5).standard_normal(64 * 512, dtype=np.float32) * np.float32(0.02)
    assert (Q.dequantize(raw6, T.Q6_K, (64, 512)) == Q.dequantize(Q.quantize(x, T.Q6_K), T.Q6_K, (64, 512))).all()
    f4 = QB.fields(T.Q4_0, _fitted_blocks(T.Q4_0, 64 * 512, 0.02, rng), 64, 512)
    assert 0.3 < float((f4["d"] < 0).mean()) < 0.7


@pytest.mark.gpu
@pytest.mark.parametrize("name,ft", MODEL_CASES)
def test_fitted_models_match_reference(gpu, fitted_models, name, ft):
    """Whole models on fitted weights, the assertions of test_iq4_models_match_reference: prefill logits vs the
    fp32 oracle of the original GGUF bytes within 5 % (40 tokens: the Mixtral experts run the grouped GEMM), then
    hipGraph decode == eager decode with three requests at once and with a single one."""
    from nats_llm_studio_amd.engine.engine import Engine, GenRequest
    from nats_llm_studio_amd.engine.sampling import SamplingParams
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.models.llama import LlamaModel
    from nats_llm_studio_amd.models.reference import ReferenceModel
    r = GGUFReader(fitted_models[name, ft])
    m = LlamaModel(r, gpu)
    ref = ReferenceModel(r)
    S = 40
    ids = list(np.random.default_rng(0).integers(0, 900, S))
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.ids[:S] = torch.tensor(ids, dtype=torch.int32)
    b.pos[:S] = torch.arange(S)
    b.slot[:S] = torch.arange(S)
    b.tok_seq[:S] = 0
    b.ctx_len[:S] = torch.arange(S) + 1
    b.block_tables[0] = torch.arange(8)
    m.forward(b, kc, vc, S, 16, n_split=2)
    rl = ref.logits(ids)
    err = (b.logits[:S].cpu() - rl).abs().max().item()
    print(f"WQ_MODEL {name} {ft} prefill logit error {err / rl.abs().max().item():.4f} of the largest logit")
    assert err < 0.05 * rl.abs().max().item(), err
    for nreq in (3, 1):
        outs = []
        for graphs in (False, True):
            eng = Engine(m, None, max_batch=4, use_graphs=graphs)
            futs = [eng.submit(GenRequest([1, 2, 3, 4 + i], SamplingParams(max_tokens=8, ignore_eos=True)))
                    for i in range(nreq)]
            while not all(f.done() for f in futs):
                eng.step()
            outs.append([f.result().token_ids for f in futs])
        assert outs[0] == outs[1], nreq
