"""The dense f16 GEMMs (modes 4 / 5 / 6 hgemm.hip, 10 hgemm10.hip, 14 hgemm14.hip, and what they share in
csrc/kernels/gemm_block.h: grid maps, block_prologue, epi_rows, epi_cols4, the split-K reduce) against fp64 references
that are independent of ops (tests/dense_ref.py), with inputs and a metric that notice ONE misplaced 16-byte chunk,
K-step, slab, row or segment offset. Every dense instance of tests/gemm_digest_cases.py runs: modes 4 and 5 at 8 / 16
waves and rt 4 / 2, (6, 8, 2), (10, 8, 1), (10, 8, 2), (14, 8, 2). Weights are f16 matrices the test writes itself,
handed to the launch as the row-major f16 copy (QWeight.d16), so the reference needs no codec.

What the older tests can and cannot see (test_old_inputs_cannot_see, on the CPU with their inputs and metric, max
|y - ref| <= 2e-2 max |ref| on random_blocks weights and Gaussian rows at K = 768, M = 130): a wrong 16-byte chunk in
EVERY row moves the worst of 40 000 outputs by 0.15 - 0.18 of the maximum and a wrong K-step by 0.27 - 0.34, 7 - 17
times their limit, where the metric here rejects the same faults by 75 000 - 180 000 times its tolerance (one affected
output is typically moved by 0.03: a fault confined to a few rows or lanes sits at the old limit). They pass a slice
boundary one step off (no test reads the slabs), a truncating f16 store, and an arg-max that takes ties at the highest
index or its key before alpha (random inputs have no ties, alpha is 1); the bit-equality chains (mode 14 == mode 4, the
digests) prove that nothing changed, not that the bits were right.

Families.
  integer  (no tolerance) weights = integers -8 .. 8 times a power of two per row (2^-3 .. 2^4, another in neighbouring
           rows), activations in {-2 .. 2}: every partial sum is exact in fp32 in any order (below 2^24 units of 2^-3
           at K <= 1536, test_families_are_what_they_claim). The f32 store, the add with alpha 1/2 onto an integer
           base, the f16 store (= round-to-nearest f16 of the exact sum, sums above 2048 included), every raw split-K
           slab (= the exact partial sum of its own K-slice) and the reduced result must EQUAL the reference.
  one-hot  (no tolerance, localising) activation row m = 1 at column k_m = (37 m + 5) % K, all K = 768 positions in one
           launch of 768 rows, against finite full-range f16 weights of both signs, subnormals included: y = W^T
           exactly; and one-hot weight rows against full-range activations: y[m, n] = x[m, k_n]. Every other addend is
           an exact zero, so a failure names its (K-step, 16-byte chunk, element) and its row.
  full     (tolerance) Gaussian operands under per-row log-uniform scales 2^-6 .. 2^6, each output judged against its
           own size B = sum_k |x_k| |w_k| (add: |base| + |alpha| B; a slab: the B of its own slice).

Metric. |y - ref| <= TOL * B with TOL = 4 x EMU, EMU the largest ratio of the fp32 emulation of the kernels' arithmetic
(dense_ref: f16 products, fp32 sum in ascending 32-deep slices, slabs in slice order, alpha after the sum) against fp64
over this module's full-family inputs, pinned by test_emulated_noise_bounds_tol: EMU = 1.3e-7 (K 1024 / ks 8 the
largest; K 768: 0.65e-7 at ks 1, 0.88e-7 at ks 3), TOL = 5.2e-7. The factor 4 covers the MFMA's internal order. f16
outputs add half an f16 ulp at the largest value the bound admits; where the value is exact (integer family) they
must EQUAL its round-to-nearest f16. SwiGLU: integer operands with a power-of-two alpha that keeps |g|, |u| <= 16 are
exact up to silu itself, so each output is within half an f16 ulp plus 4 x SILU_EMU of the fp64 silu(g) u (SILU_EMU =
1.0e-6, the emulated fp32 silu, measured 0.81e-6 by the same test); the full family propagates TOL through the
derivative as test_weight_sensitivity.test_swiglu_epilogue_full does. Arg-max (integer family, duplicated weight rows
so that maxima tie, activation rows whose outputs are all negative, alpha 1 and -1/2): the id must equal the FIRST
maximum of alpha * sum on EVERY row and the key's value that maximum.
  Everything that is no target keeps its sentinel exactly: y is 3 rows longer and 8 columns wider than its targets,
the gap between two segments, rows past M of the key buffer, and the NaN-filled workspace past the last slab; every
slab element inside is written (no NaN left).

Shapes: K = 768 (12 K-steps: the 3-deep rings of modes 4 / 5, the 2-deep ring of mode 6, mode 10's two buffers and mode
14's four slots wrap several times) with ks 1, 2, 3; mode 14 also K 1536 / ks 3 and K 1024 / ks 2; mode 10 also K 1024
with ks 2 / 4 / 8 (slice-per-XCD map) and ks 3 (default map). Weight rows: two full tiles and a partial one of 37 rows
(mode 10: 44 -- it stores four columns at a time, and its plan refuses 37: test_mode10_refuses_rows_no_multiple_of_4;
SwiGLU: 48). M = 1, BM + 2, 2 BM + 70. Two- and three-segment launches with a gap in the output columns and a partial
tile at each segment end, and the same matrices as ONE merged buffer.

Largest |y - ref| over the bound measured on the MI355X by the GPU tests below (bound: 1), full family, as f32 / add /
f16 store / slabs (an f16 store alone reaches 1 at the bottom of a binade; the fp32 outputs sit at a quarter of TOL,
the emulated noise itself):

  mode 4  rt 4 (8 and 16 waves)   0.237 / 0.236 / 0.991 / 0.263        mode 6  (8, 2)    0.199 / 0.199 / 0.993 / 0.191
  mode 4  rt 2 (8 and 16 waves)   0.199 / 0.199 / 0.993 / 0.191        mode 10 (8, 1)    0.189 / 0.183 / 0.993 / 0.244
  mode 5  rt 4 (8 and 16 waves)   0.224 / 0.217 / 0.992 / 0.233        mode 10 (8, 2)    0.197 / 0.195 / 0.991 / 0.225
  mode 5  rt 2 (8 and 16 waves)   0.194 / 0.189 / 0.992 / 0.235        mode 14 (8, 2)    0.228 / 0.228 / 0.990 / 0.194
  SwiGLU (modes 4 / 5 / 6 / 10, all eleven instances): integer 1.000, full 0.999 - 1.000, two segments 1.000 (the
  bound is reached by outputs in the f16 subnormal range that lie half an ulp from both neighbours)

EQUAL on all twelve instances: the integer family's f32 store, add, f16 store, raw slabs and reduced result on every
shape; both one-hot variants at ks 1 and 3 (f16 subnormal weights and activations included: the MFMA keeps them); the
two-, three-segment and merged launches; the arg-max ids and values on every row of the 16 launches per instance (modes
4 / 5 / 6 / 10). One fault was found, by reading epi_cols4 while choosing the partial tile: modes 9 and 10 wrote up to
three columns past a segment whose rows are no multiple of 4 (under split-K into the next row's slab and past the
workspace); the plan now refuses such launches (test_mode10_refuses_rows_no_multiple_of_4, tests/test_gemv_plan.py) and
the heuristic sends such shapes to mode 2. No recorded digest has such rows.

The GPU tests here, with the dense cases of test_rowops_sensitivity.py and the integer SwiGLU of
test_weight_sensitivity.py, were also run once against two mutated builds: h14_rope taking the row index in place of
slot[...] failed test_qkv_rope_dense_epilogues[m14w8r2k1] and both test_qkv_rope_mode14_layouts cases and nothing else;
the add of epi_rows overwriting failed test_integer_stores_and_slabs and test_full_stores_and_slabs of the ten epi_rows
instances (modes 4 / 5 / 6 / 14; mode 10 stores through epi_cols4) and nothing else -- the split-K add runs in the
reduce kernel, so the add-norm route rightly passed.

Fault models (test_fault_models_are_rejected: applied to the reference only; each changes the exact families wherever
it changes the mathematical result and is rejected by >= 10x the tolerance on the full family):
  D1 one 16-byte chunk of W from the neighbouring chunk / the neighbouring row; of x from the neighbouring row
  D2 one K-step dropped / doubled / taken from the stage one ring depth earlier (depth 2, 3, 4)
  D3 a slice boundary one step off; one K-step in two slices      D4 a slab dropped / written to the neighbouring slice
  D5 a clamped row stored past M / past rows      D6 a boundary tile at the neighbouring segment's column offset
  D7 alpha omitted / applied to the base too      D8 an add that overwrites      D9 an f16 store that truncates
  D10 a gate paired with the neighbouring group's up row; gate and up exchanged
  D11 arg-max ties at the highest index; the partial tile left out; the key taken before alpha
Pairs at which a fault cannot be seen, hence not in the grid: D3 "boundary one step off" on the REDUCED result (the sum
keeps every step: it is seen on the slabs, exact and full); D2 "stage one ring depth earlier" where that step lies in
another K-slice (the grid uses ks 1 and 2, where it does not); D6 on a one-segment launch; D7 "alpha omitted" at alpha
1 (the grid uses 1/2); D9 on the full family (a truncated store is within two rounding terms: the integer family
rejects it by equality); D11 on the full family (ids have no tolerance: exact family only), "key before alpha" at
alpha > 0."""
import functools

import numpy as np
import pytest
import torch

import dense_ref as D
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType as T

EMU = 1.3e-7                    # largest emulated ratio, full family (test_emulated_noise_bounds_tol)
TOL = 4 * EMU
SILU_EMU, SILU_TOL = D.SILU_EMU, D.SILU_TOL      # emulated relative error of silu(g) u, |g| <= 16 (same test)
ACT_ALPHA = 2.0 ** -6           # keeps the full family's f16 store inside f16 (an exact scaling)
GUARD = 4096                    # NaN floats past the last slab that must stay NaN
IDS = lambda c: "m%dw%dr%d" % c


def _shapes(cfg):
    s = [(768, 1), (768, 2), (768, 3)]
    if cfg[0] == 14:
        s += [(1536, 3), (1024, 2)]
    if cfg[0] == 10:
        s += [(1024, 2), (1024, 4), (1024, 8), (1024, 3)]
    return s


def _Ms(cfg):
    bm = D.block_rows(cfg)
    return (1, bm + 2, 2 * bm + 70)


def _rows(cfg, epi="f32"):
    return 2 * D.tile_rows(cfg) + D.partial_rows(cfg, epi)


def _full_shapes(cfg):
    return [(768, 1), (768, 3)] + ([(1536, 3)] if cfg[0] == 14 else []) + ([(1024, 8)] if cfg[0] == 10 else [])


def _full_case(cfg, K, epi):
    """(x, W, base, alpha) of the full family for one instance."""
    rows, xr = _rows(cfg, epi), D.pad64(_Ms(cfg)[2])
    x, w = D.full_rows(xr, K, 1), D.full_rows(rows, K, 2)
    base = D.full_rows(_Ms(cfg)[2] + 3, D.al4(rows) + 8, 3) if epi == "add" else None
    return x, w, base, {"act": ACT_ALPHA, "add": 0.5}.get(epi, 1.0)


@functools.lru_cache(maxsize=None)
def _swiglu_alpha(fam, rows, xr, K):
    """A power of two from the reference alone: integer -- |g|, |u| <= 16; full -- silu(g) u inside f16."""
    x, w = (D.int_acts(xr, K), D.int_weights(rows, K, 4)) if fam == "integer" else (D.full_rows(xr, K, 1),
                                                                                     D.full_rows(rows, K, 2))
    s = D.slab_products(x, w, 1)[0]
    if fam == "integer":
        return 2.0 ** np.floor(np.log2(16.0 / np.abs(s).max()))
    gi = D.interleaved(rows)
    a = 1.0
    while np.abs(D.silu64(a * s[:, gi]) * a * s[:, gi + 8]).max() >= 60000:
        a /= 2
    return a


@functools.lru_cache(maxsize=None)
def _arg_weights(rows, K):
    """Non-negative integer weights (so that rows of non-positive activations give negative outputs only) with copies of
    the rows under the largest scale: maxima tie across lanes, tiles and the partial tile."""
    w = D.int_weights(rows, K, 5, lo=0).copy()
    for n in range(6, rows, 8):                 # the rows under the largest scale, 2^4: where the maxima are
        w[(n + 3) % rows] = w[n]                # a copy in another lane
        if n % 16 == 6:
            w[(n + 101) % rows] = w[n]          # and in another tile
    return w


@functools.lru_cache(maxsize=None)
def _arg_acts(xr, K):
    x = D.int_acts(xr, K, 6).copy()
    x[::5] = -np.abs(x[::5])                    # every fifth row: outputs <= 0 (alpha > 0)
    x[1::5] = np.abs(x[1::5])                   # the next: outputs <= 0 under a negative alpha
    return x


# ------------------------------------------------------------------------------------------------------ CPU tests

def test_families_are_what_they_claim():
    """integer: exact in f16, every partial sum below 2^24 units, sums above 2048 and sums that are no f16 value
    occur and stay inside f16; one-hot: the k_m walk every K position and the weight rows every (K-step, chunk,
    element); full-range: finite, both signs, subnormals; arg-max: ties at the maximum, winners in the partial tile,
    all-negative rows under both alphas."""
    for K in (768, 1024, 1536):
        w, x = D.int_weights(549, K), D.int_acts(640, K)
        assert (D.rne_f16(w) == w).all() and (D.rne_f16(x) == x).all()
        assert float((np.abs(x) @ np.abs(w).T).max()) * 8 + 16 * 1000 < 2.0 ** 24
        s = x @ w.T
        assert (np.abs(s) > 2048).any() and np.abs(s).max() < 65504 and (D.rne_f16(s) != s).any()
        assert (w[0::2][:274] != w[1::2]).any(axis=1).all()
    assert sorted(D.hot_cols(768, 768)) == list(range(768))
    kn = D.hot_cols(293, 768)
    assert len(set(kn // 8)) == 96 and len(set(kn % 8)) == 8
    assert len({(n % 8, k % 64 // 8) for n, k in enumerate(kn)}) == 64
    fr = D.full_range(768, 768)
    sub = (np.abs(fr) < 2.0 ** -14) & (fr != 0)
    assert np.isfinite(fr).all() and sub.any() and (fr < 0).any() and (fr > 0).any() and np.abs(fr).max() > 30000
    rows, K = 293, 768
    w, x = _arg_weights(rows, K), _arg_acts(384, K)
    s = x @ w.T
    for alpha in (1.0, -0.5):
        v = alpha * s
        top = v.max(1, keepdims=True)
        assert ((v == top).sum(1) > 1).mean() > 0.1
        assert (np.argmax(v, 1) >= 256).any() and (v.max(1) < 0).any() and (v.max(1) > 0).any()
        assert (np.argmax(v, 1) != np.argmax(s, 1)).any() == (alpha < 0)


def _emu_ratio(x, segs, M, epi, **kw):
    good = D.run(x, segs, M, epi, tol=1.0, **kw)
    emu = D.run(x, segs, M, epi, emu=True, **kw)
    r = [D.judge(emu["y"], good)[0]]
    if "slabs" in good:
        r.append(D.judge_slabs(emu["slabs"], good)[0])
    return max(r)


def test_emulated_noise_bounds_tol():
    """EMU is the largest ratio of the emulated kernel arithmetic against fp64 over this module's full-family inputs
    (f32 store, add, slabs, the reduced sum; tol = 1, so the figure is |emu - ref| / B itself), SILU_EMU the largest
    relative error of the emulated fp32 silu(g) u over the integer SwiGLU inputs; both within a factor 2 below the
    constants: measurements, not guesses."""
    worst, seen = {}, set()
    for cfg in D.INSTANCES:
        for K, ks in _full_shapes(cfg):
            for epi in ("f32", "add"):
                x, w, base, alpha = _full_case(cfg, K, epi)
                key = (id(x), id(w), ks, epi)
                if key in seen:
                    continue
                seen.add(key)
                M = _Ms(cfg)[2]
                r = _emu_ratio(x, [(w, 0)], M, epi, alpha=alpha, ks=ks, base=base, nrows=M + 3)
                worst[f"K{K}ks{ks}"] = max(worst.get(f"K{K}ks{ks}", 0.0), r)
    print("emulated noise full: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert EMU / 2 <= max(worst.values()) <= EMU, max(worst.values())
    silu = 0.0
    for rows in {_rows(c, "swiglu") for c in D.INSTANCES}:
        x, w = D.int_acts(640, 768), D.int_weights(rows, 768, 4)
        alpha = _swiglu_alpha("integer", rows, 640, 768)
        v = alpha * D.slab_products(x, w, 1)[0]
        assert np.abs(v).max() <= 16
        gi = D.interleaved(rows)
        g, u = v[:, gi], v[:, gi + 8]
        ref, emu = D.silu64(g) * u, (D.silu32(g) * u.astype(np.float32)).astype(np.float64)
        silu = max(silu, float((np.abs(emu - ref)[ref != 0] / np.abs(ref)[ref != 0]).max()))
    print(f"emulated silu(g) u, integer family: {silu:.2e}")
    assert SILU_EMU / 2 <= silu <= SILU_EMU, silu


def _fault_inputs(fam, epi, M=24):
    """(x, segs, kwargs) of one family for the fault grid: 2 * 128 + 37 weight rows (SwiGLU 48), K = 768."""
    rows, K = (304 if epi == "swiglu" else 293), 768
    kw = dict(nrows=M + 3, ld=rows + 8, tile=128)
    if fam == "integer":
        x, w = (_arg_acts(64, K), _arg_weights(rows, K)) if "argmax" in epi else (D.int_acts(64, K),
                                                                                  D.int_weights(rows, K, 4))
        if epi == "add":
            kw["base"] = D.int_base(M + 3, rows + 8)
        if epi == "swiglu":
            kw["alpha"], kw["silu_tol"] = _swiglu_alpha("integer", rows, 64, K), SILU_TOL
    elif fam == "hot":
        M = K
        x, w = D.hot_acts(K), D.full_range(rows, K)
        kw.update(nrows=M + 3)
    else:
        x, w = D.full_rows(64, K, 1), D.full_rows(rows, K, 2)
        kw["tol"] = TOL
        if epi == "add":
            kw["base"] = D.full_rows(M + 3, rows + 8, 3)
        if epi == "act":
            kw["alpha"] = ACT_ALPHA
        if epi == "swiglu":
            kw["alpha"], kw["silu_tol"] = _swiglu_alpha("full", rows, 64, K), SILU_TOL
    return x, w, M, kw


def _rejection(fault, fam, epi, ks=1, two=False, slabs=False, depth=3, alpha=None):
    """How the good reference's judgement sees the faulty reference: exact families -- the number of outputs that
    differ; full -- the largest error in units of the tolerance."""
    x, w, M, kw = _fault_inputs(fam, epi, 64 if "argmax" in epi else 24)
    if alpha is not None:
        kw["alpha"] = alpha
    segs = [(w, 0)]
    if two:
        w2 = D.int_weights(165, 768, 9) if fam != "full" else D.full_rows(165, 768, 9)
        segs = [(w, 0), (w2, w.shape[0] + 16)]
        kw["ld"] = w.shape[0] + 16 + 165 + 8
        if "base" in kw:
            kw["base"] = None
    good = D.run(x, segs, M, epi, ks=ks, **kw)
    bad = D.run(x, segs, M, epi, ks=ks, fault=fault, depth=depth, **kw)
    if "argmax" in epi:
        return int((bad["ids"] != good["ids"]).sum())
    r, _, n = D.judge_slabs(bad["slabs"], good) if slabs else D.judge(bad["y"], good)
    return r if fam == "full" else n


FAULT_GRID = (            # (fault, epilogue, kwargs): every fault where it can change the result
    [(f, "f32", dict(ks=ks, depth=d)) for f in D.OPERAND_FAULTS for ks in (1, 2)
     for d in ((2, 3, 4) if "ring depth" in f else (3,))]
    + [("slice boundary one step off", "f32", dict(ks=2, slabs=True))]
    + [(f, "f32", dict(ks=2)) for f in D.SLICE_FAULTS[1:]]
    + [(f, "f32", dict(ks=2, slabs=True)) for f in D.SLICE_FAULTS[1:]]
    + [(f, "f32", dict(two=True)) for f in D.PLACE_FAULTS] + [(D.PLACE_FAULTS[0], "act", dict(ks=2))]
    + [("alpha omitted", "f32", dict(alpha=0.5)), ("alpha omitted", "add", dict(alpha=0.5)),
       ("alpha applied to the base too", "add", dict(alpha=0.5)), ("add overwrites", "add", dict(alpha=0.5)),
       ("add overwrites", "add", dict(alpha=0.5, ks=2))]
    + [(f, "swiglu", dict(ks=ks)) for f in D.SWIGLU_FAULTS for ks in (1, 2)])


def test_fault_models_are_rejected():
    """Every fault model, applied to the reference only: the integer family's outputs differ (the one-hot family's
    too, for the faults of the product), and the full family rejects it by >= 10x the tolerance. The pairs left out
    of the grid are named in the module docstring; the exact-only ones (truncation, arg-max) are asserted below."""
    seen = set()
    for fault, epi, kw in FAULT_GRID:
        n = _rejection(fault, "integer", epi, **kw)
        r = _rejection(fault, "full", epi, **kw)
        extra = ""
        if fault in D.OPERAND_FAULTS:
            h = _rejection(fault, "hot", epi, **kw)
            extra = f", one-hot outputs that differ: {h}"
            assert h > 0, (fault, kw)
        print(f"{fault} [{epi} {kw}]: rejected by {r:.0f}x tolerance; integer outputs that differ: {n}{extra}")
        assert n > 0 and r >= 10.0, (fault, epi, kw, n, r)
        seen.add(fault)
    n = _rejection("f16 store truncates", "integer", "act")
    r = _rejection("f16 store truncates", "full", "act")
    print(f"f16 store truncates: integer outputs that differ: {n}; full family {r:.2f}x its bound (not in the grid)")
    assert n > 0 and r < 10.0
    seen.add("f16 store truncates")
    for f in D.ARGMAX_FAULTS:
        ns = {alpha: _rejection(f, "integer", "argmax", alpha=alpha) for alpha in (1.0, -0.5)}
        print(f"arg-max {f}: ids that differ on {ns[1.0]} (alpha 1) and {ns[-0.5]} (alpha -1/2) of 64 rows")
        if f == "key taken before alpha":
            assert ns[1.0] == 0 and ns[-0.5] > 0
        else:       # (the winner of a row lies in the partial tile on a few rows only: one alpha suffices)
            assert max(ns.values()) > 0 and (f != "ties taken at the highest index" or min(ns.values()) > 0), (f, ns)
        seen.add(f)
    assert seen == set(D.OPERAND_FAULTS + D.SLICE_FAULTS + D.PLACE_FAULTS + D.SCALE_FAULTS + D.STORE_FAULTS
                       + D.SWIGLU_FAULTS + D.ARGMAX_FAULTS)
    # the pair that is named invisible: a boundary moved on both sides keeps the reduced sum
    assert _rejection("slice boundary one step off", "integer", "f32", ks=2) == 0


OLD_PASS = ["slice boundary one step off"]           # of the faults of the product: what the old metric lets through


def test_old_inputs_cannot_see():
    """The gap these families close, on the CPU with the older tests' inputs and metric (test_hgemm_dense /
    test_hgemm10_dense / the XCD-map test: random_blocks Q4_K weights, Gaussian rows, K = 768, max |y - ref| <= 2e-2
    max |ref|; arg-max: more than 99 % of rows agree): which faults of the product pass."""
    rows, K, M = 304, 768, 130
    rng = np.random.default_rng(0)
    w = Q.dequantize(Q.random_blocks(T.Q4_K, rows * K, 0.05, rng), T.Q4_K, (rows, K))
    w = w.astype(np.float16).astype(np.float64)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(1)).to(torch.float16).double().numpy()
    passed = []
    for fault in D.OPERAND_FAULTS + D.SLICE_FAULTS:
        ks = 2 if fault in D.SLICE_FAULTS else 1
        good = D.run(x, [(w, 0)], M, "f32", ks=ks, tol=TOL)
        bad = D.run(x, [(w, 0)], M, "f32", ks=ks, fault=fault)
        old = float(np.nan_to_num(np.abs(bad["y"] - good["y"]), nan=np.inf).max() / np.abs(good["y"]).max())
        new = max(D.judge(bad["y"], good)[0], D.judge_slabs(bad["slabs"], good)[0] if ks > 1 else 0.0)
        print(f"old inputs, {fault}: {old:.4f} of the largest value (limit 0.02); new metric {new:.0f}x tolerance")
        assert new >= 10.0, fault
        if old <= 2e-2:
            passed.append(fault)
    assert passed == OLD_PASS, passed
    good, bad = D.run(x, [(w, 0)], M, "act", tol=TOL), D.run(x, [(w, 0)], M, "act", fault="f16 store truncates")
    old = float(np.abs(bad["y"] - good["y"]).max() / np.abs(good["y"]).max())
    print(f"old inputs, f16 store truncates: {old:.4f} of the largest value (limit 0.02)")
    assert old <= 2e-2
    v = D.run(x, [(w, 0)], M, "argmax")
    for f in ("ties taken at the highest index", "key taken before alpha"):
        assert (D.run(x, [(w, 0)], M, "argmax", fault=f)["ids"] == v["ids"]).all(), f      # no ties, alpha 1: identical


# ------------------------------------------------------------------------------------------------------ GPU tests

class _Bank:
    """Device copies of the shared operands (f16), made once per module; weights as QWeight shells around the
    row-major f16 matrix the dense modes read (QWeight.d16)."""

    def __init__(self, dev):
        from nats_llm_studio_amd import ops
        self.dev, self.ops, self._t = dev, ops, {}

    def f16(self, a):
        if id(a) not in self._t:
            self._t[id(a)] = (a, torch.from_numpy(a).to(torch.float16).to(self.dev))
        return self._t[id(a)][1]

    def weight(self, d16):
        """A GGML F16 weight of these values whose row-major f16 copy IS `d16` (the d16 substitution of
        test_hgemm14_gpu.py / test_splitk_xcd_gpu.py: the dense modes read nothing else)."""
        w = self.ops.QWeight(d16.cpu().numpy().view(np.uint8).reshape(-1), T.F16, d16.shape[0], d16.shape[1], self.dev)
        w.d16 = d16
        return w

    def segs(self, segs, merged=False):
        """ops.Seg list of [(W, ycol)]; merged: the f16 copies as consecutive rows of ONE buffer (what
        QWeight.expand_dense_group leaves), which a launch with adjacent output columns sees as one segment."""
        ops = self.ops
        if merged:
            buf = torch.cat([self.f16(w) for w, _ in segs])
            r0, out = 0, []
            for w, c in segs:
                out.append(ops.Seg(self.weight(buf[r0:r0 + w.shape[0]]), c))
                r0 += w.shape[0]
            assert len(ops._merge_dense(out)) == 1
            return out
        out = [ops.Seg(self.weight(self.f16(w)), c) for w, c in segs]
        for a, b in zip(out, out[1:]):          # (a launch merges copies that are adjacent in memory and in y)
            if b.w.d16.data_ptr() == a.w.d16.data_ptr() + a.w.d16.numel() * 2:
                b.w.d16 = b.w.d16.clone()
        assert len(ops._merge_dense(out)) == len(segs)
        return out


@pytest.fixture(scope="module")
def bank(gpu):
    return _Bank(gpu)


def _gpu(bank, cfg, ks, x, segs, M, epi, alpha=1.0, base=None, merged=False):
    """One launch into sentinel buffers: y 3 rows longer and 8 columns wider than its targets, a NaN workspace GUARD
    floats longer than the slabs, keys 3 rows longer. None where the plan refuses. Returns (y, slabs, keys) on the
    host; asserts the workspace guard."""
    ops, dev = bank.ops, bank.dev
    sg = bank.segs(segs, merged)
    ld = D.ld_of(segs, epi)
    dt = ops.ACT_DTYPE if epi in ("act", "swiglu") else torch.float32
    if base is None:
        y = torch.full((M + 3, ld), D.SENT, dtype=dt, device=dev)
    else:
        y = torch.from_numpy(base).to(dt).to(dev)
        assert y.shape == (M + 3, ld)
    keys = torch.zeros(M + 3, dtype=torch.int64, device=dev) if "argmax" in epi else None
    n = ops._ws_floats(sg, M, cfg[0], ks)
    if n:
        ops._workspace(dev, n + GUARD)[:n + GUARD].fill_(float("nan"))
    xs = bank.f16(x)
    assert xs.shape[0] >= D.pad64(M)
    if not ops._launch(sg, xs, y, M, alpha, {"f32_argmax": "f32"}.get(epi, epi), (*cfg, ks), argmax=keys, soft=True):
        return None
    slabs = None
    if n:
        ws = ops._WS[dev][:n + GUARD].cpu()
        assert bool(torch.isnan(ws[n:]).all()), "the workspace past the last slab was written"
        slabs = ws[:n].view(ks, M, -1).double().numpy()
    return y.cpu().double().numpy(), slabs, None if keys is None else keys.cpu().numpy()


def _expect(cfg, epi, ks, K, res, rows=()):
    """A launch runs exactly where the plan admits it."""
    assert (res is not None) == D.admits(cfg, epi, ks, K, rows), (cfg, epi, ks, K, rows,
                                                                  "launched" if res is not None else "refused")
    return res is not None


def _judge(tag, worst, got, ref, slabs=False, K=None):
    r, i, n = D.judge_slabs(got, ref) if slabs else D.judge(got, ref)
    worst[0] = max(worst[0], r)
    rr = ref["slabs"] if slabs else ref["y"]
    assert r <= 1.0, (tag, f"{n} outputs outside their bound (0: EQUAL); worst {r:.3g} of the bound at index {i}: got "
                           f"{got[i]!r}, reference {rr[i]!r}")


def _stores(bank, cfg, fam, shapes, Ms_of, worst):
    """f32, add, f16 store, raw slabs and the reduced result of one family over the shapes."""
    for K, ks in shapes:
        for M in Ms_of(K, ks):
            for epi in ("f32", "add", "act") + (("slabs",) if ks > 1 else ()):
                if fam == "integer":
                    x, w, alpha = D.int_acts(D.pad64(_Ms(cfg)[2]), K), D.int_weights(_rows(cfg), K), 1.0
                    base = D.int_base(M + 3, D.al4(w.shape[0]) + 8, M) if epi == "add" else None
                    alpha, tol = (0.5 if epi == "add" else 1.0), 0.0
                else:
                    x, w, base, alpha = _full_case(cfg, K, epi)
                    base, tol = (None if base is None else base[:M + 3]), TOL
                res = _gpu(bank, cfg, ks, x, [(w, 0)], M, epi, alpha, base)
                if not _expect(cfg, epi, ks, K, res, (w.shape[0],)):
                    continue
                ref = D.run(x, [(w, 0)], M, epi, alpha=alpha, ks=ks, base=base, nrows=M + 3, tol=tol)
                tag = (IDS(cfg), fam, K, ks, M, epi)
                _judge(tag, worst[epi], res[0], ref)
                if ks > 1:
                    _judge(tag + ("slabs",), worst["slabs"], res[1], ref, slabs=True)


def _report(name, cfg, worst, exact):
    print(f"DG_RATIO {name} {IDS(cfg)} " + " ".join(
        f"{k}={'equal' if exact else '%.3f' % v[0]}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", D.INSTANCES, ids=IDS)
def test_integer_stores_and_slabs(gpu, bank, cfg):
    """Integer family, no tolerance: f32 store, add (alpha 1/2, integer base), f16 store, every raw slab and the
    reduced result EQUAL the reference on every shape; all three M at K 768 / ks 1 and 3, 2 BM + 70 elsewhere."""
    worst = {e: [0.0] for e in ("f32", "add", "act", "slabs")}
    _stores(bank, cfg, "integer", _shapes(cfg),
            lambda K, ks: _Ms(cfg) if (K, ks) in ((768, 1), (768, 3)) else _Ms(cfg)[2:], worst)
    _report("integer", cfg, worst, True)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", D.INSTANCES, ids=IDS)
def test_full_stores_and_slabs(gpu, bank, cfg):
    """Full family: every output within TOL of its own size B (f16: plus half an ulp), every slab of its slice's."""
    worst = {e: [0.0] for e in ("f32", "add", "act", "slabs")}
    _stores(bank, cfg, "full", _full_shapes(cfg), lambda K, ks: (_Ms(cfg)[2], 1) if K == 768 else _Ms(cfg)[2:], worst)
    _report("full", cfg, worst, False)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", D.INSTANCES, ids=IDS)
def test_one_hot(gpu, bank, cfg):
    """No tolerance, localising. x = one-hot rows walking every K position against full-range weights: y = W^T; then
    one-hot weight rows against full-range activations: y[m, n] = x[m, k_n]. ks 1 and 3 (zero slabs add exactly)."""
    K, rows = 768, _rows(cfg)
    hx, fw = D.hot_acts(K), D.full_range(rows, K)
    M2 = _Ms(cfg)[2]
    fx, hw = D.full_range(D.pad64(M2), K, 1), D.hot_weights(rows, K)
    for ks in (1, 3):
        y = _gpu(bank, cfg, ks, hx, [(fw, 0)], K, "f32")[0]
        ref = D.run(hx, [(fw, 0)], K, "f32", ks=ks, nrows=K + 3)
        r, i, n = D.judge(y, ref)
        assert r == 0, (IDS(cfg), ks, f"{n} outputs differ from W^T; first at weight row {i[1]} (row {i[1] % 8} of its "
                        f"8-row group), " + D.where(i, int(D.hot_cols(K, K)[min(i[0], K - 1)])), y[i], ref["y"][i])
        y = _gpu(bank, cfg, ks, fx, [(hw, 0)], M2, "f32")[0]
        ref = D.run(fx, [(hw, 0)], M2, "f32", ks=ks, nrows=M2 + 3)
        r, i, n = D.judge(y, ref)
        assert r == 0, (IDS(cfg), ks, f"{n} outputs differ from x[m, k_n]; first at activation row {i[0]} (row "
                        f"{i[0] % 8} of its 8-row group), " + D.where(i, int(D.hot_cols(rows, K)[min(i[1], rows - 1)])),
                        y[i], ref["y"][i])
    print(f"DG_RATIO one-hot {IDS(cfg)} equal")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [c for c in D.INSTANCES if c[0] == 10], ids=IDS)
def test_mode10_refuses_rows_no_multiple_of_4(gpu, bank, cfg):
    """Mode 10 stores four output columns (and four slab floats) behind one row check, so a segment of 37 more rows
    would write up to three columns past its targets, and under split-K into the next row's slab: the plan refuses
    such a launch (nothing runs), one segment or the second of two, every store epilogue, with and without split-K.
    The same launch with 44 rows runs (test_integer_stores_and_slabs)."""
    K, t, M = 768, D.tile_rows(cfg), D.block_rows(cfg) + 2
    x = D.int_acts(D.pad64(_Ms(cfg)[2]), K)
    one = [(D.int_weights(2 * t + 37, K), 0)]
    two = [(D.int_weights(t + 44, K, 10), 0), (D.int_weights(37, K, 11), D.al4(t + 44 + 16))]
    for segs in (one, two):
        rows = tuple(w.shape[0] for w, _ in segs)
        for ks in (1, 2, 3):
            for epi in ("f32", "add", "act", "f32_argmax") + (("slabs",) if ks > 1 else ()):
                base = D.int_base(M + 3, D.ld_of(segs), 1) if epi == "add" else None
                assert not D.admits(cfg, epi, ks, K, rows)
                assert not _expect(cfg, epi, ks, K, _gpu(bank, cfg, ks, x, segs, M, epi, base=base), rows)


def _seg_layouts(cfg, epi="f32"):
    """[(ycol, rows)] of two and three segments, each ending in a partial tile, a gap of at least 16 output columns
    after the first (every ycol a multiple of 4, as modes 10 / 14 want); and three matrices with adjacent columns for
    the merged buffer, the first two boundaries inside a tile."""
    t, p = D.tile_rows(cfg), D.partial_rows(cfg, epi)
    h = 2 if epi == "swiglu" else 1
    r = (t + p, 2 * t + p, p + 16)
    two = [(0, r[1]), (D.al4(r[1] // h + 16), r[0])]
    c1 = D.al4(r[0] // h + 16)
    three = [(0, r[0]), (c1, r[2]), (D.al4(c1 + r[2] // h), r[1])]
    m = (t + 44, 60, 2 * t + p)
    return two, three, [(0, m[0]), (m[0], m[1]), (m[0] + m[1], m[2])]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", D.INSTANCES, ids=IDS)
def test_segments(gpu, bank, cfg):
    """Integer family over two- and three-segment launches with a gap in the output columns and a partial tile at each
    segment end (tile_begin lookup, ycol, tile_begin_col), ks 1 and 2, f32 / f16 stores and slabs; then the three
    matrices as ONE merged buffer with adjacent columns (segment boundaries inside a tile). The gap keeps the
    sentinel."""
    K, M = 768, D.block_rows(cfg) + 2
    x = D.int_acts(D.pad64(_Ms(cfg)[2]), K)
    two, three, adj = _seg_layouts(cfg)
    worst = {e: [0.0] for e in ("f32", "act", "slabs")}
    for name, lay, merged in (("two", two, False), ("three", three, False), ("merged", adj, True)):
        segs = [(D.int_weights(n, K, 10 + i), c) for i, (c, n) in enumerate(lay)]
        assert all(c % 4 == 0 for _, c in segs)
        for ks in (1, 2):
            for epi in ("f32", "act") + (("slabs",) if ks > 1 else ()):
                res = _gpu(bank, cfg, ks, x, segs, M, epi, merged=merged)
                assert res is not None, (IDS(cfg), name, ks, epi)
                ref = D.run(x, segs, M, epi, ks=ks, nrows=M + 3)
                _judge((IDS(cfg), name, ks, epi), worst[epi], res[0], ref)
                if ks > 1:
                    _judge((IDS(cfg), name, ks, epi, "slabs"), worst["slabs"], res[1], ref, slabs=True)
    _report("segments", cfg, worst, True)


SWIGLU = [c for c in D.INSTANCES if c[0] != 14]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SWIGLU, ids=IDS)
def test_swiglu(gpu, bank, cfg):
    """The f16 SwiGLU epilogue (epi_rows: partner lane ^ 8; epi_cols4: lane ^ 32; the split-K reduce): interleaved
    gate / up rows. Integer family: within half an f16 ulp plus 4 x the emulated silu error of the fp64 result; full
    family: TOL propagated through the derivative. One segment at M 1 / BM + 2 / 2 BM + 70, ks 1 and 3; two segments
    with a gap (halved ycol)."""
    K, rows, xr = 768, _rows(cfg, "swiglu"), D.pad64(_Ms(cfg)[2])
    worst = {"integer": [0.0], "full": [0.0], "two": [0.0]}
    for fam in ("integer", "full"):
        x, w = (D.int_acts(xr, K), D.int_weights(rows, K, 4)) if fam == "integer" else (D.full_rows(xr, K, 1),
                                                                                         D.full_rows(rows, K, 2))
        alpha = _swiglu_alpha(fam, rows, xr, K)
        for ks in (1, 3):
            for M in _Ms(cfg):
                res = _gpu(bank, cfg, ks, x, [(w, 0)], M, "swiglu", alpha)
                assert res is not None
                ref = D.run(x, [(w, 0)], M, "swiglu", alpha=alpha, ks=ks, nrows=M + 3,
                            tol=TOL if fam == "full" else 0.0, silu_tol=SILU_TOL)
                _judge((IDS(cfg), fam, ks, M), worst[fam], res[0], ref)
    two = _seg_layouts(cfg, "swiglu")[0]
    segs = [(D.int_weights(n, K, 4), c) for c, n in two]
    alpha = min(_swiglu_alpha("integer", n, xr, K) for _, n in two)
    M = _Ms(cfg)[1]
    for ks in (1, 2):
        res = _gpu(bank, cfg, ks, D.int_acts(xr, K), segs, M, "swiglu", alpha)
        assert res is not None
        ref = D.run(D.int_acts(xr, K), segs, M, "swiglu", alpha=alpha, ks=ks, nrows=M + 3, silu_tol=SILU_TOL)
        _judge((IDS(cfg), "two segments", ks), worst["two"], res[0], ref)
    _report("swiglu", cfg, worst, False)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SWIGLU, ids=IDS)
def test_argmax(gpu, bank, cfg):
    """The arg-max epilogue (alone, and next to the f32 store; ks 1 in the kernels' epilogues, ks 3 in the reduce):
    integer family with tied maxima, all-negative rows, alpha 1 and -1/2, one and two segments. On EVERY row the id is
    the first maximum of alpha * sum and the key's value that maximum; key rows past M stay zero; the f32 store next
    to it is exact and the arg-max alone leaves y untouched."""
    K, rows, M = 768, _rows(cfg), _Ms(cfg)[2]
    x = _arg_acts(D.pad64(M), K)
    w = _arg_weights(rows, K)
    two = [(w, 0), (_arg_weights(D.tile_rows(cfg) + D.partial_rows(cfg), K), D.al4(rows + 16))]
    n = 0
    for segs in ([(w, 0)], two):
        for ks in (1, 3):
            for epi in ("argmax", "f32_argmax"):
                for alpha in (1.0, -0.5):
                    res = _gpu(bank, cfg, ks, x, segs, M, epi, alpha)
                    assert res is not None
                    ref = D.run(x, segs, M, epi, alpha=alpha, ks=ks, nrows=M + 3)
                    assert D.judge(res[0], ref)[0] == 0, (IDS(cfg), epi, ks, alpha, "y")
                    vals, ids = D.unpack_keys(res[2])
                    bad = np.flatnonzero(ids[:M] != ref["ids"])
                    assert len(bad) == 0, (IDS(cfg), epi, ks, alpha, f"{len(bad)} of {M} rows name another id",
                                           [(int(m), int(ids[m]), int(ref["ids"][m])) for m in bad[:4]])
                    assert (vals[:M] == ref["vals"]).all() and (res[2][M:] == 0).all(), (IDS(cfg), epi, ks, alpha)
                    n += 1
    print(f"DG_RATIO argmax {IDS(cfg)} equal on every row of {n} launches")
