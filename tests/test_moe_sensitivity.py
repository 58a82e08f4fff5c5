"""The MoE path -- the top-k route (moe_route_kernel, moe_route_wide_kernel, moe_norm_route_kernel, route_rows folded
into the o projection), router_logits_kernel, moe_combine_kernel<set / add> and the expert launches over row lists
(path A selected / unselected, path B, the LDS-dequant GEMM; through the expert table and as by-value segments) --
against fp64 references that are independent of ops (tests/moe_ref.py), with inputs and a metric that notice ONE
misrouted token, slot, expert or row block.

What the older tests cannot see (test_old_inputs_cannot_see, on the CPU with their inputs and their checks):
test_moe_route never reads yrows, so slots j and j + 1 exchanged in yrows (R3) pass it; test_expert_table_launches
routes randn logits over 128 experts -- its largest expert count is 11 (T = 70), so no expert owns a second m-block and
X3 changes nothing, and at T = 1, 3 no expert repeats, so the repeat-slot exit (X5) never fires; test_router_logits
has no D past 4096, so the dropped tail of a second pass (L2) changes nothing.

Metric.
  exact   sel slot by slot, counts, per expert the multiset of (xrows[i], yrows[i]) pairs (list order is the atomics'),
          every list entry at or past a count, the guard tail past E * cap, topw / sel past T * k, rows past T,
          columns past D: equality. The integer / tag families are exact in fp32 in any order: equality.
  topw    |w - ref| <= TOL_W * (ref + [ref < 2^-120 wmax] wmax) against the fp64 softmax of the logits the kernel
          read (wmax: the row's largest weight; the floor serves weights under fp32's exp range, the far family).
  logits  |lg - ref| <= TOL_L * B, B = sum |h_i| |w_i|, ref the fp64 product of the device's own f16 h.
  h       the row-ops norm bound (rowops.rms_ratio, ARITH 4 x 2.6e-7, f16 store), x the residual-add bound.
  combine within 2k + 2 fp32 roundings of |x| + |alpha| sum |w y| (rowops.x_ratio); tag: equal to one of the two
          results the compiler may form (alpha * s rounded before the add, or fused into it).
  TOL = 4 x EMU, EMU the largest ratio of the CPU fp32 emulation (moe_ref.route_emu: exp2(fp32(x log2e)), fp32 tree
  sum, divide, slot-order sum, divide; moe_ref.logit_emu: fp32 products, 8 in order per thread, tree) against fp64
  over this module's inputs, pinned by test_emulated_noise_bounds_tol:
           topw    2.2e-7 of the weight (grid 1.84, shift 1.84, census 1.89, hot 2.02, the norm + route logits 2.18)
           logits  1.2e-7 of B (gauss rows D 8 .. 8200 0.83, the norm + route rows D 4 .. 8192 1.18)
  The factor 4 covers the reduction order and the hardware exp2 / rsqrt.

Families. Route: grid (row t a permutation of -g arange(E), g = 2^-6 and 2^-10: neighbouring probabilities 9.8e-4
apart at 2^-10), census (T = E, token t's top-k = t, t + 1, .. mod E in slot order: every expert k rows, once per
slot, every lane), hot (every token the same k experts 0, E - 1, 7, 8, 63, 64 .., T = cap: lists filled to their last
entry), shift (grid +- 1e4: l - max stays exact), far (one expert +100 over the grid: slot 0, weight 1, the rest
<= tolerance, k distinct valid experts, lists consistent with sel), ties (all equal; +0.0 / -0.0; the k / k + 1 cut
inside a tie; lanes 3 / 67; the high half ahead), the NaN / +-inf rows of the two older tests. Norm + route: wr[e] =
sum_t C[t, e] u_t over the dual basis of the fp64 normed rows, so the logits are a known grid (separation pinned by
test_norm_route_logits_are_separated), the route judged against the fp64 route of the device's own logits.
Router logits: gauss; integer (h in {-1, 0, 1}, wr small integers that differ per chunk, expert and column). Combine:
tag (weights 2^-(1 + (j + t) % 8), y integer tags of (t, j, column), integer residual), gauss. Expert launches:
qblocks' integer family, E = 128 experts of [256, 256] Q4_K and Q6_K with another seed each, x in {-1, 0, 1}: outputs
EQUAL the fp64 x[xrow] @ W_e^T, untouched rows keep the sentinel; plans hot / diag / last / pairs (moe_ref.make_plan).

Largest ratios measured on the MI355X by the GPU tests below (bound 1 = TOL):

  route                                      exact outputs            toleranced (fraction of TOL)
  moe_route_kernel        E 2 / 8 / 33 / 60 / 64  sel, counts, pairs, sentinels   topw 0.045 / 0.261 / 0.230 / 0.210 / 0.199
  moe_route_wide_kernel   E 65 / 96 / 128      equal                    topw 0.208 / 0.266 / 0.179
    per family, all E     grid 0.208, shift 0.208, census 0.208, hot 0.230, ties 0.266, far 0.000 (scale: the far weight)
  moe_norm_route_kernel   D 4 / 2048 / 2052 / 6144 / 8192   equal       h 0.743 / 0.982 / 0.996 / 0.996 / 0.996
                                                                        logits 0.113 / 0.208 / 0.218 / 0.214 / 0.261
                                                                        topw 0.201 / 0.175 / 0.225 / 0.148 / 0.204
  route_rows (folded)     Q4_K / Q8_0 o projection   equal, x equal     h 0.993 / 0.990, logits 0.231 / 0.252, topw 0.282 / 0.245
  router_logits_kernel    D 8 / 768 / 4096 / 4104 / 8200   integer equal   gauss 0.174 / 0.028 / 0.015 / 0.014 / 0.014
  moe_combine_kernel      add / set            tag equal                gauss 0.433 / 0.449 (of 2k + 2 roundings)
  expert launches, integer: path A selected T 1 / 3, unselected T 16 / 32, mode 1 T 70, mode 2 rt 1 T 70, mode 2 rt 2
                          T 130 -- table and by-value launches bit-equal and EQUAL to the reference on every plan, both
                          types, both shapes (116 launch pairs); mapped split-K ks 3 on modes 1 / 2 / 3 equal
  expert launches, SwiGLU on the full family: 0.433 of the propagated bound on each of the seven routes
(h reaches 1 at the bottom of an f16 binade by the round-to-nearest store alone, as in test_rowops_sensitivity.)

No kernel fault was found. One fault of a CPU twin was: ops.moe_route ranked with torch.topk, which on a row of equal
probabilities returned e.g. experts [6, 5] of 8 and [84, 87, 86, ..] of 128 where the kernels' contract is the lowest
unused expert, and which let one NaN logit turn the whole row into NaNs (softmax) so that the NaN expert could be
chosen; the twin now ranks with a stable sort on (-p, index), NaNs last, over exp(l - max of the numbers), and
test_cpu_twin_route holds it to the same judge as the kernels.

The GPU tests were also run once against a mutated ops.hip (router_logits_kernel stopping at column 4096,
moe_combine_kernel reading the next token's slot weights): test_router_logits_families[4104], [8200] and both
test_moe_combine_families cases failed and nothing else here; of the older MoE tests test_router_logits passed all six
cases, and only the block reference of test_expert_table_launches (T >= 3) noticed the combine.

Fault models (test_fault_models_are_rejected: applied to the reference alone, each rejected by >= 10x its tolerance or
by an exact output at every grid point where it changes the mathematical result):
  R1 one (token, slot) under the neighbouring expert   R2 one row listed twice / left out   R3 slots j, j + 1
  exchanged in yrows, not in topw   R4 renormalisation flipped   R5 softmax sum / maximum over experts 0..63 only
  R6 a tie to the higher index   R7 expert index without its bit 6   L1 one 8-column chunk dropped / of the neighbouring
  expert row / token   L2 the tail past a 4096-column pass dropped   C1 slot weight of the neighbouring token
  C2 alpha also on the residual   C3 set_ adds onto the stale residual   C4 columns past the last full 256 dropped
  X1 weights of expert e + 1   X2 maps read at e * T   X3 second m-block gathers block 0's rows / unwritten
  X4 count of expert e + 1   X5 the repeat-slot exit skips a distinct expert   X6 list assumed ascending
Points where a fault cannot show: R3 at k = 1; R4 at k = E (the k weights already sum to 1); R5 at E <= 64, the sum
also wherever the weights are renormalised (it cancels), the maximum everywhere in exact arithmetic (it shows as an
overflow to NaN in the emulation of the far family with the far expert >= 64); R6 without a tie (every family but
ties); R7 without a chosen expert >= 64; L1 neighbouring token at T = 1; L2 at D <= 4096; C1 at T = 1; C2 at alpha = 1
and with set_; C3 without set_; C4 at D a multiple of 256; X2 at cap = T; X3 with no count past 64; X4 where the
neighbour's count is the same (hot: among the hot experts); X5 on the unselected routes and without a repeat; X6 on
ascending lists (diag, pairs).
"""
import functools

import numpy as np
import pytest
import torch

import moe_ref as MR
import rowops as R
from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf.constants import GGMLType

SENT, GUARD = MR.SENT, MR.GUARD
# largest emulated ratios (test_emulated_noise_bounds_tol); norm: the figure test_rowops_sensitivity pins
EMU = {"topw": 2.2e-7, "logit": 1.2e-7, "norm": 2.6e-7}
TOL = {k: 4 * v for k, v in EMU.items()}
GEMV_TOL = 6.8e-4               # test_weight_sensitivity.TOL["full"]: the bound of test_swiglu_epilogue_full
SWIGLU_ALPHA = 2.0 ** -6
NARROW, WIDE, KS, TS = (2, 8, 33, 60, 64), (65, 96, 128), (1, 2, 8), (1, 4, 5, 70)
GRIDS = (("grid", 2.0 ** -6), ("grid", 2.0 ** -10), ("shift+", 2.0 ** -6), ("shift-", 2.0 ** -10), ("far", 2.0 ** -6))


# ---------------------------------------------------------------------------------------------------- case lists

def route_cases(E):
    """(family, k, T, g, renorm, cap) of one expert count: every (k, T, renorm) with cap = T and 72 on the grid
    families, census at T = E, hot at T = cap = 5 and 72, the tie rows."""
    out = []
    for k in KS:
        if k > E:
            continue
        for renorm in (True, False):
            for T in TS:
                for cap in sorted({T, 72}):
                    if cap >= T:
                        out += [(fam, k, T, g, renorm, cap) for fam, g in GRIDS]
            out += [("census", k, E, g, renorm, cap) for g in (2.0 ** -6, 2.0 ** -10) for cap in (E, 72)]
            out += [("hot", k, cap, 2.0 ** -6, renorm, cap) for cap in (5, 72)]
            out.append(("ties", k, 5 if E > 64 else 3, 0.0, renorm, 72))
    return out


@functools.lru_cache(maxsize=None)
def _logits(fam, E, k, T, g):
    return MR.route_logits(fam, E, k, T, g)


NR_DS, NR_ES, NR_TS = (4, 2048, 2052, 6144, 8192), (2, 4, 8), (1, 4)


@functools.lru_cache(maxsize=None)
def _nr_case(E, T, D):
    return MR.norm_route_case(E, T, D)


LG_DS, LG_TS = (8, 768, 4096, 4104, 8200), (1, 5, 9)
CB_KEYS = [(T, k, D) for T in (1, 5) for k in (1, 2, 8) for D in (4, 68, 256, 2052)]
ALPHAS = (1.0, 0.5, 0.22)


# ------------------------------------------------------------------------------------------- running a route

def _route(dev, lg, k, cap, renorm):
    """ops.moe_route on `dev` over sentinel-filled buffers with stale counts -> numpy arrays (moe_ref.route_arrays)."""
    T, E = lg.shape
    i32 = dict(dtype=torch.int32, device=dev)
    topw = torch.full(((T + 1) * k,), float(SENT), device=dev)
    counts = torch.full((E,), 3, **i32)
    xr, yr = torch.full((E * cap + GUARD,), SENT, **i32), torch.full((E * cap + GUARD,), SENT, **i32)
    sel = torch.full(((T + 1) * k,), SENT, **i32)
    ops.moe_route(torch.from_numpy(lg).to(dev), T, k, topw, counts, xr, yr, cap, renorm, sel=sel)
    return _arrays(topw, counts, xr, yr, sel)


def _arrays(topw, counts, xr, yr, sel):
    return dict(topw=topw.double().cpu().numpy(), counts=counts.cpu().numpy().astype(np.int64),
                xr=xr.cpu().numpy().astype(np.int64), yr=yr.cpu().numpy().astype(np.int64),
                sel=sel.cpu().numpy().astype(np.int64))


def _judge_route(what, out, lg, k, cap, renorm, far=False):
    """Exact outputs and the weight ratio of one route against the fp64 route of `lg`. far: slot 0 is the far
    expert with weight 1, the other weights <= tolerance, k distinct valid experts, lists consistent with sel."""
    T, E = lg.shape
    sel, w = MR.route_ref(lg, k, renorm)
    if far:
        got = out["sel"][:T * k].reshape(T, k)
        assert (got[:, 0] == sel[:, 0]).all(), (what, "slot 0 is not the far expert")
        assert all(len(set(r)) == k and min(r) >= 0 and max(r) < E for r in got.tolist()), (what, got)
        sel = got
    bad, r = MR.route_compare(out, MR.route_arrays(sel, w, E, cap, rows=T + 1), T, E, k, cap, TOL["topw"])
    assert not bad, (what, bad)
    assert r <= 1.0, (what, f"topw {r:.3f} of the tolerance")
    return r


def _route_sweep(dev, E):
    worst = {}
    for fam, k, T, g, renorm, cap in route_cases(E):
        lg = _logits(fam, E, k, T, g)
        out = _route(dev, lg, k, cap, renorm)
        r = _judge_route((fam, E, k, T, g, renorm, cap), out, lg, k, cap, renorm, far=fam == "far")
        worst[fam] = max(worst.get(fam, 0.0), r)
    return worst


def _nonfinite(dev, E, k=8):
    """The NaN / +-inf rows of test_moe_route_nan_rows_stay_in_bounds and test_wide_route_ties_and_nonfinite_rows:
    k distinct valid experts whatever the row holds, an all-NaN row takes the lowest experts, a NaN never beats a
    number, -inf loses to every finite logit; lists consistent with sel, sentinels intact."""
    T, cap, hi = 6, 64, E // 2 + E // 4
    k = min(k, E // 2)
    lg = np.random.default_rng(5).standard_normal((T, E)).astype(np.float32)
    lg[1] = np.nan
    lg[2, 3] = lg[2, hi] = np.inf
    lg[3, :E - k - 1] = -np.inf
    lg[4, 5 % E] = lg[4, hi] = np.nan
    lg[5, E // 2:] = np.nan
    out = _route(dev, lg, k, cap, True)
    s = out["sel"][:T * k].reshape(T, k)
    assert all(len(set(r)) == k and min(r) >= 0 and max(r) < E for r in s.tolist()), s
    assert s[1].tolist() == list(range(k))
    assert sorted(s[3].tolist()) == sorted(MR.rank(lg[3].astype(np.float64), k).tolist())
    assert 5 % E not in s[4] and hi not in s[4] and (s[5] < E // 2).all()
    want, _ = MR.route_ref(lg[:1], k)
    assert s[0].tolist() == want[0].tolist()
    ref = MR.route_arrays(s, out["topw"][:T * k], E, cap, rows=T + 1)
    bad, _ = MR.route_compare(out, ref, T, E, k, cap, 1.0)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------ CPU tests

def test_families_are_what_they_claim():
    """grid rows are permutations and exact after the shift; census gives every expert k rows, once per slot; hot
    fills k lists to T and leaves the rest empty; the tie rows resolve to the lowest index."""
    for E in NARROW + WIDE:
        for k in (k for k in KS if k <= E):
            for fam, g in GRIDS[:4]:
                lg = _logits(fam, E, k, 5, g).astype(np.float64)
                d = lg - lg.max(-1, keepdims=True)
                assert (np.sort(-d / g, -1) == np.arange(E)).all(), (fam, E)
            sel, _ = MR.route_ref(_logits("census", E, k, E, 2.0 ** -10), k)
            assert (sel == (np.arange(E)[:, None] + np.arange(k)[None, :]) % E).all()
            sel, _ = MR.route_ref(_logits("hot", E, k, 72, 2.0 ** -6), k)
            ls = MR.lists_of(sel, E)
            H = MR.hot_experts(E, k)
            assert all(len(ls[e]) == (72 if e in H else 0) for e in range(E))
            assert {0, E - 1} <= set(H) or k == 1
            for j in range(k):
                assert {int(sel[t, j]) for t in range(k)} == set(H)       # every hot expert in every slot
            sel, w = MR.route_ref(_logits("ties", E, k, 3, 0.0), k)
            assert sel[0].tolist() == list(range(k)) and sel[1].tolist() == list(range(k))
            if k < E:       # the k - 1 leaders, then the lowest index of the tie across the cut
                assert sel[2].tolist() == [E - 1 - j for j in range(k - 1)] + [0]
            if E == 128 and k == 8:
                assert sel[3].tolist() == [3, 67, 0, 1, 2, 4, 5, 6] and sel[4].tolist() == list(range(64, 72))
    p = np.exp(-2.0 ** -10 * np.arange(3.0))
    assert abs((p[0] - p[1]) / p[0] - 9.8e-4) < 1e-5


def test_norm_route_logits_are_separated():
    """The fp64 logits of every norm + route case (the f16-rounded wr against the fp64 normed rows) follow the grid C
    and lie >= 100x the logit tolerance TOL_L * B apart; so do those of the folded-route cases (_fold_case)."""
    cases = [_nr_case(E, T, D) for E in NR_ES for T in NR_TS for D in NR_DS]
    cases += [_fold_case(t, D, E, M) for t in FOLD_TYPES for D in (256, 2048) for E in FOLD_ES for M in (1, 4)]
    for c in cases:
        lg, B = MR.logit_ref(c["n"], c["wr"])
        s = np.sort(lg, -1)
        gap = (s[:, 1:] - s[:, :-1]).min()
        assert gap >= 100 * TOL["logit"] * B.max(), (gap, B.max())
        assert (MR.rank(lg, lg.shape[1]) == MR.rank(c["C"], lg.shape[1])).all()
        assert np.abs(lg - c["C"]).max() < c["g"] / 8


def _noise():
    topw, logit = {}, {}
    for E in NARROW + WIDE:
        for fam, k, T, g, renorm, cap in route_cases(E):
            if fam in ("far", "ties") or cap != 72:
                continue
            lg = _logits(fam, E, k, T, g)
            (sel, w), (sel32, w32) = MR.route_ref(lg, k, renorm), MR.route_emu(lg, k, renorm)
            assert (sel == sel32).all()
            topw[fam] = max(topw.get(fam, 0.0), MR.w_ratio(w32, w, 1.0))
    for E in NR_ES:
        for T in NR_TS:
            for D in NR_DS:
                c = _nr_case(E, T, D)
                h = c["n"].astype(np.float16).astype(np.float64)
                ref, B = MR.logit_ref(h, c["wr"])
                l32 = MR.logit_emu(h, c["wr"], 4)
                logit["norm-route"] = max(logit.get("norm-route", 0.0), MR.logit_ratio(l32, ref, B))
                for k in (1, E):
                    (sel, w), (sel32, w32) = MR.route_ref(l32, k), MR.route_emu(l32, k)
                    assert (sel == sel32).all()
                    topw["norm-route"] = max(topw.get("norm-route", 0.0), MR.w_ratio(w32, w, 1.0))
    for E in (2, 8):
        for T in LG_TS:
            for D in LG_DS:
                h, wr = MR.logit_case("gauss", E, T, D)
                ref, B = MR.logit_ref(h, wr)
                logit["gauss"] = max(logit.get("gauss", 0.0), MR.logit_ratio(MR.logit_emu(h, wr), ref, B))
                hi, wi = MR.logit_case("integer", E, T, D)
                assert (MR.logit_emu(hi, wi) == MR.logit_ref(hi, wi)[0]).all()
                assert (np.abs(hi) @ np.abs(wi).T).max() < 2 ** 24
    return topw, logit


def test_emulated_noise_bounds_tol():
    """EMU is the largest ratio of the emulated fp32 arithmetic against fp64 over this module's inputs, within a
    factor 2 below the constant: the measurement, not a guess. The swiglu cases' products stay inside the emulated
    noise that test_weight_sensitivity pins for its full family (1.7e-4 of B)."""
    topw, logit = _noise()
    for name, per in (("topw", topw), ("logit", logit)):
        print(f"emulated noise {name}: " + " ".join(f"{k}={v:.2e}" for k, v in per.items()))
        worst = max(per.values())
        assert EMU[name] / 2 <= worst <= EMU[name], (name, worst)
    import qblocks as QB
    x = MR.acts("full", 16)
    for e in (0, 64, 127):
        raw = MR.expert_raw(GGMLType.Q4_K, "full", e)
        emu = x @ QB.emulate(QB.fields(GGMLType.Q4_K, raw, MR.ROWS, MR.K)).T
        W, mag = MR.expert_dense(GGMLType.Q4_K, "full", e), MR.expert_mag(GGMLType.Q4_K, "full", e)
        r = np.abs(emu - x @ W.T) / (np.abs(x) @ mag.T)
        assert r.max() <= 1.7e-4, r.max()


def _stand_in(e):
    """A cheap exact expert for the CPU plan tests: integers that name expert, row and column."""
    r, c = np.arange(16)[:, None], np.arange(MR.K)[None, :]
    return ((7 * e + 3 * r + c) % 13 - 6).astype(np.float64)


def _expert_points():
    """(plan, M, selected, block) over the GPU tests' routes (test_expert_launches_integer)."""
    for route, T, cap, sel, cfg in EXPERT_ROUTES:
        block = 128 if cfg and cfg["mode"] == 2 and cfg["rt"] == 2 else 64
        for name, order in _plans(sel, T):
            yield MR.make_plan(name, T, 8, 128, cap, order), T, sel, block, (route, name, order)


def test_fault_models_are_rejected():
    """Every fault model applied to the reference alone: rejected by >= 10x the tolerance or by an exact output at
    every grid point where it changes the mathematical result; the points where it cannot are those of the module
    docstring, and nowhere else."""
    seen = {}

    def note(name, hit, can):
        assert hit or not can, (name, "not rejected where it changes the result")
        seen[name] = seen.get(name, 0) + int(hit)

    # route
    for E in NARROW + WIDE:
        for fam, k, T, g, renorm, cap in route_cases(E):
            if fam == "far" or cap != 72:
                continue
            lg = _logits(fam, E, k, T, g)
            sel, w = MR.route_ref(lg, k, renorm)
            ref = MR.route_arrays(sel, w, E, cap + 1)
            for name, arr in MR.route_faults(sel, w, E, cap):
                bad = arr is not None and MR.route_compare(arr, ref, T, E, k, cap + 1, TOL["topw"])[0]
                note(name, bool(bad), arr is not None)
            for name, can in (("R4 renormalisation flipped", k < E),
                              ("R5 sum over experts 0..63", E > 64 and not renorm),
                              ("R6 tie to the higher index", fam == "ties")):
                s2, w2 = MR.route_ref(lg, k, renorm, fault=name)
                bad, r = MR.route_compare(MR.route_arrays(s2, w2, E, cap + 1), ref, T, E, k, cap + 1, TOL["topw"])
                note(name, bool(bad) or r >= 10, can and (name[:2] != "R6" or k < E))
                if not can and name[:2] != "R6":
                    assert not bad and r <= 1e-3, (name, "changes a result it should not", E, k, fam)
    lg = _logits("far", 128, 8, 5, 2.0 ** -6)
    lg = np.roll(lg, 70 - int(lg[0].argmax()), 1)
    _, w32 = MR.route_emu(lg, 8, low_max=True)
    note("R5 maximum over experts 0..63 (emulated)", not np.isfinite(w32[0]).all(), True)
    # router logits
    for E in (2, 8):
        for T in LG_TS:
            for D in LG_DS:
                for fam in ("gauss", "integer"):
                    h, wr = MR.logit_case(fam, E, T, D)
                    ref, B = MR.logit_ref(h, wr)
                    for name in MR.LOGIT_FAULTS:
                        f, _ = MR.logit_ref(h, wr, name)
                        can = not (name.endswith("token") and T == 1) and not (name[:2] == "L2" and D <= 4096)
                        if fam == "integer":
                            note(name, not np.array_equal(f, ref), can)
                        else:
                            note(name + " (gauss)", MR.logit_ratio(f, ref, B) >= 10 * TOL["logit"], can)
    # combine
    for T, k, D in CB_KEYS:
        for alpha in ALPHAS:
            for set_ in (False, True):
                for fam in ("tag", "gauss"):
                    resid, y, wt = MR.combine_case(fam, T, k, D)
                    ref, size = MR.combine_ref(resid, y, wt, alpha, set_)
                    for name in MR.COMBINE_FAULTS:
                        f, _ = MR.combine_ref(resid, y, wt, alpha, set_, name)
                        can = {"C1": T > 1, "C2": alpha != 1 and not set_, "C3": set_, "C4": D % 256 != 0}[name[:2]]
                        if fam == "tag":
                            cands = MR.combine_tag_candidates(resid, y, wt, alpha, set_)
                            f32 = f.astype(np.float32).astype(np.float64)
                            note(name, not any(np.array_equal(f32, c) for c in cands), can)
                        else:
                            note(name + " (gauss)", R.x_ratio(f, ref, size, 2 * k + 2) >= 10, can)
    # expert launches
    x = MR.acts("integer", 130 * 8 + GUARD)
    for p, M, sel, block, what in _expert_points():
        for down in (False, True):
            ref = MR.expert_ref(p, _stand_in, x, M, down, sel, block)
            for name in MR.EXPERT_FAULTS:
                f = MR.expert_ref(p, _stand_in, x, M, down, sel, block, fault=name)
                hit = not np.array_equal(f, ref)
                cnt = p["counts"]
                served = set(p["sel"].tolist()) if sel else range(128)      # the experts whose tiles run at all
                can = {"X1": True, "X2": p["cap"] != p["T"] and (cnt[1:] > 0).any(), "X3": cnt.max() > block,
                       "X4": any(cnt[e] != cnt[(e + 1) % 128] for e in served if 0 <= e < 128),
                       "X5": sel and what[1] == "pairs", "X6": what[1] in ("hot", "last") and cnt.max() > 1}[name[:2]]
                note(name, hit, can)
                assert can or not hit or name[:2] in ("X1", "X6"), (name, what, "changes a result it should not")
    print("rejections per fault: " + ", ".join(f"{k} {v}" for k, v in seen.items()))
    assert all(v > 0 for v in seen.values()), seen


def test_old_inputs_cannot_see():
    """The older tests' inputs and checks on the CPU: R3 passes test_moe_route; on test_expert_table_launches' own
    logits no expert count passes 11 and no expert repeats at T = 1, 3, so X3 and X5 change nothing; test_router_logits
    has no tail past a 4096-column pass, so L2 changes nothing. This module's checks reject all four."""
    # test_moe_route: randn logits, T = 10, E = 8, k = 2; topw close, then token sets of xrows per expert
    T, E, k = 10, 8, 2
    lg = torch.randn(T, E, generator=torch.Generator().manual_seed(0)).numpy()
    sel, w = MR.route_ref(lg, k)
    ref = MR.route_arrays(sel, w, E, 65)
    name, arr = [f for f in MR.route_faults(sel, w, E, 64) if f[0].startswith("R3")][0]
    for ex in range(E):        # its check, on the faulty lists
        c = int(arr["counts"][ex])
        assert sorted(arr["xr"][ex * 65:ex * 65 + c].tolist()) == sorted(t for t in range(T) if ex in sel[t].tolist())
    assert int(arr["counts"].sum()) == T * k and np.array_equal(arr["topw"], ref["topw"])
    assert MR.route_compare(arr, ref, T, E, k, 65, TOL["topw"])[0]
    # test_expert_table_launches: its generator, its logits
    worst = 0
    for T in (1, 3, 16, 70):
        g = torch.Generator().manual_seed(100 + T)
        torch.randn(T, 256, generator=g)
        sel, _ = MR.route_ref(torch.randn(T, 128, generator=g).numpy(), 8)
        ls = MR.lists_of(sel, 128)
        cap = (T + 63) // 64 * 64
        worst = max(worst, max(len(v) for v in ls.values()))
        p = dict(T=T, k=8, E=128, cap=cap, sel=sel.reshape(-1), counts=np.array([len(ls[e]) for e in range(128)]),
                 xrows=np.zeros(128 * cap, np.int64), yrows=np.zeros(128 * cap, np.int64))
        for e, pr in ls.items():
            for i, (a, b) in enumerate(pr):
                p["xrows"][e * cap + i], p["yrows"][e * cap + i] = a, b
        x = MR.acts("integer", T * 8 + GUARD)
        selected = T <= 3
        if selected:
            assert len(set(sel.reshape(-1).tolist())) == T * 8
        ref = MR.expert_ref(p, _stand_in, x, T, False, selected)
        for name in MR.EXPERT_FAULTS:
            if name[:2] in ("X3", "X5"):
                assert np.array_equal(MR.expert_ref(p, _stand_in, x, T, False, selected, fault=name), ref), (name, T)
    assert worst == 11
    # test_router_logits: D in {4096, 1024, 768}
    for T, E, D in ((5, 8, 4096), (7, 4, 1024), (33, 2, 768)):
        h, wr = MR.logit_case("gauss", E, T, D)
        assert np.array_equal(MR.logit_ref(h, wr, MR.LOGIT_FAULTS[3])[0], MR.logit_ref(h, wr)[0])
    h, wr = MR.logit_case("gauss", 8, 5, 8200)
    ref, B = MR.logit_ref(h, wr)
    assert MR.logit_ratio(MR.logit_ref(h, wr, MR.LOGIT_FAULTS[3])[0], ref, B) >= 10 * TOL["logit"]


@pytest.mark.parametrize("E", NARROW + WIDE)
def test_cpu_twin_route(E):
    """ops.moe_route on CPU tensors through every family, the tie rows and the non-finite rows included: the same
    judge as the kernels (lowest unused expert on ties, NaNs last)."""
    _route_sweep("cpu", E)
    if E >= 8:
        _nonfinite("cpu", E)


def test_cpu_twins_logits_norm_route_combine():
    """The CPU twins of ops.router_logits, ops.moe_norm_route and ops.moe_combine through the GPU tests' cases."""
    for E in (2, 8):
        for T in LG_TS:
            for D in LG_DS:
                for fam in ("gauss", "integer"):
                    _run_logits("cpu", fam, E, T, D, zero=True)
    for E in NR_ES:
        for T in NR_TS:
            for D in (4, 2052, 6144):
                for k in sorted({1, 2, E}):
                    _run_norm_route("cpu", E, k, T, D)
    for key in CB_KEYS:
        for alpha in ALPHAS:
            for set_ in (False, True):
                for fam in ("tag", "gauss"):
                    _run_combine("cpu", fam, *key, alpha, set_, pad=12)


# ------------------------------------------------------------------------------------------- GPU: routing

@pytest.mark.gpu
@pytest.mark.parametrize("E", NARROW + WIDE)
def test_route_families(gpu, E):
    """moe_route_kernel (E <= 64) / moe_route_wide_kernel: every family, k 1 / 2 / 8, T 1 .. 70 and T = E, both
    renorm settings, cap = T and 72, stale counts, sentinels in every list entry past a count."""
    worst = _route_sweep(gpu, E)
    print(f"MOE_RATIO route E={E} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("E", [8, 64, 96, 128])
def test_route_nonfinite_rows(gpu, E):
    _nonfinite(gpu, E)


def _run_norm_route(dev, E, k, T, D, renorm=True):
    """ops.moe_norm_route over strided x / h with NaN / sentinel columns past D; h by the norm bound, the logits
    against the fp64 product of the stored h, the route against the fp64 route of the stored logits (and the grid
    C the case was built for). Returns (h ratio, logit ratio / TOL, topw ratio)."""
    c = _nr_case(E, T, D)
    cap = T
    i32 = dict(dtype=torch.int32, device=dev)
    x = torch.full((T + 1, D + 8), float("nan"))
    x[:T, :D] = torch.from_numpy(c["x"])
    x = x.to(dev)
    h = torch.full((T + 1, D + 12), float(SENT), dtype=ops.ACT_DTYPE, device=dev)
    lg = torch.full((T + 1, E), float(SENT), device=dev)
    topw = torch.full(((T + 1) * k,), float(SENT), device=dev)
    counts = torch.full((E,), 3, **i32)
    xr, yr = torch.full((E * cap + GUARD,), SENT, **i32), torch.full((E * cap + GUARD,), SENT, **i32)
    sel = torch.full(((T + 1) * k,), SENT, **i32)
    wr = torch.from_numpy(c["wr"]).to(torch.float16).contiguous().to(dev)
    assert ops.moe_norm_route(x[:, :D], torch.from_numpy(c["nw"]).to(dev), c["eps"], wr, h[:, :D], lg, T, k, topw,
                              counts, xr, yr, cap, renorm, sel=sel)
    return _judge_norm_route((E, k, T, D), c, h, lg, _arrays(topw, counts, xr, yr, sel), k, cap, renorm)


def _judge_norm_route(what, c, h, lg, out, k, cap, renorm, n=None):
    n = c["n"] if n is None else n
    T, D = n.shape
    E = c["wr"].shape[0]
    hn, lgn = h.double().cpu().numpy(), lg.double().cpu().numpy()
    rh, where = R.rms_ratio(hn, n, R.F16, TOL["norm"])
    assert rh <= 1.0, (what, f"h {rh:.3f} of the tolerance at {where}")
    assert (lgn[T:] == SENT).all(), (what, "logit rows past T were written")
    ref, B = MR.logit_ref(hn[:T, :D], c["wr"])
    rl = MR.logit_ratio(lgn[:T], ref, B) / TOL["logit"]
    assert rl <= 1.0, (what, f"logits {rl:.3f} of the tolerance")
    l32 = lg[:T].float().cpu().numpy()
    assert (MR.route_ref(l32, k)[0] == MR.rank(c["C"], k)).all(), (what, "the stored logits leave the grid's order")
    return rh, rl, _judge_route(what, out, l32, k, cap, renorm)


@pytest.mark.gpu
@pytest.mark.parametrize("D", NR_DS)
def test_moe_norm_route_families(gpu, D):
    """moe_norm_route_kernel<2 / 4 / 8>: k 1 / 2 / E, T 1 / 4, D 4 .. 8192 (6144: a partial fourth load round),
    both renorm settings."""
    worst = np.zeros(3)
    for E in NR_ES:
        for T in NR_TS:
            for k in sorted({1, 2, E}):
                for renorm in (True, False):
                    worst = np.maximum(worst, _run_norm_route(gpu, E, k, T, D, renorm))
    print(f"MOE_RATIO norm_route D={D} h={worst[0]:.3f} logits={worst[1]:.3f} topw={worst[2]:.3f}")
    T5 = torch.zeros(8, D, device=gpu)
    assert not ops.moe_norm_route(T5, torch.ones(D, device=gpu), 1e-5, torch.zeros(2, D, dtype=torch.float16, device=gpu),
                                  torch.zeros(8, D, dtype=ops.ACT_DTYPE, device=gpu), torch.zeros(8, 2, device=gpu), 5, 1,
                                  torch.zeros(16, device=gpu), torch.zeros(2, dtype=torch.int32, device=gpu),
                                  torch.zeros(16, dtype=torch.int32, device=gpu),
                                  torch.zeros(16, dtype=torch.int32, device=gpu), 8)      # > 4 tokens: not taken


FOLD_TYPES, FOLD_ES = (GGMLType.Q4_K, GGMLType.Q8_0), (2, 8, 33, 64)


@functools.lru_cache(maxsize=None)
def _fold_case(t, D, E, M):
    """The o projection [D, 256] on qblocks' integer family with {-1, 0, 1} inputs, alpha 1/2 and an integer
    residual: the new residual rows are exact, and the norm + route case is built on them."""
    import qblocks as QB
    from nats_llm_studio_amd.gguf import quants as Q
    raw = QB.structured_blocks(t, D, 256, "integer", np.random.default_rng(31 + int(t) + D))
    W = Q.dequantize(raw, t, (D, 256)).astype(np.float64)
    rng = np.random.default_rng(D + E + M)
    xin = MR.acts("integer", 16, seed=9)
    base = rng.integers(-64, 65, (M, D)).astype(np.float64)
    xnew = base + 0.5 * (xin[:M] @ W.T)
    c = MR.norm_route_case(E, M, D, rows=xnew)
    assert np.array_equal(c["x"].astype(np.float64), xnew)
    c.update(raw=raw, xin=xin, base=base, t=t)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("t", FOLD_TYPES, ids=lambda t: t.name)
def test_folded_route(gpu, t):
    """route_rows (ops.qgemv_add_norm_route: o projection += into the residual, then norm, router and route in the
    last workgroup): E 2 / 8 / 33 / 64, M 1 / 4, D 256 / 2048. The residual is exact; h, logits, route as above."""
    worst = np.zeros(3)
    for D in (256, 2048):
        for E in FOLD_ES:
            for M in (1, 4):
                for k in sorted({1, min(2, E), min(8, E)}):
                    c = _fold_case(t, D, E, M)
                    cap = 4
                    i32 = dict(dtype=torch.int32, device=gpu)
                    w = ops.QWeight(c["raw"], t, D, 256, gpu)
                    x = torch.full((M + 1, D + 8), float(SENT), device=gpu)
                    x[:M, :D] = torch.from_numpy(c["base"]).float().to(gpu)
                    h = torch.full((M + 1, D + 12), float(SENT), dtype=ops.ACT_DTYPE, device=gpu)
                    lg = torch.full((M + 1, E), float(SENT), device=gpu)
                    topw = torch.full(((M + 1) * k,), float(SENT), device=gpu)
                    counts = torch.full((E,), 3, **i32)
                    xr, yr = torch.full((E * cap + GUARD,), SENT, **i32), torch.full((E * cap + GUARD,), SENT, **i32)
                    sel = torch.full(((M + 1) * k,), SENT, **i32)
                    counter = torch.zeros(1, **i32)
                    xin = torch.from_numpy(c["xin"]).to(ops.ACT_DTYPE).to(gpu)
                    wr = torch.from_numpy(c["wr"]).to(torch.float16).contiguous().to(gpu)
                    assert ops.qgemv_add_norm_route(ops.Seg(w), xin, x[:, :D], torch.from_numpy(c["nw"]).to(gpu), h[:, :D],
                                                    M, 0.5, c["eps"], counter, wr, lg, k, topw, counts, xr, yr, cap,
                                                    sel=sel), (t, D, E, M, k)
                    xn = x.double().cpu().numpy()
                    assert np.array_equal(xn[:M, :D], c["x"].astype(np.float64)), "the residual is not exact"
                    assert (xn[M:] == SENT).all() and (xn[:, D:] == SENT).all() and int(counter) == 0
                    worst = np.maximum(worst, _judge_norm_route((t.name, D, E, M, k), c, h, lg,
                                                                _arrays(topw, counts, xr, yr, sel), k, cap, True))
    print(f"MOE_RATIO folded_route {t.name} h={worst[0]:.3f} logits={worst[1]:.3f} topw={worst[2]:.3f}")


# ------------------------------------------------------------------------------------------- GPU: router logits

def _run_logits(dev, fam, E, T, D, zero):
    h64, wr64 = MR.logit_case(fam, E, T, D)
    h = torch.full((T + 2, D + 16), float("nan"), dtype=ops.ACT_DTYPE)
    h[:T, :D] = torch.from_numpy(h64).to(ops.ACT_DTYPE)
    lg = torch.full((T + 2, E), float(SENT), device=dev)
    counts = torch.full((E * 3,), 5, dtype=torch.int32, device=dev)
    wr = torch.from_numpy(wr64).to(torch.float16).contiguous().to(dev)
    ops.router_logits(h.to(dev), wr, lg, T, zero=counts if zero else None)
    out = lg.double().cpu().numpy()
    assert (out[T:] == SENT).all(), "rows past T were written"
    assert (counts.cpu() == (0 if zero else 5)).all()
    ref, B = MR.logit_ref(h64, wr64)
    if fam == "integer":
        assert np.array_equal(out[:T], ref), (fam, E, T, D)
        return 0.0
    r = MR.logit_ratio(out[:T], ref, B) / TOL["logit"]
    assert r <= 1.0, ((fam, E, T, D), f"{r:.3f} of the tolerance")
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("D", LG_DS)
def test_router_logits_families(gpu, D):
    """router_logits_kernel<2 / 4 / 8>: T 1 / 5 / 9, rows wider than D with NaN past it, zero= given and absent;
    4104 / 8200: the one-thread tail of a second 4096-column pass. integer: equality."""
    worst = 0.0
    for E in (2, 4, 8):
        for T in LG_TS:
            for zero in (True, False):
                worst = max(worst, _run_logits(gpu, "gauss", E, T, D, zero))
                _run_logits(gpu, "integer", E, T, D, zero)
    print(f"MOE_RATIO router_logits D={D} gauss={worst:.3f} integer=equal")


# ------------------------------------------------------------------------------------------------- GPU: combine

def _run_combine(dev, fam, T, k, D, alpha, set_, pad):
    resid, y, wt = MR.combine_case(fam, T, k, D)
    x = torch.full((T + 1, D + pad), float(SENT), device=dev)
    x[:T, :D] = torch.from_numpy(resid).float().to(dev)
    yd = torch.full((T * k + 1, D), float("nan"), device=dev)
    yd[:T * k] = torch.from_numpy(y).float().to(dev)
    ops.moe_combine(yd, torch.from_numpy(wt).float().reshape(-1).to(dev), T, k, x[:, :D], alpha, set_)
    out = x.double().cpu().numpy()
    what = (fam, T, k, D, alpha, set_, pad)
    assert (out[T:] == SENT).all() and (out[:, D:] == SENT).all(), (what, "past the rows was written")
    if fam == "tag":
        cands = MR.combine_tag_candidates(resid, y, wt, alpha, set_)
        ok = np.zeros(resid.shape, bool)
        for c in cands:
            ok |= out[:T, :D] == c
        assert ok.all(), (what, "not equal")
        return 0.0
    ref, size = MR.combine_ref(resid, y, wt, float(np.float32(alpha)), set_)
    r = R.x_ratio(out[:T, :D], ref, size, 2 * k + 2)
    assert r <= 1.0, (what, f"{r:.3f} of the tolerance")
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("set_", [False, True], ids=["add", "set"])
def test_moe_combine_families(gpu, set_):
    """moe_combine_kernel<SET>: T 1 / 5, k 1 / 2 / 8, D 4 .. 2052, ldr = D and D + 12, alpha 1 / 0.5 / 0.22 onto a
    non-zero residual. tag: equality."""
    worst = 0.0
    for key in CB_KEYS:
        for alpha in ALPHAS:
            for pad in (0, 12):
                worst = max(worst, _run_combine(gpu, "gauss", *key, alpha, set_, pad))
                _run_combine(gpu, "tag", *key, alpha, set_, pad)
    print(f"MOE_RATIO combine set={set_} gauss={worst:.3f} tag=equal")


# ------------------------------------------------------------------------------------------ GPU: expert launches

E_, K_ = 128, 8
EXPERT_ROUTES = [("A selected", 1, 1, True, None), ("A selected", 3, 3, True, None),
                 ("A unselected", 16, 18, False, None), ("A unselected", 32, 34, False, None),
                 ("mode 1", 70, 72, False, dict(mode=1, waves=8, rt=1, ks=1)),
                 ("mode 2 rt 1", 70, 72, False, dict(mode=2, waves=8, rt=1, ks=1)),
                 ("mode 2 rt 2", 130, 136, False, dict(mode=2, waves=8, rt=2, ks=1))]


def _plans(selected, T):
    pairs = [("pairs", "")] if selected and T == 3 else []
    return [("hot", "desc"), ("hot", "shuffled"), ("diag", ""), ("last", "")] + pairs


_BANKS = {}


def _bank(dev, t, fam):
    """The 128 experts of one (type, family) on the device with their table (shared, read-only)."""
    if (t, fam) not in _BANKS:
        ws = [ops.QWeight(MR.expert_raw(t, fam, e), t, MR.ROWS, MR.K, dev) for e in range(E_)]
        _BANKS[t, fam] = (ws, ops.ExpertTable(ws))
    return _BANKS[t, fam]


def _dev_plan(p, dev):
    return {n: torch.from_numpy(p[n]).to(torch.int32).to(dev) for n in ("xrows", "yrows", "counts", "sel")}


def _launch_experts(bank, p, dv, x, M, down, table, selected, cfg, epi="f32", alpha=1.0):
    ws, tab = bank
    T, k, E, cap = p["T"], p["k"], p["E"], p["cap"]
    xm, ym, cn = (dv["yrows"] if down else dv["xrows"]), dv["yrows"], dv["counts"]
    y = torch.full((T * k + GUARD, MR.ROWS if epi == "f32" else MR.ROWS // 2), float(SENT),
                   dtype=torch.float32 if epi == "f32" else ops.ACT_DTYPE, device=x.device)
    cfg = cfg or {}

    def sel(s0):
        return (dv["sel"], T * k, s0) if selected else None
    if table:
        ops.qgemv([ops.Seg(ws[0], 0, xm, ym, cn)], x, y, M, alpha, epi, sel=sel(0), table=(tab, cap), **cfg)
    else:
        for s0 in range(0, E, 8):
            segs = [ops.Seg(ws[e], 0, xm[e * cap:], ym[e * cap:], cn[e:e + 1]) for e in range(s0, s0 + 8)]
            ops.qgemv(segs, x, y, M, alpha, epi, sel=sel(s0), **cfg)
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("route,T,cap,selected,cfg", EXPERT_ROUTES,
                         ids=[f"{r[0].replace(' ', '_')}-T{r[1]}" for r in EXPERT_ROUTES])
def test_expert_launches_integer(gpu, route, T, cap, selected, cfg):
    """Hand-written row lists (hot descending / shuffled, diag, last, pairs) over 128 integer experts, Q4_K and Q6_K,
    the gate|up shape (xrows -> yrows) and the down shape (yrows -> yrows): through the expert table and as 16
    launches of 8 by-value segments, bit-equal to each other and EQUAL to the fp64 reference, every unlisted row
    still the sentinel."""
    n = 0
    for t in (GGMLType.Q4_K, GGMLType.Q6_K):
        bank = _bank(gpu, t, "integer")
        W = functools.partial(MR.expert_dense, t, "integer")
        for name, order in _plans(selected, T):
            p = MR.make_plan(name, T, K_, E_, cap, order)
            dv = _dev_plan(p, gpu)
            for down in (False, True):
                nx = T * K_ + GUARD if down else 256
                x64 = MR.acts("integer", nx, seed=2 + down)
                x = torch.from_numpy(x64).to(ops.ACT_DTYPE).to(gpu)
                ref = MR.expert_ref(p, W, x64, T, down, selected)
                ys = [_launch_experts(bank, p, dv, x, T, down, table, selected, cfg) for table in (True, False)]
                what = (route, T, t.name, name, order, "down" if down else "gate|up")
                assert torch.equal(ys[0], ys[1]), (what, "table and by-value launches differ")
                got = ys[0].double().cpu().numpy()
                if not np.array_equal(got, ref):
                    rows = np.nonzero((got != ref).any(1))[0]
                    raise AssertionError((what, f"{len(rows)} rows differ, the first {rows[:8].tolist()}"))
                n += 1
    print(f"MOE_RATIO experts {route} T={T}: {n} launches pairs equal")


@pytest.mark.gpu
@pytest.mark.parametrize("route,T,cap,selected,cfg", EXPERT_ROUTES,
                         ids=[f"{r[0].replace(' ', '_')}-T{r[1]}" for r in EXPERT_ROUTES])
def test_expert_launches_swiglu_full(gpu, route, T, cap, selected, cfg):
    """The f16 SwiGLU epilogue of every route on qblocks' full family (Q4_K, Gaussian rows, the hot plan): the
    propagated bound of test_swiglu_epilogue_full per element, table and by-value launches bit-equal."""
    t = GGMLType.Q4_K
    bank = _bank(gpu, t, "full")
    p = MR.make_plan("hot", T, K_, E_, cap, "shuffled")
    dv = _dev_plan(p, gpu)
    x64 = MR.acts("full", 256, seed=4)
    x = torch.from_numpy(x64).to(ops.ACT_DTYPE).to(gpu)
    ys = [_launch_experts(bank, p, dv, x, T, False, table, selected, cfg, "swiglu", SWIGLU_ALPHA)
          for table in (True, False)]
    assert torch.equal(ys[0], ys[1])
    got = ys[0].double().cpu().numpy()
    gi = (np.arange(128) // 8) * 16 + np.arange(128) % 8
    a = SWIGLU_ALPHA
    full = MR.expert_ref(p, lambda e: MR.expert_dense(t, "full", e), x64, T, False, selected)
    mag = MR.expert_ref(p, lambda e: MR.expert_mag(t, "full", e), np.abs(x64), T, False, selected)
    listed = np.zeros(len(got), bool)
    for e in np.nonzero(p["counts"])[0]:
        listed[p["yrows"][e * cap:e * cap + int(p["counts"][e])]] = True
    assert listed.sum() == T * K_ and (got[~listed] == SENT).all()
    ref, lim = MR.swiglu_bound(a * full[listed][:, gi], a * full[listed][:, gi + 8], a * mag[listed][:, gi],
                               a * mag[listed][:, gi + 8], GEMV_TOL)
    r = np.abs(got[listed] - ref) / lim
    r = float(np.where(np.isfinite(r), r, np.inf).max())
    print(f"MOE_RATIO experts swiglu {route} T={T} {r:.3f} of the propagated bound")
    assert r <= 1.0, (route, T, r)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(1, 8, 1, 3), (2, 8, 2, 3), (3, 4, 6, 3)], ids=lambda c: "m%dw%dr%dk%d" % c)
def test_mapped_splitk_down_integer(gpu, cfg):
    """The mapped split-K down projection (slabs indexed by the y row, M = T * k) over 4 by-value integer experts
    [256, 768], the hot plan (T = 70, k = 2, every y row written once): EQUAL to the reference."""
    import qblocks as QB
    from nats_llm_studio_amd.gguf import quants as Q
    E, k, T, cap, K = 4, 2, 70, 72, 768
    t = GGMLType.Q4_K
    raws = [QB.structured_blocks(t, MR.ROWS, K, "integer", np.random.default_rng(900 + e)) for e in range(E)]
    Ws = [Q.dequantize(r, t, (MR.ROWS, K)).astype(np.float64) for r in raws]
    ws = [ops.QWeight(r, t, MR.ROWS, K, gpu) for r in raws]
    p = MR.make_plan("hot", T, k, E, cap, "shuffled")
    dv = _dev_plan(p, gpu)
    x64 = MR.acts("integer", T * k + GUARD, K, seed=6)
    x = torch.from_numpy(x64).to(ops.ACT_DTYPE).to(gpu)
    ref = MR.expert_ref(p, lambda e: Ws[e], x64, T * k, True, nrows=T * k)
    y = torch.full((T * k, MR.ROWS), float(SENT), device=gpu)
    segs = [ops.Seg(ws[e], 0, dv["yrows"][e * cap:], dv["yrows"][e * cap:], dv["counts"][e:e + 1]) for e in range(E)]
    mode, waves, rt, ks = cfg
    ops.qgemv(segs, x, y, T * k, epi="f32", mode=mode, waves=waves, rt=rt, ks=ks)
    assert np.array_equal(y.double().cpu().numpy(), ref), cfg
