"""The sampler (csrc/kernels/sample.hip: sample_kernel, sample_decode_kernel, sample_decode_cand_kernel, topc_kernel with
hist_threshold, sample_topk_fast and draw_index_order) against a reference written from the definition in numpy fp64
(tests/sampler_ref.py), with inputs and variates that notice ONE dropped, leaked or misdrawn token.

Metric. A draw with variate u is right when u lies in the drawn token's interval [c_lo, c_hi) of the reference's
index-order CDF, widened by g on both sides. Designed variates sit at interval midpoints and 4 g inside both interval ends,
all targeted intervals are >= 8 g wide, so for them the metric is token == reference token, with no allowance. Only
u = 0, u = 1 - 2^-24 and the (seed, position) variates of the decode kernels can land within 4 g of a step; those are
judged by the widened interval.
  EMU = 2.0e-7 (measured 1.79e-7: test_emulated_noise_bounds_g), the largest |cdf32 - cdf64| of a float32 emulation of
  the kernel's sums (per-tile butterfly, per-thread run, wave and block scans, the 1024-thread scan of the fast path,
  float32 exponent arguments) over this module's inputs -- two rows of every carriers case and one of every other
  case, for run time, so the pinned figure is a lower bound of the quantity over all rows; g = 4 EMU = 8.0e-7.
  A cut is fair when the reference's logit gap at it exceeds hist_threshold's stated resolution (b - a) / NB^2 plus
  one ulp of the largest logit (sampler_ref.ref_row: margins), the mass on both sides of a top-p cut is >= 8 g away
  from top_p Z, and the kept tokens more than 30 temperatures down hold < g in all. Smallest margins per family
  (logit margin as a multiple of the rule, mass, narrowest targeted interval):
    carriers   9.3e5 / 1.1e-2 / 9.6e-3        cuts    1.4e3 / 6.4e-5 / 1.8e-4      ties  240 (exact ties apart) / 7.3e-3 / 1.7e-4
    masked     407 / - / 6.4e-6 (= 8 g)       offset  1.72 / - / 2.9e-3            penalties  3.1e3 / 4.3e-3 / 4.2e-3
  offset and masked rows are random: a row whose margin fails the rule is left out (offset: of 64 rows 64 / 24 / 56 /
  56 stay at k = 40 and 64 / 0 / 20 / 20 at k = 300) or drawn at its widest interval (masked). The kept tokens more
  than 30 T down hold at most 1.4e-14 of the mass.
  On the random rows of the older test at most 1 % of the variates may lie within g of a step (measured: 0 of 192).

Families (sampler_ref): carriers (48 planted tokens of comparable weight at ids 0, 63, 64, 65, V - 2, V - 1, 65535,
65536, the last partial tile and both sides of thread-run boundaries 64 per t, every other logit 40 T lower: the
position logic of draw_index_order and of the compaction, V from 1 to 262144, per = 1 .. 4), cuts (geometric weights
scattered over the ids: every top-k / min-p / top-p cut, inside drawn, outside never), ties (exact ties across the
k-th place and the top-p cut at ids 1024 j - 1 / 1024 j, all-equal rows, 600 ties that overflow CCAP), masked (-inf on
all but m tokens under top_k 40, NaN among them, all-NaN / all -inf rows), offset (rows far from zero: N(50, 1),
N(-1000, 0.01), +-1e4), penalties (repeats, ids -1 and >= V, both signs and a zero, a full window, a token moved across
the cut each way, penalised arg-max), mixed launch (rows of all of these with their own params and n_hist in one launch,
ld = V + 24 with 1e30 in the padding, unaligned row start).

Findings (float32 emulation of hist_threshold's count mode, test_threshold_emulation; the kept set differs from the
definition's in this many rows before the fix / after it):
  1  top_k >= finite count: the fall-through returned b - 1024 / scale, above the true minimum in
     masked m = 3 / 10 / 40: 11 / 12 / 18 of 64 rows before, 0 after (m = 1 and 41: 0)
  2  returned edge against binning: offset N(50,1) / N(-1000,.01) / +1e4 / -1e4 at k = 40: 0 of 64 / 3 of 30 / 5 of 58 /
     5 of 58 rows lose the k-th token before, 0 after; at k = 300: 0 / - / 6 of 29 / 6 of 29 before, 0 after
  The fix: the second pass selects the crossing bin's logits by the same bin expression as the first, and the
  threshold is the smallest logit counted toward the target (an LDS minimum per sub-bin), never a computed edge; a
  search without a crossing returns the lower end of the range. No pass over the vocabulary was added.
  The MI355X confirmed both, on sample_kernel with the kernel as it was (rows whose token differed from the
  reference's):
    finding 1  masked m = 3 / 10 / 40 under top_k 40: 11 / 11 / 9 of 64 rows, the same under top_k 300 (general path);
               m = 41 under top_k 300: 7 of 64; m = 10 with NaN entries: 10 of 64; m = 1, and m = 41 under top_k 40: 0
    finding 2  offset N(-1000,.01) k 40: 2 of 24; +1e4 and -1e4: 5 of 56 at k 40, 5 of 20 at k 300; N(50,1): 0 of 64
  (fewer rows than the emulation counts where the dropped token's interval is narrower than 8 g and the row is drawn
  elsewhere). After the fix all 147 GPU cases pass, and every draw of every entry point -- sample_kernel,
  sample_decode_kernel, sample_decode_cand_kernel -- equals the reference's token: the widened interval was never
  needed, the largest |u - nearest step| / g among draws accepted with another token is 0 on all three.
  topc_kernel ordered -0.0 below +0.0 (the radix key of the sign bit), so ties of zeros across the cut did not take
  the lowest indices (test_topc_kernel_reference, row 3, failed at C = 1, 128, 1024); its keys now treat the two
  zeros as one value, as logprob_kernel's always did.
  tools/sample_bench.py (B 512, V 128256, median us of 10; parent twice | fix twice, alternating in one session):
    service (T 0.7, top-p 0.95; half greedy)   361.6 362.2 | 364.8 365.5
    T 0.7, top-k 40, top-p 0.95                676.1 679.2 | 542.4 542.5
    T 1.0, no truncation                       312.7 311.9 | 199.9 199.2
    T 0.7, top-p 0.95, repeat 1.1              718.7 721.4 | 585.2 585.6
  The service mix is 0.9 % slower, which is OUTSIDE the parent's own spread of 0.2 %: the second histogram pass now
  evaluates the bin expression for the logits inside a guard band and keeps a minimum per sub-bin. The other three
  sets are 19 - 36 % faster; the no-truncation set does not call hist_threshold at all, so that gain is the compiler's
  doing (presumably the register allocation of the whole kernel), not the algorithm's.

Mutated builds (never committed), the GPU tests run once against each (sample_decode_kernel then ran carriers at V =
65, 4097, 128256 and 262144 only; the other nine sizes were added to it afterwards):
  `v >= lo` -> `v > lo` in draw_index_order: 36 cases fail -- carriers variant 3 at V = 2 and every V >= 1000,
    cuts 5 / 6 / 11 - 14 / 18, ties 2 / 5 / 8 - 11, masked m = 1 .. 41 under top_k 300, offset N(50,1) / +1e4 / -1e4 at
    k 300, penalties 3, the mixed launch, sample_decode_kernel carriers-4097 / -128256 / -262144 and cuts
  per forced to 1: 18 cases fail -- carriers variants 0, 1, 3, 4 at V = 65537, 128256, 151936, 262144 (variant 2 is the
    fast path, which does not walk tiles), sample_decode_kernel carriers-128256 / -262144

Fault models (test_fault_models_are_rejected; applied to the reference, each changes the token of at least one
designed variate; in brackets the designed variates it changes per family, the weakest family that sees it last):
  F1  k-th dropped, (k+1)-th kept [offset 304, cuts 160, masked 109, penalties 38, carriers 13; ties 0]
  F2  ties at a cut dropped [ties 1213, cuts 642, offset 304, masked 109, penalties 49, carriers 13]
  F3  lowest finite dropped when top_k >= finite count [masked 546; no other family has such a row]
  F4  top-p over the untruncated mass [cuts 312, ties 50]       F5  min-p bound without the temperature [cuts 34]
  F6  draw in value order [cuts 2747, ties 645, masked 488, carriers 320, offset 303, penalties 275]
  F7  tiles past 1024 ignored [carriers V = 128256: 50 of 54]   F8  last partial tile reads past V [mixed launch 380]
  F9  neighbouring token returned [every family; penalties 554 the fewest]
  F10 penalties per occurrence [penalties 125]                  F11 repeat_penalty divides negative logits [penalties 42]
  F12 window one short [decode penalties 4] / append at pos % S [31]      F13 row stride V for ld [mixed launch 376]
test_old_inputs_cannot_see: with the inputs and the acceptance of the older tests F3 and F7 change nothing; F1 on
EVERY row changes no token of the twin test's sets that have top-p behind top-k, and 72 of 256 at top_k 5; applied
to one row in 300, the rate of finding 2, on a row whose token it changes, it passes the twin test's acceptance.
"""
import functools
import math

import numpy as np
import pytest
import torch

import sampler_ref as S

EMU = 2.0e-7
G = 4 * EMU
SENT = -7
HIST = 64


# ------------------------------------------------------------------------------------------------ judging

def _refs(case):
    """Reference of every row of a case; rows that share logits, params and history share the reference."""
    out, memo = [], {}
    shared = case.logits.strides[0] == 0
    for r in range(len(case.us)):
        k = (0 if shared else r, id(case.params[r]), tuple(case.hists[r]))
        if k not in memo:
            memo[k] = S.ref_row(case.logits[r], case.params[r], case.hists[r])
        out.append(memo[k])
    return out


def _judge(refs, us, toks, where, stats=None):
    """Token == reference token wherever u is >= 3.9 g from every step; the widened interval otherwise."""
    bad = []
    for r, (ref, u, t) in enumerate(zip(refs, us, toks)):
        t = int(t)
        want = S.draw(ref, u)
        d = S.step_distance(ref, u)
        ok = S.accepted(ref, u, t, G) if (want is None or d < 3.9 * G) else t == want
        if ok and stats is not None and t != want and want is not None:
            stats["near"] = max(stats.get("near", 0.0), d / G)
        if not ok:
            bad.append((where, r, u, t, want, d / G))
    return bad


def all_cases():
    """Every case of the families that run through sample_kernel (name, builder)."""
    out = []
    for V in S.CARRIER_VS:
        for v in range(len(S.CARRIER_PARAMS)):
            out.append((f"carriers-{V}-{v}", functools.partial(S.carriers, V, G, v)))
    for i in range(len(S.cut_params())):
        out.append((f"cuts-{i}", functools.partial(S.cuts, G, i)))
    for i in range(len(S.tie_cases(G))):
        out.append((f"ties-{i}", lambda i=i: S.tie_cases(G)[i]))
    for m in S.MASK_M:
        out.append((f"masked-{m}", functools.partial(S.masked_case, m, G)))
        out.append((f"masked-{m}-k300", functools.partial(S.masked_case, m, G, 300)))
    out.append(("masked-10-nan", functools.partial(S.masked_case, 10, G, 40, True)))
    out.append(("masked-41-nan", functools.partial(S.masked_case, 41, G, 40, True)))
    for name, _, _ in S.OFFSETS:
        for k in (40, 300):
            if (name, k) != ("N(-1000,.01)", 300):       # no row of it passes the margin rule at the 300-th place
                out.append((f"offset-{name}-{k}", functools.partial(S.offset_case, name, G, k)))
    for i in range(len(S.penalty_cases(G))):
        out.append((f"penalties-{i}", lambda i=i: S.penalty_cases(G)[i]))
    return out


CASES = all_cases()


# ------------------------------------------------------------------------------------------------ CPU tests

def test_emulated_noise_bounds_g():
    """EMU is the largest emulated |cdf32 - cdf64| over this module's inputs (two rows of every carriers case, one
    of every other case), and every designed row is fair: margins from the reference alone."""
    worst = 0.0
    for name, build in CASES:
        c = build()
        if not len(c.us):
            continue
        for r in ((0, len(c.us) - 1) if name.startswith("carriers") else (0,)):
            worst = max(worst, S.emu_noise(c.logits[r], c.params[r], c.hists[r]))
    assert EMU / 2 <= worst <= EMU, worst


def test_designed_rows_are_fair():
    for name, build in CASES:
        c = build()
        refs = _refs(c)
        for ref, u in zip(refs, c.us):
            if ref.greedy or not ref.kept.size:
                continue
            m = ref.margins
            assert m["negl"] < G and m["mass"] >= 8 * G, (name, m)
            assert m["logit"] > 1.0, (name, m)
            j = min(int(np.searchsorted(ref.edges[1:], u, side="right")), ref.kept.size - 1)
            if 0.0 < u < 1.0 - 2.0 ** -23:
                assert ref.edges[j + 1] - ref.edges[j] >= 8 * G and S.step_distance(ref, u) >= 3.9 * G, (name, u)


def test_random_rows_skip_cap():
    """On the random rows of the older twin test at most 1 % of the variates lie within g of a step; and the
    reference judged by itself passes."""
    L, us, hist = S.random_rows()
    near = n = 0
    for p in (S.P(temperature=0.7, top_p=0.95, top_k=40), S.P(top_k=5), S.P(temperature=0.8, top_k=300, top_p=0.9)):
        for r in range(0, 256, 4):
            ref = S.ref_row(L[r], p, hist[r])
            near += S.step_distance(ref, us[r]) < G
            n += 1
            assert not _judge([ref], [us[r]], [S.draw(ref, us[r])], "self")
    assert near <= 0.01 * n, (near, n)


def _kept32(x, t):
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((x >= np.float32(t)) & (x > np.float32(S.NEG)))


def test_threshold_emulation():
    """CPU witness of findings 1 and 2: hist_threshold's count mode in float32, before the fix (the numbers of the
    module docstring) and after it (the reference's kept set on every row of masked and offset; for k <= 256 the
    fast path sorts the compacted set, so there the threshold has to keep a superset no larger than CCAP)."""
    old, new = {}, {}
    for m in S.MASK_M:
        L = S.masked_rows(m)
        p = S.P(top_k=40)
        bo = bn = 0
        for r in range(L.shape[0]):
            ref = S.ref_row(L[r], p)
            bo += not np.array_equal(_kept32(L[r], S.emu_threshold_old(L[r], 40)), ref.kept)
            bn += not np.array_equal(_kept32(L[r], S.emu_threshold_new(L[r], 40)), ref.kept)
        old["masked", m], new["masked", m] = bo, bn
    for name, _, sd in S.OFFSETS:
        L = S.offset_rows(name)
        for k in (40, 300):
            bo = bn = 0
            for r in range(L.shape[0]):
                ref = S.ref_row(L[r], S.P(top_k=k, temperature=3 * sd))
                if not ref.margins["logit"] > 1.0:
                    continue
                for which, f in (("o", S.emu_threshold_old), ("n", S.emu_threshold_new)):
                    kept = _kept32(L[r], f(L[r], k))
                    good = (set(ref.kept) <= set(kept) and len(kept) <= S.CCAP) if k <= S.KFAST else \
                        np.array_equal(kept, ref.kept)
                    bo += which == "o" and not good
                    bn += which == "n" and not good
            old[name, k], new[name, k] = bo, bn
    assert not any(new.values()), new
    assert [old["masked", m] for m in S.MASK_M] == [0, 11, 12, 18, 0], old
    assert [old[n, 40] for n, _, _ in S.OFFSETS] == [0, 3, 5, 5] and [old[n, 300] for n, _, _ in S.OFFSETS] == \
        [0, 0, 6, 6], old


def _twin_rows(case, step=1):
    from nats_llm_studio_amd.engine.sampling import SamplingParams, sample_rows
    rows = list(range(0, len(case.us), step))
    ps = [SamplingParams(**case.params[r]) for r in rows]
    lg = torch.from_numpy(np.ascontiguousarray(case.logits[rows]))
    return rows, sample_rows(lg, ps, [list(case.hists[r]) for r in rows], [float(case.us[r]) for r in rows])


def test_cpu_twin_matches_reference():
    """engine.sampling.sample_rows and the CPU branch of ops.sample_decode_cand against the same reference, families
    and metric (every 8th row of the cases with V > 65536: the twin sorts the whole vocabulary per row)."""
    bad = []
    for name, build in CASES:
        c = build()
        if not len(c.us):
            continue
        refs = _refs(c)
        rows, toks = _twin_rows(c, 8 if c.logits.shape[1] > 65536 else 2 if c.logits.shape[1] > 4097 else 1)
        bad += _judge([refs[r] for r in rows], [c.us[r] for r in rows], toks, name)
    lg = np.full((2, 3000), np.nan, np.float32)
    lg[1] = S.NEG
    from nats_llm_studio_amd.engine.sampling import SamplingParams, sample_rows
    toks = sample_rows(torch.from_numpy(lg), [SamplingParams(temperature=0.7, top_k=40, top_p=0.9)] * 2, [[], []],
                       [0.3, 0.3])
    assert all(0 <= t < 3000 for t in toks), toks
    bad += _cand_check(None)
    assert not bad, (len(bad), bad[:6])


# ---- fault models

def _tok_changes(case, fault, shift=0, rows=None):
    """Number of designed variates of a case whose token the fault changes."""
    n = 0
    memo = {}
    shared = case.logits.strides[0] == 0
    for r in (rows if rows is not None else range(len(case.us))):
        k = (0 if shared else r)
        if k not in memo:
            memo[k] = (S.ref_row(case.logits[r], case.params[r], case.hists[r]),
                       S.ref_row(case.logits[r], case.params[r], case.hists[r], fault=fault))
        good, bad = memo[k]
        n += S.draw(good, case.us[r]) != S.draw(bad, case.us[r], shift)
    return n


def _f7(ref):
    """Tiles past 1024 ignored: tokens from id 65536 on carry no weight."""
    k = ref.kept < 65536
    w = ref.w[k]
    return ref._replace(kept=ref.kept[k], w=w, edges=np.concatenate([[0.0], np.cumsum(w)]) / w.sum())


def _family(prefix):
    return [b() for n, b in CASES if n.startswith(prefix)]


def test_fault_models_are_rejected():
    seen = {}
    fams = {f: _family(f) for f in ("cuts", "ties", "masked", "offset", "penalties")}
    fams["carriers"] = [S.carriers(V, G, v) for V in (65, 4097, 128256) for v in (0, 2)]
    for f in ("F1", "F2", "F3", "F4", "F5", "F6", "F10", "F11"):
        seen[f] = {name: sum(_tok_changes(c, f) for c in cs) for name, cs in fams.items()}
    seen["F9"] = {name: sum(_tok_changes(c, None, s) for c in cs for s in (-1, 1)) for name, cs in fams.items()}
    c = S.carriers(128256, G, 0)
    refs = _refs(c)
    seen["F7"] = {"carriers": sum(S.draw(r, u) != S.draw(_f7(r), u) for r, u in zip(refs, c.us))}
    # F8 / F13 on the mixed launch's buffer: the row as a faulty kernel would read it
    buf, ld, off, mc = _mixed_buffer()
    V = mc.logits.shape[1]
    n8 = n13 = 0
    for r in range(len(mc.us)):
        good = S.draw(S.ref_row(mc.logits[r], mc.params[r], mc.hists[r]), mc.us[r])
        past = buf[off + r * ld: off + r * ld + (V + 63) // 64 * 64]
        n8 += S.draw(S.ref_row(past, mc.params[r], mc.hists[r]), mc.us[r]) != good
        n13 += S.draw(S.ref_row(buf[off + r * V: off + r * V + V], mc.params[r], mc.hists[r]), mc.us[r]) != good
    seen["F8"], seen["F13"] = {"mixed": n8}, {"mixed": n13}
    # F12 on the decode rows
    n12 = {"F12a": 0, "F12b": 0}
    for row in _decode_rows("penalties"):
        good = S.decode_ref(row["l"], row["p"], row["ring"], row["pos"], row["seed"], row["ctx"])
        for f in n12:
            bad = S.decode_ref(row["l"], row["p"], row["ring"], row["pos"], row["seed"], row["ctx"], fault=f)
            n12[f] += (good[0], good[3]) != (bad[0], bad[3])
    seen["F12"] = n12
    for f, d in seen.items():
        assert max(d.values()) > 0, (f, d)
    assert all(v > 0 for v in n12.values()), n12
    # the families each fault was designed for
    assert seen["F1"]["offset"] and seen["F1"]["cuts"] and seen["F2"]["ties"] and seen["F3"]["masked"]
    assert seen["F4"]["cuts"] and seen["F5"]["cuts"] and seen["F6"]["cuts"] and seen["F9"]["carriers"]
    assert seen["F10"]["penalties"] and seen["F11"]["penalties"]


def test_old_inputs_cannot_see():
    """The older tests' inputs and acceptance: V = 5000 / 6000 / 32000 gives per == 1 (F7 changes nothing), the masked
    test has 3000 finite logits under top_k 3 (F3 never applies), and the twin test forgives 2 rows of 256 -- F1 on
    one row in 300, the rate of finding 2 on N(50, 1) rows, is applied and passes that acceptance."""
    for V in (5000, 6000, 32000):
        assert ((V + 63) // 64 + S.NT - 1) // S.NT == 1
    rng = np.random.default_rng(1)
    base = rng.standard_normal(6000).astype(np.float32)
    base[::2] = S.NEG
    base[[101, 303, 505]] = (7.0, 6.8, 6.6)
    p = S.P(top_k=3)
    assert np.array_equal(S.ref_row(base, p).kept, S.ref_row(base, p, fault="F3").kept)
    L, us, hist = S.random_rows()
    def f1_rows(p, rows):
        return sum(S.draw(S.ref_row(L[r], p, hist[r]), us[r]) != S.draw(S.ref_row(L[r], p, hist[r], fault="F1"), us[r])
                   for r in rows)
    # with top-p behind top-k the k-th token is cut anyway: F1 on EVERY row changes no token of these sets
    assert f1_rows(S.P(temperature=0.7, top_p=0.95, top_k=40), range(0, 256, 2)) == 0
    assert f1_rows(S.P(temperature=0.8, top_k=300, top_p=0.9), range(0, 256, 2)) == 0
    # top_k 5 alone: F1 on every row would be seen (72 rows of 256). As finding 2 produces it -- one faulty row in 300,
    # here the first row whose token F1 does change -- the twin test's own acceptance (same >= n - 2) passes
    p5, n = S.P(top_k=5), 256
    want = [S.draw(S.ref_row(L[r], p5, hist[r]), us[r]) for r in range(n)]
    f1 = [S.draw(S.ref_row(L[r], p5, hist[r], fault="F1"), us[r]) for r in range(n)]
    changed = [r for r in range(n) if f1[r] != want[r]]
    assert len(changed) > 2, len(changed)
    got = [f1[r] if r == changed[0] else want[r] for r in range(n)]
    same = sum(a == b for a, b in zip(want, got))
    assert same == n - 1 and same >= n - 2
    # the frequency check of test_sample_kernel forgives 0.05: F1 on one row in 300 moves a frequency by <= 1 / 300
    assert 1.0 / 300 < 0.05


# ------------------------------------------------------------------------------------------------ GPU helpers

def _L():
    from nats_llm_studio_amd.ops import _lib
    return _lib.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _params_dev(case, dev, nh=None):
    raw = b"".join(S.pbytes(case.params[r], case.us[r], len(case.hists[r]) if nh is None else nh[r])
                   for r in range(len(case.us)))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)


def _hist_dev(case, dev, stride=HIST):
    h = np.full((len(case.us), stride), -1, np.int32)
    for r, hh in enumerate(case.hists):
        h[r, :len(hh)] = hh
    return torch.from_numpy(h).to(dev)


def _run_sample(case, dev):
    n, V = len(case.us), case.logits.shape[1]
    assert n <= (64 if V > 65536 else 600)
    lg = torch.from_numpy(np.ascontiguousarray(case.logits)).to(dev)
    pb, hd = _params_dev(case, dev), _hist_dev(case, dev)
    out = torch.full((n,), SENT, dtype=torch.int32, device=dev)
    rc = _L().nls_sample(lg.data_ptr(), V, n, V, pb.data_ptr(), hd.data_ptr(), HIST, out.data_ptr(), _stream(dev))
    assert rc == 0
    return out.cpu().numpy(), lg.cpu().numpy()


def _check_logits(case, refs, after, where):
    """A sampled row's logits change only at the distinct in-range history ids, by the penalty formula (within 2 ulp
    of |v'| + |presence| + |frequency count|: the product / quotient, the penalty sum and the difference round)."""
    bad = []
    for r, ref in enumerate(refs):
        before = np.asarray(case.logits[r], np.float32)
        diff = np.flatnonzero(before.view(np.int32) != after[r].view(np.int32))
        if not set(diff) <= set(ref.pen):
            bad.append((where, r, "stray", sorted(set(diff) - set(ref.pen))[:4]))
        p = case.params[r]
        cnt = {i: list(case.hists[r]).count(i) for i in ref.pen}
        for i, v in ref.pen.items():
            scale = abs(v) + 2 * (abs(p["presence_penalty"]) + abs(p["frequency_penalty"]) * cnt[i])
            if not abs(float(after[r, i]) - v) <= 2 * 2.0 ** -23 * scale:
                bad.append((where, r, i, float(after[r, i]), v))
    return bad


# ------------------------------------------------------------------------------------------------ sample_kernel

STATS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_sample_kernel_families(gpu, name):
    c = dict(CASES)[name]()
    if not len(c.us):
        pytest.fail("empty case")
    refs = _refs(c)
    toks, after = _run_sample(c, gpu)
    bad = _judge(refs, c.us, toks, name, STATS.setdefault("sample", {})) + _check_logits(c, refs, after, name)
    print(name, "rows", len(c.us), "bad", len(bad), "near", STATS["sample"].get("near", 0.0))
    assert not bad, (len(bad), len(c.us), bad[:6])


@pytest.mark.gpu
def test_sample_kernel_nonfinite_rows(gpu):
    """All-NaN and all -inf rows return an id inside the vocabulary on every path."""
    V = 3000
    L = np.full((6, V), np.nan, np.float32)
    L[3:] = S.NEG
    ps = [S.P(top_k=40, top_p=0.9), S.P(top_k=300), S.P(top_p=0.9)] * 2
    toks, _ = _run_sample(S.Case("nonfinite", L, ps, [()] * 6, [0.3] * 6), gpu)
    assert all(0 <= t < V for t in toks), toks


@functools.lru_cache(maxsize=None)
def _mixed_case():
    """Rows of every family at V = 1000 with their own params and history."""
    rows, ps, hs, us = [], [], [], []
    V = 1000
    for v in range(len(S.CARRIER_PARAMS)):
        c = S.carriers(V, G, v)
        for r in (0, 17, 47, 48, 53):
            rows.append(c.logits[r]); ps.append(c.params[r]); hs.append(c.hists[r]); us.append(c.us[r])
    for c in S.penalty_cases(G):
        for r in range(0, len(c.us), 5):
            rows.append(c.logits[r]); ps.append(c.params[r]); hs.append(c.hists[r]); us.append(c.us[r])
    base = S.cut_row(V, 1.0)
    for i, p in enumerate(S.cut_params(V)):
        c = S._sweep(base, p, (), G, "mixed cut")
        for r in range(0, len(c.us), 9):
            rows.append(c.logits[r]); ps.append(p); hs.append(()); us.append(c.us[r])
    return S.Case("mixed", np.stack(rows), ps, hs, us)


def _mixed_buffer():
    """The mixed launch's memory: ld = V + 24, 1e30 in the padding columns, the first row 3 floats into the buffer."""
    c = _mixed_case()
    n, V = c.logits.shape
    ld, off = V + 24, 3
    buf = np.full(off + n * ld + 64, 1e30, np.float32)
    for r in range(n):
        buf[off + r * ld: off + r * ld + V] = c.logits[r]
    return buf, ld, off, c


@pytest.mark.gpu
def test_sample_kernel_mixed_launch(gpu):
    """One launch, every row its own params and n_hist, ld > V with 1e30 in the padding, unaligned rows: each row
    equals its reference (which the single-row launches of test_sample_kernel_families are held to as well); the
    padding stays untouched."""
    buf, ld, off, c = _mixed_buffer()
    n, V = c.logits.shape
    dbuf = torch.from_numpy(buf).to(gpu)
    pb, hd = _params_dev(c, gpu), _hist_dev(c, gpu)
    out = torch.full((n,), SENT, dtype=torch.int32, device=gpu)
    rc = _L().nls_sample(dbuf.data_ptr() + 4 * off, ld, n, V, pb.data_ptr(), hd.data_ptr(), HIST, out.data_ptr(),
                         _stream(gpu))
    assert rc == 0
    after = dbuf.cpu().numpy()
    refs = _refs(c)
    rows_after = np.stack([after[off + r * ld: off + r * ld + V] for r in range(n)])
    bad = _judge(refs, c.us, out.cpu().numpy(), "mixed") + _check_logits(c, refs, rows_after, "mixed")
    mask = np.ones(len(buf), bool)
    for r in range(n):
        mask[off + r * ld: off + r * ld + V] = False
    assert np.array_equal(after[mask], buf[mask])
    assert not bad, (len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------ decode kernels

SEEDS = (0, (1 << 64) - 1, 1, 0x9E3779B97F4A7C15, 12345678901234567)
POSS = (0, 5, HIST - 1, HIST, 3 * HIST + 7)


def _ring_for(l, V, rng, S_=HIST):
    hot = np.argsort(-np.where(np.isfinite(l), l, -np.inf))[:12]
    ring = rng.choice(hot, S_).astype(np.int32)            # repeats: counts
    ring[rng.integers(0, S_, 5)] = -1
    ring[rng.integers(0, S_, 3)] = V + 3
    return ring


@functools.lru_cache(maxsize=None)
def _decode_rows(fam):
    """Rows for the decode kernels: (logits row, params, ring, pos, seed, ctx_len). Every (pos, seed) pair occurs;
    every 7th row is padding (ctx_len 0 or -3, in turn) and greedy unpenalised rows are mixed in: both must be skipped."""
    rows = []
    if fam.startswith("carriers"):
        V = int(fam.split("-")[1])
        nc = min(V, S.NCAR)                                # rows 0, 11, 30, 47 of the case, clamped below 48 tokens
        src = [(S.carriers(V, G, v).logits[r], S.CARRIER_PARAMS[v]) for v in (0, 2, 3)
               for r in sorted({min(r, nc - 1) for r in (0, 11, 30, 47)})]
    elif fam == "cuts":
        src = [(S.cut_row(), p) for p in S.cut_params()]
    else:
        src = [(c.logits[0], c.params[0]) for c in S.penalty_cases(G)]
        src += [(c.logits[0], dict(c.params[0], top_k=20, top_p=0.9)) for c in S.penalty_cases(G)[:4]]
    rng = S._rng("decode", fam)
    i = 0
    for l, p in src:
        for _ in range(-(-24 // len(src)) if fam.startswith("carriers") else 3):     # carriers: 24 rows at every V
            pos, seed = POSS[i % 5], SEEDS[(i // 5 + i) % 5]
            pp = p
            if fam != "penalties" and i % 3 == 1:
                pp = dict(p, repeat_penalty=float(np.float32(1.2)), frequency_penalty=float(np.float32(0.1)))
            if i % 11 == 10:
                pp = S.P(temperature=0.0)                   # greedy, unpenalised: skipped
            rows.append(dict(l=np.asarray(l, np.float32), p=pp, ring=_ring_for(l, len(l), rng), pos=pos, seed=seed,
                             ctx=(0, -3)[i // 7 % 2] if i % 7 == 6 else pos + 1))
            i += 1
    return rows


def _u64(seeds, dev):
    return torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).to(dev)


DECODE_FAMS = tuple(f"carriers-{V}" for V in S.CARRIER_VS) + ("cuts", "penalties")


@pytest.mark.gpu
@pytest.mark.parametrize("fam", DECODE_FAMS)
def test_sample_decode_kernel(gpu, fam):
    rows = _decode_rows(fam)
    n, V = len(rows), len(rows[0]["l"])
    assert n <= (64 if V > 65536 else 600)
    L = np.stack([r["l"] for r in rows])
    ring = np.stack([r["ring"] for r in rows])
    lg = torch.from_numpy(L).to(gpu)
    rg = torch.from_numpy(ring).to(gpu)
    pb = torch.frombuffer(bytearray(b"".join(S.pbytes(r["p"]) for r in rows)), dtype=torch.uint8).to(gpu)
    pos = torch.tensor([r["pos"] for r in rows], dtype=torch.int32, device=gpu)
    ctx = torch.tensor([r["ctx"] for r in rows], dtype=torch.int32, device=gpu)
    nxt = torch.full((n,), SENT, dtype=torch.int32, device=gpu)
    rc = _L().nls_sample_decode(lg.data_ptr(), V, n, V, pb.data_ptr(), _u64([r["seed"] for r in rows], gpu).data_ptr(),
                                pos.data_ptr(), ctx.data_ptr(), rg.data_ptr(), HIST, nxt.data_ptr(), _stream(gpu))
    assert rc == 0
    toks, la, ra = nxt.cpu().numpy(), lg.cpu().numpy(), rg.cpu().numpy()
    bad, skipped = [], 0
    st = STATS.setdefault("decode", {})
    for i, r in enumerate(rows):
        want, u, window, slot, ref = S.decode_ref(r["l"], r["p"], r["ring"], r["pos"], r["seed"], r["ctx"])
        if ref is None:                                    # skipped: sentinel, ring and logits bit-equal
            skipped += 1
            if toks[i] != SENT or not np.array_equal(ra[i], ring[i]) or \
                    not np.array_equal(la[i].view(np.int32), L[i].view(np.int32)):
                bad.append((fam, i, "skipped row touched"))
            continue
        bad += _judge([ref], [u], [toks[i]], (fam, i), st)
        exp = ring[i].copy()
        exp[slot] = toks[i]
        if slot != (r["pos"] + 1) % HIST or not np.array_equal(ra[i], exp):
            bad.append((fam, i, "ring", np.flatnonzero(ra[i] != exp)[:4].tolist()))
        c1 = S.Case("", L[i:i + 1], [r["p"]], [tuple(window)], [u])
        bad += _check_logits(c1, [ref], la[i:i + 1], (fam, i))
    print(fam, "rows", n, "skipped", skipped, "bad", len(bad), "near", st.get("near", 0.0))
    assert skipped >= 2 and not bad, (len(bad), bad[:6])


def _cand_rows(M):
    """Candidate rows of width M from full-vocabulary rows (V = 8192): the M - pad largest logits in vocabulary order,
    (-inf, -1) padding inside the row, history with ids that are no candidates. top_k <= M - pad - HIST, penalties
    that only lower logits: Engine._cand_ok."""
    V, pad = 8192, 9
    rng = S._rng("cand", M)
    ps = [S.P(temperature=0.8, top_k=40, top_p=0.95, repeat_penalty=1.2), S.P(temperature=1.3, top_k=min(64, M - pad - HIST),
                                                                            min_p=0.02, presence_penalty=0.5),
          S.P(temperature=0.5, top_k=5), S.P(top_k=1), S.P(temperature=0.0, repeat_penalty=1.5),
          S.P(temperature=0.9, top_k=min(55, M - pad - HIST), top_p=0.5, frequency_penalty=0.3), S.P(temperature=0.0)]
    rows = []
    for i in range(20):
        l = (rng.standard_normal(V) * 3.0).astype(np.float32)
        top = np.sort(np.argsort(-l)[:M - pad])
        at = np.sort(rng.permutation(M)[:M - pad])
        vals, ids = np.full(M, S.NEG, np.float32), np.full(M, -1, np.int32)
        vals[at], ids[at] = l[top], top
        ring = rng.choice(np.argsort(-l)[:30], HIST).astype(np.int32)
        ring[rng.integers(0, HIST, 6)] = rng.integers(0, V, 6)          # mostly absent from the candidates
        ring[rng.integers(0, HIST, 3)] = -1
        rows.append(dict(l=l, vals=vals, ids=ids, p=ps[i % len(ps)], ring=ring, pos=POSS[i % 5], seed=SEEDS[i % 5],
                         ctx=0 if i == 13 else -1 if i == 6 else 1))
    return rows


def _cand_check(dev):
    """sample_decode_cand (dev None: the CPU branch of ops) against the full-vocabulary reference."""
    from nats_llm_studio_amd import ops
    bad = []
    for M in (128, 1000, 1024):
        rows = _cand_rows(M)
        n = len(rows)
        to = (lambda a: torch.from_numpy(a).to(dev)) if dev is not None else torch.from_numpy
        vals, ids = to(np.stack([r["vals"] for r in rows])), to(np.stack([r["ids"] for r in rows]))
        ring0 = np.stack([r["ring"] for r in rows])
        rg = to(ring0.copy())
        pb = torch.frombuffer(bytearray(b"".join(S.pbytes(r["p"]) for r in rows)), dtype=torch.uint8).view(n, -1)
        pb = pb.to(dev) if dev is not None else pb
        seeds = torch.from_numpy(np.array([r["seed"] for r in rows], dtype=np.uint64).view(np.int64))
        pos = torch.tensor([r["pos"] for r in rows], dtype=torch.int32)
        ctx = torch.tensor([r["ctx"] for r in rows], dtype=torch.int32)
        nxt = torch.full((n,), SENT, dtype=torch.int32)
        if dev is not None:
            seeds, pos, ctx, nxt = seeds.to(dev), pos.to(dev), ctx.to(dev), nxt.to(dev)
        ops.sample_decode_cand(vals, ids, n, pb, seeds, pos, ctx, rg, nxt)
        toks, ra = nxt.cpu().numpy(), rg.cpu().numpy()
        for i, r in enumerate(rows):
            want, u, window, slot, ref = S.decode_ref(r["l"], r["p"], r["ring"], r["pos"], r["seed"], r["ctx"])
            if ref is None:
                if toks[i] != SENT or not np.array_equal(ra[i], ring0[i]):
                    bad.append(("cand", M, i, "skipped row touched"))
                continue
            bad += _judge([ref], [u], [toks[i]], ("cand", M, i), STATS.setdefault("cand", {}))
            exp = ring0[i].copy()
            exp[slot] = toks[i]
            if not np.array_equal(ra[i], exp):
                bad.append(("cand", M, i, "ring"))
    return bad


@pytest.mark.gpu
def test_sample_decode_cand_kernel(gpu):
    bad = _cand_check(gpu)
    print("cand near", STATS.get("cand", {}).get("near", 0.0))
    assert not bad, (len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------ topc_kernel

def _topc_ref(x, valid, C, lo):
    """The C largest of x[:valid] (ties at the cut: lowest indices; -0.0 == +0.0) in vocabulary order, padded."""
    k = min(C, max(valid, 0))
    v, i = np.full(C, S.NEG, np.float32), np.full(C, -1, np.int32)
    if k:
        xs = x[:valid].astype(np.float64) + 0.0
        order = np.lexsort((np.arange(valid), -xs))[:k]
        order.sort()
        v[:k], i[:k] = x[order], order + lo
    return v, i


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 128, 1024])
def test_topc_kernel_reference(gpu, C):
    from nats_llm_studio_amd import ops
    rng = S._rng("topc", C)
    for valid in (0, 1, C - 1, C, C + 1, 64128):
        width = max(valid, 1) + 24
        x = (rng.standard_normal((6, width)) * 2).astype(np.float32)
        x[:, max(valid, 0):] = 1e30                                   # ld > valid: never read
        if valid > 1:
            k = min(C, valid)
            for r in (1, 2, 3):                                       # ties straddling the cut
                srt = np.argsort(-x[r, :valid])
                tied = srt[max(0, k - 3):min(valid, k + 4)]
                x[r, tied] = x[r, srt[k - 1]]
            o2 = np.argsort(-x[2, :valid])
            x[2, o2[0]], x[2, o2[-1]] = np.inf, -np.inf
            o3, a, b = np.argsort(-x[3, :valid]), max(0, k - 3), min(valid, k + 4)   # -0.0 / +0.0 across the cut
            x[3, o3[:a]] = 1.0 + np.abs(x[3, o3[:a]])
            x[3, o3[b:]] = -1.0 - np.abs(x[3, o3[b:]])
            x[3, o3[a:b]] = np.where(np.arange(b - a) % 2 == 0, -0.0, 0.0)
            x[4, :valid] = 0.5                                        # all equal
        v, i = ops.topc_candidates(torch.from_numpy(x).to(gpu), 6, C, 1000, valid)
        v, i = v.cpu().numpy(), i.cpu().numpy()
        for r in range(6):
            rv, ri = _topc_ref(x[r], valid, C, 1000)
            assert np.array_equal(i[r], ri), (C, valid, r, np.flatnonzero(i[r] != ri)[:5])
            assert np.array_equal(v[r].view(np.int32), rv.view(np.int32)), (C, valid, r)


# ------------------------------------------------------------------------------------------------ refusals

@pytest.mark.gpu
def test_entry_points_refuse(gpu):
    """V = 262145, M = 1025 and hist_stride 0 / 1025 return an error and launch nothing (outputs keep the sentinel)."""
    L = _L()
    V = 262145
    lg = torch.zeros(1, V, device=gpu)
    c = S.Case("", None, [S.P(top_k=40)], [()], [0.5])
    pb = _params_dev(c, gpu)
    hd = torch.full((1, 1025), -1, dtype=torch.int32, device=gpu)
    out = torch.full((1,), SENT, dtype=torch.int32, device=gpu)
    seeds, pos, ctx = _u64([1], gpu), torch.zeros(1, dtype=torch.int32, device=gpu), torch.ones(1, dtype=torch.int32,
                                                                                                  device=gpu)
    st = _stream(gpu)
    assert L.nls_sample(lg.data_ptr(), V, 1, V, pb.data_ptr(), hd.data_ptr(), HIST, out.data_ptr(), st) != 0
    assert L.nls_sample_decode(lg.data_ptr(), V, 1, V, pb.data_ptr(), seeds.data_ptr(), pos.data_ptr(), ctx.data_ptr(),
                               hd.data_ptr(), HIST, out.data_ptr(), st) != 0
    rec = torch.full((1, 44), SENT, dtype=torch.int32, device=gpu)
    ntop = torch.zeros(1, dtype=torch.int32, device=gpu)
    assert L.nls_logprobs(lg.data_ptr(), V, 1, V, ntop.data_ptr(), None, None, None, None, 0, rec.data_ptr(), None,
                          st) != 0
    for hs in (0, 1025):
        assert L.nls_sample_decode(lg.data_ptr(), V, 1, 1000, pb.data_ptr(), seeds.data_ptr(), pos.data_ptr(),
                                   ctx.data_ptr(), hd.data_ptr(), hs, out.data_ptr(), st) != 0
        ids = torch.zeros(1, 1025, dtype=torch.int32, device=gpu)
        assert L.nls_sample_decode_cand(lg.data_ptr(), 1024, 1, 1024, ids.data_ptr(), 1025, pb.data_ptr(),
                                        seeds.data_ptr(), pos.data_ptr(), ctx.data_ptr(), hd.data_ptr(), hs,
                                        out.data_ptr(), st) != 0
    ids = torch.zeros(1, 1025, dtype=torch.int32, device=gpu)
    assert L.nls_sample_decode_cand(lg.data_ptr(), 1025, 1, 1025, ids.data_ptr(), 1025, pb.data_ptr(), seeds.data_ptr(),
                                    pos.data_ptr(), ctx.data_ptr(), hd.data_ptr(), HIST, out.data_ptr(), st) != 0
    torch.cuda.synchronize()
    assert int(out[0]) == SENT and bool((rec == SENT).all()) and bool((hd == -1).all()) and float(lg.abs().max()) == 0.0
