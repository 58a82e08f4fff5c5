"""Shared by the tensor-parallel logprob tests: the rows of a vocabulary cut into W consecutive shards, the cases of
the kernel test (tests/test_tp_logprobs_gpu.py), an fp64 reference of the shard-partial / merge pair whose faults can
be switched on one at a time (the self-test of tests/test_tp_logprobs.py), and the per-record structure checks."""
import math

import numpy as np
import torch

from test_logprobs_gpu import KINDS, N_TOPS, SENTINEL, _reference, _row

LP_TOP, LP_REC = 20, 44
PAD_VALUE = 1e30                       # the padding columns would win every comparison
SHARD_KINDS = ("dead_shard", "far_maxima", "top_in_one", "top_spread", "shard_ties")
ALL_KINDS = KINDS + SHARD_KINDS
VS, WS, NS = (19, 1000, 1025, 32000, 128256), (1, 2, 8), (1, 3, 17)
MUTANTS = ("z_owner", "no_rescale", "local_ids", "few_cands", "chosen_rank0", "empty_m0", "pad_read")


def shard_bounds(V: int, W: int):
    """(width, [(vocab_lo, valid)] per rank): consecutive column slices of width ceil(V / W); the tail ranks of a
    small vocabulary hold fewer columns, or none (V = 19 at 8 ranks: rank 6 holds one id, rank 7 none)."""
    per = -(-V // W)
    return per, [(p * per, max(0, min(V, (p + 1) * per) - p * per)) for p in range(W)]


def shard_row(kind: str, V: int, W: int, s: int, g: torch.Generator, cut: int = 5) -> torch.Tensor:
    """One row of logits; the kinds of tests/test_logprobs_gpu.py plus those that only a sharded vocabulary has
    (s: the shard the kind singles out; cut: the n_top whose cut a shard_ties row's tie straddles)."""
    if kind in KINDS:
        return _row(kind, V, g)
    per, bounds = shard_bounds(V, W)
    lo, valid = bounds[s]
    x = torch.randn(V, generator=g) * 4
    if kind == "dead_shard":
        # one shard entirely -inf, every other maximum far below 0: an empty partial must not enter the maximum
        x -= 1e4
        if W > 1:                                      # (one shard: the row keeps its finite entries)
            x[lo:lo + valid] = float("-inf")
    elif kind == "far_maxima":
        # shard maxima 1e4 apart: the rescale exp(m_r - M) underflows for every shard but one
        keep = x[lo:lo + valid].clone()
        x -= 1e4
        x[lo:lo + valid] = keep
    elif kind == "top_in_one":
        # the whole top 20 inside one shard: a shard must contribute n_top candidates, not its share of them
        k = min(LP_TOP + 1, valid)
        at = lo + torch.randperm(valid, generator=g)[:k]
        x[at] = 40 + torch.rand(k, generator=g) * 8
    elif kind == "top_spread":
        # the top 20 one per shard, round-robin: rank j lives in shard j % W
        for j in range(LP_TOP + 1):
            l2, v2 = bounds[j % W]
            if j // W < v2:
                x[l2 + v2 - 1 - j // W] = 60 - j * 0.5
    elif kind == "shard_ties":
        # an exact tie on the last id of a shard and the first id of the next, across the cut of n_top = `cut`: the
        # two are the row's entries number cut - 1 and cut (counted from 0), so the first is kept and the second
        # dropped by the id order alone -- and they come from different ranks
        nb = max(0, min(W - 1, (V - 1) // per))            # boundaries with an id on either side
        if nb and cut + 2 <= V:
            first = (s % nb + 1) * per
            last = first - 1
            rest = torch.cat([x[:last], x[first + 1:]]).sort(descending=True).values
            x[last] = x[first] = (rest[cut - 1] + 1 if cut == 1 else (rest[cut - 2] + rest[cut - 1]) / 2)
    return x


def tie_at_cut(row: torch.Tensor, W: int, cut: int) -> bool:
    """Whether the row's entries number cut - 1 and cut under (value descending, id ascending) are an exact tie on
    the last id of one shard and the first id of the next."""
    V = len(row)
    per, _ = shard_bounds(V, W)
    if cut + 1 > V:
        return False
    order = np.lexsort((np.arange(V), -row.numpy().astype(np.float64)))
    a, b = int(order[cut - 1]), int(order[cut])
    return b == a + 1 and b % per == 0 and float(row[a]) == float(row[b])


def make_case(V: int, W: int, n: int):
    """The inputs of one launch of the kernel test: (logits [n, V] without the padding, n_top, chosen ids, ctx_len,
    kinds). Chosen tokens come in turn from every shard (a random, mostly non-top id), the arg-max, the id range of
    the empty tail (>= V) and -1; row 1 of a launch of three or more has ctx_len = 0.

    Kinds go round over the rows that are computed (n_top >= 0 and ctx_len > 0; a skipped row uses up none), rotated
    by V and W: the 13 computed rows of a launch of 17 hold every kind once and shard_ties twice more. The k-th
    computed shard_ties row of a launch has n_top = (1, 5, 20)[k % 3] and its tie across that very cut, so every cut is
    tested where it decides an id. The chosen-token modes go round over the computed rows too, at their own pace (a
    far_maxima row takes no turn), so a launch of 17 rows at 8 ranks takes its chosen token from every rank.
    coverage() counts what the cases hold; the self-test of tests/test_tp_logprobs.py asserts it."""
    g = torch.Generator().manual_seed(100003 * V + 101 * W + n)
    per, bounds = shard_bounds(V, W)
    rot = VS.index(V) * 5 + WS.index(W) * 3 if V in VS and W in WS else 0
    n_top = [N_TOPS[(r + n) % len(N_TOPS)] for r in range(n)]
    if n == 1:
        n_top = [20]
    ctx = [0 if (r == 1 and n >= 3) else 5 + r for r in range(n)]
    single = [(r + rot) % W for r in range(n)]             # the shard a row's kind singles out
    kinds, k, ties = [], 0, 0
    for r in range(n):
        computed = n_top[r] >= 0 and ctx[r] > 0
        kinds.append(ALL_KINDS[(k + rot) % len(ALL_KINDS)] if k < len(ALL_KINDS) or not computed else "shard_ties")
        k += computed                                      # (a skipped row uses up no kind)
        if computed and kinds[r] == "shard_ties" and n > 1:
            n_top[r] = (1, 5, 20)[ties % 3]
            ties += 1
        up = bounds[single[r]][1]
        if kinds[r] == "far_maxima" and 0 < up < n_top[r]:
            # an entry of a shard 1e4 below the maximum has a logprob near -1e4, where neighbouring f32 values are
            # 9.8e-4 apart: the record cannot hold it to 1e-4. So the top list of such a row stays inside the shard
            # that stayed up -- the largest n_top of the set that the shard can fill (a small vocabulary only: 3
            # ids per shard at V = 19 and 8 ranks) -- as its chosen token does, below
            n_top[r] = max(t for t in N_TOPS if t <= up)
    host = torch.stack([shard_row(kinds[r], V, W, single[r], g, cut=n_top[r] if n_top[r] in (1, 5, 20) else 5)
                        for r in range(n)])
    modes = [("shard", p) for p in range(W)] + ["argmax", "tail", "none"]
    # (the modes start elsewhere than the kinds, and the distance between the two changes with V: at 8 ranks there
    # are as many modes as kinds, and the same start would give every kind the same mode in every launch)
    chosen, turn = [], 2 * VS.index(V) if V in VS else 0
    for r in range(n):
        if kinds[r] == "far_maxima":
            # a token of a shard 1e4 below the maximum has a logprob near -1e4, which the record's f32 holds to
            # 5e-4 only: the chosen token of such a row comes from the shard that stayed up (and takes no turn)
            mode = ("shard", single[r])
        elif kinds[r] == "dead_shard":
            # (no turn: the dead shard has no finite entry to choose, and whose turn it is must not depend on that)
            mode = ("shard", (single[r] + 1) % W)
        else:
            mode = modes[turn % len(modes)]
            turn += n_top[r] >= 0 and ctx[r] > 0           # (a skipped row takes no turn either)
        if mode == "argmax":
            chosen.append(int(host[r].argmax()))
        elif mode == "tail":
            chosen.append(min(V + 2, W * per - 1) if W * per > V else V)
        elif mode == "none":
            chosen.append(-1)
        else:
            lo, valid = bounds[mode[1]]
            fin = torch.nonzero(host[r, lo:lo + valid] > float("-inf")).flatten()
            chosen.append(lo + int(fin[int(torch.randint(len(fin), (1,), generator=g))]) if len(fin) else V)
    return host, n_top, chosen, ctx, kinds


def coverage(V: int, W: int):
    """What the computed rows (n_top >= 0, ctx_len > 0) of the launches of (V, W) hold: the kinds, the cuts that a
    shard_ties row with that very n_top straddles with a cross-shard tie, the ranks that own a chosen token, the
    ranks that own a chosen token outside the row's top 20, and the kinds of the rows whose chosen token is owned,
    unowned (-1 or >= V) and the row's arg-max."""
    per, bounds = shard_bounds(V, W)
    f32_err = 0.0                                          # the worst rounding of an expected logprob to the record's f32
    kinds_seen, cuts, owners, low_owners, chosen_kinds = set(), set(), set(), set(), {"own": set(), "none": set(),
                                                                                      "tail": set(), "argmax": set()}
    for n in NS:
        host, n_top, chosen, ctx, kinds = make_case(V, W, n)
        for r in range(n):
            if n_top[r] < 0 or ctx[r] <= 0:
                continue
            kinds_seen.add(kinds[r])
            lp, _, lps = reference(host[r].numpy(), V, n_top[r], chosen[r])
            f32_err = max([f32_err] + [abs(float(np.float32(v)) - v) for v in [lp] + list(lps) if math.isfinite(v)])
            if kinds[r] == "shard_ties" and n_top[r] > 0 and tie_at_cut(host[r], W, n_top[r]):
                cuts.add(n_top[r])
            c = chosen[r]
            if 0 <= c < V:
                owners.add(c // per)
                chosen_kinds["own"].add(kinds[r])
                if c == int(host[r].argmax()):
                    chosen_kinds["argmax"].add(kinds[r])
                if c not in torch.topk(host[r], min(LP_TOP, V)).indices.tolist():
                    low_owners.add(c // per)
            else:
                chosen_kinds["none" if c < 0 else "tail"].add(kinds[r])
    return dict(kinds=kinds_seen, cuts=cuts, owners=owners, low_owners=low_owners, chosen=chosen_kinds, f32_err=f32_err)


def padded(host: torch.Tensor, W: int) -> torch.Tensor:
    """[n, V + pad]: the padding (every shard slice of width ceil(V / W) lies inside the buffer, plus three columns
    that leave the row stride odd) holds PAD_VALUE."""
    n, V = host.shape
    per, _ = shard_bounds(V, W)
    out = torch.full((n, W * per + 3), PAD_VALUE)
    out[:, :V] = host
    return out


def reference(row: np.ndarray, V: int, n_top: int, chosen: int):
    """_reference of the whole row; a chosen id that no shard owns (-1, >= V) has logprob -inf."""
    own = 0 <= chosen < V
    lp, ids, lps = _reference(row[:V], n_top, chosen if own else 0)
    return (lp if own else -math.inf), ids, lps


# ---------------------------------------------------------------------------------------------------------------
# fp64 reference of the pair, faults switchable
def ref_partial(cols: np.ndarray, lo: int, valid: int, n_top: int, chosen: int, mutant: str = "", W: int = 1):
    """Shard partial of one row: cols = the shard's columns (padding included), of which [0, valid) are real."""
    if mutant == "pad_read":
        valid = len(cols)
    x32 = cols[:valid]
    idx = np.nonzero(x32 > -np.inf)[0]
    x = x32[idx].astype(np.float64)
    k = min(n_top // W if mutant == "few_cands" else n_top, len(idx))
    order = np.lexsort((idx, -x))[:k]
    own = lo <= chosen < lo + valid
    return dict(m=float(x.max()) if len(idx) else -math.inf, z=float(np.exp(x - x.max()).sum()) if len(idx) else 0.0,
                vals=[float(v) for v in x[order]],
                ids=[int(i) + (0 if mutant == "local_ids" else lo) for i in idx[order]],
                own=own, raw=float(x32[chosen - lo]) if own else 0.0)


def ref_merge(parts: list, n_top: int, chosen: int, mutant: str = ""):
    """The record (chosen logprob, top ids, top logprobs) from the W partials."""
    live = [p for p in parts if p["z"] > 0 or mutant == "empty_m0"]
    ms = [(0.0 if p["z"] <= 0 else p["m"]) for p in live]
    M = max(ms) if ms else 0.0
    if mutant == "z_owner":
        owner = next((p for p in parts if p["own"]), parts[0])
        Z = owner["z"] * math.exp(owner["m"] - M) if owner["z"] > 0 else 0.0
    elif mutant == "no_rescale":
        Z = sum(p["z"] for p in live)
    else:
        Z = sum(p["z"] * math.exp(m - M) for p, m in zip(live, ms) if p["z"] > 0)
    logz = math.log(Z) if Z > 0 else (-math.inf if live else 0.0)
    if not any(p["z"] > 0 for p in parts):
        M = logz = 0.0
    cand = sorted((-v, i) for p in parts for v, i in zip(p["vals"], p["ids"]))[:max(n_top, 0)]
    raw = -math.inf
    if mutant == "chosen_rank0":
        raw = parts[0]["raw"]
    else:
        for p in parts:
            if p["own"]:
                raw = p["raw"]
    return (raw - M) - logz, [i for _, i in cand], [(-v - M) - logz for v, _ in cand]


def ref_rows(buf: np.ndarray, V: int, W: int, n_top, chosen, ctx, mutant: str = ""):
    """ref_partial + ref_merge over the rows of a padded buffer; None for a row that is skipped."""
    per, bounds = shard_bounds(V, W)
    out = []
    for r in range(buf.shape[0]):
        if n_top[r] < 0 or ctx[r] <= 0:
            out.append(None)
            continue
        parts = [ref_partial(buf[r, lo:lo + per], lo, valid, n_top[r], chosen[r], mutant, W) for lo, valid in bounds]
        out.append(ref_merge(parts, n_top[r], chosen[r], mutant))
    return out


def _close(a: float, b: float, tol: float) -> bool:
    return a == b or abs(a - b) <= tol           # (-inf == -inf; nan is never close)


def mismatch(got, want, tol: float):
    """Why a record (lp, ids, lps) is not `want` within tol: a string, or None when it is."""
    if got[1] != want[1]:
        return f"ids {got[1]} != {want[1]}"
    if not _close(got[0], want[0], tol):
        return f"chosen logprob {got[0]} != {want[0]}"
    bad = [(a, b) for a, b in zip(got[2], want[2]) if not _close(a, b, tol)]
    return f"top logprobs {bad[:3]}" if bad else None


def check_structure(res_tokens, lps, n_top: int, greedy: bool):
    """Per-record structure of one request's logprobs: one record per token, the chosen ids are the tokens, top
    lists of n_top entries sorted by descending logprob with sum exp <= 1, and a greedy row's first entry is its
    token."""
    assert lps is not None and [e[0] for e in lps] == list(res_tokens), (lps, res_tokens)
    for tid, lp, top in lps:
        top = [tuple(e) for e in top]
        assert len(top) == n_top and lp <= 0, (tid, lp, top)
        vals = [v for _, v in top]
        assert vals == sorted(vals, reverse=True) and sum(math.exp(v) for v in vals) <= 1 + 1e-6, top
        if greedy and top:
            assert top[0] == (tid, lp), (tid, lp, top[0])
