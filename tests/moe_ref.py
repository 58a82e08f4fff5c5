"""fp64 references, input families, the metrics and the fault models of tests/test_moe_sensitivity.py: the top-k
route with its per-expert row lists, the router logits, the weighted combine and the expert launches over row lists.
Nothing here calls ops or torch.topk: the references are numpy, the ranking is a stable sort on (-value, index) with
NaNs last, and the float32 variants (route_emu, logit_emu) ARE the emulation of the kernels' arithmetic."""
import functools

import numpy as np

import qblocks as QB
import rowops as R
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType

SENT = -7                       # what every list entry, sel entry and output row holds before the launch
GUARD = 64                      # list entries past E * cap: never written
LOG2E = np.float32(1.4426950408889634)
NEAR_ZERO = 2.0 ** -120         # a weight below this fraction of its row's largest: under fp32's exp range


# ------------------------------------------------------------------------------------------------ route: families

def _perms(rng, T, E):
    return np.stack([rng.permutation(E) for _ in range(T)])


def route_logits(fam, E, k, T, g=2.0 ** -6, seed=0):
    """f32 logits [T, E] of one family (module docstring of the tests); every value is exact in fp32 and so is
    l - max. census ignores T (T = E), ties has its own rows."""
    rng = np.random.default_rng(1000 * E + 10 * T + k + seed)
    e = np.arange(E)
    if fam in ("grid", "shift+", "shift-", "far"):
        lg = -g * _perms(rng, T, E).astype(np.float64)
        if fam == "far":
            lg[np.arange(T), (np.arange(T) * 7 + E - 1) % E] = 100.0     # token 0: the last expert
        return (lg + {"shift+": 1e4, "shift-": -1e4}.get(fam, 0.0)).astype(np.float32)
    if fam == "census":         # token t: experts t, t + 1, .. in slot order; every expert k rows, once per slot
        return (-g * ((e[None, :] - e[:, None]) % E)).astype(np.float32)
    if fam == "hot":            # the same k experts for every token, their slot rotating with the token
        H = hot_experts(E, k)
        lg = -g * (k + _perms(rng, T, E)).astype(np.float64)
        for t in range(T):
            for j in range(k):
                lg[t, H[(j + t) % k]] = -g * j
        return lg.astype(np.float32)
    if fam == "ties":
        rows = [np.zeros(E), np.where(e % 2 == 0, -0.0, 0.0), np.zeros(E)]
        for j in range(k - 1):                      # k - 1 distinct leaders from the top end, the cut inside a tie
            rows[2][E - 1 - j] = 5.0 - 0.5 * j
        if E > 64:
            r = np.zeros(E)
            a = min(3, E - 65)
            r[a] = r[a + 64] = 5.0                  # the same lane in both halves (3 and 67): the low one first
            rows.append(r)
            r = np.zeros(E)
            r[64:] = 1.0                            # the high half ahead of the low half
            rows.append(r)
        return np.stack(rows).astype(np.float32)
    raise ValueError(fam)


def hot_experts(E, k):
    """k experts: 0, E - 1, then both sides of a multiple of 8 and of 64 where E allows."""
    out = []
    for v in (0, E - 1, 7, 8, 63, 64, 1, E - 2, 2, 3, 4, 5, 6):
        if 0 <= v < E and v not in out:
            out.append(v)
    return out[:k]


# ------------------------------------------------------------------------------------------------ route: reference

def rank(p, k, high=False):
    """The k first of a stable sort on (-p, index), NaNs last (high: ties to the HIGHER index, fault R6)."""
    key = np.where(np.isnan(p), np.inf, -p)
    if high:
        E = p.shape[-1]
        return E - 1 - np.argsort(key[..., ::-1], axis=-1, kind="stable")[..., :k]
    return np.argsort(key, axis=-1, kind="stable")[..., :k]


def route_ref(lg, k, renorm=True, fault=None):
    """fp64 softmax -> top-k in slot order -> weights. Returns (sel [T, k], w [T, k])."""
    l = np.asarray(lg, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.exp(l - np.nanmax(l, -1, keepdims=True))
        s = (p[:, :64] if fault == "R5 sum over experts 0..63" else p).sum(-1, keepdims=True)
        sel = rank(p, k, high=fault == "R6 tie to the higher index")
        w = np.take_along_axis(p, sel, -1) / s
        if renorm != (fault == "R4 renormalisation flipped"):
            w = w / w.sum(-1, keepdims=True)
    return sel, w


def tree_sum32(p):
    """fp32 sum over the last axis as a binary tree (the xor-shuffle reductions)."""
    p = np.asarray(p, np.float32)
    n = 1 << max(0, int(p.shape[-1] - 1).bit_length())
    p = np.concatenate([p, np.zeros((*p.shape[:-1], n - p.shape[-1]), np.float32)], -1)
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p


def route_emu(lg, k, renorm=True, low_max=False):
    """The kernels' arithmetic in fp32: exp as exp2(fp32(x * log2e)), the fp32 tree sum, the divide, the slots' sum
    in slot order and the second divide. low_max: the maximum over experts 0..63 only (fault R5)."""
    l = np.asarray(lg, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.nanmax(l[:, :64] if low_max else l, -1, keepdims=True)
        t = ((l - mx).astype(np.float32) * LOG2E).astype(np.float32)
        p = np.exp2(t.astype(np.float64)).astype(np.float32)
        s = tree_sum32(p)
        sel = rank(p, k)
        w = (np.take_along_axis(p, sel, -1) / s).astype(np.float32)
        if renorm:
            ws = np.zeros((l.shape[0], 1), np.float32)
            for j in range(k):
                ws = (ws + w[:, j:j + 1]).astype(np.float32)
            w = (w / ws).astype(np.float32)
    return sel, w


def w_ratio(w, ref, tol):
    """|w - ref| over tol * (ref, plus the row's largest weight where ref is below fp32's exp range). NaN: inf."""
    w, ref = np.asarray(w, np.float64), np.asarray(ref, np.float64)
    wmax = ref.max(-1, keepdims=True)
    scale = ref + np.where(ref < NEAR_ZERO * wmax, wmax, 0.0)
    r = np.abs(w - ref) / (tol * scale)
    return float(np.where(np.isfinite(r), r, np.inf).max())


def lists_of(sel, E):
    """Expert -> [(x row, y row)] of a choice sel [T, k]: token t, row t * k + j."""
    T, k = sel.shape
    out = {e: [] for e in range(E)}
    for t in range(T):
        for j in range(k):
            out[int(sel[t, j])].append((t, t * k + j))
    return out


def route_arrays(sel, w, E, cap, lists=None, rows=None):
    """What a correct route leaves in its buffers (lists in token order): dict of topw [rows * k], sel [rows * k],
    counts [E], xr / yr [E * cap + GUARD]; everything that is no target holds SENT."""
    T, k = sel.shape
    rows = rows or T
    lists = lists_of(sel, E) if lists is None else lists
    o = dict(topw=np.full(rows * k, float(SENT)), sel=np.full(rows * k, SENT, np.int64), counts=np.zeros(E, np.int64),
             xr=np.full(E * cap + GUARD, SENT, np.int64), yr=np.full(E * cap + GUARD, SENT, np.int64))
    o["topw"][:T * k], o["sel"][:T * k] = np.asarray(w, np.float64).reshape(-1), sel.reshape(-1)
    for e, pr in lists.items():
        o["counts"][e] = len(pr)
        for i, (x, y) in enumerate(pr):
            o["xr"][e * cap + i], o["yr"][e * cap + i] = x, y
    return o


def route_compare(out, ref, T, E, k, cap, tol):
    """(what differs among the exact outputs or "", largest weight ratio): sel slot by slot, counts, per expert the
    multiset of (x row, y row) pairs (list order is free), every list entry at or past a count, the guard tail, and
    topw / sel past T * k."""
    bad = []
    if not np.array_equal(out["sel"], ref["sel"]):
        bad.append("sel")
    if not np.array_equal(out["counts"], ref["counts"]):
        bad.append("counts")
    for e in range(E):
        c, co = int(ref["counts"][e]), max(0, min(cap, int(out["counts"][e])))
        a = sorted(zip(out["xr"][e * cap:e * cap + co].tolist(), out["yr"][e * cap:e * cap + co].tolist()))
        b = sorted(zip(ref["xr"][e * cap:e * cap + c].tolist(), ref["yr"][e * cap:e * cap + c].tolist()))
        if a != b:
            bad.append(f"pairs of expert {e}")
        rest = slice(e * cap + co, (e + 1) * cap)
        if (out["xr"][rest] != SENT).any() or (out["yr"][rest] != SENT).any():
            bad.append(f"entries past the count of expert {e}")
    if (out["xr"][E * cap:] != SENT).any() or (out["yr"][E * cap:] != SENT).any():
        bad.append("guard tail")
    if (out["topw"][T * k:] != SENT).any():
        bad.append("topw past T * k")
    r = w_ratio(out["topw"][:T * k].reshape(T, k), ref["topw"][:T * k].reshape(T, k), tol)
    return "; ".join(bad[:4]), r


def route_faults(sel, w, E, cap):
    """(name, faulty arrays) of the list faults R1 - R3 and R7 on a reference choice; None where the fault does not
    apply (R3 at k = 1, R7 without an expert >= 64)."""
    T, k = sel.shape
    t, j = T // 2, k - 1
    e = int(sel[t, j])
    ls = lists_of(sel, E)
    ls[e].remove((t, t * k + j))
    ls[(e + 1) % E].append((t, t * k + j))
    yield "R1 one (token, slot) under the neighbouring expert", route_arrays(sel, w, E, cap + 1, ls)
    ls = lists_of(sel, E)
    ls[e].append(ls[e][-1])
    yield "R2 one row listed twice", route_arrays(sel, w, E, cap + 1, ls)
    ls = lists_of(sel, E)
    ls[e].pop()
    yield "R2 one row left out", route_arrays(sel, w, E, cap + 1, ls)
    if k > 1:
        ls = lists_of(sel, E)
        a, b = int(sel[t, 0]), int(sel[t, 1])
        ls[a][ls[a].index((t, t * k))] = (t, t * k + 1)
        ls[b][ls[b].index((t, t * k + 1))] = (t, t * k)
        yield "R3 slots j and j + 1 exchanged in yrows, not in topw", route_arrays(sel, w, E, cap + 1, ls)
    else:
        yield "R3 slots j and j + 1 exchanged in yrows, not in topw", None
    if (sel >= 64).any():
        yield "R7 expert index without its bit 6", route_arrays(sel & ~64, w, E, cap + 1)
    else:
        yield "R7 expert index without its bit 6", None


# --------------------------------------------------------------------------------------------------- router logits

def logit_ref(h, wr, fault=None):
    """(h @ wr^T, B = |h| @ |wr|^T) in fp64 over h [T, D], wr [E, D]. fault: L1 / L2 of the tests' docstring."""
    h, wr = np.asarray(h, np.float64), np.asarray(wr, np.float64)
    T, D = h.shape
    c0 = (D // 8 // 2) * 8                  # the chunk the L1 faults touch
    ref, B = h @ wr.T, np.abs(h) @ np.abs(wr).T
    if fault is None:
        return ref, B
    hc, wc = h[:, c0:c0 + 8], wr[:, c0:c0 + 8]
    if fault == "L1 one 8-column chunk dropped":
        return ref - hc @ wc.T, B
    if fault == "L1 chunk of the neighbouring expert row":
        return ref - hc @ wc.T + hc @ np.roll(wc, 1, 0).T, B
    if fault == "L1 chunk of the neighbouring token":
        return ref - hc @ wc.T + np.roll(hc, 1, 0) @ wc.T, B
    if fault == "L2 tail past a 4096-column pass dropped":
        n = D // 4096 * 4096 if D > 4096 else D
        return h[:, :n] @ wr[:, :n].T, B
    raise ValueError(fault)


LOGIT_FAULTS = ["L1 one 8-column chunk dropped", "L1 chunk of the neighbouring expert row",
                "L1 chunk of the neighbouring token", "L2 tail past a 4096-column pass dropped"]


def logit_emu(h, wr, group=8):
    """fp32 products; a thread adds its `group` consecutive products in order, the partial sums meet in a tree."""
    h, wr = np.asarray(h, np.float32), np.asarray(wr, np.float32)
    T, D = h.shape
    out = np.zeros((T, wr.shape[0]), np.float32)
    pad = -D % group
    for e in range(wr.shape[0]):
        pr = np.concatenate([(h * wr[e][None, :]).astype(np.float32), np.zeros((T, pad), np.float32)], 1)
        pr = pr.reshape(T, -1, group)
        acc = np.zeros(pr.shape[:2], np.float32)
        for i in range(group):
            acc = (acc + pr[:, :, i]).astype(np.float32)
        out[:, e] = tree_sum32(acc)[:, 0]
    return out


def logit_ratio(lg, ref, B):
    err = np.abs(np.asarray(lg, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, err / B, np.where(err > 0, np.inf, 0.0))
    return float(np.where(np.isfinite(r), r, np.inf).max())


def logit_case(fam, E, T, D, seed=0):
    """h [T, D] (f16 values) and wr [E, D] (f16 values) as float64. integer: h in {-1, 0, 1}, wr small integers that
    differ in every 8-column chunk, expert row and column -- every partial sum is exact in fp32."""
    rng = np.random.default_rng(100 * D + 10 * T + E + seed)
    if fam == "integer":
        h = rng.integers(-1, 2, (T, D)).astype(np.float64)
        c, e = np.arange(D)[None, :], np.arange(E)[:, None]
        return h, ((3 * (c // 8) + 5 * e + c % 8) % 17 - 8).astype(np.float64)
    h = rng.standard_normal((T, D)).astype(np.float16).astype(np.float64)
    return h, (0.05 * rng.standard_normal((E, D))).astype(np.float16).astype(np.float64)


# --------------------------------------------------------------------------------- norm + router + route in one launch

def norm_route_case(E, T, D, seed=0, rows=None):
    """x [T, D] f32, nw [D] f32, wr [E, D] f16 values with wr[e] = sum_t C[t, e] u_t, u_t the dual basis of the fp64
    normed rows n_t (n_s . u_t = [s == t]): the fp64 logits are C, row t a permutation of the grid g * (1 + arange(E))
    (g = 1/4; 2^-5 from E = 33), up to the f16 rounding of wr. rows: given rows to use instead of Gaussian ones."""
    rng = np.random.default_rng(1000 * D + 10 * E + T + seed)
    if rows is None:
        x = (3.0 * rng.standard_normal((T, D))).astype(np.float32)
        if D < 16:
            x[:, :T] += 8.0 * np.eye(T, dtype=np.float32)       # D = 4, T = 4: keep the rows apart
    else:
        x = np.asarray(rows, np.float32)
    nw = (rng.choice([-1.0, 1.0], D) * 2.0 ** (-4 + 2 * rng.random(D))).astype(np.float32)
    n = R.rms_ref(x, nw, 1e-5)
    U = n.T @ np.linalg.inv(n @ n.T)
    g = 0.25 if E <= 8 else 2.0 ** -5
    C = g * (1 + _perms(rng, T, E))
    wr = np.ascontiguousarray((U @ C).T).astype(np.float16).astype(np.float64)
    return dict(x=x, nw=nw, eps=1e-5, wr=wr, n=n, C=C, g=g)


# --------------------------------------------------------------------------------------------------------- combine

COMBINE_FAULTS = ["C1 slot weight of the neighbouring token", "C2 alpha also on the residual",
                  "C3 set_ adds onto the stale residual", "C4 columns past the last full 256 dropped"]


def combine_case(fam, T, k, D, seed=0):
    """resid [T, D], y [T * k, D], wt [T, k] as float64 of f32 values. tag: weights 2^-(1 + (j + t) % 8) (the
    neighbouring token's and the neighbouring slot's differ), y integer tags of (t, j, column), integer residual."""
    rng = np.random.default_rng(100 * D + 10 * T + k + seed)
    if fam == "tag":
        t, j, c = np.arange(T)[:, None, None], np.arange(k)[None, :, None], np.arange(D)[None, None, :]
        y = (((t * k + j) * D + c) % 251 + 1).astype(np.float64).reshape(T * k, D)
        wt = 2.0 ** -(1 + (j[:, :, 0] + t[:, :, 0]) % 8)
        return rng.integers(-1000, 1001, (T, D)).astype(np.float64), y, wt
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return f(rng.standard_normal((T, D))), f(rng.standard_normal((T * k, D))), f(rng.random((T, k)) + 0.05)


def combine_ref(resid, y, wt, alpha, set_, fault=None):
    """(resid + alpha sum_j wt[t, j] y[t k + j], or the sum alone with set_; its size |x| + |alpha| sum |w y|)."""
    T, k = wt.shape
    D = resid.shape[1]
    if fault == "C1 slot weight of the neighbouring token":
        wt = np.roll(wt, 1, 0)
    t = alpha * wt[:, :, None] * y.reshape(T, k, D)
    base = resid if (not set_ or fault == "C3 set_ adds onto the stale residual") else np.zeros_like(resid)
    if fault == "C2 alpha also on the residual":
        base = alpha * base
    out, size = base + t.sum(1), np.abs(base) + np.abs(t).sum(1)
    if fault == "C4 columns past the last full 256 dropped":
        out[:, D // 256 * 256:] = resid[:, D // 256 * 256:]
    return out, size


def combine_tag_candidates(resid, y, wt, alpha, set_):
    """The tag family's result is exact up to ONE choice the compiler has: alpha * s is rounded to fp32 before the
    add, or fused into it. Both candidates (equal unless alpha has more than a few bits)."""
    T, k = wt.shape
    s = (wt[:, :, None] * y.reshape(T, k, -1)).sum(1)                 # exact: 8-bit tags under 8 binary places
    prod = float(np.float32(alpha)) * s                               # exact in fp64 (24 + 17 bits)
    if set_:
        return [prod.astype(np.float32).astype(np.float64)]
    return [(resid + prod).astype(np.float32).astype(np.float64),
            (resid + prod.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)]


# ------------------------------------------------------------------------------------- expert launches over row lists

ROWS, K = 256, 256


@functools.lru_cache(maxsize=None)
def expert_raw(t, fam, e):
    """Block bytes of expert e's [256, 256] weights (qblocks' family `fam`), another seed per expert."""
    rng = np.random.default_rng(7000 + 131 * int(t) + e + (500 if fam == "full" else 0))
    return QB.structured_blocks(t, ROWS, K, fam, rng)


@functools.lru_cache(maxsize=None)
def expert_dense(t, fam, e, k=K, rows=ROWS):
    return Q.dequantize(expert_raw(t, fam, e), t, (rows, k)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def expert_mag(t, fam, e):
    return QB.decode(QB.fields(t, expert_raw(t, fam, e), ROWS, K))[1]


def acts(fam, rows, k=K, seed=1):
    """f16 activation values [rows, k] as float64: {-1, 0, 1} (integer) or Gaussian (full)."""
    rng = np.random.default_rng(seed)
    if fam == "integer":
        return rng.integers(-1, 2, (rows, k)).astype(np.float64)
    return rng.standard_normal((rows, k)).astype(np.float16).astype(np.float64)


def make_plan(name, T, k, E, cap, order="desc", seed=0):
    """Hand-written row lists: dict(xrows, yrows [E * cap + GUARD], counts [E], sel [T * k]). hot: all tokens to the
    same k experts (0, E - 1, 7, 8, 63, 64, ..), each count = T, lists descending or shuffled; diag: every expert at
    most one row; last: slot 0 of every token to expert E - 1; pairs (T = 3): later slots repeat earlier ones, one
    sel entry outside the table. List entries past a count hold row 0 (x) and the never-written row T * k + 1 (y);
    sel of an unlisted slot is -1."""
    rng = np.random.default_rng(seed + 17 * T)
    ls = {e: [] for e in range(E)}
    sel = np.full(T * k, -1, np.int64)
    if name == "hot":
        H = hot_experts(E, k)
        for t in range(T):
            for j in range(k):
                ls[H[(j + t) % k]].append((t, t * k + j))
        for e in H:
            ls[e] = ls[e][::-1] if order == "desc" else [ls[e][i] for i in rng.permutation(T)]
    elif name == "diag":
        slots = rng.permutation(T * k)[:E]
        for s, e in zip(slots, rng.permutation(E)):
            ls[int(e)].append((int(s) // k, int(s)))
    elif name == "last":
        ls[E - 1] = [(t, t * k) for t in range(T)][::-1]
    elif name == "pairs":
        assert T == 3 and k == 8
        rows = [[5, 9, E - 1, 0, 64, 33, 7, 8], [9, 5, 0, E - 1, E + 72, 64, 8, 70], [E - 1, 0, 5, 9, 8, 7, 33, 64]]
        for t in range(T):
            for j in range(k):
                if rows[t][j] < E:
                    ls[rows[t][j]].append((t, t * k + j))
                else:
                    sel[t * k + j] = rows[t][j]
    else:
        raise ValueError(name)
    p = dict(name=name, T=T, k=k, E=E, cap=cap, xrows=np.zeros(E * cap + GUARD, np.int64),
             yrows=np.full(E * cap + GUARD, T * k + 1, np.int64), counts=np.zeros(E, np.int64), sel=sel)
    for e, pr in ls.items():
        p["counts"][e] = len(pr)
        for i, (x, y) in enumerate(pr):
            p["xrows"][e * cap + i], p["yrows"][e * cap + i] = x, y
            sel[y] = e
    return p


EXPERT_FAULTS = ["X1 weights of expert e + 1", "X2 maps read at e * T", "X3 second m-block gathers block 0's rows",
                 "X3 second m-block left unwritten", "X4 count of expert e + 1", "X5 repeat exit skips a distinct expert",
                 "X6 list assumed ascending"]


def expert_ref(p, W, x, M, down=False, selected=False, block=64, fault=None, nrows=None):
    """Output rows [nrows, W rows] of a launch over plan p: row yrows[i] = x[xmap[i]] @ W(e)^T for the first
    min(count, M) entries of every expert (selected: of every expert some sel slot names), xmap = xrows (gate|up
    shape) or yrows (down shape); every other row keeps SENT. W: expert -> float64 [rows, K]."""
    T, k, E, cap = p["T"], p["k"], p["E"], p["cap"]
    nrows = nrows or T * k + GUARD
    out = None
    stride = T if fault == "X2 maps read at e * T" else cap
    experts = range(E)
    if selected:        # a slot exits when an earlier slot names its expert (X5: or that of the slot before it)
        experts, sl = [], p["sel"].tolist()
        for i, s in enumerate(sl):
            exits = s in sl[:i]
            if fault == "X5 repeat exit skips a distinct expert" and i >= 1 and sl[i - 1] in sl[:i - 1]:
                exits = True
            if 0 <= s < E and not exits and s not in experts:
                experts.append(s)
    for e in experts:
        c = min(int(p["counts"][(e + 1) % E if fault == "X4 count of expert e + 1" else e]), M)
        if c <= 0:
            continue
        yi = p["yrows"][e * stride:e * stride + c]
        xi = yi if down else p["xrows"][e * stride:e * stride + c]
        if fault == "X6 list assumed ascending":
            xi = np.sort(xi)
        if fault == "X3 second m-block gathers block 0's rows" and c > block:
            xi = np.concatenate([xi[:block], xi[:c - block]])
        if fault == "X3 second m-block left unwritten":
            yi, xi = yi[:block], xi[:block]
        w = W((e + 1) % E if fault == "X1 weights of expert e + 1" else e)
        if out is None:
            out = np.full((nrows, w.shape[0]), float(SENT))
        out[yi] = x[xi] @ w.T
    if out is None:
        out = np.full((nrows, W(0).shape[0]), float(SENT))
    return out


def swiglu_bound(g, u, Bg, Bu, tol):
    """(silu(g) u, its bound): the propagated bound of test_weight_sensitivity.test_swiglu_epilogue_full -- g and u
    each within tol * B of their reference, silu'' <= 1/2, plus the f16 rounding of the output."""
    sg = 1.0 / (1.0 + np.exp(-g))
    ref = g * sg * u
    lim = tol * (np.abs(sg * (1 + g * (1 - sg)) * u) * Bg + np.abs(g * sg) * Bu) + tol * tol * Bg * Bu / 2 \
        + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return ref, lim
