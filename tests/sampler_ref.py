"""Reference of the sampler (csrc/kernels/sample.hip) written from its definition, in numpy fp64, with the input
families of tests/test_sampler_sensitivity.py, float32 emulations of the kernel's sums and of hist_threshold, and the
fault models. Nothing here imports ops or engine.sampling, except pbytes() for the byte image of SampleParams.

One row, one parameter set (ref_row):
  penalties    distinct window ids in [0, V), count of each id in the window; v / rp for v > 0 else v * rp; minus
               presence + frequency * count
  kept set     temperature, then top-k (the k-th largest finite logit, ties kept; top_k >= finite count keeps every
               finite logit), then min-p (l >= max + T ln min_p), then top-p (the smallest top set of the kept tokens
               whose mass reaches top_p of the kept mass, ties of its last weight kept); NaN and -inf are never kept
  intervals    the kept ids in index order, token j owns u in [c_j, c_j+1) of the normalised cumulative mass
  margins      logit: for every active cut, (gap between the cut and the nearest non-tied logit on the side that
               decides) / (what the kernel resolves: (b - a) / NB^2 of hist_threshold's search range plus one ulp of the
               largest logit; min-p, which is no search: 4 ulp plus T |ln min_p| 2^-21 for the fast logarithm);
               mass: distance of top_p Z from the cumulative mass on both sides of the (tie group at the) cut, over Z;
               interval: the narrowest interval among kept tokens within 30 temperatures of the maximum (`negl`: the
               total mass of the kept tokens further down, which a designed row keeps below g).
The decode kernels add (decode_ref): window = ring slots [0, min(S, pos + 1)), ids outside [0, V) ignored (-1 = empty),
u = uniform01(seed, pos) (splitmix64 in integers), the token appended at slot (pos + 1) % S.
"""
import collections
import functools
import math

import numpy as np

NT, NB, MAXT, KFAST, CCAP, MAXC = 1024, 1024, 4096, 256, 512, 1024
f32, f64 = np.float32, np.float64
NEG = float("-inf")
_FIELDS = ("temperature", "top_p", "min_p", "repeat_penalty", "presence_penalty", "frequency_penalty")


def P(**kw):
    """A parameter set; float fields as the float32 the device struct holds."""
    d = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repeat_penalty=1.0, presence_penalty=0.0,
             frequency_penalty=0.0)
    d.update(kw)
    for k in _FIELDS:
        d[k] = float(f32(d[k]))
    return d


def penal(p):
    return p["repeat_penalty"] != 1.0 or p["presence_penalty"] != 0.0 or p["frequency_penalty"] != 0.0


def pbytes(p, u=0.0, n_hist=0):
    from nats_llm_studio_amd.ops import _lib
    return bytes(_lib.SampleParams(p["temperature"], p["top_p"], p["min_p"], p["repeat_penalty"], p["presence_penalty"],
                                   p["frequency_penalty"], u, int(p["top_k"]), int(n_hist), 0))


_M64 = (1 << 64) - 1


def uniform01(seed, pos):
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(pos) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def ulp32(x):
    return float(np.spacing(f32(abs(x)))) if math.isfinite(x) else 0.0


Ref = collections.namedtuple("Ref", "x pen greedy tok kept edges w margins")


def penalise(l32, p, window, per_occurrence=False, divide_negative=False):
    """fp64 penalised row and {id: new value}. The two flags are fault models F10 / F11."""
    x = np.asarray(l32, dtype=f32).astype(f64)
    V, pen = x.shape[0], {}
    if penal(p):
        ids = [int(i) for i in window if 0 <= int(i) < V]
        cnt = collections.Counter(ids)
        for i in (ids if per_occurrence else cnt):
            v = x[i]
            if p["repeat_penalty"] != 1.0:
                v = v / p["repeat_penalty"] if (v > 0 or divide_negative) else v * p["repeat_penalty"]
            v -= p["presence_penalty"] + p["frequency_penalty"] * cnt[i]
            x[i] = pen[i] = v
    return x, pen


def ref_row(l32, p, window=(), fault=None):
    """The definition. fault: one of F1 - F6 (kept-set / order faults applied to the reference), F10 / F11."""
    x, pen = penalise(l32, p, window, fault == "F10", fault == "F11")
    V, T = x.shape[0], p["temperature"]
    with np.errstate(invalid="ignore"):
        fin = x > NEG                                  # NaN compares false
    m = dict(logit=math.inf, mass=math.inf, interval=math.inf, negl=0.0)
    if T <= 0.0:
        if fin.any():
            tok = int(np.flatnonzero(fin & (x == x[fin].max()))[0])
        else:
            neg = np.flatnonzero(x == NEG)
            tok = int(neg[0]) if neg.size else 0
        return Ref(x, pen, True, tok, None, None, None, m)
    if not fin.any():
        return Ref(x, pen, False, None, np.zeros(0, np.int64), np.zeros(1), np.zeros(0), m)
    xs = np.where(fin, x, NEG)
    mx, mn = float(x[fin].max()), float(x[fin].min())
    big = ulp32(max(abs(mx), abs(mn)))
    keep = fin.copy()
    k, nf = int(p["top_k"]), int(fin.sum())
    if 0 < k < V:
        if k < nf:
            srt = np.sort(xs[fin])[::-1]
            vk = srt[k] if fault == "F1" else srt[k - 1]
            keep &= (xs > vk) if fault == "F2" else (xs >= vk)
            if fault == "F1":
                keep &= ~(xs == srt[k - 1]) | (srt[k - 1] == srt[k])
            below = srt[srt < srt[k - 1]]
            if below.size:
                m["logit"] = min(m["logit"], (srt[k - 1] - below[0]) / ((mx - mn) / NB ** 2 + big))
        elif fault == "F3":
            keep &= xs > mn
    if p["min_p"] > 0.0:
        lo = mx + (1.0 if fault == "F5" else T) * math.log(p["min_p"])
        cand = xs[keep]
        if cand.size:
            need = 4 * ulp32(max(abs(mx), abs(lo))) + T * abs(math.log(p["min_p"])) * 2.0 ** -21
            m["logit"] = min(m["logit"], float(np.abs(cand - lo).min()) / need)
        keep &= xs >= lo
    w = np.where(keep, np.exp((xs - mx) / T), 0.0)
    if p["top_p"] < 1.0 and keep.any():
        ids = np.flatnonzero(keep)
        base = np.where(fin, np.exp((xs - mx) / T), 0.0) if fault == "F4" else w
        order = ids[np.argsort(-xs[ids], kind="stable")]
        sv, cum = xs[order], np.cumsum(w[order])
        target = p["top_p"] * float(base.sum())
        n_keep = min(int(np.searchsorted(cum, target, side="left")) + 1, len(order))
        thr = sv[n_keep - 1]
        g0, g1 = int(np.searchsorted(-sv, -thr, side="left")), int(np.searchsorted(-sv, -thr, side="right"))
        # (past the last kept token nothing can be cut, and above the maximum's group the mass is exactly 0 < target:
        # only the other side counts there)
        if fault != "F4":
            m["mass"] = min(m["mass"], (target - cum[g0 - 1]) / cum[-1] if g0 else math.inf,
                            (cum[g1 - 1] - target) / cum[-1] if g1 < len(order) else math.inf)
        if g1 < len(order):
            a = max(float(sv[-1]), mx - 30.0 * T)
            m["logit"] = min(m["logit"], (thr - sv[g1]) / ((mx - a) / NB ** 2 + big))
        keep &= (xs > thr) if fault == "F2" else (xs >= thr)
        w = np.where(keep, w, 0.0)
    kept = np.flatnonzero(keep)
    wk = w[kept]
    if fault == "F6" and kept.size:                     # the draw walks in value order
        o = np.argsort(-xs[kept], kind="stable")
        kept, wk = kept[o], wk[o]
    Z = wk.sum()
    edges = np.concatenate([[0.0], np.cumsum(wk)]) / Z if kept.size else np.zeros(1)
    if kept.size:
        edges[-1] = 1.0
        heavy = wk >= math.exp(-30.0) * wk.max()
        m["interval"] = float(np.diff(edges)[heavy].min())
        m["negl"] = float(wk[~heavy].sum() / Z)
    return Ref(x, pen, False, None, kept, edges, wk, m)


def draw(r, u, shift=0):
    """The reference's token for variate u (None: nothing kept, any id in range). shift: fault F9."""
    if r.greedy:
        return r.tok
    if not r.kept.size:
        return None
    j = int(np.searchsorted(r.edges[1:], u, side="right"))
    j = min(j, r.kept.size - 1)
    return int(r.kept[min(max(j + shift, 0), r.kept.size - 1)])


def accepted(r, u, tok, g):
    """The metric: u lies in tok's interval widened by g on both sides."""
    if r.greedy:
        return tok == r.tok
    if not r.kept.size:
        return 0 <= tok < r.x.shape[0]
    j = np.flatnonzero(r.kept == tok)
    return bool(j.size) and r.edges[j[0]] - g <= u < r.edges[j[0] + 1] + g


def step_distance(r, u):
    return float(np.abs(r.edges - u).min()) if not r.greedy and r.kept.size else math.inf


def fair(r, g):
    m = r.margins
    return m["logit"] > 1.0 and m["mass"] >= 8 * g and m["interval"] >= 8 * g and m["negl"] < g


def decode_ref(l32, p, ring, pos, seed, ctx_len=1, fault=None):
    """sample_decode_kernel on one row: (token or None when the row is skipped, u, window, append slot)."""
    S = len(ring)
    if ctx_len <= 0 or (p["temperature"] <= 0.0 and not penal(p)):
        return None, None, (), None, None
    n = min(S, pos + 1)
    if fault == "F12a":
        n = min(S, pos)                                  # window one short
    window = [int(t) for t in ring[:n]]
    u = uniform01(seed, pos)
    r = ref_row(l32, p, window)
    return draw(r, u), u, window, ((pos if fault == "F12b" else pos + 1) % S), r


# ---------------------------------------------------------------------------------------- float32 emulations

def _hs_scan(a):
    """Hillis-Steele inclusive scan along the last axis (length 64), float32, as the __shfl_up loops."""
    a = a.astype(f32).copy()
    o = 1
    while o < a.shape[-1]:
        b = a.copy()
        b[..., o:] = a[..., o:] + a[..., :-o]
        a, o = b, o * 2
    return a


def _weights32(x32, lo, mx, T):
    it = f32(1.0) / f32(T)
    with np.errstate(invalid="ignore", over="ignore"):
        k = (x32 >= f32(lo)) & (x32 > f32(NEG))
        arg = ((x32 - f32(mx)) * it).astype(f32)
    return np.where(k, np.exp(np.where(k, arg, 0).astype(f64)).astype(f32), f32(0))


def emu_cdf_general(x32, lo, mx, T, per_one=False):
    """draw_index_order's sums in float32: (cdf32 per token as before + c, Z32)."""
    V = x32.shape[0]
    nt = (V + 63) // 64
    w = np.zeros(nt * 64, f32)
    w[:V] = _weights32(x32, lo, mx, T)
    w = w.reshape(nt, 64)
    t = w.copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        t = (t + t[:, lanes ^ o]).astype(f32)
    tile = t[:, 0]
    per = 1 if per_one else (nt + NT - 1) // NT
    tp = np.zeros(NT * per, f32)
    tp[:min(nt, NT * per)] = tile[:NT * per]
    tp = tp.reshape(NT, per)
    loc = np.zeros(NT, f32)
    for j in range(per):
        loc = (loc + tp[:, j]).astype(f32)
    incl = _hs_scan(loc.reshape(16, 64))
    red = incl[:, 63]
    off, Z, offs = f32(0), f32(0), []
    for i in range(16):
        offs.append(off)
        off = f32(off + red[i])
    Z = off
    excl = ((np.asarray(offs, f32)[:, None] + incl).astype(f32) - loc.reshape(16, 64)).astype(f32).reshape(NT)
    before = np.zeros((NT, per), f32)
    acc = excl.copy()
    for j in range(per):
        before[:, j] = acc
        acc = (acc + tp[:, j]).astype(f32)
    before = before.reshape(-1)[:nt]
    c = _hs_scan(w[:len(before)])
    return (before[:, None] + c).astype(f32).reshape(-1)[:V], float(Z)


def emu_cdf_fast(wk32):
    """sample_topk_fast's final scan: <= CCAP weights in index order, one per thread of the block."""
    w = np.zeros(NT, f32)
    w[:len(wk32)] = wk32
    incl = _hs_scan(w.reshape(16, 64))
    off, out = f32(0), []
    for i in range(16):
        out.append((off + incl[i]).astype(f32))
        off = f32(off + incl[i, 63])
    cdf = np.concatenate(out)
    return cdf[:len(wk32)], float(cdf[-1])


def emu_noise(l32, p, window=()):
    """Largest |cdf32 - cdf64| over the kept tokens of one row, general path and (if it applies) fast path."""
    r = ref_row(l32, p, window)
    if r.greedy or not r.kept.size:
        return 0.0
    x32 = r.x.astype(f32)
    with np.errstate(invalid="ignore"):
        fin = x32 > f32(NEG)
    mx, lo = float(x32[fin].max()), float(x32[r.kept].min())
    cdf, Z = emu_cdf_general(x32, lo, mx, p["temperature"])
    e = float(np.abs(cdf[r.kept].astype(f64) / Z - r.edges[1:]).max())
    if r.kept.size <= CCAP:
        cf, Zf = emu_cdf_fast(_weights32(x32[r.kept], lo, mx, p["temperature"]))
        e = max(e, float(np.abs(cf.astype(f64) / Zf - r.edges[1:]).max()))
    return e


def _bins(b, v, scale):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.minimum(NB - 1, ((f32(b) - v).astype(f32) * f32(scale)).astype(f32).astype(np.int64))


def _cross(h, above, target):
    cum = above + np.cumsum(h)
    hit = np.flatnonzero(cum >= target)
    if not hit.size:
        return -1, above + h.sum()
    return int(hit[0]), float(cum[hit[0]] - h[hit[0]])


def emu_threshold_old(x32, k):
    """hist_threshold's count mode as it was before the fix, operation for operation in float32."""
    with np.errstate(invalid="ignore"):
        fin = x32 > f32(NEG)
    v = x32[fin]
    a, b, above = f32(v.min()), f32(v.max()), 0.0
    for _ in range(2):
        if not b > a:
            break
        scale = f32(NB) / f32(b - a)
        sel = (v >= a) & (v <= b)
        h = np.bincount(_bins(b, v[sel], scale), minlength=NB)
        bn, before = _cross(h, above, float(k))
        if bn < 0:
            bn, before = NB - 1, above + h.sum()
        above = before
        a, b = f32(b - f32(f32(bn + 1) / scale)), f32(b - f32(f32(bn) / scale))
    return float(a)


def emu_threshold_new(x32, k):
    """The fixed arithmetic: the second pass takes the logits of the crossing bin by the same bin expression and
    returns the smallest logit counted toward the target; no crossing returns the lower end of the range."""
    with np.errstate(invalid="ignore"):
        fin = x32 > f32(NEG)
    v = x32[fin]
    a, b = f32(v.min()), f32(v.max())
    if not b > a:
        return float(a)
    scale = f32(NB) / f32(b - a)
    b0 = _bins(b, v, scale)
    bn, above = _cross(np.bincount(b0, minlength=NB), 0.0, float(k))
    if bn < 0:
        return float(a)
    nb_, na = f32(b - f32(f32(bn) / scale)), f32(b - f32(f32(bn + 1) / scale))
    s1 = f32(NB) / f32(nb_ - na) if f32(nb_ - na) > f32(1e-30) else f32(0)
    guard = f32(1.9e-6) * f32(max(abs(a), abs(b)))
    sub = v[(b0 == bn) & (v >= f32(na - guard)) & (v <= f32(nb_ + guard))]
    assert sub.size == int((b0 == bn).sum())          # the guard band only saves work: it may turn nothing away
    b1 = np.maximum(0, _bins(nb_, sub, s1))
    bn1, _ = _cross(np.bincount(b1, minlength=NB), above, float(k))
    return float(sub[b1 <= (NB - 1 if bn1 < 0 else bn1)].min())


# --------------------------------------------------------------------------------------------------- families

Case = collections.namedtuple("Case", "name logits params hists us")       # one launch: row i of each


def _rng(*key):
    return np.random.default_rng(int.from_bytes(repr(key).encode(), "little") % (1 << 63))


CARRIER_VS = (1, 2, 63, 64, 65, 1000, 1025, 4097, 65536, 65537, 128256, 151936, 262144)
NCAR = 48


def carrier_ids(V, row):
    """<= NCAR ids where the position logic can slip: 0, 63, 64, 65, V - 1, both sides of thread-run boundaries
    64 * per * t (t rotating with the row), 65535 / 65536, the last partial tile; random ids fill up."""
    nt = (V + 63) // 64
    per = (nt + NT - 1) // NT
    ids = [0, 63, 64, 65, V - 1, V - 2, 65535, 65536, (V - 1) // 64 * 64, (V - 1) // 64 * 64 - 1]
    ts = [1, 2, 63, 64, 65, 512, 1022, 1023] + [3 + (7 * row + 131 * j) % 1019 for j in range(6)]
    for t in ts:
        ids += [64 * per * t - 1, 64 * per * t]
    ids = list(dict.fromkeys(i for i in ids if 0 <= i < V))[:NCAR]
    rng = _rng("carrier", V, row)
    while len(ids) < min(V, NCAR):
        i = int(rng.integers(0, V))
        if i not in ids:
            ids.append(i)
    return sorted(ids)


CARRIER_PARAMS = (P(), P(top_k=300), P(top_k=NCAR), P(top_k=NCAR + 8, top_p=0.999, min_p=1e-6),
                  P(temperature=0.7, min_p=1e-9))


@functools.lru_cache(maxsize=None)
def _carrier_logits(V):
    """Shared by the parameter variants: carriers in [-3, -2), every other logit at -43 (40 T lower for T <= 1)."""
    rows = []
    for r in range(min(V, NCAR) + 6):
        ids = carrier_ids(V, r)
        rng = _rng("cw", V, r)
        l = np.full(V, -43.0, f32)
        l[ids] = (rng.uniform(0.0, 1.0, len(ids)) - 3.0).astype(f32)
        rows.append(l)
    L = np.stack(rows)
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def carriers(V, g, variant):
    """One row per carrier (its own carrier set and weights), u at that carrier's midpoint; six more rows with u = 0,
    1 - 2^-24 and 4 g inside each end of the first and the last interval. Every other logit is 40 T lower."""
    p = CARRIER_PARAMS[variant]
    n0 = min(V, NCAR)
    rows, us = range(n0 + 6), []
    L = _carrier_logits(V)
    for r in range(n0 + 6):
        ref = ref_row(L[r], p)
        heavy = np.flatnonzero(ref.w >= math.exp(-30.0) * ref.w.max())
        e = ref.edges
        if r < n0:
            j = heavy[r]
            us.append(0.5 * (e[j] + e[j + 1]))
        else:
            f, l_ = heavy[0], heavy[-1]
            us.append([0.0, 1.0 - 2.0 ** -24, e[f] + 4 * g, e[f + 1] - 4 * g, e[l_] + 4 * g, e[l_ + 1] - 4 * g][r - n0])
    us = [float(f32(min(max(u, 0.0), 1.0 - 2.0 ** -24))) for u in us]
    return Case(f"carriers V={V} {variant}", L, [p] * len(rows), [()] * len(rows), us)


def _sweep(L, p, hist, g, name):
    """One row per kept midpoint and per point 4 g inside either end of a kept interval, plus u = 0 and 1 - 2^-24: a
    token outside a cut can then never be drawn, the tokens just inside are drawn at their midpoints, and no edge of
    the CDF can move by more than 4 g."""
    ref = ref_row(L, p, hist)
    if ref.greedy or not ref.kept.size:
        us = [0.5]
    else:
        e = ref.edges
        heavy = np.flatnonzero(ref.w >= math.exp(-30.0) * ref.w.max())
        if heavy.size > 80:                              # about 64 of them, and always the first and last four
            heavy = np.unique(np.concatenate([heavy[:4], heavy[::max(4, -(-heavy.size // 64))], heavy[-4:]]))
        us = [0.0, 1.0 - 2.0 ** -24] + [0.5 * (e[j] + e[j + 1]) for j in heavy]
        # and 4 g inside both ends of each of these intervals: an edge that moves by more than 4 g is seen
        us += [u for j in heavy if e[j + 1] - e[j] >= 8 * g for u in (e[j] + 4 * g, e[j + 1] - 4 * g)]
    us = [float(f32(u)) for u in us]
    n = len(us)
    return Case(name, np.broadcast_to(L, (n, L.shape[0])), [p] * n, [tuple(hist)] * n, us)


CUT_V = 300


def cut_params(V=CUT_V):
    out = [P(top_k=k) for k in (1, 2, 40, 255, 256, 257, V - 1, V, V + 1)]
    out += [P(top_k=40, top_p=tp) for tp in (0.5, 0.9)] + [P(top_p=tp) for tp in (1e-6, 0.3, 0.95, 1.0 - 2.0 ** -24)]
    out += [P(min_p=mp) for mp in (0.5, 0.05, 1e-3)] + [P(temperature=0.7, top_k=257, top_p=0.9, min_p=0.01),
                                                        P(temperature=1.5, top_k=100, top_p=0.8, min_p=0.02)]
    return out


@functools.lru_cache(maxsize=None)
def cut_row(V=CUT_V, T=1.0):
    """Geometric weights, ratio 0.985 per rank, over ranks scattered through the ids (so value order != index
    order): every top-k / min-p / top-p cut has a logit margin of 0.015 T."""
    perm = _rng("cut", V).permutation(V)
    l = np.empty(V, f32)
    l[perm] = (2.0 + np.arange(V) * math.log(0.985) * T).astype(f32)
    return l


def cuts(g, i, V=CUT_V):
    p = cut_params(V)[i]
    return _sweep(cut_row(V, 1.0), p, (), g, f"cuts {i} {p}")


@functools.lru_cache(maxsize=None)
def tie_cases(g):
    out = []
    V = 4097
    base = cut_row(V, 1.0).copy()
    order = np.argsort(-base)
    # the k-th and (k+1)-th largest tied, at ids 1024 j - 1 and 1024 j
    for j, k, extra in ((1, 5, {}), (2, 40, {}), (3, 300, {}), (1, 5, dict(top_p=0.9)), (2, 40, dict(top_p=0.5))):
        l = base.copy()
        a, b = 1024 * j - 1, 1024 * j
        # move the pair to ranks k-1, k (0-based) by swapping values, then tie them
        for tgt, rank in ((a, k - 1), (b, k)):
            src = int(np.flatnonzero(l == base[order[rank]])[0])
            l[src], l[tgt] = l[tgt], l[src]
        l[b] = l[a]
        out.append(_sweep(l, P(top_k=k, **extra), (), g, f"ties k={k} at {a},{b} {extra}"))
    # a tie across the top-p cut: ranks 2 and 3 tied, top_p between the mass of 2 and of 3 tokens
    l = base.copy()
    for tgt, rank in ((2047, 2), (2048, 3)):
        src = int(np.flatnonzero(l == base[order[rank]])[0])
        l[src], l[tgt] = l[tgt], l[src]
    l[2048] = l[2047]
    w = np.sort(np.exp(l.astype(f64) - l.max()))[::-1]
    tp = float((w[:2].sum() + 0.5 * w[2]) / w.sum())
    out.append(_sweep(l, P(top_p=tp), (), g, "ties across top-p (general)"))
    out.append(_sweep(l, P(top_k=64, top_p=float((w[:2].sum() + 0.5 * w[2]) / w[:64].sum())), (), g,
                      "ties across top-p (fast)"))
    # all equal
    for V2 in (65, 1000):
        out.append(_sweep(np.full(V2, 1.25, f32), P(top_k=7), (), g, f"all equal V={V2}"))
        out.append(_sweep(np.full(V2, 1.25, f32), P(top_p=0.5), (), g, f"all equal top-p V={V2}"))
    # more than CCAP ties at the fast path's threshold: 30 distinct above, 600 tied at the 40-th place
    l = np.full(V, -60.0, f32)
    ids = _rng("ccap").permutation(V)
    l[ids[:30]] = (3.0 - 0.05 * np.arange(30)).astype(f32)
    l[ids[30:630]] = f32(1.0)
    out.append(_sweep(l, P(top_k=40), (), g, "ties overflow CCAP"))
    return out


MASK_M = (1, 3, 10, 40, 41)


@functools.lru_cache(maxsize=None)
def masked_rows(m, n=64, V=6000, nan=False):
    """n rows of N(0, 2.5) with -inf on all but m tokens (and NaN on a tenth of the masked ones)."""
    rng = _rng("masked", m, V, nan)
    L = (rng.standard_normal((n, V)) * 2.5).astype(f32)
    for r in range(n):
        keep = rng.permutation(V)[:m]
        row = np.full(V, NEG, f32)
        row[keep] = L[r, keep]
        if nan:
            row[rng.permutation(np.setdiff1d(np.arange(V), keep))[:V // 10]] = np.nan
        L[r] = row
    return L


def masked_case(m, g, top_k=40, nan=False):
    """Finding 1: every row drawn at the midpoint of its LOWEST finite token (the one a threshold above the minimum
    drops) when that interval is fair, else at the widest interval's."""
    L = masked_rows(m, nan=nan)
    p = P(top_k=top_k)
    us = []
    for r in range(L.shape[0]):
        ref = ref_row(L[r], p)
        e = ref.edges
        j = int(np.argmin(ref.w)) if len(ref.w) <= top_k else int(np.argmax(ref.w))
        if e[j + 1] - e[j] < 8 * g:
            j = int(np.argmax(ref.w))
        us.append(float(f32(0.5 * (e[j] + e[j + 1]))))
    n = L.shape[0]
    return Case(f"masked m={m} k={top_k} nan={nan}", L, [p] * n, [()] * n, us)


OFFSETS = (("N(50,1)", 50.0, 1.0), ("N(-1000,.01)", -1000.0, 0.01), ("+1e4", 1e4, 1.0), ("-1e4", -1e4, 1.0))


@functools.lru_cache(maxsize=None)
def offset_rows(name, n=64, V=32000):
    mu, sd = {o[0]: o[1:] for o in OFFSETS}[name]
    return (mu + sd * _rng("offset", name).standard_normal((n, V))).astype(f32)


def offset_case(name, g, top_k, T=None):
    """Finding 2: rows far from zero under top-k; each row drawn at the midpoint of its k-th largest token (the one a
    bin edge above it drops). Rows whose logit margin at the cut fails the rule are left out (counted by the test)."""
    L = offset_rows(name)
    sd = {o[0]: o[2] for o in OFFSETS}[name]
    p = P(top_k=top_k, temperature=sd * 3.0 if T is None else T)      # flat enough that the k-th interval is wide
    rows, us = [], []
    for r in range(L.shape[0]):
        ref = ref_row(L[r], p)
        j = int(np.argmin(ref.w))
        e = ref.edges
        if not fair(ref, g) or len(ref.kept) != top_k:
            continue
        rows.append(r)
        us.append(float(f32(0.5 * (e[j] + e[j + 1]))))
    n = len(rows)
    return Case(f"offset {name} k={top_k}", L[rows], [p] * n, [()] * n, us)


@functools.lru_cache(maxsize=None)
def penalty_cases(g):
    """Histories with repeats, ids -1 and >= V, logits of both signs and a zero under repeat_penalty, a full 64-entry
    window, penalties that move a token across the top-k cut in each direction, penalised arg-max with ties."""
    V = 1000
    rng = _rng("pen")
    l = np.full(V, -45.0, f32)
    hot = rng.permutation(V)[:24]
    l[hot] = np.linspace(2.0, -1.5, 24).astype(f32)      # both signs
    l[hot[10]] = 0.0                                      # a zero logit
    h_rep = [int(hot[0])] * 3 + [int(hot[5])] * 2 + [int(hot[10]), -1, V, V + 7, int(hot[20]), int(hot[10])]
    h_full = [int(hot[i % 24]) for i in range(50)] + [-1] * 4 + [V + 1] * 4 + [int(hot[3])] * 6
    out = []
    for hist, p in ((h_rep, P(repeat_penalty=1.3)), (h_rep, P(presence_penalty=0.4, frequency_penalty=0.3)),
                    (h_rep, P(top_k=12, repeat_penalty=1.5, frequency_penalty=0.2)),
                    (h_full, P(top_k=30, top_p=0.95, repeat_penalty=1.1, presence_penalty=0.1, frequency_penalty=0.05)),
                    # out of the top-8: hot[7] (rank 8) pushed below hot[8]; into it: everything above pushed down
                    ([int(hot[7])], P(top_k=8, presence_penalty=0.5)),
                    ([int(hot[i]) for i in range(8)], P(top_k=8, repeat_penalty=3.0, presence_penalty=2.5)),
                    ([int(hot[0]), int(hot[0]), int(hot[1])], P(temperature=0.0, repeat_penalty=2.0)),
                    ([int(hot[0])], P(temperature=0.0, frequency_penalty=0.1))):
        out.append(_sweep(l, p, hist, g, f"penalties {p} n_hist={len(hist)}"))
    # penalised arg-max with a tie: hot[0] pushed down exactly onto hot[1]'s value -> the lower id
    lt = l.copy()
    lt[hot[0]], lt[hot[1]] = 2.0, 1.5
    out.append(_sweep(lt, P(temperature=0.0, presence_penalty=0.5), [int(hot[0])], g, "penalised arg-max tie"))
    return out


def random_rows(seed=3, n=256, V=32000):
    """The inputs of test_kernels_gpu.test_sample_kernel_matches_cpu_twin, rebuilt with numpy."""
    rng = _rng("random", seed)
    L = (rng.standard_normal((n, V)) * 2.5).astype(f32)
    us = [float(f32(u)) for u in rng.random(n)]
    hist = [tuple(int(t) for t in rng.integers(0, V, 12)) for _ in range(n)]
    return L, us, hist
