"""Inputs and a numpy twin of the sampler's logit_bias stage (csrc/kernels/sample.hip sample_one_biased), shared by
tests/test_logit_bias.py (CPU) and tests/test_logit_bias_gpu.py.

The oracle of both needs no tolerance: a bias is a pre-transform of the logits row, so the biased call on the raw row
must return exactly the token of the unbiased call on a copy whose biased entries were pre-added in float32
(`prebiased`). The inputs keep every such sum out of the subnormal range (`launch` asserts it), where a kernel that
flushes subnormals and numpy could differ.

A launch is 5 rows of one vocabulary size, one kind each:
  plain    ids 0 and V - 1 among the biased ones, -100 on the raw arg-max
  history  the first biased ids sit in the row's history window as well (penalty(l + b))
  tie      a bias lifts a token exactly to the value of the row's maximum, which has the LOWER index
  neginf   a +100 bias on a -inf logit (stays -inf), further -inf entries without one
  nan      a bias on a NaN logit (stays NaN, never kept)
Row r of variant v has COUNTS[(r + v) % 6] entries (clipped to V: ids are distinct) and PARAMS[(r + v) % 5], so the 6
variants give every kind every count and every parameter set, and the rows of one launch all differ in their counts.
Entry order in a table is a random permutation: which entry decides a row's token is not tied to its position.

The twin (`twin`) is stage 0 from its definition -- table row r, entries j < n_bias, ids outside [0, V) skipped,
raw + value in float32, the sampler of tests/sampler_ref.py on the result, raw words back -- with switchable faults:
  after      the bias added behind the penalties
  wave       entries j >= 64 dropped
  stride     row r reads row r + 1's table
  off1       id + 1
  norestore  the raw words are not written back: seen by a SECOND call on the same buffer (judged on the rows
             without penalties: a penalised row's history logits are rewritten in place, as they always were)
  skip0      the in-graph kernel's early return skips a temperature-0 row that has only a bias
test_logit_bias.py::test_case_list_notices_each_fault shows that each changes a token of the case list.
"""
import collections
import functools

import numpy as np

import sampler_ref as S

f32 = np.float32
HIST = 64
STRIDE = 300                          # engine.sampling.LOGIT_BIAS_MAX: the width of the tables
VS = (19, 1025, 128256)
COUNTS = (0, 1, 63, 64, 65, 300)
KINDS = ("plain", "history", "tie", "neginf", "nan")
PARAMS = (S.P(temperature=0.0),
          S.P(temperature=0.9, top_k=40),
          S.P(temperature=0.9, top_k=300),
          S.P(temperature=0.9, top_k=48, top_p=0.999, min_p=1e-6),
          S.P(temperature=0.9, repeat_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.5))
SEEDS = (0, (1 << 64) - 1, 1, 0x9E3779B97F4A7C15, 12345678901234567)
POSS = (0, 5, HIST - 1, HIST, 3 * HIST + 7)
FAULTS = ("after", "wave", "stride", "off1", "norestore", "skip0")

Launch = collections.namedtuple("Launch", "name V logits params hists us ids vals nb ring pos seed")


def _row(kind, V, nb, rng):
    """(logits row, table ids, table values, history window) of one row."""
    l = (rng.standard_normal(V) * 1.5).astype(f32)
    top = int(np.argmax(l))
    ids = []
    if nb >= 1:
        ids.append(top)
    for t in (0, V - 1):
        if len(ids) < nb and t not in ids:
            ids.append(t)
    rest = [int(t) for t in rng.permutation(V) if t not in ids][:max(0, nb - len(ids))]
    ids = np.array(ids + rest, dtype=np.int32)
    vals = (rng.integers(-64, 65, len(ids)) / 8.0).astype(f32)          # multiples of 1/8 in [-8, 8]
    vals[vals == 0] = f32(0.125)
    if nb >= 1:
        vals[0] = f32(-100.0)                                           # the raw arg-max: banned
    if nb >= 8:
        vals[len(ids) // 2] = f32(100.0) if rng.integers(0, 3) == 0 else f32(7.875)
    hist = [int(t) for t in rng.choice(np.argsort(-l)[:12], 20)] + [-1, V + 3]
    if kind == "history" and nb >= 1:
        hist = [int(ids[-1])] * 2 + [int(t) for t in ids[:6]] + hist     # biased ids in the window, one repeated
    if kind == "tie" and nb >= 1:
        b = int(ids[-1])                                                 # the last entry lifts b to the maximum ...
        free = [t for t in range(b) if t not in set(ids.tolist())]
        if free:                                                         # ... which an untouched LOWER index holds
            l[free[0]], l[b], vals[-1] = f32(120.0), f32(118.0), f32(2.0)     # (every other sum is < 8 + 100 + 8)
    if kind == "neginf" and nb >= 1:
        l[ids[-1]] = S.NEG
        vals[-1] = f32(100.0)
        l[rng.integers(0, V, max(1, V // 50))] = S.NEG
        l[ids[-1]] = S.NEG
    if kind == "nan" and nb >= 1:
        l[ids[-1]] = np.nan
        vals[-1] = f32(100.0)
    perm = rng.permutation(len(ids))
    return l, ids[perm], vals[perm], hist[:HIST]


@functools.lru_cache(maxsize=None)
def launch(V, variant):
    """The 5 rows of (V, variant): what sample_kernel gets (hists, us) and what sample_decode_kernel gets (ring, pos,
    seed; its window is ring[:min(HIST, pos + 1)], its variate uniform01(seed, pos))."""
    rng = S._rng("logit_bias", V, variant)
    n = len(KINDS)
    L = np.zeros((n, V), f32)
    ids = np.full((n, STRIDE), -1, np.int32)
    vals = np.zeros((n, STRIDE), f32)
    nbs, ps, hists, rings = [], [], [], []
    for r, kind in enumerate(KINDS):
        nb = min(COUNTS[(r + variant) % len(COUNTS)], V)
        l, i, v, h = _row(kind, V, nb, rng)
        L[r], ids[r, :nb], vals[r, :nb] = l, i, v
        assert len(set(i.tolist())) == nb and i.min(initial=0) >= 0 and i.max(initial=0) < V
        with np.errstate(invalid="ignore"):
            s = np.abs(l[i] + v)
        assert not ((s > 0) & (s < 1.2e-38)).any()                      # no subnormal sum
        nbs.append(nb)
        ps.append(PARAMS[(r + variant) % len(PARAMS)])
        hists.append(tuple(h))
        ring = np.full(HIST, -1, np.int32)
        ring[:len(h)] = h
        rings.append(ring)
    assert len(set(nbs)) == n or V < 63
    us = [float(f32(u)) for u in rng.uniform(0.02, 0.98, n)]
    return Launch(f"V{V}-v{variant}", V, L, ps, hists, us, ids, vals, nbs, np.stack(rings),
                  [POSS[(r + variant) % 5] for r in range(n)], [SEEDS[(r + 2 * variant) % 5] for r in range(n)])


def launches(big=True):
    return [launch(V, v) for V in VS if big or V < 100000 for v in range(len(COUNTS))]


def prebiased(c):
    """The logits with every row's biases pre-added in float32 on the host."""
    out = c.logits.copy()
    for r, nb in enumerate(c.nb):
        i = c.ids[r, :nb]
        with np.errstate(invalid="ignore"):
            out[r, i] = (c.logits[r, i] + c.vals[r, :nb]).astype(f32)
    return out


def penalised_ids(c, r, window):
    """Where a call may leave other bits than it found: the distinct in-range history ids of a penalised row."""
    return {int(t) for t in window if 0 <= int(t) < c.V} if S.penal(c.params[r]) else set()


def decode_window(c, r):
    return [int(t) for t in c.ring[r, :min(HIST, c.pos[r] + 1)]]


def twin(c, decode=False, fault=None, calls=2, skipped=-7):
    """Tokens of `calls` successive launches on ONE copy of the buffer, and the buffer afterwards. decode: the
    in-graph kernel's inputs and its skip rule (`skipped` stands for a row it leaves alone)."""
    buf = c.logits.copy()
    n = len(c.nb)
    toks = []
    for _ in range(calls):
        out = []
        for r in range(n):
            p = c.params[r]
            window = decode_window(c, r) if decode else list(c.hists[r])
            u = S.uniform01(c.seed[r], c.pos[r]) if decode else c.us[r]
            nb = c.nb[r]
            if decode and p["temperature"] <= 0.0 and not S.penal(p) and (nb <= 0 or fault == "skip0"):
                out.append(skipped)
                continue
            tr = (r + 1) % n if fault == "stride" else r
            ent = [(int(c.ids[tr, j]) + (fault == "off1"), c.vals[tr, j]) for j in range(nb)
                   if not (fault == "wave" and j >= 64)]
            ent = [(t, v) for t, v in ent if 0 <= t < c.V]
            raw = {t: buf[r, t] for t, _ in ent}
            if fault == "after":
                x, _ = S.penalise(buf[r], p, window)
                for t, v in ent:
                    x[t] += v
                ref = S.ref_row(x.astype(f32), dict(p, repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0))
            else:
                with np.errstate(invalid="ignore"):
                    for t, v in ent:
                        buf[r, t] = f32(raw[t] + v)
                ref = S.ref_row(buf[r], p, window)
            tok = S.draw(ref, u)
            out.append(0 if tok is None else tok)
            if fault != "norestore":
                for t, _ in ent:
                    buf[r, t] = raw[t]
        toks.append(out)
    return toks, buf
