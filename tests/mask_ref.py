"""Inputs and a numpy twin of the sampler's allowed-token mask stage (csrc/kernels/sample.hip sample_one_biased, stage
-1), shared by tests/test_response_format.py (CPU) and tests/test_response_format_gpu.py.

The oracle needs no tolerance: a mask is a pre-transform of the logits row, so the masked call on the raw row must
return exactly the token of the unmasked call on a copy whose disallowed entries were set to -inf on the host
(`premasked`), and must leave exactly the buffer that call leaves.

A launch is 5 rows of one vocabulary size:
  0  min      one allowed token, and it is the row's minimum logit
  1  none     mask_rows = -1, between masked rows (its table row would be another row's mask)
  2  notop    an allowed set of A tokens without the arg-max; top-k below A (variant bit 2 clear) or above it (set)
  3  ones     an all-ones mask
  4  mixed    +100 bias on a disallowed token, a bias on an allowed one, a penalty history that overlaps both
Variant bits: 1 = temperature 0.8 instead of 0, 2 = the bits at t >= V of the last word all set instead of all
clear, 4 = top-k above the allowed count. The table rows are permuted against the logits rows (mask_rows), and the
table is `stride` >= ceil(V/32) words wide, the words past the needed ones all ones.

The twin (`twin`) is the stage from its definition with switchable faults:
  invert      bit sense inverted
  word        word index off by one across the 31 / 32 boundary ((t + 1) >> 5)
  pastv       bits at t >= V honoured: -inf written past the row's V entries
  rowid       row r reads table row r instead of mask_rows[r]
  neg1        a -1 row masked anyway (with table row 0)
  aftertopk   mask applied behind top-k (top-k counts disallowed tokens)
  afterargmax mask applied behind the arg-max at temperature 0
test_response_format.py::test_case_list_notices_each_fault shows that each changes a token or a buffer word.
"""
import collections
import functools

import numpy as np

import sampler_ref as S

f32 = np.float32
HIST = 64
VS = (19, 32, 33, 1025, 128256)
VARIANTS = tuple(range(8))
ROWS = ("min", "none", "notop", "ones", "mixed")
MASK_ROWS = (2, -1, 0, 3, 1)            # logits row -> table row
FAULTS = ("invert", "word", "pastv", "rowid", "neg1", "aftertopk", "afterargmax")
PEN = dict(repeat_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.5)

Launch = collections.namedtuple("Launch", "name V logits params hists us mask mask_rows stride bias allowed")


def words(allowed, V, stride, tail):
    """A bool [V] allowed set as `stride` mask words; the bits at t >= V of the last needed word are `tail`, the words
    behind it all ones."""
    nw = (V + 31) // 32
    bits = np.full(stride * 32, 1, np.uint8)
    bits[:V] = allowed
    bits[V:nw * 32] = tail
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


@functools.lru_cache(maxsize=None)
def launch(V, variant, extra_stride=0):
    rng = S._rng("mask", V, variant)
    T = 0.8 if variant & 1 else 0.0
    tail = (variant >> 1) & 1
    n = len(ROWS)
    nw = (V + 31) // 32
    stride = nw + extra_stride
    L = (rng.standard_normal((n, V)) * 1.5).astype(f32)
    allowed = np.ones((n, V), bool)
    # 0: the minimum alone
    allowed[0] = False
    allowed[0, int(np.argmin(L[0]))] = True
    # 1: no mask; the table row a kernel that ignores the -1 would take (row 0's, whatever the fault) bans its arg-max
    # 2: A tokens, the arg-max not among them, tokens on both sides of a word boundary where V allows
    A = min(12, V // 2)
    order = [int(t) for t in np.argsort(-L[2])]
    pick = [t for t in (31, 32, 0, V - 1) if t < V and t != order[0]]
    pick += [t for t in order[1:] if t not in pick]
    allowed[2] = False
    allowed[2, pick[:A]] = True
    # 4: about half of the tokens, the arg-max banned
    allowed[4] = rng.integers(0, 2, V).astype(bool)
    top4 = int(np.argmax(L[4]))
    allowed[4, top4] = False
    on = [int(t) for t in np.flatnonzero(allowed[4])]
    off = [int(t) for t in np.flatnonzero(~allowed[4])]
    b_off, b_on = top4, on[len(on) // 2]
    bias = {4: ((b_off, f32(100.0)), (b_on, f32(2.0)))}
    hist4 = [b_off, b_on, b_on] + on[:5] + off[:5] + [-1, V + 3]
    k2 = A + 8 if variant & 4 else max(1, A - 4)
    ps = [S.P(temperature=T, top_k=40), S.P(temperature=T, top_k=40), S.P(temperature=T, top_k=k2),
          S.P(temperature=T, top_k=40), S.P(temperature=T, top_k=40, **PEN)]
    hists = [(), (), (), (), tuple(hist4)]
    table = np.zeros((max(MASK_ROWS) + 1, stride), np.uint32)
    for r, tr in enumerate(MASK_ROWS):
        if tr >= 0:
            table[tr] = words(allowed[r], V, stride, tail)
    us = [float(f32(u)) for u in rng.uniform(0.02, 0.98, n)]
    return Launch(f"V{V}-v{variant}", V, L, ps, hists, us, table, np.array(MASK_ROWS, np.int32), stride, bias, allowed)


def launches(big=True):
    return [launch(V, v) for V in VS if big or V < 100000 for v in VARIANTS]


def effective(c):
    """bool [n, V]: what each row may draw (the -1 row: everything)."""
    a = c.allowed.copy()
    a[np.asarray(c.mask_rows) < 0] = True
    return a


def premasked(c):
    out = c.logits.copy()
    out[~effective(c)] = S.NEG
    return out


def bit(table, tr, t, fault=None):
    w = (t + 1) >> 5 if fault == "word" else t >> 5
    if w >= table.shape[1]:
        return 1
    b = (int(table[tr, w]) >> (t & 31)) & 1
    return 1 - b if fault == "invert" else b


def twin(c, fault=None, ld=None, bias=True):
    """(tokens, buffer [n, ld] afterwards) of one launch on a copy of the rows laid out with row pitch ld >= V (the
    padding holds 1e30)."""
    n, V = c.logits.shape
    ld = V if ld is None else ld
    flat = np.full(n * ld + 64, f32(1e30), f32)
    buf = flat[:n * ld].reshape(n, ld)
    buf[:, :V] = c.logits
    toks = []
    for r in range(n):
        p = c.params[r]
        tr = int(c.mask_rows[r])
        if fault == "rowid":
            tr = r % c.mask.shape[0]
        if tr < 0 and fault == "neg1":
            tr = 0
        banned = []
        if tr >= 0:
            top = ((V + 31) // 32) * 32 if fault == "pastv" else V
            banned = [t for t in range(top) if not bit(c.mask, tr, t, fault)] if V < 4096 or fault else \
                list(np.flatnonzero(~_bits(c.mask[tr], V)))
        late = fault == "aftertopk" or (fault == "afterargmax" and p["temperature"] <= 0.0)
        if not late:
            for t in banned:
                flat[r * ld + t] = S.NEG
        ent = [(t, v) for t, v in (c.bias.get(r, ()) if bias else ()) if 0 <= t < V]
        raw = {t: buf[r, t] for t, _ in ent}
        for t, v in ent:
            buf[r, t] = f32(raw[t] + v)
        ref = S.ref_row(buf[r, :V], p, list(c.hists[r]))
        if late:
            ban = np.zeros(V, bool)
            ban[[t for t in banned if t < V]] = True
            if ref.greedy:
                tok = ref.tok if not ban[ref.tok] else int(np.flatnonzero(~ban)[0]) if (~ban).any() else 0
            else:
                keep = ~ban[ref.kept]
                kept, wk = ref.kept[keep], ref.w[keep]
                if kept.size:
                    edges = np.concatenate([[0.0], np.cumsum(wk)]) / wk.sum()
                    tok = int(kept[min(int(np.searchsorted(edges[1:], c.us[r], side="right")), kept.size - 1)])
                else:
                    tok = 0
        else:
            tok = S.draw(ref, c.us[r])
        toks.append(0 if tok is None else tok)
        for t, _ in ent:
            buf[r, t] = raw[t]
    return toks, flat.copy()


def _bits(w, V):
    return np.unpackbits(np.ascontiguousarray(w).astype("<u4").view(np.uint8), bitorder="little")[:V].astype(bool)
