"""Attention kernels against an independent fp64 reference, with inputs and a metric that notice ONE key
dropped, leaked, doubled or misplaced at any context length.

Metric. Every (token, head) row is judged against its own size: max|out - ref| / rms(ref row); rows
without keys must be exactly zero. The tolerance comes from the reference side only: EMU_NOISE is the largest
row ratio of a CPU emulation of the kernels' arithmetic against fp64 (fp64 scores, p = exp(s - max) rounded
to bf16 for P.V, the unrounded sum as denominator, f16 output) over the inputs of this module
(test_emulated_noise_bounds_row_tol pins it), and ROW_TOL = 4 * EMU_NOISE covers the summation order, the
per-wave / per-split merges and exp2f. The census family has a derived tolerance instead (CENSUS_*).

Emulated noise 0.0085 (largest row: the random family, prefill, D = 64; ladders 0.003-0.004, spikes ~0), so
ROW_TOL = 0.034. Largest row ratio measured on the MI355X by the GPU tests below (non-census families; the
census families stayed within 0.29 / 0.44 of their own tolerance, decode / prefill, on every variant):

  kernel variant            no split    combine kernel   in-kernel merge
  decode MFMA, 8 waves      0.0058      0.0065           0.0065  (merge_splits)
  decode MFMA, 4 waves      0.0074      0.0074           0.0074  (merge_splits)
  decode MFMA, 1 wave       0.0084      0.0074           0.0074  (merge_splits)
  decode VALU, 4 waves      -           0.0016           0.0016  (fused ticket merge)
  decode VALU, 8 waves      -           0.0016           0.0016  (fused ticket merge)
  prefill (attn_prefill2)   0.0090
  prefill v1                0.0086

Every correct kernel stays within 0.27 ROW_TOL, at the emulated noise itself (the VALU kernel keeps P in fp32,
hence its lower figure).

Fault models (test_fault_models_are_rejected shows the metric rejects each by >= 10x its tolerance at every
grid point where the fault changes the mathematical result, using the reference alone):
  F1 last valid key dropped      F2 one key counted twice        F3 first masked key included
  F4 one key tile dropped (start / middle / end; 32 keys decode, 64 prefill, 96 prefill v1)
  F5 one page read through the neighbouring block-table entry
  F6 split merge: one active split ignored / all splits weighted equally
  F7 accumulator not rescaled when the running max grows in a later tile
Families: random (decode: with a poisoned tail), census (q = 0, one-hot V: the output counts every key
exactly once; two encodings), ladder (scores rising / falling by ~1 nat per key, or one +60 nat spike at the
last / first key; V random). census catches F1-F5 at single-key granularity at every length, the rising
ladder and the spikes F1, F3, F6 and F7, random F4, F5 and head mix-ups.

Not detectable in principle, hence outside the grid of the self-test: F2 on a one-key row (softmax of one key
is that key's V whatever its count), F1 / F2 / F4 / F5 on a row without keys, F6 with one active split, F7
with a single tile.

Fixed chunk: chunk > 0 covers n_split * chunk keys by the kernel's definition (the engine only passes
chunk <= 0), so for (n_split, chunk) = (3, 512) the 2049-key row is expected to attend to its first 1536 keys.
"""
import functools
import math
import os

import pytest
import torch

from nats_llm_studio_amd import ops

BS = 16
EMU_NOISE = 0.0085          # largest emulated row ratio (test_emulated_noise_bounds_row_tol)
ROW_TOL = 4 * EMU_NOISE
CENSUS_REL, CENSUS_ABS = 2.0 ** -10, 1e-5      # one f16 ulp of the exact count / ctx + the fp32 split merge

DECODE_CTX = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1039, 1040, 2049]
VALU8_ROWS = [0, 1, 4, 9, 13, 14, 16]          # ctx 0, 1, 33, 256, 1025, 1039, 2049: keeps the grid < 1024 workgroups
SPLITS = [(1, 0), (4, 0), (8, -16), (3, 512)]
# prefill chunks (seq, pos0, n) per query-block size: 64 (attn_prefill2: 32-token wave halves, 64-key tiles) and
# 32 (the first kernel: 16-token sub-tiles, 96-key tiles)
PREFILL_CHUNKS = {
    64: [(0, 0, 1), (1, 0, 33), (2, 0, 64), (3, 5, 63), (4, 31, 65), (5, 63, 2), (6, 100, 130), (7, 1000, 97)],
    32: [(0, 0, 1), (1, 0, 17), (2, 0, 32), (3, 5, 31), (4, 80, 33), (5, 95, 2), (6, 100, 130), (7, 1000, 97)],
}
PREFILL_TILE = {64: 64, 32: 96}
FAMILIES = ["random", "census_mod", "census_div", "ladder_up", "ladder_down", "spike_last", "spike_first"]
F8 = torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------ reference (fp64, CPU)

def _gather(cache, bt_row, nk):
    p = torch.arange(nk)
    slots = bt_row[p // BS].long() * BS + p % BS
    return cache[slots].float().double()          # the stored (rounded) values, converted exactly


def _causal_plan(pos0, n, extra=0):
    """Key plan of a chunk: counts[i, k] = how often row i (position pos0 + i) uses key k."""
    k = torch.arange(pos0 + n + extra)
    return (k[None, :] <= (pos0 + torch.arange(n))[:, None]).double()


def _scores(q, kc, bt, chunk, t, nk, Hq, Hkv, D, scale):
    seq, pos0, n = chunk
    K = _gather(kc, bt[seq], nk)
    Q = q[t:t + n].double().view(n, Hkv, Hq // Hkv, D)
    return torch.einsum("nhgd,khd->nhgk", Q, K) * scale       # [n, Hkv, G, nk]


def _ref_attention(q, kc, vc, bt, chunks, Hq, Hkv, D, scale, plan=None, emulate=False):
    """Paged GQA attention in fp64. chunks: (seq, pos0, n) -- n consecutive query rows at positions pos0 ..,
    causal (a decode row with ctx keys is (seq, ctx - 1, 1)). plan: per chunk None or counts[n, nk] (the keys
    0 .. nk - 1 of the sequence and how often each row uses them). emulate: the kernels' roundings (see top)."""
    T = sum(n for _, _, n in chunks)
    out = torch.zeros(T, Hq * D, dtype=torch.float64)
    t = 0
    for ci, (seq, pos0, n) in enumerate(chunks):
        w = plan[ci] if plan is not None and plan[ci] is not None else _causal_plan(pos0, n)
        nk = w.shape[1]
        if nk:
            S = _scores(q, kc, bt, (seq, pos0, n), t, nk, Hq, Hkv, D, scale)
            wb = w[:, None, None, :]
            S = S.masked_fill(wb == 0, -math.inf)
            m = S.amax(-1, keepdim=True)
            P = torch.exp(S - torch.where(torch.isinf(m), torch.zeros_like(m), m)) * wb
            den = P.sum(-1, keepdim=True)
            if emulate:
                P = P.to(torch.bfloat16).double()
            O = torch.einsum("nhgk,khd->nhgd", P, _gather(vc, bt[seq], nk))
            O = torch.where(den > 0, O / den.clamp_min(1e-300), torch.zeros_like(O))
            if emulate:
                O = O.to(torch.float16).double()
            out[t:t + n] = O.reshape(n, Hq * D)
        t += n
    return out


def _ref_tiled(q, kc, vc, bt, chunks, Hq, Hkv, D, scale, tiles_of, merge):
    """The same attention as a two-pass online softmax in fp64: per key range (a, b) of tiles_of(chunk) the
    partial (m, l, O), then a merge -- "exact", "skip_first" / "skip_last" (one active range ignored), "equal"
    (all ranges weighted 1 instead of e^(m_s - M)) or "norescale" (sequential, O not rescaled when the max
    grows)."""
    T = sum(n for _, _, n in chunks)
    out = torch.zeros(T, Hq * D, dtype=torch.float64)
    t = 0
    for seq, pos0, n in chunks:
        nk = pos0 + n
        if nk:
            S = _scores(q, kc, bt, (seq, pos0, n), t, nk, Hq, Hkv, D, scale)
            S = S.masked_fill(_causal_plan(pos0, n)[:, None, None, :] == 0, -math.inf)
            V = _gather(vc, bt[seq], nk)
            parts = []
            for a, b in tiles_of((seq, pos0, n)):
                m = S[..., a:b].amax(-1, keepdim=True)
                P = torch.exp(S[..., a:b] - torch.where(torch.isinf(m), torch.zeros_like(m), m))
                parts.append((m, P.sum(-1, keepdim=True), torch.einsum("nhgk,khd->nhgd", P, V[a:b])))
            ms = torch.stack([p[0] for p in parts])                 # [nt, n, Hkv, G, 1]
            ls = torch.stack([p[1] for p in parts])
            os_ = torch.stack([p[2] for p in parts])
            act = ~torch.isinf(ms)
            if merge == "norescale":
                m = torch.full_like(ms[0], -math.inf)
                l = torch.zeros_like(ls[0])
                o = torch.zeros_like(os_[0])
                for i in range(len(parts)):
                    mn = torch.maximum(m, ms[i])
                    safe = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
                    l = l * torch.exp(m - safe) + ls[i] * torch.exp(ms[i] - safe)
                    o = o + os_[i] * torch.exp(ms[i] - safe)
                    m = mn
                L, O = l, o
            else:
                keep = act.clone()
                if merge in ("skip_first", "skip_last"):
                    order = torch.cumsum(act.long(), 0)
                    tgt = 1 if merge == "skip_first" else order[-1:]
                    keep &= ~(order == tgt)
                M = ms.amax(0, keepdim=True)
                f = torch.ones_like(ms) if merge == "equal" else torch.exp(ms - torch.where(torch.isinf(M), torch.zeros_like(M), M))
                f = torch.where(keep, f, torch.zeros_like(f))
                L, O = (ls * f).sum(0), (os_ * f).sum(0)
            O = torch.where(L > 0, O / L.clamp_min(1e-300), torch.zeros_like(O))
            out[t:t + n] = O.reshape(n, Hq * D)
        t += n
    return out


def _row_ratio(out, ref, Hq, D):
    """max|out - ref| / rms(ref row) per (token, head); a row whose reference is all zero (no keys) must be
    exactly zero (ratio inf otherwise)."""
    o = out.double().reshape(-1, Hq, D)
    r = ref.double().reshape(-1, Hq, D)
    rms = r.pow(2).mean(-1).sqrt()
    err = (o - r).abs().amax(-1)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    empty = torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf))
    return torch.where(rms > 0, err / rms.clamp_min(1e-300), empty)


def _judge(fam, out, ref, Hq, D):
    """Per (token, head) row: error in units of the family's tolerance (passes iff <= 1)."""
    if fam.startswith("census"):
        o = out.double().reshape(-1, Hq, D)
        r = ref.double().reshape(-1, Hq, D)
        e = ((o - r).abs() / (CENSUS_REL * r.abs() + CENSUS_ABS)).amax(-1)
        return torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    return _row_ratio(out, ref, Hq, D) / ROW_TOL


# ------------------------------------------------------------------------------------------------- input families

def _ladder_dims(D):
    a = [1, D // 4 + 3, D // 2 + 5, D - 2]
    b = [2, D // 4 + 6, D // 2 + 9, D - 5]
    return (a, torch.tensor([.5, .5, -.5, .5])), (b, torch.tensor([.5, -.5, .5, .5]))      # two orthogonal unit vectors


@functools.lru_cache(maxsize=16)
def _case(kind, fam, D, G, Hkv, kvt, qt=64):
    """Inputs + fp64 reference of one family. kind "decode": one row per DECODE_CTX entry, each its own
    sequence; "prefill": PREFILL_CHUNKS[qt]. Every sequence owns end // BS + 2 scattered pages (so key `end`
    and the page after it exist) and every further block-table entry points to the sequence's tail page."""
    Hq = Hkv * G
    scale = D ** -0.5
    chunks = [(i, c - 1, 1) for i, c in enumerate(DECODE_CTX)] if kind == "decode" else PREFILL_CHUNKS[qt]
    g = torch.Generator().manual_seed(1000 * D + 10 * G + Hkv + (7 if kind == "decode" else 0))
    ends = [p0 + n for _, p0, n in chunks]
    npg = [e // BS + 2 for e in ends]
    W = max(npg) + 3
    perm = torch.randperm(sum(npg) + len(chunks), generator=g).to(torch.int32)
    bt = torch.zeros(len(chunks), W, dtype=torch.int32)
    at = 0
    for s, k in enumerate(npg):
        bt[s, :k] = perm[at:at + k]
        bt[s, k:] = perm[at + k]
        at += k + 1
    T = sum(n for _, _, n in chunks)
    slots = int(perm.numel()) * BS
    kc = torch.randn(slots, Hkv, D, generator=g)
    vc = torch.randn(slots, Hkv, D, generator=g)
    q = torch.randn(T, Hq * D, generator=g)
    if fam.startswith("census"):
        q.zero_()
    elif fam != "random":
        (da, ua), (db, ub) = _ladder_dims(D)
        q.zero_()
        qv = q.view(T, Hq, D)
        c = torch.tensor([[(1 + ((h + t) % 4) / 4) / scale for h in range(Hq)] for t in range(T)]).to(torch.bfloat16).float()
        qv[:, :, da] = 16 * c[:, :, None] * ua
        qv[:, :, db] = c[:, :, None] * ub
    q = q.to(torch.bfloat16)
    t = 0
    for s, (_, p0, n) in enumerate(chunks):
        end = ends[s]
        p = torch.arange(npg[s] * BS)
        sl = bt[s, p // BS].long() * BS + p % BS
        tail = bt[s, npg[s]].long() * BS + torch.arange(BS)
        if fam == "random" and kind == "decode":
            # poisoned tail: every slot past ctx and every further block-table entry -- any over-read dominates
            sign = torch.sign(q[t].float().view(Hkv, G, D)[:, 0, :])
            sign = torch.where(sign == 0, torch.ones_like(sign), sign)
            for dst in (sl[end:], tail):
                kc[dst] = 64 * sign
                vc[dst] = 448.0 if kvt == F8 else 1000.0
        elif fam.startswith("census"):
            key = p if fam == "census_mod" else p // D
            hot = (key[:, None] + torch.arange(Hkv)[None, :]) % D          # [P, Hkv]
            vc[sl] = torch.nn.functional.one_hot(hot, D).float()
        elif fam != "random":
            x = {"ladder_up": p - (end - 1), "ladder_down": -p,
                 "spike_last": 60 * (p == end - 1).long(), "spike_first": 60 * (p == 0).long()}[fam]
            hi = torch.div(x, 16, rounding_mode="floor")
            lo = x - 16 * hi
            row = torch.zeros(len(p), D)
            row[:, da] = hi[:, None].float() * ua
            row[:, db] = lo[:, None].float() * ub
            kc[sl] = row[:, None, :].expand(-1, Hkv, -1)
        t += n
    kc, vc = kc.to(kvt), vc.to(kvt)
    ref = _ref_attention(q, kc, vc, bt, chunks, Hq, Hkv, D, scale)
    return dict(q=q, kc=kc, vc=vc, bt=bt, chunks=chunks, ref=ref, T=T, Hq=Hq, Hkv=Hkv, D=D, scale=scale, fam=fam)


def _args(c):
    return c["q"], c["kc"], c["vc"], c["bt"], c["chunks"], c["Hq"], c["Hkv"], c["D"], c["scale"]


def _split_chunk(chunk, ctx, n_split, short_min):
    """attention.hip split_chunk: keys per flash-decoding split."""
    if chunk > 0:
        return chunk
    mn = -chunk if chunk else (256 if ctx >= 2048 else (128 if ctx >= 1024 else short_min))
    return max(mn, ((ctx + n_split - 1) // n_split + BS - 1) // BS * BS)


def _split_ranges(ctx, n_split, chunk, short_min):
    ch = _split_chunk(chunk, ctx, n_split, short_min)
    return [(s * ch, min(ctx, (s + 1) * ch)) for s in range(n_split) if s * ch < ctx]


# ------------------------------------------------------------------------------------------------------ CPU tests

def _f16_ulp(x):
    _, e = torch.frexp(x.abs().double())
    ulp = torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 11)
    return torch.where(x == 0, torch.zeros_like(ulp), ulp).clamp_min(2.0 ** -24)


@pytest.mark.parametrize("kvt", [torch.bfloat16, F8])
@pytest.mark.parametrize("G", [1, 4, 7])
def test_cpu_attention_matches_fp64_reference(G, kvt):
    """The CPU branch of ops.attention (the oracle of the older GPU tests) against the independent reference:
    within one f16 ulp of every reference element."""
    Hkv, D, nblk = 2, 64, 40
    Hq = Hkv * G
    ctx = [0, 1, 17, 300]
    T = len(ctx)
    g = torch.Generator().manual_seed(G)
    kc = torch.randn(nblk * BS, Hkv, D, generator=g).to(kvt)
    vc = torch.randn(nblk * BS, Hkv, D, generator=g).to(kvt)
    bt = torch.stack([torch.randperm(nblk, generator=g)[:20] for _ in range(T)]).to(torch.int32)
    q = torch.randn(T, Hq * D, generator=g).to(torch.bfloat16)
    out = torch.full((T, Hq * D), 7.0, dtype=ops.ACT_DTYPE)
    ops.attention(q, kc, vc, bt, torch.arange(T, dtype=torch.int32), torch.tensor(ctx, dtype=torch.int32), out, T,
                  Hq, Hkv, D, BS, D ** -0.5)
    ref = _ref_attention(q, kc, vc, bt, [(i, c - 1, 1) for i, c in enumerate(ctx)], Hq, Hkv, D, D ** -0.5)
    assert float(out[0].abs().max()) == 0.0
    assert bool(((out.double() - ref).abs() <= _f16_ulp(ref)).all())


def _cpu_cases():
    for D, G, kvt in ((128, 4, torch.bfloat16), (64, 4, F8)):
        yield "decode", D, G, kvt, 64
        yield "prefill", D, G, kvt, 64
        yield "prefill", D, G, kvt, 32


def test_emulated_noise_bounds_row_tol():
    """EMU_NOISE is the largest row ratio of the emulated kernel arithmetic over this module's inputs (within
    a factor 2 below it: the constant is the measurement, not a guess), and an emulated row with no keys is 0."""
    worst = 0.0
    for kind, D, G, kvt, qt in _cpu_cases():
        for fam in FAMILIES:
            c = _case(kind, fam, D, G, 1, kvt, qt)
            emu = _ref_attention(*_args(c), emulate=True)
            if fam.startswith("census"):
                assert float(_judge(fam, emu, c["ref"], c["Hq"], D).max()) <= 1.0
            else:
                worst = max(worst, float(_row_ratio(emu, c["ref"], c["Hq"], D).max()))
    print(f"emulated noise: largest row ratio {worst:.5f}")
    assert EMU_NOISE / 2 <= worst <= EMU_NOISE, worst


def _faults(c, kind, tile):
    """(name, applicable[chunk], faulty output) for F1-F7 on case c."""
    chunks = c["chunks"]
    args = _args(c)
    ends = [p0 + n for _, p0, n in chunks]

    def planned(fn, extra=0):
        plans = []
        for _, p0, n in chunks:
            w = _causal_plan(p0, n, extra)
            fn(w, p0, n)
            plans.append(w)
        return _ref_attention(*args, plan=plans)

    def f1(w, p0, n):
        for i in range(n):
            if p0 + i >= 0:
                w[i, p0 + i] = 0

    def f2(w, p0, n):
        for i in range(n):
            if p0 + i >= 0:
                w[i, (p0 + i) // 2] = 2

    def f3(w, p0, n):
        for i in range(n):
            w[i, p0 + i + 1] = 1

    yield "F1 last key dropped", [e >= 1 for e in ends], planned(f1)
    yield "F2 key counted twice", [e >= 2 for e in ends], planned(f2)
    yield "F3 first masked key included", [True] * len(chunks), planned(f3, extra=1)
    for where in ("start", "middle", "end"):
        def f4(w, p0, n, where=where):
            nt = (p0 + n + tile - 1) // tile
            a = {"start": 0, "middle": nt // 2, "end": nt - 1}[where] * tile
            w[:, a:a + tile] = 0
        yield f"F4 {tile}-key tile dropped at the {where}", [e >= 1 for e in ends], planned(f4)
    for where in ("first", "last"):
        bt = c["bt"].clone()
        for s, e in enumerate(ends):
            j = 0 if where == "first" else max(e - 1, 0) // BS
            bt[s, j] = c["bt"][s, j + 1]
        a = list(args)
        a[3] = bt
        yield f"F5 {where} page through the next block-table entry", [e >= 1 for e in ends], _ref_attention(*a)
    yield (f"F7 no rescale over {tile}-key tiles", [e > tile for e in ends],
           _ref_tiled(*args, lambda ch: [(a, min(a + tile, ch[1] + ch[2])) for a in range(0, ch[1] + ch[2], tile)],
                      "norescale"))
    if kind == "decode":
        for n_split, chunk in SPLITS[1:] + [(65, 0)]:
            for short_min in (64, 256):
                tiles = lambda ch: _split_ranges(min(ch[1] + 1, n_split * chunk) if chunk > 0 else ch[1] + 1,
                                                 n_split, chunk, short_min)
                # (a row longer than a fixed chunk covers is expected to be cut short: outside this grid)
                many = [len(tiles(ch)) >= 2 and not (chunk > 0 and ch[1] + 1 > n_split * chunk) for ch in chunks]
                for merge in ("skip_first", "skip_last", "equal"):
                    yield (f"F6 {merge} n_split={n_split} chunk={chunk} short_min={short_min}", many,
                           _ref_tiled(*args, tiles, merge))


def test_tiled_reference_is_the_reference():
    """The two-pass online-softmax form used for F6 / F7 reproduces the reference when nothing is broken."""
    for fam in ("random", "ladder_up", "spike_first"):
        c = _case("decode", fam, 128, 4, 1, torch.bfloat16)
        tiled = _ref_tiled(*_args(c), lambda ch: _split_ranges(ch[1] + 1, 8, -16, 64), "exact")
        assert float(_row_ratio(tiled, c["ref"], c["Hq"], 128).max()) < 1e-9


@pytest.mark.parametrize("kind,D,G,kvt,qt", list(_cpu_cases()),
                         ids=[f"{k}-D{D}-{'fp8' if t == F8 else 'bf16'}-qt{qt}" for k, D, _, t, qt in _cpu_cases()])
def test_fault_models_are_rejected(kind, D, G, kvt, qt):
    """Every fault model, applied to the reference, is rejected by >= 10x the tolerance by at least one family at
    every grid point (context length / prefill chunk) where it changes the mathematical result -- and the families
    named for it in the module docstring are among those that do."""
    tile = 32 if kind == "decode" else PREFILL_TILE[qt]
    cases = {fam: _case(kind, fam, D, G, 1, kvt, qt) for fam in FAMILIES}
    chunks = cases["random"]["chunks"]
    rows = torch.tensor([ci for ci, (_, _, n) in enumerate(chunks) for _ in range(n)])
    res = {}                       # fault -> (applies, {family: rejection per chunk, in units of the tolerance})
    for fam, c in cases.items():
        for name, applies, bad in _faults(c, kind, tile):
            r = _judge(fam, bad, c["ref"], c["Hq"], D).amax(-1)
            res.setdefault(name, (applies, {}))[1][fam] = torch.stack([r[rows == ci].max() for ci in range(len(chunks))])
    named = {"F1": ("census", "ladder_up", "spike_last"), "F2": ("census",), "F3": ("census", "ladder_up"),
             "F4": ("census", "random"), "F5": ("census", "random"), "F6": ("ladder", "spike", "census"),
             "F7": ("ladder_up", "spike_last")}
    for name, (applies, by_fam) in res.items():
        idx = [i for i, a in enumerate(applies) if a]
        assert idx, name
        resp = torch.stack([v for f, v in by_fam.items() if f.startswith(named[name[:2]])]).amax(0)
        catchers = sorted(f for f, v in by_fam.items() if all(float(v[i]) >= 10 for i in idx))
        worst = min(float(resp[i]) for i in idx)
        print(f"{kind} qt={qt} {name}: weakest grid point rejected by {worst:.0f}x tolerance; "
              f"families that reject it at every grid point: {catchers}")
        assert worst >= 10.0, (name, [(chunks[i], float(resp[i])) for i in idx if resp[i] < 10])


# ------------------------------------------------------------------------------------------------------ GPU tests

def _no_overrides():
    ov = sorted(k for k in os.environ if k.startswith("NLS_ATTN_"))
    if ov:
        pytest.skip(f"kernel selection overridden by {ov}: the dispatcher thresholds asserted here do not hold")


def _dispatch(T, Hkv, G, D, n_split):
    """attention.hip attn_decode_impl: which kernel a launch gets."""
    wg = T * Hkv * n_split
    if D in (64, 128) and G <= 16 and BS >= 16 and n_split <= 64:
        return "mfma1" if wg >= 1024 else ("mfma8" if wg <= 256 else "mfma4")
    return "valu8" if wg < 1024 else "valu4"


def _grid_shape(variant, n_split):
    """(repeats of the context rows, Hkv) that put T * Hkv * n_split into the variant's workgroup range."""
    lo, hi = {"mfma8": (1, 256), "mfma4": (257, 1023), "mfma1": (1024, 1 << 30)}[variant]
    for reps, Hkv in [(1, 2), (1, 1), (1, 8), (2, 8), (3, 8), (8, 8)]:
        if lo <= reps * len(DECODE_CTX) * Hkv * n_split <= hi:
            return reps, Hkv
    raise AssertionError((variant, n_split))


def _decode_params():
    out = []
    for D in (128, 64):
        for G in (1, 4, 7):
            for kvt in (torch.bfloat16, F8):
                if kvt == F8 and G == 7:
                    continue
                full = D == 128 and kvt == torch.bfloat16
                cfgs = SPLITS if full else (SPLITS[:3] if D == 128 else SPLITS[:2])
                kn = "bf16" if kvt == torch.bfloat16 else "fp8"
                for variant in ("mfma8", "mfma4", "mfma1"):
                    for n_split, chunk in cfgs:
                        for fused in ((False,) if n_split == 1 else (False, True)):
                            out.append(pytest.param(variant, D, G, kvt, n_split, chunk, fused,
                                                    id=f"{variant}-D{D}-G{G}-{kn}-s{n_split}c{chunk}-{'fused' if fused else 'combine'}"))
                for variant in ("valu4", "valu8"):
                    for fused in (False, True):
                        out.append(pytest.param(variant, D, G, kvt, 65, 0, fused,
                                                id=f"{variant}-D{D}-G{G}-{kn}-s65c0-{'fused' if fused else 'combine'}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant,D,G,kvt,n_split,chunk,fused", _decode_params())
def test_decode_families(gpu, variant, D, G, kvt, n_split, chunk, fused):
    """Every family through ops.attention on one kernel variant (the workgroup count picks it, asserted below),
    one split configuration and one merge path; fused launches run twice and must leave the counters zero."""
    _no_overrides()
    if variant.startswith("valu"):
        reps, Hkv = 1, 2
        sel = VALU8_ROWS if variant == "valu8" else list(range(len(DECODE_CTX)))
    else:
        reps, Hkv = _grid_shape(variant, n_split)
        sel = list(range(len(DECODE_CTX)))
    Hq = Hkv * G
    rows = torch.tensor(sel * reps)
    T = len(rows)
    assert _dispatch(T, Hkv, G, D, n_split) == variant, (T, Hkv, n_split)
    path = "direct" if n_split == 1 else ("combine" if not fused else
                                          ("fused" if variant.startswith("valu") else "merge_splits"))
    for fam in FAMILIES:
        c = _case("decode", fam, D, G, Hkv, kvt)
        ref = c["ref"].clone()
        for i, ctx in enumerate(DECODE_CTX):
            if chunk > 0 and ctx > n_split * chunk:     # a fixed chunk covers n_split * chunk keys (module docstring)
                one = _ref_attention(c["q"][i:i + 1], c["kc"], c["vc"], c["bt"], [(i, n_split * chunk - 1, 1)], Hq,
                                     Hkv, D, c["scale"])
                ref[i] = one[0]
        ref = ref[rows]
        q = c["q"][rows].contiguous().to(gpu)
        kc, vc, bt = c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu)
        ts = rows.to(torch.int32).to(gpu)
        cl = torch.tensor(DECODE_CTX, dtype=torch.int32)[rows].to(gpu)
        cnt = torch.zeros(T * Hkv, dtype=torch.int32, device=gpu) if fused else None
        for _ in range(2 if fused else 1):
            out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
            ops.attention(q, kc, vc, bt, ts, cl, out, T, Hq, Hkv, D, BS, c["scale"], chunk=chunk, n_split=n_split,
                          counters=cnt)
            r = _judge(fam, out.cpu(), ref, Hq, D)
            print(f"ATTN_RATIO decode {variant} {path} {fam} {float(r.max()) * (1 if fam.startswith('census') else ROW_TOL):.5f}")
            assert float(out.cpu()[cl.cpu() == 0].abs().max()) == 0.0, "rows without keys must be exactly zero"
            assert float(r.max()) <= 1.0, (fam, [(DECODE_CTX[int(rows[i])], float(v)) for i, v in enumerate(r.amax(-1)) if v > 1][:8])
        if fused:
            assert int(cnt.abs().sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kvt", [torch.bfloat16, F8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("Hkv", [1, 2])
@pytest.mark.parametrize("D,G", [(128, 4), (128, 8), (64, 4), (64, 8)])
@pytest.mark.parametrize("kernel", ["v2", "v1"])
def test_prefill_families(gpu, monkeypatch, kernel, D, G, Hkv, kvt):
    """Every family through ops.attention_prefill, on attn_prefill2 (64-token blocks) and on the first prefill
    kernel (ops.PREFILL_V1 / PREFILL_QT = 32, both read at call time)."""
    _no_overrides()
    import numpy as np
    qt = 64 if kernel == "v2" else 32
    monkeypatch.setattr(ops, "PREFILL_V1", kernel == "v1")
    monkeypatch.setattr(ops, "PREFILL_QT", qt)
    Hq = Hkv * G
    assert ops.attention_prefill_ok(Hq, Hkv, D)
    for fam in FAMILIES:
        c = _case("prefill", fam, D, G, Hkv, kvt, qt)
        T = c["T"]
        pos = np.concatenate([np.arange(p0, p0 + n) for _, p0, n in c["chunks"]]).astype(np.int32)
        tseq = np.concatenate([np.full(n, s) for s, _, n in c["chunks"]]).astype(np.int32)
        qb = ops.prefill_blocks(tseq, pos, T)
        assert int(qb[:, 1].max()) == qt and int(qb[:, 1].sum()) == T
        out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
        ops.attention_prefill(c["q"].to(gpu), c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu),
                              torch.from_numpy(qb).to(gpu), len(qb), None, None, out, T, Hq, Hkv, D, BS, c["scale"])
        r = _judge(fam, out.cpu(), c["ref"], Hq, D)
        print(f"ATTN_RATIO prefill {kernel} - {fam} {float(r.max()) * (1 if fam.startswith('census') else ROW_TOL):.5f}")
        assert float(r.max()) <= 1.0, (fam, [(int(pos[i]), float(v)) for i, v in enumerate(r.amax(-1)) if v > 1][:8])
