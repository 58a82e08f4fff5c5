"""Sliding-window and sink attention (the decode and prefill kernels and the CPU twin of ops.attention) against the
fp64 reference, inputs and tolerance of test_attention_sensitivity: _ref_attention with the window cut out of
_causal_plan, times sigmoid(logsumexp(used scores) - sink) for the sink denominator.
Largest row ratio measured on the MI355X (tolerance ROW_TOL = 0.034; profiles/attn_window.txt): decode MFMA 0.0074
(8 waves) / 0.0083 (4 waves, 1 wave), decode VALU 0.0019, prefill 0.0088 (attn_prefill2) / 0.0090 (rows kernel); the
census family within 0.41 of its own tolerance on every variant."""
import functools
import math

import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from test_attention_sensitivity import BS, DECODE_CTX, F8, ROW_TOL, _case, _causal_plan, _f16_ulp, _judge, _ref_attention

FAMS = ["random", "census_mod", "spike_first"]       # spike_first: +60 nats on key 0, which every window excludes
CTX = [0, 1, 16, 17, 40, 255, 257, 1039, 2049]       # row i reads sequence SEQ[i] of the decode case (long enough)
SEQ = [next(i for i, c in enumerate(DECODE_CTX) if c >= x) for x in CTX]
DEC_W = [1, 15, 16, 17, 64, 300, 4096]
PRE_W = [1, 5, 16, 17, 64, 65, 100, 4096]
PRE_CHUNKS = [(0, 0, 1), (2, 0, 64), (6, 103, 64), (7, 37, 130), (7, 300, 7)]    # (seq of the prefill case, pos0, n)
KVT = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(F8, id="fp8")]


def _sinks(Hq):
    s = 2 * torch.randn(Hq, generator=torch.Generator().manual_seed(Hq))
    s[0], s[1] = 60.0, -math.inf
    return s


@functools.lru_cache(maxsize=64)
def _ref(kind, fam, D, G, Hkv, kvt, W, sink):
    """fp64 reference of the module's rows (decode: CTX, prefill: PRE_CHUNKS) with window W and, if sink, _sinks."""
    c = _case(kind, fam, D, G, Hkv, kvt)
    chunks = [(s, x - 1, 1) for s, x in zip(SEQ, CTX)] if kind == "decode" else PRE_CHUNKS
    Hq, T = c["Hq"], sum(n for _, _, n in chunks)
    q = c["q"][torch.tensor(SEQ)] if kind == "decode" else c["q"][:T]
    plans = [_causal_plan(p0, n) * (torch.arange(p0 + n)[None, :] > (p0 + torch.arange(n))[:, None] - W) for _, p0, n in chunks]
    ref = _ref_attention(q, c["kc"], c["vc"], c["bt"], chunks, Hq, Hkv, D, c["scale"], plan=plans).view(T, Hq, D)
    if sink:
        t = 0
        for (s, p0, n), w in zip(chunks, plans):
            p = torch.arange(max(p0 + n, 1))                 # (a row without keys: key 0 masked, the factor is 0)
            K = c["kc"][c["bt"][s, p // BS].long() * BS + p % BS].float().double()
            S = torch.einsum("nhgd,khd->nhgk", q[t:t + n].double().view(n, Hkv, G, D), K) * c["scale"]
            used = w[:, None, None, :] != 0 if p0 + n else torch.zeros(1, 1, 1, 1, dtype=torch.bool)
            lse = torch.logsumexp(S.masked_fill(~used, -math.inf), -1).reshape(n, Hq)
            ref[t:t + n] *= torch.sigmoid(lse - _sinks(Hq).double()).nan_to_num(0.0)[..., None]
            t += n
        # a row that the +60 sink pushes wholly below half of f16's smallest subnormal is a zero row in f16
        ref[ref.abs().amax(-1) < 2.0 ** -25] = 0
    return q, ref.reshape(T, Hq * D)


def _check(tag, fam, out, ref, Hq, D, worst):
    assert not bool(torch.isnan(out).any()), f"{tag}: NaN (a row met an all-masked tile or split with m = -inf)"
    r = float(_judge(fam, out.cpu(), ref, Hq, D).max())
    worst[fam.startswith("census")] = max(worst[fam.startswith("census")], r)
    assert r <= 1.0, (tag, fam, r)


# variant -> (rows of CTX, repeats, Hkv, n_split, chunk): T * Hkv * n_split workgroups pick the kernel as
# test_attention_sensitivity._dispatch says (mfma8 <= 256 < mfma4 < 1024 <= mfma1; n_split > 64: valu8 < 1024 <= valu4)
ALL, V8 = list(range(len(CTX))), [0, 1, 3, 4, 6, 7, 8]
VARIANTS = {"mfma8": [(ALL, 1, 2, 1, 0), (ALL, 1, 2, 4, 0), (ALL, 1, 2, 8, -16)],
            "mfma4": [(ALL, 4, 8, 1, 0), (ALL, 1, 8, 4, 0), (ALL, 1, 8, 8, -16)],
            "mfma1": [(ALL, 15, 8, 1, 0), (ALL, 4, 8, 4, 0), (ALL, 2, 8, 8, -16)],
            "valu8": [(V8, 1, 2, 65, 0)], "valu4": [(ALL, 1, 2, 65, 0)]}


@pytest.mark.gpu
@pytest.mark.parametrize("kvt", KVT)
@pytest.mark.parametrize("D,G", [(D, G) for D in (128, 64) for G in (1, 4, 7)])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_decode_window_sinks(gpu, variant, D, G, kvt):
    """One kernel variant unsplit, with the combine kernel and with the in-kernel merge (counters back at zero)."""
    worst = [0.0, 0.0]
    for sel, reps, Hkv, n_split, chunk in VARIANTS[variant]:
        Hq, rows = Hkv * G, torch.tensor(sel * reps)
        T = len(rows)
        sinks = _sinks(Hq).to(gpu)
        ts = torch.tensor(SEQ, dtype=torch.int32)[rows].to(gpu)
        cl = torch.tensor(CTX, dtype=torch.int32)[rows].to(gpu)
        for fam in FAMS:
            c = _case("decode", fam, D, G, Hkv, kvt)
            kc, vc, bt = c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu)
            for W, sink, fused in [(W, s, f) for W in DEC_W for s in (False, True) for f in ((False, True) if n_split > 1 else (False,))]:
                q, ref = _ref("decode", fam, D, G, Hkv, kvt, W, sink)
                cnt = torch.zeros(T * Hkv, dtype=torch.int32, device=gpu) if fused else None
                out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
                ops.attention(q[rows].contiguous().to(gpu), kc, vc, bt, ts, cl, out, T, Hq, Hkv, D, BS, c["scale"], chunk=chunk,
                              n_split=n_split, counters=cnt, window=W, sinks=sinks if sink else None)
                assert float(out[cl == 0].abs().max()) == 0.0, "rows without keys must be exactly zero"
                _check(f"{variant} s{n_split} W{W} sink{sink} fused{fused}", fam, out, ref[rows], Hq, D, worst)
                assert cnt is None or int(cnt.abs().sum()) == 0
    print(f"ATTN_RATIO window decode {variant} D{D} G{G} {worst[0] * ROW_TOL:.5f} census {worst[1]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kvt", KVT)
@pytest.mark.parametrize("D,G", [(128, 4), (64, 8), (128, 7), (128, 1)])
def test_prefill_window_sinks(gpu, D, G, kvt):
    """attn_prefill2 (G % 4 == 0) / the rows kernel: an unaligned first tile, all-masked first tiles, a ragged chunk."""
    Hkv, worst = 2, [0.0, 0.0]
    Hq, T = Hkv * G, sum(n for _, _, n in PRE_CHUNKS)
    pos = np.concatenate([np.arange(p0, p0 + n) for _, p0, n in PRE_CHUNKS]).astype(np.int32)
    tseq = np.concatenate([np.full(n, s) for s, _, n in PRE_CHUNKS]).astype(np.int32)
    qb = torch.from_numpy(ops.prefill_blocks(tseq, pos, T)).to(gpu)
    for fam in FAMS:
        c = _case("prefill", fam, D, G, Hkv, kvt)
        kc, vc, bt = c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu)
        for W, sink in [(W, s) for W in PRE_W for s in (False, True)]:
            q, ref = _ref("prefill", fam, D, G, Hkv, kvt, W, sink)
            out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
            ops.attention_prefill(q.to(gpu), kc, vc, bt, qb, len(qb), None, None, out, T, Hq, Hkv, D, BS, c["scale"],
                                  window=W, sinks=_sinks(Hq).to(gpu) if sink else None)
            _check(f"prefill W{W} sink{sink}", fam, out, ref, Hq, D, worst)
    print(f"ATTN_RATIO window prefill D{D} G{G} {worst[0] * ROW_TOL:.5f} census {worst[1]:.3f}")


def test_cpu_attention_window_sinks():
    """The CPU branch of ops.attention: within one f16 ulp of the reference; window 0, no sinks: bit for bit as before."""
    D, G, Hkv, kvt = 64, 4, 1, torch.bfloat16
    c = _case("decode", "random", D, G, Hkv, kvt)
    Hq, T = Hkv * G, len(CTX)
    a = (c["kc"], c["vc"], c["bt"], torch.tensor(SEQ, dtype=torch.int32), torch.tensor(CTX, dtype=torch.int32))

    def run(q, **kw):
        return ops.attention(q, *a, torch.full((T, Hq * D), 7.0, dtype=ops.ACT_DTYPE), T, Hq, Hkv, D, BS, c["scale"], **kw)

    for W, sink in [(1, False), (15, True), (17, False), (300, True), (4096, True)]:
        q, ref = _ref("decode", "random", D, G, Hkv, kvt, W, sink)
        out = run(q, window=W, sinks=_sinks(Hq) if sink else None)
        assert float(out[0].abs().max()) == 0.0 and bool(((out.double() - ref).abs() <= _f16_ulp(ref)).all()), (W, sink)
    assert torch.equal(run(q, window=0, sinks=None), run(q))
