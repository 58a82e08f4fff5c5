"""Head size 256 (attn_d256.hip and the D = 256 Q/K-norm instantiations) against the fp64 references, inputs and
tolerances of test_attention_sensitivity, test_attn_window_gpu and test_qwen3_gpu.

Largest row ratio measured on the MI355X (non-census families; tolerance ROW_TOL = 0.034): decode 0.0098 (G = 16,
bf16, both workgroup forms; 0.0058 .. 0.0074 at G = 1 / 4 / 7), prefill 0.0088 (quad form, G = 16, fp8), window and
sinks 0.0087; the census families within 0.24 (decode), 0.45 (prefill) and 0.41 (window) of their own tolerance
(profiles/attn_d256.txt)."""
import numpy as np
import pytest
import torch

import test_attn_window_gpu as tw
import test_qwen3_gpu as tq
from nats_llm_studio_amd import ops
from test_attention_sensitivity import BS, DECODE_CTX, F8, FAMILIES, ROW_TOL, SPLITS, _case, _judge, _ref_attention

D, HKV = 256, 2
KVT = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(F8, id="fp8")]


def _reps(waves, rows, n_split):
    """Repeats of `rows` context rows that put T * Hkv * n_split on the side of 1024 workgroups at which
    attn_decode_impl takes the one-wave (>= 1024) or the four-wave form."""
    return 1 if waves == 4 else -(-1024 // (rows * HKV * n_split))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [4, 1])
@pytest.mark.parametrize("kvt", KVT)
@pytest.mark.parametrize("G", [1, 4, 7, 16])
def test_decode_families_d256(gpu, G, kvt, waves):
    """Every family through ops.attention on both workgroup forms, every split configuration of SPLITS, with the
    combine kernel and with the in-kernel merge (run twice: the counters must come back to zero)."""
    Hq, worst = HKV * G, [0.0, 0.0]
    for fam in FAMILIES:
        c = _case("decode", fam, D, G, HKV, kvt)
        kc, vc, bt = c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu)
        for n_split, chunk in SPLITS:
            rows = torch.arange(len(DECODE_CTX)).repeat(_reps(waves, len(DECODE_CTX), n_split))
            T = len(rows)
            assert (T * HKV * n_split >= 1024) == (waves == 1)
            ref = c["ref"].clone()
            for i, ctx in enumerate(DECODE_CTX):
                if chunk > 0 and ctx > n_split * chunk:     # a fixed chunk covers n_split * chunk keys
                    ref[i] = _ref_attention(c["q"][i:i + 1], c["kc"], c["vc"], c["bt"], [(i, n_split * chunk - 1, 1)],
                                            Hq, HKV, D, c["scale"])[0]
            q, ts = c["q"][rows].contiguous().to(gpu), rows.to(torch.int32).to(gpu)
            cl = torch.tensor(DECODE_CTX, dtype=torch.int32)[rows].to(gpu)
            for fused in ((False,) if n_split == 1 else (False, True)):
                cnt = torch.zeros(T * HKV, dtype=torch.int32, device=gpu) if fused else None
                for _ in range(2 if fused else 1):
                    out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
                    ops.attention(q, kc, vc, bt, ts, cl, out, T, Hq, HKV, D, BS, c["scale"], chunk=chunk,
                                  n_split=n_split, counters=cnt)
                    assert float(out[cl == 0].abs().max()) == 0.0, "rows without keys must be exactly zero"
                    r = _judge(fam, out.cpu(), ref[rows], Hq, D)
                    worst[fam.startswith("census")] = max(worst[fam.startswith("census")], float(r.max()))
                    assert float(r.max()) <= 1.0, (fam, n_split, chunk, fused, [
                        (DECODE_CTX[int(rows[i])], float(v)) for i, v in enumerate(r.amax(-1)) if v > 1][:8])
                assert cnt is None or int(cnt.abs().sum()) == 0
    print(f"ATTN_RATIO decode d256 w{waves} G{G} {worst[0] * ROW_TOL:.5f} census {worst[1]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kvt", KVT)
@pytest.mark.parametrize("G", [1, 3, 4, 7, 8, 16])
def test_prefill_families_d256(gpu, monkeypatch, G, kvt):
    """Every family through ops.attention_prefill: the quad form (G = 4, 8, 16) and the rows form (1, 3, 7)."""
    assert all(ops.attention_prefill_ok(2 * g, 2, D) for g in range(1, 17))
    monkeypatch.setattr(ops, "PREFILL_V1", True)
    assert not any(ops.attention_prefill_ok(2 * g, 2, D) for g in range(1, 17))
    monkeypatch.undo()
    Hq, qt, worst = HKV * G, 64, [0.0, 0.0]
    for fam in FAMILIES:
        c = _case("prefill", fam, D, G, HKV, kvt, qt)
        T = c["T"]
        pos = np.concatenate([np.arange(p0, p0 + n) for _, p0, n in c["chunks"]]).astype(np.int32)
        tseq = np.concatenate([np.full(n, s) for s, _, n in c["chunks"]]).astype(np.int32)
        qb = ops.prefill_blocks(tseq, pos, T)
        assert int(qb[:, 1].max()) == qt and int(qb[:, 1].sum()) == T
        out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
        ops.attention_prefill(c["q"].to(gpu), c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu),
                              torch.from_numpy(qb).to(gpu), len(qb), None, None, out, T, Hq, HKV, D, BS, c["scale"])
        r = _judge(fam, out.cpu(), c["ref"], Hq, D)
        worst[fam.startswith("census")] = max(worst[fam.startswith("census")], float(r.max()))
        assert float(r.max()) <= 1.0, (fam, [(int(pos[i]), float(v)) for i, v in enumerate(r.amax(-1)) if v > 1][:8])
    print(f"ATTN_RATIO prefill d256 G{G} {worst[0] * ROW_TOL:.5f} census {worst[1]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kvt", KVT)
@pytest.mark.parametrize("G", [1, 4, 7])
def test_window_sinks_d256(gpu, G, kvt):
    """The rows, windows (15 and 17 are no multiple of the 16-slot block) and sinks (+60 and -inf among them) of
    test_attn_window_gpu: decode on both forms with splits (combine kernel and in-kernel merge), then prefill."""
    Hq, worst = HKV * G, [0.0, 0.0]
    sinks = tw._sinks(Hq).to(gpu)
    for fam in tw.FAMS:
        c = _case("decode", fam, D, G, HKV, kvt)
        kc, vc, bt = c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu)
        for waves, n_split, chunk in [(4, 4, 0), (1, 8, -16)]:
            rows = torch.arange(len(tw.CTX)).repeat(_reps(waves, len(tw.CTX), n_split))
            T = len(rows)
            ts = torch.tensor(tw.SEQ, dtype=torch.int32)[rows].to(gpu)
            cl = torch.tensor(tw.CTX, dtype=torch.int32)[rows].to(gpu)
            for W, sink, fused in [(W, s, f) for W in (1, 15, 17, 64, 300) for s in (False, True) for f in (False, True)]:
                q, ref = tw._ref("decode", fam, D, G, HKV, kvt, W, sink)
                cnt = torch.zeros(T * HKV, dtype=torch.int32, device=gpu) if fused else None
                out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
                ops.attention(q[rows].contiguous().to(gpu), kc, vc, bt, ts, cl, out, T, Hq, HKV, D, BS, c["scale"],
                              chunk=chunk, n_split=n_split, counters=cnt, window=W, sinks=sinks if sink else None)
                assert float(out[cl == 0].abs().max()) == 0.0, "rows without keys must be exactly zero"
                tw._check(f"decode w{waves} s{n_split} W{W} sink{sink} fused{fused}", fam, out, ref[rows], Hq, D, worst)
                assert cnt is None or int(cnt.abs().sum()) == 0
    T = sum(n for _, _, n in tw.PRE_CHUNKS)
    pos = np.concatenate([np.arange(p0, p0 + n) for _, p0, n in tw.PRE_CHUNKS]).astype(np.int32)
    tseq = np.concatenate([np.full(n, s) for s, _, n in tw.PRE_CHUNKS]).astype(np.int32)
    qb = torch.from_numpy(ops.prefill_blocks(tseq, pos, T)).to(gpu)
    for fam in tw.FAMS:
        c = _case("prefill", fam, D, G, HKV, kvt)
        kc, vc, bt = c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu)
        for W, sink in [(W, s) for W in (1, 17, 33, 64, 100) for s in (False, True)]:
            q, ref = tw._ref("prefill", fam, D, G, HKV, kvt, W, sink)
            out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
            ops.attention_prefill(q.to(gpu), kc, vc, bt, qb, len(qb), None, None, out, T, Hq, HKV, D, BS, c["scale"],
                                  window=W, sinks=sinks if sink else None)
            tw._check(f"prefill W{W} sink{sink}", fam, out, ref, Hq, D, worst)
    print(f"ATTN_RATIO window d256 G{G} {worst[0] * ROW_TOL:.5f} census {worst[1]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kvt", [torch.bfloat16, F8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("neox", [False, True], ids=["adjacent", "neox"])
def test_qknorm_rope_kv_d256(gpu, neox, kvt):
    """ops.qk_norm_rope_kv at one wave per head: 7 heads leave the second workgroup's last wave without a head, ks = 5
    takes the run-time slab loop, two rows have slot -1. Bounds of test_qwen3_gpu: one bf16 / e4m3 ulp, V exact."""
    eps, Hq, Hkv = 1e-6, 5, 1
    g = torch.Generator().manual_seed(D + int(neox))
    qw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    kw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    cs = ops.rope_table(64, D, 1e6, "cpu")
    close = tq._bf16_close if kvt == torch.bfloat16 else tq._fp8_close
    for T, ks in ((1, 1), (17, 1), (17, 3), (5, 5)):
        ncol = (Hq + 2 * Hkv) * D
        ld, ldq, nslot = ncol + 8, Hq * D + 8, T + 5
        slabs = torch.randn(ks, T, ld, generator=g)
        pos = torch.arange(T, dtype=torch.int32) * 3
        pos[-1] = cs.shape[0] - 1
        slot = torch.randperm(nslot, generator=g)[:T].to(torch.int32)
        if T >= 3:
            slot[1] = slot[T - 1] = -1
        q = torch.full((T, ldq), tq.SENT, dtype=torch.bfloat16, device=gpu)
        kc = torch.full((nslot, Hkv, D), tq.SENT, device=gpu).to(kvt)
        vc = kc.clone()
        ops.qk_norm_rope_kv(slabs.to(gpu).view(ks * T, ld), pos.to(gpu), slot.to(gpu), cs.to(gpu), q, kc, vc, T, Hq, Hkv,
                            D, qw.to(gpu), kw.to(gpu), eps, neox, ks=ks, slab=T * ld)
        rq, rk, rv = tq._ref_qknorm_rope(slabs.numpy(), pos.numpy(), cs.numpy(), qw.numpy(), kw.numpy(), eps, Hq, Hkv, D,
                                         neox)
        q, kc, vc = q.cpu(), kc.cpu(), vc.cpu()
        tq._bf16_close(q[:, :Hq * D].float().numpy().reshape(T, Hq, D), rq, (T, ks))
        ok = slot.numpy() >= 0
        sl = slot.numpy()[ok]
        close(kc[sl].float().numpy(), rk[ok], (T, ks))
        if kvt == torch.bfloat16:
            assert torch.equal(vc[sl], torch.from_numpy(rv[ok]).to(torch.bfloat16)), (T, ks)
        else:
            close(vc[sl].float().numpy(), rv[ok], (T, ks))
        rest = [i for i in range(nslot) if i not in set(sl.tolist())]
        assert tq._is_sent(q[:, Hq * D:]) and tq._is_sent(kc[rest]) and tq._is_sent(vc[rest]), (T, ks)
