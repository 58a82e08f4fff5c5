"""Qwen3 on the MI355X: the per-head Q/K RMSNorm + RoPE + KV-append kernel (csrc/kernels/qknorm.hip) against an
inline float64 reference, ops.qkv_rope_kv(qk_norm=...) end to end, and the whole model against the fp32 oracle."""
import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType

pytestmark = pytest.mark.gpu

SENT = -7.0          # exact in bf16 and in fp8 e4m3


def _ref_qknorm_rope(slabs, pos, cs, qw, kw, eps, Hq, Hkv, D, neox):
    """float64: slab sum -> per-head RMSNorm (Q and K heads) -> rotation. slabs [ks, T, >= (Hq+2Hkv)*D] f32,
    cs [P, D/2, 2]. Returns q [T, Hq, D], k [T, Hkv, D] (float64) and v [T, Hkv, D]: the fp32 sum in slab order."""
    s = np.asarray(slabs, np.float32)
    T = s.shape[1]
    ncol = (Hq + 2 * Hkv) * D
    x = s[:, :, :ncol].astype(np.float64).sum(0)
    v32 = s[0, :, (Hq + Hkv) * D:ncol].copy()
    for k in range(1, s.shape[0]):
        v32 = (v32 + s[k, :, (Hq + Hkv) * D:ncol]).astype(np.float32)
    c = np.asarray(cs, np.float64)[np.asarray(pos, np.int64)]        # [T, D/2, 2]
    cc, sn = c[:, None, :, 0], c[:, None, :, 1]

    def head(h, w):
        h = h / np.sqrt((h * h).mean(-1, keepdims=True) + eps) * np.asarray(w, np.float64)
        if neox:
            x0, x1 = h[..., :D // 2], h[..., D // 2:]
            return np.concatenate([x0 * cc - x1 * sn, x0 * sn + x1 * cc], -1)
        x0, x1 = h[..., 0::2], h[..., 1::2]
        return np.stack([x0 * cc - x1 * sn, x0 * sn + x1 * cc], -1).reshape(h.shape)

    q = head(x[:, :Hq * D].reshape(T, Hq, D), qw)
    k = head(x[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D), kw)
    return q, k, v32.reshape(T, Hkv, D)


def _bf16_close(out, ref, what):
    """One bf16 ulp per element: the fp32 arithmetic error is orders below it and can only flip a rounding."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    bad = np.abs(out - ref) > 2.0 ** -7 * np.abs(ref) + 1e-5
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(out - ref).max()))


def _fp8_close(out, ref, what):
    """e4m3 (3 mantissa bits, 2^-9 the smallest subnormal step), the reference saturated at +-448."""
    out, ref = np.asarray(out, np.float64), np.clip(np.asarray(ref, np.float64), -448.0, 448.0)
    bad = np.abs(out - ref) > 2.0 ** -3 * np.abs(ref) + 2.0 ** -9
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(out - ref).max()))


def _is_sent(t):
    return bool((t.float() == SENT).all())


@pytest.mark.parametrize("kvt", [torch.bfloat16, torch.float8_e4m3fn])
@pytest.mark.parametrize("neox", [False, True])
@pytest.mark.parametrize("D", [128, 64])
def test_qknorm_rope_kv_kernel(gpu, D, neox, kvt):
    """Random f32 qkv rows straight into the kernel (no GEMM). 7 heads are no multiple of a workgroup's heads; ks = 5
    takes the run-time slab loop; rows and q rows are strided; two rows have slot -1; the last row sits on the
    table's last position. bf16 outputs within one ulp, fp8 within one e4m3 ulp, V exactly bf16(x); everything that
    is no target keeps its sentinel."""
    eps = 1e-6
    g = torch.Generator().manual_seed(D + int(neox))
    qw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    kw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    cs = ops.rope_table(256, D, 1e6, "cpu")
    csg, qwg, kwg = cs.to(gpu), qw.to(gpu), kw.to(gpu)
    close = _bf16_close if kvt == torch.bfloat16 else _fp8_close
    for T in (1, 3, 17, 70):
        for Hq, Hkv in ((4, 2), (5, 1)):
            for ks in (1, 2, 3, 5):
                what = (T, Hq, Hkv, ks)
                ncol = (Hq + 2 * Hkv) * D
                ld, ldq, nslot = ncol + 8, Hq * D + 8, T + 5
                slabs = torch.randn(ks, T, ld, generator=g)
                pos = torch.arange(T, dtype=torch.int32) * 3
                pos[-1] = cs.shape[0] - 1
                slot = torch.randperm(nslot, generator=g)[:T].to(torch.int32)
                if T >= 3:
                    slot[1] = -1
                    slot[T - 1] = -1
                q = torch.full((T, ldq), SENT, dtype=torch.bfloat16, device=gpu)
                kc = torch.full((nslot, Hkv, D), SENT, device=gpu).to(kvt)
                vc = kc.clone()
                ops.qk_norm_rope_kv(slabs.to(gpu).view(ks * T, ld), pos.to(gpu), slot.to(gpu), csg, q, kc, vc, T, Hq,
                                    Hkv, D, qwg, kwg, eps, neox, ks=ks, slab=T * ld)
                rq, rk, rv = _ref_qknorm_rope(slabs.numpy(), pos.numpy(), cs.numpy(), qw.numpy(), kw.numpy(), eps, Hq,
                                              Hkv, D, neox)
                q, kc, vc = q.cpu(), kc.cpu(), vc.cpu()
                _bf16_close(q[:, :Hq * D].float().numpy().reshape(T, Hq, D), rq, what)
                assert _is_sent(q[:, Hq * D:]), what
                ok = slot.numpy() >= 0
                sl = slot.numpy()[ok]
                close(kc[sl].float().numpy(), rk[ok], what)
                if kvt == torch.bfloat16:
                    assert torch.equal(vc[sl], torch.from_numpy(rv[ok]).to(torch.bfloat16)), what
                else:
                    close(vc[sl].float().numpy(), rv[ok], what)
                rest = [i for i in range(nslot) if i not in set(sl.tolist())]
                assert len(rest) == nslot - int(ok.sum())
                assert _is_sent(kc[rest]) and _is_sent(vc[rest]), what


def test_qknorm_rope_kv_rejects_other_head_sizes(gpu):
    """An unsupported head size is the usual error, not a launch."""
    T, Hq, Hkv, D = 2, 2, 1, 96
    qkv = torch.zeros(T, (Hq + 2 * Hkv) * D, device=gpu)
    z = torch.zeros(T, dtype=torch.int32, device=gpu)
    w = torch.ones(D, device=gpu)
    q = torch.full((T, Hq * D), SENT, dtype=torch.bfloat16, device=gpu)
    kc = torch.full((4, Hkv, D), SENT, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(RuntimeError):
        ops.qk_norm_rope_kv(qkv, z, z, ops.rope_table(8, D, 1e4, gpu), q, kc, kc.clone(), T, Hq, Hkv, D, w, w, 1e-6)
    torch.cuda.synchronize()
    assert _is_sent(q.cpu()) and _is_sent(kc.cpu())


def _qw(rows, K, t, dev, seed):
    rng = np.random.default_rng(seed)
    raw = Q.random_blocks(t, rows * K, 0.05, rng)
    return ops.QWeight(raw, t, rows, K, dev), ops.QWeight(raw, t, rows, K, "cpu").dense()


@pytest.mark.parametrize("cfg,M,dense", [((0, 4, 1, 1), 3, False), ((1, 8, 1, 2), 16, False), ((2, 8, 4, 2), 70, False),
                                         ((10, 8, 1, 1), 70, True), (None, 1, False)])
@pytest.mark.parametrize("neox", [False, True])
def test_qkv_rope_kv_with_qk_norm(gpu, cfg, M, dense, neox):
    """Q4_K / Q4_K / Q6_K projection + the norm kernel through ops.qkv_rope_kv: path A, split-K GEMV slabs, the LDS
    GEMM's slabs, a dense mode-10 launch and the tuned default. Reference: x @ W^T in fp32, then the float64
    reference; the GEMM's f16 inputs dominate the error (3e-2 of the largest value, as the fused-RoPE tests)."""
    Hq, Hkv, D, K, eps = 4, 2, 128, 512, 1e-6
    wq, Wq = _qw(Hq * D, K, GGMLType.Q4_K, gpu, 21)
    wk, Wk = _qw(Hkv * D, K, GGMLType.Q4_K, gpu, 22)
    wv, Wv = _qw(Hkv * D, K, GGMLType.Q6_K, gpu, 23)
    if dense:
        for w in (wq, wk, wv):
            w.expand_dense()
    segs = [ops.Seg(wq, 0), ops.Seg(wk, Hq * D), ops.Seg(wv, (Hq + Hkv) * D)]
    g = torch.Generator().manual_seed(1)
    pad = (M + 63) // 64 * 64
    x = torch.zeros(pad, K, dtype=ops.ACT_DTYPE)
    x[:M] = torch.randn(M, K, generator=g).to(ops.ACT_DTYPE)
    qw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    kw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    cs = ops.rope_table(4 * pad, D, 10000.0, "cpu")
    pos = torch.arange(pad, dtype=torch.int32) * 3
    slot = torch.arange(pad, dtype=torch.int32)
    qkv = torch.zeros(pad, (Hq + 2 * Hkv) * D, device=gpu)
    q = torch.zeros(pad, Hq * D, dtype=torch.bfloat16, device=gpu)
    kc = torch.zeros(pad, Hkv, D, dtype=torch.bfloat16, device=gpu)
    vc = torch.zeros_like(kc)
    ops.qkv_rope_kv(segs, x.to(gpu), qkv, pos.to(gpu), slot.to(gpu), cs.to(gpu), q, kc, vc, M, Hq, Hkv, D, neox,
                    cfg=cfg, qk_norm=(qw.to(gpu), kw.to(gpu), eps))
    ref = (x[:M].float() @ torch.cat([Wq, Wk, Wv]).t()).numpy()
    rq, rk, rv = _ref_qknorm_rope(ref[None], pos[:M].numpy(), cs.numpy(), qw.numpy(), kw.numpy(), eps, Hq, Hkv, D, neox)
    for out, r in ((q[:M].view(M, Hq, D), rq), (kc[:M], rk), (vc[:M], rv)):
        err = np.abs(out.float().cpu().numpy() - r).max()
        assert err <= 3e-2 * (np.abs(r).max() + 1e-6), err


def test_tiny_qwen3_prefill_and_graph_decode(gpu, tmp_path):
    """tiny-qwen3 prefill logits vs the fp32 oracle (prompt, buffers and bounds of
    test_model_gpu.test_prefill_logits_match_reference), then hipGraph decode == eager decode: the norm kernel is
    captured and replayed, at batch 1 (folded input RMSNorm) and on multi-row steps."""
    from nats_llm_studio_amd.engine.engine import Engine, GenRequest
    from nats_llm_studio_amd.engine.sampling import SamplingParams
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel
    from nats_llm_studio_amd.models.reference import ReferenceModel
    path = str(tmp_path / "tiny-qwen3.gguf")
    write_synthetic_gguf(path, "tiny-qwen3", "Q4_K_M", seed=0)
    r = GGUFReader(path)
    m = LlamaModel(r, gpu)
    ref = ReferenceModel(r)
    S = 40
    ids = list(np.random.default_rng(0).integers(0, 900, S))
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.ids[:S] = torch.tensor(ids, dtype=torch.int32)
    b.pos[:S] = torch.arange(S)
    b.slot[:S] = torch.arange(S)
    b.tok_seq[:S] = 0
    b.ctx_len[:S] = torch.arange(S) + 1
    b.block_tables[0] = torch.arange(8)
    m.forward(b, kc, vc, S, 16, n_split=2)
    rl = ref.logits(ids)
    err = (b.logits[:S].cpu() - rl).abs().max().item()
    assert err < 0.05 * rl.abs().max().item(), err
    agree = (b.next_ids[:S].cpu() == rl.argmax(1)).float().mean().item()
    assert agree > 0.9
    outs = []
    for graphs in (False, True):
        eng = Engine(m, None, max_batch=4, use_graphs=graphs)
        futs = [eng.submit(GenRequest([1, 2, 3, 4 + i], SamplingParams(max_tokens=8, ignore_eos=True)))
                for i in range(3)]
        while not all(f.done() for f in futs):
            eng.step()
        futs.append(eng.submit(GenRequest([9, 8, 7], SamplingParams(max_tokens=8, ignore_eos=True))))   # alone: batch 1
        while not futs[-1].done():
            eng.step()
        outs.append([f.result().token_ids for f in futs])
        assert all(len(t) == 8 for t in outs[-1])
    assert outs[0] == outs[1]
