"""IQ4_NL / IQ4_XS on the HIP kernels (MI355X only): kernel type-set 4 (device format IQ4 with the Q5_K / Q6_K / Q8_0
tensors of its mixes) against the fp32 product with the numpy decode of the ORIGINAL bytes."""
import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import SamplingParams
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
from nats_llm_studio_amd.models.llama import LlamaModel
from nats_llm_studio_amd.models.reference import ReferenceModel
from nats_llm_studio_amd.ops import transcode

pytestmark = pytest.mark.gpu

IQ4 = [GGMLType.IQ4_NL, GGMLType.IQ4_XS]
CFGS = [(0, 8, 1, 1), (0, 4, 2, 1), (1, 8, 1, 1), (1, 4, 2, 2), (1, 8, 1, 4)]


def _qw(rows, K, t, dev, seed=0):
    raw = Q.random_blocks(t, rows * K, 0.05, np.random.default_rng(seed))
    return ops.QWeight(raw, t, rows, K, dev), torch.from_numpy(Q.dequantize(raw, t, (rows, K)).copy())


def _x(M, K, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((M + 63) // 64 * 64, K, dtype=ops.ACT_DTYPE)
    x[:M] = torch.randn(M, K, generator=g).to(ops.ACT_DTYPE)
    return x.to(dev)


def _close(a, b, rtol=2e-2):
    err = (a.float().cpu() - b.float().cpu()).abs().max().item()
    scale = b.float().abs().max().item() + 1e-6
    assert err <= rtol * scale, f"max err {err} vs scale {scale}"


@pytest.fixture(scope="module")
def gemv_case(gpu):
    """rows = 200, K = 1024 of each type, the activations of 64 tokens and the fp32 products (shared, read-only)."""
    out = {}
    x = _x(64, 1024, gpu)
    for t in IQ4:
        w, Wd = _qw(200, 1024, t, gpu)
        out[t] = (w, x, x.float().cpu() @ Wd.t())
    return out


@pytest.mark.parametrize("t", IQ4)
@pytest.mark.parametrize("M", [1, 7, 16, 33, 64])
@pytest.mark.parametrize("cfg", CFGS)
def test_qgemv_iq4(gpu, gemv_case, t, M, cfg):
    w, x, ref = gemv_case[t]
    assert w.type == transcode.QT_IQ4
    y = torch.zeros(64, 200, device=gpu)
    mode, waves, rt, ks = cfg
    ops.qgemv([ops.Seg(w)], x, y, M, mode=mode, waves=waves, rt=rt, ks=ks)
    _close(y[:M], ref[:M])


@pytest.mark.parametrize("t", IQ4)
def test_dequant_kernel_iq4(gpu, t):
    """The register dequant (codebook lookup, then the int8 magic-number path) vs the numpy decode: the f16
    rounding of the scale (IQ4_XS) and of the value only."""
    w, Wd = _qw(48, 512, t, gpu, seed=3)
    d = w.dense().float().cpu()
    torch.testing.assert_close(d, Wd, rtol=2e-3, atol=2e-3 * Wd.abs().max().item())


@pytest.mark.parametrize("t", IQ4)
@pytest.mark.parametrize("M", [65, 300])
def test_iq4_large_m_and_dense(gpu, t, M):
    """Prefill sizes: path B (mode 1, split-K 2), the automatic config, mode 10 on the f16 copy, mode 9 on the
    raw tile-blocks; modes 2 and 3 refuse the type."""
    rows, K = 200, 1024
    w, Wd = _qw(rows, K, t, gpu)
    x = _x(M, K, gpu)
    ref = x[:M].float().cpu() @ Wd.t()
    y = torch.zeros(x.shape[0], rows, device=gpu)
    ops.qgemv([ops.Seg(w)], x, y, M, mode=1, waves=8, rt=1, ks=2)
    _close(y[:M], ref)
    y.zero_()
    assert ops.gemv_config([ops.Seg(w)], M)[0] in (0, 1)
    ops.qgemv([ops.Seg(w)], x, y, M)                      # automatic launch config
    _close(y[:M], ref)
    if M == 300:
        y.zero_()
        ops.qgemv([ops.Seg(w)], x, y, M, mode=9, waves=8, rt=2, ks=1)
        _close(y[:M], ref)
    for mode, waves, rt in ((2, 8, 4), (3, 4, 16)):
        with pytest.raises(RuntimeError, match="code -1"):        # refused by the dispatcher, nothing launched
            ops.qgemv([ops.Seg(w)], x, y, M, mode=mode, waves=waves, rt=rt, ks=1)
    w.expand_dense()
    y.zero_()
    ops.qgemv([ops.Seg(w)], x, y, M, mode=10, waves=8, rt=1, ks=1)
    _close(y[:M], ref)


def test_iq4_mixed_segments(gpu):
    """An IQ4 model's fused launch: IQ4 segments next to Q6_K, Q5_K and Q8_0 ones in ONE launch (type-set 4)."""
    K = 512
    a, Ad = _qw(64, K, GGMLType.IQ4_XS, gpu, 1)
    b, Bd = _qw(48, K, GGMLType.Q6_K, gpu, 2)
    c, Cd = _qw(32, K, GGMLType.Q5_K, gpu, 3)
    d, Dd = _qw(16, K, GGMLType.Q8_0, gpu, 4)
    e, Ed = _qw(32, K, GGMLType.IQ4_NL, gpu, 5)
    assert ops.kernel_set([a.type, b.type, c.type, d.type, e.type]) == 4
    W = torch.cat([Ad, Bd, Cd, Dd, Ed])
    segs = [ops.Seg(a, 0), ops.Seg(b, 64), ops.Seg(c, 112), ops.Seg(d, 144), ops.Seg(e, 160)]
    for M in (3, 40):
        x = _x(M, K, gpu)
        y = torch.zeros(64, 192, device=gpu)
        ops.qgemv(segs, x, y, M)
        _close(y[:M], x[:M].float().cpu() @ W.t())


@pytest.mark.parametrize("cfg", CFGS)
def test_iq4_swiglu(gpu, cfg):
    mode, waves, rt, ks = cfg
    K, F, t = 512, 256, GGMLType.IQ4_XS
    rng = np.random.default_rng(5)
    g_raw = Q.random_blocks(t, F * K, 0.05, rng)
    u_raw = Q.random_blocks(t, F * K, 0.05, rng)
    w = ops.QWeight(ops.interleave_gate_up(g_raw, u_raw, t, F, K), t, 2 * F, K, gpu)
    G = torch.from_numpy(Q.dequantize(g_raw, t, (F, K)).copy())
    U = torch.from_numpy(Q.dequantize(u_raw, t, (F, K)).copy())
    for M in (3, 40):
        x = _x(M, K, gpu)
        y = torch.zeros(64, F, dtype=ops.ACT_DTYPE, device=gpu)
        ops.qgemv([ops.Seg(w)], x, y, M, epi="swiglu", mode=mode, waves=waves, rt=rt, ks=ks)
        xf = x[:M].float().cpu()
        _close(y[:M], torch.nn.functional.silu(xf @ G.t()) * (xf @ U.t()), 3e-2)


@pytest.mark.parametrize("t", IQ4)
def test_iq4_embed(gpu, t):
    raw = Q.random_blocks(t, 50 * 512, 0.05, np.random.default_rng(11))
    qw = ops.QWeight(raw, t, 50, 512, gpu, layout="rows")
    Wd = torch.from_numpy(Q.dequantize(raw, t, (50, 512)).copy())
    ids = torch.tensor([0, 49, 7], dtype=torch.int32, device=gpu)
    e = torch.zeros(3, 512, device=gpu)
    ops.embed(ids, qw, e, 3, 2.0)
    ref = 2.0 * Wd[[0, 49, 7]]
    torch.testing.assert_close(e.cpu(), ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())


@pytest.mark.parametrize("T,mode,waves,rt", [(10, 0, 4, 2), (40, 1, 8, 1), (40, 1, 8, 2)])
def test_iq4_mapped_moe(gpu, T, mode, waves, rt):
    """Grouped MoE launches over IQ4_XS experts (mapped rows): path A at few tokens, the mapped path B that
    LlamaModel._moe_gemm_cfg picks for expert formats without a mode-2 case."""
    E, k, K, F, qt = 4, 2, 512, 256, GGMLType.IQ4_XS
    logits = torch.randn(T, E, device=gpu)
    cap = T
    topw = torch.zeros(T * k, device=gpu)
    counts = torch.zeros(E, dtype=torch.int32, device=gpu)
    xrows = torch.zeros(E * cap, dtype=torch.int32, device=gpu)
    yrows = torch.zeros(E * cap, dtype=torch.int32, device=gpu)
    ops.moe_route(logits, T, k, topw, counts, xrows, yrows, cap)
    rng = np.random.default_rng(9)
    gus, G, U = [], [], []
    for e in range(E):
        g_raw = Q.random_blocks(qt, F * K, 0.05, rng)
        u_raw = Q.random_blocks(qt, F * K, 0.05, rng)
        gus.append(ops.QWeight(ops.interleave_gate_up(g_raw, u_raw, qt, F, K), qt, 2 * F, K, gpu))
        G.append(torch.from_numpy(Q.dequantize(g_raw, qt, (F, K)).copy()))
        U.append(torch.from_numpy(Q.dequantize(u_raw, qt, (F, K)).copy()))
    dns = [_qw(K, F, qt, gpu, 40 + e) for e in range(E)]
    x = _x(T, K, gpu)
    act = torch.zeros(T * k, F, dtype=ops.ACT_DTYPE, device=gpu)
    yexp = torch.full((T * k, K), 5.0, device=gpu)
    cfg = dict(mode=mode, waves=waves, rt=rt, ks=1)
    segs = [ops.Seg(gus[e], 0, xrows[e * cap:], yrows[e * cap:], counts[e:e + 1]) for e in range(E)]
    ops.qgemv(segs, x, act, T, epi="swiglu", **cfg)
    segs = [ops.Seg(dns[e][0], 0, yrows[e * cap:], yrows[e * cap:], counts[e:e + 1]) for e in range(E)]
    ops.qgemv(segs, act, yexp, T, epi="f32", **cfg)
    torch.cuda.synchronize()
    cnt, xr, yr = counts.cpu(), xrows.cpu(), yrows.cpu()
    assert int(cnt.sum()) == T * k
    xf = x.float().cpu()
    for e in range(E):
        n = int(cnt[e])
        xi, yi = xr[e * cap:e * cap + n].long(), yr[e * cap:e * cap + n].long()
        ref = torch.nn.functional.silu(xf[xi] @ G[e].t()) * (xf[xi] @ U[e].t())
        _close(act[yi], ref, 3e-2)
        _close(yexp[yi], act[yi].float().cpu() @ dns[e][1].t(), 3e-2)


@pytest.fixture(scope="module")
def iq4_models(tmp_path_factory):
    d = tmp_path_factory.mktemp("iq4gpu")
    out = {}
    for name, ft in (("tiny-llama", "IQ4_NL"), ("tiny-llama", "IQ4_XS"), ("tiny-mixtral", "IQ4_XS")):
        out[name, ft] = str(d / f"{name}-{ft}.gguf")
        write_synthetic_gguf(out[name, ft], name, ft, seed=0)
    return out


@pytest.mark.parametrize("name,ft", [("tiny-llama", "IQ4_NL"), ("tiny-llama", "IQ4_XS"), ("tiny-mixtral", "IQ4_XS")])
def test_iq4_models_match_reference(gpu, iq4_models, name, ft):
    """Whole models in the IQ4 mixes on the GPU kernels: prefill logits vs the fp32 oracle of the original GGUF
    bytes (40 tokens: the Mixtral experts run the grouped GEMM), then hipGraph decode == eager decode, with three
    requests at once and with a single one (batch 1: the fused-norm GEMV and the fused RoPE / KV-append epilogue)."""
    r = GGUFReader(iq4_models[name, ft])
    m = LlamaModel(r, gpu)
    # Q|K|V of IQ4 q / k with a Q5_K v stays one quantised launch
    assert [s.w.type for s in m.layers[1].qkv] == [transcode.QT_IQ4, transcode.QT_IQ4, int(GGMLType.Q5_K)]
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
    for nreq in (3, 1):
        outs = []
        for graphs in (False, True):
            eng = Engine(m, None, max_batch=4, use_graphs=graphs)
            futs = [eng.submit(GenRequest([1, 2, 3, 4 + i], SamplingParams(max_tokens=8, ignore_eos=True)))
                    for i in range(nreq)]
            while not all(f.done() for f in futs):
                eng.step()
            outs.append([f.result().token_ids for f in futs])
        assert outs[0] == outs[1], nreq
