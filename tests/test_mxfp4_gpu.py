"""MXFP4 on the HIP kernels (MI355X only): kernel type-set 5 (device format MXFP4) against the fp64 product of the
f16 activations with the numpy decode of the ORIGINAL bytes. Weights and activations are exact f16 and their
products exact in fp32, so a kernel differs from the reference by its fp32 summation order alone."""
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

from test_iq4_gpu import _close, _x

pytestmark = pytest.mark.gpu

MX = GGMLType.MXFP4
CFGS = [(0, 8, 1, 1), (0, 4, 2, 1), (1, 8, 1, 1), (1, 4, 2, 2), (1, 8, 1, 4)]


def _qw(rows, K, dev, seed=0):
    raw = Q.random_blocks(MX, rows * K, 0.05, np.random.default_rng(seed))
    return ops.QWeight(raw, MX, rows, K, dev), torch.from_numpy(Q.dequantize(raw, MX, (rows, K)).copy()), raw


def _sum_order_close(y, x, Wd):
    """|y - x W^T| <= K * 2^-23 * sum_k |x_k w_k| per element: K fp32 additions in any order, u = 2^-23 so that a
    truncating MFMA accumulate is covered."""
    xd, wd = x.double().cpu(), Wd.double()
    err = (y.double().cpu() - xd @ wd.t()).abs()
    bound = x.shape[1] * 2.0 ** -23 * (xd.abs() @ wd.abs().t())
    print(f"largest |err| / bound: {(err / bound).max().item():.4f}")
    assert (err <= bound).all(), (err / bound).max().item()


@pytest.fixture(scope="module")
def gemv_case(gpu):
    """rows = 200, K = 1024, the activations of 300 tokens and the decoded weights (shared, read-only)."""
    w, Wd, raw = _qw(200, 1024, gpu)
    return w, _x(300, 1024, gpu), Wd, raw


def test_dequant_is_exact(gpu):
    """QWeight.dense() == the numpy decode bit for bit: block exponents e - 127 uniform in [-13, 13] (every non-zero
    value a normal f16), uniform nibbles; 40 rows leave a padded tile. Settles the nibble order, the byte selection
    and the scale construction of the fragment."""
    rows, K = 40, 512
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, size=(rows * K // 32, 17), dtype=np.uint8)
    raw[:, 0] = 127 + rng.integers(-13, 14, size=raw.shape[0])
    w = ops.QWeight(raw.reshape(-1), MX, rows, K, gpu)
    assert w.type == transcode.QT_MXFP4
    ref = torch.from_numpy(Q.dequantize(raw.reshape(-1), MX, (rows, K)).astype(np.float16))
    assert torch.equal(w.dense(torch.float16).cpu(), ref)


@pytest.mark.parametrize("M", [1, 7, 16, 33, 64])
@pytest.mark.parametrize("cfg", CFGS)
def test_qgemv_mxfp4(gpu, gemv_case, M, cfg):
    w, x, Wd, _ = gemv_case
    y = torch.zeros(64, 200, device=gpu)
    mode, waves, rt, ks = cfg
    ops.qgemv([ops.Seg(w)], x, y, M, mode=mode, waves=waves, rt=rt, ks=ks)
    _sum_order_close(y[:M], x[:M], Wd)


@pytest.mark.parametrize("M", [65, 300])
def test_mxfp4_large_m_and_dense(gpu, gemv_case, M):
    """Prefill sizes: path B with split-K 2, the automatic config, the LDS-dequant GEMM (mode 2) at 128- and 256-row
    blocks, mode 9 on the raw tile-blocks, mode 10 on the f16 copy; mode 3 refuses the type."""
    w, x, Wd, raw = gemv_case
    y = torch.zeros(x.shape[0], 200, device=gpu)
    cfgs = [dict(mode=1, waves=8, rt=1, ks=2), {}, dict(mode=2, waves=8, rt=2, ks=1), dict(mode=2, waves=8, rt=4, ks=1)]
    if M == 300:
        cfgs.append(dict(mode=9, waves=8, rt=2, ks=1))
    for cfg in cfgs:
        y.zero_()
        ops.qgemv([ops.Seg(w)], x, y, M, **cfg)
        _sum_order_close(y[:M], x[:M], Wd)
    with pytest.raises(RuntimeError, match="code -1"):        # refused by the dispatcher, nothing launched
        ops.qgemv([ops.Seg(w)], x, y, M, mode=3, waves=4, rt=16, ks=1)
    wd = ops.QWeight(raw, MX, 200, 1024, gpu)                  # (its own copy: the shared weight keeps no f16 copy)
    wd.expand_dense()
    y.zero_()
    ops.qgemv([ops.Seg(wd)], x, y, M, mode=10, waves=8, rt=1, ks=1)
    _sum_order_close(y[:M], x[:M], Wd)


@pytest.mark.parametrize("T,mode,waves,rt", [(10, 0, 4, 2), (40, 1, 8, 1), (40, 2, 8, 2)])
def test_mxfp4_mapped_moe(gpu, T, mode, waves, rt):
    """Grouped MoE launches over MXFP4 experts (mapped rows): path A at few tokens, path B and the LDS-dequant GEMM
    at 40; SwiGLU epilogue, then down on the f16 activation (hence 3e-2 of max)."""
    E, k, K, F = 4, 2, 512, 256
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
        g_raw = Q.random_blocks(MX, F * K, 0.05, rng)
        u_raw = Q.random_blocks(MX, F * K, 0.05, rng)
        gus.append(ops.QWeight(ops.interleave_gate_up(g_raw, u_raw, MX, F, K), MX, 2 * F, K, gpu))
        G.append(torch.from_numpy(Q.dequantize(g_raw, MX, (F, K)).copy()))
        U.append(torch.from_numpy(Q.dequantize(u_raw, MX, (F, K)).copy()))
    dns = [_qw(K, F, gpu, 40 + e) for e in range(E)]
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


@pytest.mark.parametrize("name", ["tiny-mixtral", "tiny-qwen3moe"])
def test_mxfp4_moe_models_match_reference(gpu, tmp_path, name):
    """The MoE models as MXFP4_MOE on the GPU kernels: 40-token prefill logits vs the fp32 oracle of the original
    bytes (tiny-qwen3moe: 128 experts, so the expert table and the wide router), then hipGraph decode == eager decode
    with three requests at once and with a single one. Prompt seed 2: of seeds 0-7 the one whose 40 tokens leave the
    oracle's widest smallest gap between the 8th and 9th router logit of the tiny-qwen3moe file (2.19e-3; the others
    1.2e-4 ... 1.7e-3) -- the rule and, as it happens, the seed of tests/test_qwen3moe_gpu.py."""
    path = str(tmp_path / f"{name}-MXFP4_MOE.gguf")
    write_synthetic_gguf(path, name, "MXFP4_MOE", seed=0)
    r = GGUFReader(path)
    m = LlamaModel(r, gpu)
    for lw in m.layers:                                        # no silent f16 detour
        assert {w.type for w in lw.exp_gateup + lw.exp_down} == {transcode.QT_MXFP4}
    S = 40
    ids = list(np.random.default_rng(2).integers(0, 900, S))
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.ids[:S] = torch.tensor(ids, dtype=torch.int32)
    b.pos[:S] = torch.arange(S)
    b.slot[:S] = torch.arange(S)
    b.tok_seq[:S] = 0
    b.ctx_len[:S] = torch.arange(S) + 1
    b.block_tables[0] = torch.arange(8)
    m.forward(b, kc, vc, S, 16, n_split=2)
    rl = ReferenceModel(r).logits(ids)
    err = (b.logits[:S].cpu() - rl).abs().max().item()
    print(f"max logit error {err:.4f} of max |logit| {rl.abs().max().item():.4f}")
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
