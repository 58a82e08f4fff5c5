"""The expert FFN of gpt-oss -- per-expert biases and the clamped SwiGLU (`epi="swiglu_oai"`) on MXFP4 experts -- on
the CPU: what the dispatcher's plan takes and refuses (through `nls_qgemv_plan` with dummy pointers: nothing is
launched, as in tests/test_gemv_plan.py), the CPU twin of the epilogues against the formula in fp64, and a tiny model
with such experts against the fp32 oracle."""
import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
from nats_llm_studio_amd.ops import transcode

from test_gemv_plan import EXPERT, F, P, Q4_K, S, TAB, plan

MX = transcode.QT_MXFP4
ACT = dict(act_alpha=1.702, act_limit=7.0)
GU = dict(type=MX, rows=48, K=512)       # an interleaved gate|up weight: three 16-row groups
DN = dict(type=MX, rows=40, K=512)       # a down weight: rows no multiple of 16
PROMPT_SEED = 4                          # of the model tests (see test_tiny_model_matches_the_oracle)


def oai_ref(v, bias, act, dv=None, up1=1.0):
    """fp64: v [T, rows] = alpha * acc of interleaved gate|up rows ([g0..g7, u0..u7] per 16), bias [rows] or None ->
    (out [T, rows / 2], g, u, tol) with g, u the biased pre-activations in front of the clamps. up1 = 0: plain
    silu(g) * u when the limit is out of reach. tol (with dv, the error bound of each element of v): what dv becomes
    through out -- the clamps have slope <= 1, d/dg [g sigmoid(a g)] lies in [-0.1, 1.1] -- plus one f16 rounding of
    the output (2^-11, and 2^-25 below the normals) and 2^-18 for the hardware exp and reciprocal of the sigmoid."""
    v = v.double() if bias is None else v.double() + bias.double()
    halves = lambda t: (t.view(t.shape[0], -1, 2, 8)[:, :, 0].reshape(t.shape[0], -1),
                        t.view(t.shape[0], -1, 2, 8)[:, :, 1].reshape(t.shape[0], -1))
    g, u = halves(v)
    gc, uc = g.clamp(max=act[1]), u.clamp(-act[1], act[1])
    out = (uc + up1) * gc * torch.sigmoid(act[0] * gc)
    if dv is None:
        return out, g, u, None
    dg, du = halves(dv.double())
    return out, g, u, 1.1 * (uc + up1).abs() * dg + gc.abs() * du + (2.0 ** -11 + 2.0 ** -18) * out.abs() + 2.0 ** -25


# (name, segments, plan() keywords, accepted)
CASES = [
    ("A, gate|up", [S(**GU)], dict(M=5, epi="swiglu_oai", cfg=(0, 4, 2, 1), fz=F(ebias=P, ldeb=48, **ACT)), True),
    ("A, down + bias", [S(**DN)], dict(M=5, epi="f32", cfg=(0, 4, 2, 1), fz=F(ebias=P, ldeb=40)), True),
    ("B", [S(**GU)], dict(M=40, epi="swiglu_oai", cfg=(1, 8, 1, 1), fz=F(ebias=P, ldeb=48, **ACT)), True),
    ("LDS GEMM", [EXPERT(**GU)], dict(M=65, epi="swiglu_oai", cfg=(2, 8, 2, 1), fz=F(ebias=P, ldeb=48, **ACT)), True),
    ("table", [EXPERT(**GU)], dict(M=5, epi="swiglu_oai", cfg=(1, 8, 1, 1), fz=F(ebias=P, ldeb=48, **ACT, **TAB)), True),
    ("Q4_K", [S(Q4_K, rows=48, K=512)], dict(M=5, epi="swiglu_oai", cfg=(0, 4, 2, 1), fz=F(**ACT)), False),
    ("split-K", [S(**GU)],
     dict(M=5, epi="swiglu_oai", cfg=(1, 8, 1, 2), ws=P, ws_floats=1 << 20, fz=F(ebias=P, ldeb=48, **ACT)), False),
    ("argmax", [S(**DN)], dict(M=5, cfg=(0, 4, 2, 1), argmax=P, fz=F(ebias=P, ldeb=40)), False),
    ("add + bias", [S(**DN)], dict(M=5, epi="add", cfg=(0, 4, 2, 1), fz=F(ebias=P, ldeb=40)), False),
    ("input norm", [S(**GU)],
     dict(M=5, epi="swiglu_oai", cfg=(0, 4, 2, 1), fz=F(xf=P, ldxf=512, nw=P, eps=1e-5, **ACT)), False),
    ("rows % 16", [S(**DN)], dict(M=5, epi="swiglu_oai", cfg=(0, 4, 2, 1), fz=F(**ACT)), False),
]


@pytest.mark.parametrize("name,segs,kw,ok", CASES, ids=[c[0] for c in CASES])
def test_plan(name, segs, kw, ok):
    """Fails without the feature: `ops.EPI` has no "swiglu_oai", NlsFuse no `ebias`."""
    got, p = plan(segs, **kw)
    assert got == ok
    if ok:
        assert p.kset == 5 and p.reduce == 0


def test_cpu_twin_matches_the_formula():
    """ops.qgemv on CPU tensors (an expert table, counts 5 / 0 / 2, biases distinct per expert and row) against
    oai_ref over the decoded weights; the bias helper is interleave_gate_up's permutation."""
    E, cap, K, Fw = 3, 5, 512, 24
    rng = np.random.default_rng(0)
    gb, ub = rng.standard_normal((E, Fw)).astype(np.float32), rng.standard_normal((E, Fw)).astype(np.float32)
    bias = ops.interleave_gate_up_bias(gb, ub)
    assert bias.shape == (E, 48)
    assert np.array_equal(bias[:, 16:24], gb[:, 8:16]) and np.array_equal(bias[:, 24:32], ub[:, 8:16])
    raws = [ops.interleave_gate_up(Q.random_blocks(GGMLType.MXFP4, Fw * K, 0.05, rng),
                                   Q.random_blocks(GGMLType.MXFP4, Fw * K, 0.05, rng), GGMLType.MXFP4, Fw, K)
            for _ in range(E)]
    ws = [ops.QWeight(r, GGMLType.MXFP4, 48, K, "cpu") for r in raws]
    x = (8.0 * torch.randn(16, K, generator=torch.Generator().manual_seed(1))).to(ops.ACT_DTYPE)
    xr = torch.tensor([0, 1, 2, 3, 4, 0, 0, 0, 0, 0, 5, 6, 0, 0, 0], dtype=torch.int32)
    yr = torch.tensor([6, 5, 4, 3, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0], dtype=torch.int32)
    counts = torch.tensor([5, 0, 2], dtype=torch.int32)
    eb = torch.from_numpy(bias)
    y = torch.zeros(8, Fw, dtype=ops.ACT_DTYPE)
    ops.qgemv([ops.Seg(ws[0], 0, xr, yr, counts)], x, y, cap, alpha=0.5, epi="swiglu_oai",
              table=(ops.ExpertTable(ws), cap), ebias=eb)
    for e in (0, 2):
        n = int(counts[e])
        xi, yi = xr[e * cap:e * cap + n].long(), yr[e * cap:e * cap + n].long()
        W = ws[e].dense().double()
        # f32 sums of K products: K * 2^-24 of sum |x w| each
        dv = K * 2.0 ** -24 * 0.5 * (x[xi].double().abs() @ W.abs().t())
        ref, g, u, tol = oai_ref(0.5 * (x[xi].double() @ W.t()), eb[e], ops.SWIGLU_OAI_ACT, dv)
        assert (g > 7).any() and (u > 7).any() and (u < -7).any()
        assert ((y[yi].double() - ref).abs() <= tol).all()


def test_tiny_model_matches_the_oracle(tmp_path):
    """tiny-moe-oai as MXFP4_MOE (16 experts in a table, top 4, expert biases, swiglu_oai) on the CPU path against the
    fp32 oracle: the bounds of tests/test_qwen3moe.py. Prompt seed 4, by the rule of tests/test_qwen3moe_gpu.py: of
    seeds 0-7 the one whose 40 tokens leave the oracle's widest smallest gap between the 4th and 5th router logit
    (6.0e-3; the others 1.0e-4 ... 5.7e-3), so that no f16 rounding of the router's input flips an expert."""
    from nats_llm_studio_amd.models.reference import ReferenceModel
    from test_qwen3moe import _model_logits
    path = str(tmp_path / "tiny-moe-oai.gguf")
    write_synthetic_gguf(path, "tiny-moe-oai", "MXFP4_MOE", seed=0)
    ids = list(np.random.default_rng(PROMPT_SEED).integers(0, 900, 40))
    m, lg = _model_logits(path, ids)
    lw = m.layers[0]
    assert m.cfg.expert_act == "swiglu_oai" and lw.exp_gateup_bias.shape == (16, 512) and lw.exp_down_bias.shape == (16, 256)
    rl = ReferenceModel(GGUFReader(path)).logits(ids)
    err = (lg - rl).abs().max().item() / rl.abs().max().item()
    agree = (lg.argmax(1) == rl.argmax(1)).float().mean().item()
    print(f"max logit error {err:.4f} of the largest |logit|, arg-max agreement {agree:.3f}")
    assert err < 0.05 and agree > 0.9
