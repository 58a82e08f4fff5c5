"""The expert FFN of gpt-oss on the MI355X: the per-expert bias and the clamped SwiGLU (`epi="swiglu_oai"`) as
epilogues of the MXFP4 kernels (type-set 5) on every route MXFP4 experts take, against an fp64 reference over the
device-form weights (f16(E2M1(q) * 2^(e - 127)), exact) and the f16 activations; and tiny-moe-oai against the oracle.

Shapes: K = 512 (two super-blocks), gate|up 48 rows (three 16-row groups: the last 32-row tile of path A is partial),
down 40 rows (no multiple of 16), 3 experts at cap 5 with 5 / 0 / 2 routed rows (an empty and a partial expert).
Output column j of gate|up: j % 4 == 0 has a hot gate row, j % 4 == 1 a hot up row (block exponents 2^-2: pre-activation
std about 16 against limit 7, so gates above the limit and ups beyond both clamps), the other rows 2^-5 (std about 2: in
range). Bounds: the per-element summation-order bound of tests/test_mxfp4_gpu.py (K * 2^-23 * sum |x w|) on alpha * acc,
carried through the activation and its one f16 rounding by test_moe_oai.oai_ref."""
import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType

from test_iq4_gpu import _x
from test_moe_oai import PROMPT_SEED, oai_ref

pytestmark = pytest.mark.gpu

MX = GGMLType.MXFP4
E, CAP, K, FW, DR = 3, 5, 512, 24, 40
XR = [0, 1, 2, 3, 4, 0, 0, 0, 0, 0, 5, 6, 0, 0, 0]     # expert e's x rows at e * CAP; counts 5 / 0 / 2
YR = [6, 5, 4, 3, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
COUNTS = [5, 0, 2]
SENT = 77.0
# route -> (launch config, form of the launch): by-value segments, device-selected segments, expert table
ROUTES = {"A": (dict(mode=0, waves=4, rt=2, ks=1), "segs"), "A-sel": (dict(mode=0, waves=4, rt=2, ks=1), "sel"),
          "A-table": (dict(mode=0, waves=4, rt=2, ks=1), "table"), "B-table": (dict(mode=1, waves=8, rt=1, ks=1), "table"),
          "LDS-table": (dict(mode=2, waves=8, rt=1, ks=1), "table")}


@pytest.fixture(scope="module")
def case(gpu):
    """Weights, activations, maps and biases (shared, read-only) with the fp64 products and their error bounds."""
    rng = np.random.default_rng(5)

    def raw(exps):           # MXFP4 rows with the block exponent 2^exps[row], uniform nibbles
        r = rng.integers(0, 256, size=(len(exps), K // 32, 17), dtype=np.uint8)
        r[:, :, 0] = (127 + np.asarray(exps))[:, None]
        return r.reshape(-1)
    j = np.arange(FW)
    c = dict(gu=[], dn=[], Wgu=[], Wdn=[])
    for e in range(E):
        gu = ops.interleave_gate_up(raw(np.where(j % 4 == 0, -2, -5)), raw(np.where(j % 4 == 1, -2, -5)), MX, FW, K)
        dn = raw(np.full(DR, -5))
        c["gu"].append(ops.QWeight(gu, MX, 2 * FW, K, gpu))
        c["dn"].append(ops.QWeight(dn, MX, DR, K, gpu))
        c["Wgu"].append(torch.from_numpy(Q.dequantize(gu, MX, (2 * FW, K)).copy()).double())
        c["Wdn"].append(torch.from_numpy(Q.dequantize(dn, MX, (DR, K)).copy()).double())
    c["tab_gu"], c["tab_dn"] = ops.ExpertTable(c["gu"]), ops.ExpertTable(c["dn"])
    c["x"] = _x(7, K, gpu)
    c["xr"], c["yr"] = (torch.tensor(t, dtype=torch.int32, device=gpu) for t in (XR, YR))
    c["counts"] = torch.tensor(COUNTS, dtype=torch.int32, device=gpu)
    c["sel"] = torch.tensor([2, 0, 2, 1], dtype=torch.int32, device=gpu)     # a repeated and an empty expert
    # distinct per expert and row: a row of the wrong expert, or in gate / up order, moves every output
    c["b_gu"] = torch.tensor([[(e * 100 + r) * 0.01 for r in range(2 * FW)] for e in range(E)], device=gpu)
    c["b_dn"] = torch.tensor([[(e * 100 + r) * 0.01 for r in range(DR)] for e in range(E)], device=gpu)
    return c


def _launch(c, route, which, epi, y, ebias, **kw):
    cfg, form = ROUTES[route]
    ws, tab = c[which], c["tab_" + which]
    ymap = c["yr"]
    if form == "table":
        ops.qgemv([ops.Seg(ws[0], 0, c["xr"], ymap, c["counts"])], c["x"], y, CAP, epi=epi, table=(tab, CAP),
                  ebias=ebias, **cfg, **kw)
    else:
        segs = [ops.Seg(w, 0, c["xr"][e * CAP:], ymap[e * CAP:], c["counts"][e:e + 1]) for e, w in enumerate(ws)]
        ops.qgemv(segs, c["x"], y, CAP, epi=epi, sel=(c["sel"], 4, 0) if form == "sel" else None, ebias=ebias,
                  **cfg, **kw)
    torch.cuda.synchronize()
    return y.double().cpu()


def _products(c, which, e):
    """fp64 x W^T of expert e's routed rows, its bound, and the y rows they land in."""
    n = COUNTS[e]
    xs = c["x"][XR[e * CAP:e * CAP + n]].double().cpu()
    W = c["W" + which][e]
    return xs @ W.t(), K * 2.0 ** -23 * (xs.abs() @ W.abs().t()), YR[e * CAP:e * CAP + n]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_expert_epilogues(gpu, case, route, bias):
    """gate|up through swiglu_oai and down through the f32 store, with and without the expert bias. Measured on one
    MI355X: largest error / bound 0.19 with the bias, 0.22 without, on every route (profiles/moe_oai.txt)."""
    c = case
    act = torch.full((8, FW), SENT, dtype=ops.ACT_DTYPE, device=gpu)
    yd = torch.full((8, DR), SENT, device=gpu)
    a = _launch(c, route, "gu", "swiglu_oai", act, c["b_gu"] if bias else None)
    d = _launch(c, route, "dn", "f32", yd, c["b_dn"] if bias else None)
    seen = torch.zeros(4, dtype=torch.bool)
    worst = 0.0
    for e in (0, 2):
        v, dv, yi = _products(c, "gu", e)
        ref, g, u, tol = oai_ref(v, c["b_gu"][e].cpu() if bias else None, ops.SWIGLU_OAI_ACT, dv)
        seen |= torch.stack([(g > 7).any(), (u > 7).any(), (u < -7).any(), ((g.abs() < 7) & (u.abs() < 7)).any()])
        worst = max(worst, ((a[yi] - ref).abs() / tol).max().item())
        v, dv, yi = _products(c, "dn", e)
        ref = v + c["b_dn"][e].double().cpu() if bias else v
        worst = max(worst, ((d[yi] - ref).abs() / (dv + 2.0 ** -24 * ref.abs())).max().item())   # (+ the bias's one f32 add)
    assert seen.all(), seen          # the inputs: every clamp bites somewhere, and some elements are in range
    print(f"{route} bias={bias}: largest |err| / bound {worst:.4f}")
    assert worst <= 1.0
    assert bool((a[7:] == SENT).all()) and bool((d[7:] == SENT).all())


@pytest.mark.parametrize("route", ["A", "B-table", "LDS-table"])
def test_unclamped_oai_is_swiglu_plus_silu(gpu, case, route):
    """act = (1.0, 1e30) and a zero bias: swiglu_oai - swiglu = silu(g), element by element -- the new branch reads the
    rows and writes the columns of the old one."""
    c = case
    ya = torch.zeros(8, FW, dtype=ops.ACT_DTYPE, device=gpu)
    ys = torch.zeros(8, FW, dtype=ops.ACT_DTYPE, device=gpu)
    a = _launch(c, route, "gu", "swiglu_oai", ya, torch.zeros_like(c["b_gu"]), act=(1.0, 1e30), alpha=0.125)
    s = _launch(c, route, "gu", "swiglu", ys, None, alpha=0.125)
    for e in (0, 2):
        v, dv, yi = _products(c, "gu", e)
        ra, g, u, ta = oai_ref(0.125 * v, None, (1.0, 1e30), 0.125 * dv)
        rs, _, _, ts = oai_ref(0.125 * v, None, (1.0, 1e30), 0.125 * dv, up1=0.0)
        assert ((s[yi] - rs).abs() <= ts).all()
        assert ((a[yi] - s[yi] - g * torch.sigmoid(g)).abs() <= ta + ts).all()


def test_tiny_moe_oai_prefill_and_decode(gpu, tmp_path):
    """tiny-moe-oai as MXFP4_MOE: 36 tokens of prefill (the grouped GEMM over the expert table) and 4 decode steps
    (device-selected path A) against the fp32 oracle, with the bounds of tests/test_qwen3moe_gpu.py."""
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel
    from nats_llm_studio_amd.models.reference import ReferenceModel
    path = str(tmp_path / "tiny-moe-oai.gguf")
    write_synthetic_gguf(path, "tiny-moe-oai", "MXFP4_MOE", seed=0)
    r = GGUFReader(path)
    m = LlamaModel(r, gpu)
    assert m.layers[0].tab_gateup is not None and m.layers[0].exp_gateup_bias is not None
    S, P = 40, 36
    ids = list(np.random.default_rng(PROMPT_SEED).integers(0, 900, S))
    rl = ReferenceModel(r).logits(ids)
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.block_tables[0] = torch.arange(8)
    lg = torch.zeros(S, rl.shape[1])
    for t0, n in [(0, P)] + [(t, 1) for t in range(P, S)]:
        b.ids[:n] = torch.tensor(ids[t0:t0 + n], dtype=torch.int32)
        b.pos[:n] = torch.arange(t0, t0 + n)
        b.slot[:n] = torch.arange(t0, t0 + n)
        b.tok_seq[:n] = 0
        b.ctx_len[:n] = torch.arange(t0, t0 + n) + 1
        m.forward(b, kc, vc, n, 16)
        lg[t0:t0 + n] = b.logits[:n].cpu()
    err = (lg - rl).abs().max(1).values
    print(f"max logit error: prefill {err[:P].max().item():.4f}, decode {err[P:].max().item():.4f} "
          f"of max |logit| {rl.abs().max().item():.4f}")
    assert err.max().item() < 0.05 * rl.abs().max().item()
    assert (lg.argmax(1) == rl.argmax(1)).float().mean().item() > 0.9
