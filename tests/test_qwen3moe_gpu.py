"""Qwen3 MoE on the MI355X: the route kernel for 64 < E <= 128 experts, expert launches over an expert table (one
launch per projection whatever E is), the whole tiny-qwen3moe model against the fp32 oracle, and the number of
kernel nodes of the decode graphs, which must not depend on E."""
import dataclasses
import glob
import os

import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf.constants import GGMLType

import moe_blocks as MB

pytestmark = pytest.mark.gpu

PROMPT_SEED = 2      # of seeds 0-7 the prompt with the widest smallest 8th/9th router-logit gap (see the model test)


# ------------------------------------------------------------------------------------------------ route
def _route(lg, T, k, cap, dev, stale=0, guard=64):
    E = lg.shape[1]
    topw = torch.zeros(T * k, device=dev)
    counts = torch.full((E,), stale, dtype=torch.int32, device=dev)
    xr = torch.full((E * cap + guard,), -7, dtype=torch.int32, device=dev)
    yr = torch.full((E * cap + guard,), -7, dtype=torch.int32, device=dev)
    sel = torch.full((T * k,), -1, dtype=torch.int32, device=dev)
    ops.moe_route(lg, T, k, topw, counts, xr, yr, cap, sel=sel)
    torch.cuda.synchronize()
    return topw, counts.cpu(), xr.cpu(), yr.cpu(), sel.cpu()


def _check_lists(e, T, E, k, cap, counts, xr, yr, sel):
    """Row lists, counts and sel against the expert choice e [T, k] (slot order)."""
    assert sel.view(T, k).tolist() == e.tolist()
    assert counts.sum().item() == T * k
    for ex in range(E):
        c = int(counts[ex])
        want = sorted((t, t * k + j) for t in range(T) for j in range(k) if int(e[t, j]) == ex)
        got = sorted(zip(xr[ex * cap:ex * cap + c].tolist(), yr[ex * cap:ex * cap + c].tolist()))
        assert got == want, ex
    assert (xr[E * cap:] == -7).all() and (yr[E * cap:] == -7).all()


@pytest.mark.parametrize("T", [1, 4, 5, 70])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("E", [65, 96, 128])
def test_wide_route_matches_softmax_topk(gpu, E, k, T):
    """Random f32 logits (no ties): softmax -> top-k -> renormalise in torch is the unambiguous reference."""
    g = torch.Generator().manual_seed(1000 * E + 10 * T + k)
    lg = torch.randn(T, E, generator=g).to(gpu)
    cap = 72
    topw, counts, xr, yr, sel = _route(lg, T, k, cap, gpu, stale=3 if T <= 4 else 0)
    w, e = torch.topk(torch.softmax(lg.cpu(), -1), k, -1)
    w = w / w.sum(-1, keepdim=True)
    torch.testing.assert_close(topw.cpu().view(T, k), w, rtol=1e-5, atol=1e-6)
    _check_lists(e, T, E, k, cap, counts, xr, yr, sel)


def test_wide_route_ties_and_nonfinite_rows(gpu):
    """Ties and NaNs resolve to the lowest unused expert; k distinct valid experts whatever the row holds; stale
    counts of a one-workgroup launch (T <= 4) are zeroed in the kernel."""
    E, k, cap = 128, 8, 64
    lg = torch.zeros(4, E)
    lg[1, 3] = lg[1, 67] = 5.0            # the same lane in both halves: 3 first, then 67
    lg[2, 127] = 2.0                      # the last expert (lane 63, high half) wins alone
    lg[3, 64:] = 1.0                      # the high half ahead of the low half: 64..71
    topw, counts, xr, yr, sel = _route(lg.to(gpu), 4, k, cap, gpu, stale=5)
    s = sel.view(4, k).tolist()
    assert s[0] == list(range(8))
    assert s[1] == [3, 67, 0, 1, 2, 4, 5, 6]
    assert s[2] == [127, 0, 1, 2, 3, 4, 5, 6]
    assert s[3] == list(range(64, 72))
    torch.testing.assert_close(topw.cpu().view(4, k).sum(1), torch.ones(4), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(topw.cpu()[:8], torch.full((8,), 0.125), rtol=1e-5, atol=1e-6)
    _check_lists(torch.tensor(s), 4, E, k, cap, counts, xr, yr, sel)
    # NaN / +-inf rows (the rows of test_moe_route_nan_rows_stay_in_bounds, in both halves)
    T, E = 6, 96
    lg = torch.randn(T, E, generator=torch.Generator().manual_seed(5))
    lg[1] = float("nan")
    lg[2, 3] = float("inf")
    lg[2, 70] = float("inf")
    lg[3, :80] = float("-inf")
    lg[4, 5] = float("nan")
    lg[4, 69] = float("nan")
    lg[5, 64:] = float("nan")
    topw, counts, xr, yr, sel = _route(lg.to(gpu), T, k, cap, gpu)
    assert counts.sum().item() == T * k and (counts >= 0).all() and (counts <= T).all()
    assert (xr[E * cap:] == -7).all() and (yr[E * cap:] == -7).all()
    s = sel.view(T, k).tolist()
    assert all(len(set(r)) == k and all(0 <= v < E for v in r) for r in s), s
    assert s[1] == list(range(8))                                   # all NaN: the lowest experts
    assert sorted(s[3]) == sorted(torch.topk(lg[3], k).indices.tolist())   # the finite ones
    assert 5 not in s[4] and 69 not in s[4] and all(v < 64 for v in s[5])  # a NaN never beats a number
    _check_lists(torch.tensor(s), T, E, k, cap, counts, xr, yr, sel)


def test_route_refuses_more_than_128_experts(gpu):
    T, E, k, cap = 5, 129, 8, 64
    lg = torch.randn(T, E, device=gpu)
    bufs = [torch.full((T * k,), -7.0, device=gpu)] + [
        torch.full((n,), -7, dtype=torch.int32, device=gpu) for n in (E, E * cap, E * cap, T * k)]
    with pytest.raises(RuntimeError):
        ops.moe_route(lg, T, k, bufs[0], bufs[1], bufs[2], bufs[3], cap, sel=bufs[4])
    torch.cuda.synchronize()
    assert all(bool((b == -7).all()) for b in bufs)


# ------------------------------------------------------------------------------------------------ expert tables
E_, K_, F_, D_, k_ = 128, 256, 256, 256, 8
_EXPERTS = {}


def _experts(mix, gpu):
    """One set of 128 experts per quant mix for the whole module (the references share it, nobody writes it)."""
    if mix not in _EXPERTS:
        gu, dn = {"Q4_K_M": (GGMLType.Q4_K, GGMLType.Q6_K), "Q5_K_M": (GGMLType.Q5_K, GGMLType.Q6_K)}[mix]
        _EXPERTS[mix] = MB.Experts(E_, K_, F_, D_, gu, dn, gpu, seed=11)
    return _EXPERTS[mix]


# T = 1, 3: device-selected path A; 16: unselected path A; 70: one launch each on path B (mode 1) and on the
# LDS-dequant GEMM (mode 2)
_CASES = [("Q4_K_M", 1, "sel", None), ("Q4_K_M", 3, "sel", None), ("Q4_K_M", 16, "all", None),
          ("Q4_K_M", 70, "all", dict(mode=1, waves=8, rt=1, ks=1)), ("Q4_K_M", 70, "all", dict(mode=2, waves=8, rt=2, ks=1)),
          ("Q5_K_M", 3, "sel", None), ("Q5_K_M", 70, "all", dict(mode=2, waves=8, rt=2, ks=1))]


@pytest.mark.parametrize("mix,T,path,cfg", _CASES)
def test_expert_table_launches(gpu, mix, T, path, cfg):
    """Route on the device, gate|up (SwiGLU) and down through the expert tables, combine: against the fp32 block
    reference over the device's own sel / topw (MB.BLOCK_TOL), bit-equal to the launches of 8 by-value segments
    (what NLS_MOE_TABLE=0 runs), unrouted rows untouched."""
    ex = _experts(mix, gpu)
    g = torch.Generator().manual_seed(100 + T)
    pad = (T + 63) // 64 * 64
    x = torch.zeros(pad, K_, dtype=ops.ACT_DTYPE)
    x[:T] = torch.randn(T, K_, generator=g).to(ops.ACT_DTYPE)
    x = x.to(gpu)
    lg = torch.randn(T, E_, generator=g).to(gpu)
    outs = []
    for table in (True, False):
        b = MB.buffers(E_, T, k_, F_, D_, gpu)
        out = MB.run_block(ex, x, lg, T, k_, b, table=table, selected=path == "sel", gu_cfg=cfg, dn_cfg=cfg)
        torch.cuda.synchronize()
        outs.append((out, b))
    (out, b), (out8, b8) = outs
    assert torch.equal(b["sel"], b8["sel"]) and torch.equal(b["topw"], b8["topw"])
    assert torch.equal(b["act"], b8["act"]) and torch.equal(b["yexp"], b8["yexp"]) and torch.equal(out, out8)
    ref, rows = MB.block_reference(ex, x, b["sel"], b["topw"], T, k_)
    err, err_rows = MB.rel_err(out, ref), MB.rel_err(b["yexp"][:T * k_], rows)
    print(f"{mix} T={T} {path} {cfg}: block error {err:.2e}, expert rows {err_rows:.2e} of the largest value")
    assert err <= MB.BLOCK_TOL and err_rows <= MB.BLOCK_TOL, (err, err_rows)
    assert bool((b["act"][T * k_:] == MB.SENT).all()) and bool((b["yexp"][T * k_:] == MB.SENT).all())
    assert bool((b["xrows"][E_ * b["cap"]:] == int(MB.SENT)).all())


def test_expert_table_refuses_what_it_does_not_run(gpu):
    """Split-K, the DMA GEMM and more rows than path A takes are errors, not silent fallbacks."""
    ex = _experts("Q4_K_M", gpu)
    T = 70
    b = MB.buffers(E_, T, k_, F_, D_, gpu)
    x = torch.zeros(128, K_, dtype=ops.ACT_DTYPE, device=gpu)
    seg = [ops.Seg(ex.gu[0], 0, b["xrows"], b["yrows"], b["counts"])]
    for cfg in (dict(mode=3, waves=4, rt=6, ks=1), dict(mode=1, waves=8, rt=1, ks=2), dict(mode=0, waves=4, rt=2, ks=1)):
        with pytest.raises(RuntimeError):
            ops.qgemv(seg, x, b["act"], T, epi="swiglu", table=(ex.tab_gu, b["cap"]), **cfg)
    torch.cuda.synchronize()
    assert bool((b["act"] == MB.SENT).all())


# ------------------------------------------------------------------------------------------------ whole model
def _router_gap(ref, ids, k):
    """Smallest gap between the k-th and (k+1)-th router logit over the oracle's (token, layer) pairs: the
    difference of their log-probabilities is the difference of the logits."""
    gaps = []
    topk = torch.topk

    def spy(p, kk, *a, **kw):
        if kk == k and p.dim() == 2 and p.shape[-1] == ref.cfg.n_expert:
            s = torch.sort(p.double(), -1, descending=True).values
            gaps.append((s[:, k - 1].log() - s[:, k].log()).min().item())
        return topk(p, kk, *a, **kw)
    torch.topk = spy
    try:
        rl = ref.logits(ids)
    finally:
        torch.topk = topk
    return rl, min(gaps), len(gaps)


def test_tiny_qwen3moe_prefill_and_graph_decode(gpu, tmp_path, monkeypatch):
    """tiny-qwen3moe prefill logits vs the fp32 oracle (bounds of test_tiny_qwen3_prefill_and_graph_decode), the
    same logits bit for bit with NLS_MOE_TABLE=0, then hipGraph decode == eager decode at batch 1 and on a 3-row
    step. Prompt seed 2: the oracle's smallest 8th/9th router-logit gap over the 80 (token, layer) pairs of this
    file is printed (measured on the CPU: 1.27e-3 for Q4_K_M; seeds 0-7 give 2.0e-4 ... 1.27e-3, and 3.4e-5 ... 1.90e-3
    for Q5_K_M, seed 2 the widest for both). Measured on one MI355X: max logit error 0.050 of max |logit| 2.68
    (bound 0.134)."""
    from nats_llm_studio_amd.engine.engine import Engine, GenRequest
    from nats_llm_studio_amd.engine.sampling import SamplingParams
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel
    from nats_llm_studio_amd.models.reference import ReferenceModel
    path = str(tmp_path / "tiny-qwen3moe.gguf")
    write_synthetic_gguf(path, "tiny-qwen3moe", "Q4_K_M", seed=0)
    r = GGUFReader(path)
    m = LlamaModel(r, gpu)
    assert m.layers[0].tab_gateup is not None and len(m.layers[0].tab_down) == 128
    S = 40
    ids = list(np.random.default_rng(PROMPT_SEED).integers(0, 900, S))
    rl, gap, n = _router_gap(ReferenceModel(r), ids, m.cfg.n_expert_used)
    print(f"smallest 8th/9th router-logit gap of the oracle over {n} layers x {S} tokens: {gap:.3e}")

    def prefill():
        b = m.step_buffers(64, 4, 8)
        kc, vc = m.kv_cache(8, 16)
        b.ids[:S] = torch.tensor(ids, dtype=torch.int32)
        b.pos[:S] = torch.arange(S)
        b.slot[:S] = torch.arange(S)
        b.tok_seq[:S] = 0
        b.ctx_len[:S] = torch.arange(S) + 1
        b.block_tables[0] = torch.arange(8)
        m.forward(b, kc, vc, S, 16, n_split=2)
        return b.logits[:S].cpu(), b.next_ids[:S].cpu()
    lg, nxt = prefill()
    err = (lg - rl).abs().max().item()
    print(f"max logit error {err:.4f} of max |logit| {rl.abs().max().item():.4f}")
    assert err < 0.05 * rl.abs().max().item(), err
    assert (nxt == rl.argmax(1)).float().mean().item() > 0.9
    monkeypatch.setenv("NLS_MOE_TABLE", "0")
    lg8, _ = prefill()
    monkeypatch.delenv("NLS_MOE_TABLE")
    assert torch.equal(lg, lg8)
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


def test_decode_graph_nodes_do_not_depend_on_expert_count(gpu, tmp_path, monkeypatch):
    """Two files that differ only in E (64 and 128, k = 8): their captured decode graphs hold the same number of
    kernel nodes at the buckets of the device-selected path (1), the unselected path A (16) and the grouped GEMM
    (32). Launches of 8 by-value segments would give 8 against 16 expert launches per projection."""
    from nats_llm_studio_amd.engine.engine import Engine
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import MOE_SPECS, write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel
    nodes = {}
    for E in (64, 128):
        spec = dataclasses.replace(MOE_SPECS["tiny-qwen3moe"], name=f"moe-e{E}", n_expert=E)
        path = str(tmp_path / f"moe-e{E}.gguf")
        write_synthetic_gguf(path, spec.name, "Q4_K_M", seed=0, spec=spec)
        dump = tmp_path / f"dump{E}"
        monkeypatch.setenv("NLS_GRAPH_DUMP", str(dump))
        eng = Engine(LlamaModel(GGUFReader(path), gpu), None, max_batch=32, use_graphs=True)
        eng.capture_all(buckets=[1, 16, 32])
        torch.cuda.synchronize()
        for B in (1, 16, 32):
            f, = glob.glob(os.path.join(str(dump), f"w1_r0_B{B}_logits0_dsamp0.nodes"))
            with open(f) as fh:
                names = [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]
            nodes[E, B] = names
        del eng
    for B in (1, 16, 32):
        a, b = nodes[64, B], nodes[128, B]
        print(f"bucket {B}: {len(a)} kernel nodes at E=64, {len(b)} at E=128")
        assert len(a) == len(b) and len(a) > 0, (B, len(a), len(b))
