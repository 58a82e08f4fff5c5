"""Qwen3 MoE (`qwen3moe`: Qwen3 attention, 128 routed experts of their own width, top 8) on the CPU path: config,
the whole model against the fp32 oracle, the expert-table twin against the launches of 8 segments, EP = 2, the
service, and what the fp32 block reference of the GPU expert-table tests can see."""
import dataclasses
import json
import queue
import shutil
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf.constants import GGMLType
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import MOE_SPECS, SPECS, find_spec, write_synthetic_gguf
from nats_llm_studio_amd.models.config import ModelConfig

import moe_blocks as MB


@pytest.fixture(scope="module")
def moe_path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("qwen3moe") / "tiny-qwen3moe.gguf")
    write_synthetic_gguf(p, "tiny-qwen3moe", "Q4_K_M", seed=0)
    return p


# ------------------------------------------------------------------------------------------------ config
def test_config(moe_path, tmp_path):
    """Fails without the feature: ModelConfig.from_gguf raised NotImplementedError for `qwen3moe`."""
    r = GGUFReader(moe_path)
    cfg = ModelConfig.from_gguf(r.metadata, r.tensors.keys())
    assert (cfg.arch, cfg.n_expert, cfg.n_expert_used) == ("qwen3moe", 128, 8)
    assert (cfg.d_ff, cfg.expert_ff) == (768, 256)                  # the expert key, not the dense one
    assert cfg.qk_norm and cfg.rope_neox and cfg.tied_embeddings
    assert (cfg.head_dim, cfg.q_dim, cfg.d_model) == (128, 512, 256)
    assert r.tensors["blk.0.ffn_gate_exps.weight"].np_shape == (128, 256, 256)
    assert r.tensors["blk.1.ffn_down_exps.weight"].np_shape == (128, 256, 256)
    assert r.tensors["blk.0.ffn_gate_inp.weight"].ggml_type == GGMLType.F32
    assert "blk.0.attn_q_norm.weight" in r.tensors and "blk.0.ffn_gate.weight" not in r.tensors
    # without expert_feed_forward_length the experts are feed_forward_length wide (Mixtral)
    md = {k: v for k, v in r.metadata.items() if k != "qwen3moe.expert_feed_forward_length"}
    assert ModelConfig.from_gguf(md, r.tensors.keys()).expert_ff == 768
    mix = str(tmp_path / "mix.gguf")
    write_synthetic_gguf(mix, "tiny-mixtral", "Q4_K_M", seed=0)
    rm = GGUFReader(mix)
    assert "llama.expert_feed_forward_length" not in rm.metadata
    cm = ModelConfig.from_gguf(rm.metadata, rm.tensors.keys())
    assert cm.expert_ff == cm.d_ff == 512
    # a qwen3moe file has experts
    md = {k: v for k, v in r.metadata.items() if k != "qwen3moe.expert_count"}
    with pytest.raises(NotImplementedError, match="expert_count"):
        ModelConfig.from_gguf(md, r.tensors.keys())


def test_specs():
    s = find_spec("qwen3-30b-a3b")
    assert (s.arch, s.n_layer, s.d_model, s.n_head, s.n_kv_head, s.head_dim) == ("qwen3moe", 48, 2048, 32, 4, 128)
    assert (s.d_ff, s.expert_ff, s.n_expert, s.n_expert_used, s.vocab, s.ctx) == (6144, 768, 128, 8, 151936, 40960)
    assert s.rope_base == 1e6 and s.eps == 1e-6 and not s.tied_embeddings
    assert SPECS["mixtral-8x7b"].expert_ff == 14336 and SPECS["tiny-mixtral"].d_ff_expert == 0
    assert not set(SPECS) & set(MOE_SPECS) and find_spec("tiny-llama") is SPECS["tiny-llama"]
    with pytest.raises(KeyError, match="no-such-model"):
        find_spec("no-such-model")


# ------------------------------------------------------------------------------------------------ the model
def _model_logits(path, ids):
    from nats_llm_studio_amd.models.llama import LlamaModel
    m = LlamaModel(GGUFReader(path), "cpu")
    S = len(ids)
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.ids[:S] = torch.tensor(ids, dtype=torch.int32)
    b.pos[:S] = torch.arange(S)
    b.slot[:S] = torch.arange(S)
    b.tok_seq[:S] = 0
    b.ctx_len[:S] = torch.arange(S) + 1
    b.block_tables[0] = torch.arange(8)
    m.forward(b, kc, vc, S, 16)
    return m, b.logits[:S].clone()


def test_cpu_prefill_matches_reference(moe_path, monkeypatch):
    """LlamaModel(cpu) vs the oracle on 40 tokens: the bounds of the model tests (max error < 5 % of the largest
    |logit|, arg-max agreement > 0.9; measured 1.8 % and 100 %), with the expert tables and, bit for bit, without."""
    from nats_llm_studio_amd.models.reference import ReferenceModel
    ids = list(np.random.default_rng(0).integers(0, 900, 40))
    m, lg = _model_logits(moe_path, ids)
    assert m.exp_ffn == 256 and m.layers[0].exp_gateup[0].rows == 512 and m.layers[0].exp_down[0].K == 256
    assert len(m.layers[0].tab_gateup) == 128 and m.layers[0].router16 is None
    rl = ReferenceModel(GGUFReader(moe_path)).logits(ids)
    err = (lg - rl).abs().max().item() / rl.abs().max().item()
    agree = (lg.argmax(1) == rl.argmax(1)).float().mean().item()
    print(f"max logit error {err:.4f} of the largest |logit|, arg-max agreement {agree:.3f}")
    assert err < 0.05 and agree > 0.9
    monkeypatch.setenv("NLS_MOE_TABLE", "0")
    _, lg8 = _model_logits(moe_path, ids)
    assert torch.equal(lg, lg8)


def _generate(path, prompts, n=6):
    from nats_llm_studio_amd.engine.engine import Engine, GenRequest
    from nats_llm_studio_amd.engine.sampling import SamplingParams
    from nats_llm_studio_amd.models.llama import LlamaModel
    eng = Engine(LlamaModel(GGUFReader(path), "cpu"), None, max_batch=4, max_prefill_tokens=64, num_blocks=64,
                 use_graphs=False, ctx=256)
    futs = [eng.submit(GenRequest(list(p), SamplingParams(max_tokens=n, ignore_eos=True))) for p in prompts]
    while not all(f.done() for f in futs):
        eng.step()
    return [f.result().token_ids for f in futs]


def test_generation_same_with_and_without_tables(moe_path, monkeypatch):
    """Greedy generation through the Engine: the CPU twin of the table launch is the arithmetic of the launches of 8."""
    prompts = [[1, 2, 3, 4, 5], [9, 8, 7]]
    a = _generate(moe_path, prompts)
    monkeypatch.setenv("NLS_MOE_TABLE", "0")
    b = _generate(moe_path, prompts)
    assert a == b and all(len(t) == 6 for t in a)


def test_tensor_parallel_needs_ep(moe_path):
    """256-wide experts cannot be TP-sliced into K-quant super-blocks; expert parallelism is the multi-rank mode."""
    from nats_llm_studio_amd.models.llama import LlamaModel, ShardSpec
    with pytest.raises(ValueError, match="multiples of 256"):
        LlamaModel(GGUFReader(moe_path), "cpu", ShardSpec(0, 2, False))


# ------------------------------------------------------------------------------------------------ EP
def test_ep2_matches_one_process(tmp_path):
    """Two gloo ranks with 64 whole experts each produce one process's tokens."""
    from test_parallel import _engine, _free_port, _run, _worker
    spec = dataclasses.replace(MOE_SPECS["tiny-qwen3moe"], name="ep-qwen3moe")
    path = str(tmp_path / "ep-qwen3moe.gguf")
    write_synthetic_gguf(path, spec.name, "Q4_K_M", seed=1, spec=spec)
    ref_toks, ref_lg = _run(_engine(path))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, path, True, q)) for r in range(2)]
    for p in procs:
        p.start()
    t0 = time.time()
    try:
        while True:
            try:
                toks, lg, n_ar, ctr = q.get(timeout=2)
                break
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs) or time.time() - t0 > 300:
                    raise AssertionError(f"EP workers failed: {[p.exitcode for p in procs]}")
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    assert n_ar > 0
    assert toks == ref_toks
    ref = ref_lg[:, :lg.shape[1]].numpy()
    assert lg.shape[1] == spec.vocab
    assert abs(lg - ref).max() / (abs(ref).max() + 1e-6) < 1e-3


# ------------------------------------------------------------------------------------------------ service
def test_service_lists_and_chats(moe_path, tmp_path):
    from nats_llm_studio_amd.natsio import Client, EmbeddedServer
    from nats_llm_studio_amd.service.config import WorkerConfig
    from nats_llm_studio_amd.service.service import Service
    d = tmp_path / "models" / "synthetic" / "tiny-qwen3moe-GGUF"
    d.mkdir(parents=True)
    shutil.copy(moe_path, d / "tiny-qwen3moe-Q4_K_M.gguf")
    srv = EmbeddedServer().start()
    cfg = WorkerConfig(nats_url=srv.url, models_dir=str(tmp_path / "models"), backend="engine", device="cpu",
                       max_batch=4, max_ctx=256, max_loaded_models=1)
    svc = Service(cfg).start()
    cli = Client().connect(srv.url)

    def req(name, payload, timeout=60):
        return json.loads(cli.request(f"lmstudio.{name}", json.dumps(payload).encode(), timeout).data)
    try:
        lm = req("list_models", {})
        assert lm["ok"], lm
        entry = [m for m in lm["data"]["models"]["data"] if m["id"] == "tiny-qwen3moe"]
        assert len(entry) == 1 and entry[0]["arch"] == "qwen3moe", lm
        msgs = [{"role": "user", "content": "hello there"}]
        r = req("chat_model", {"model": "tiny-qwen3moe", "messages": msgs, "max_tokens": 6, "ignore_eos": True,
                               "temperature": 0}, timeout=120)
        assert r["ok"] and r["data"]["http_status"] == 200, r
        resp = r["data"]["response"]
        assert resp["model_info"]["arch"] == "qwen3moe"
        assert resp["usage"]["completion_tokens"] == 6
        assert isinstance(resp["choices"][0]["message"]["content"], str)
        assert "<|im_start|>" in GGUFReader(moe_path).metadata["tokenizer.chat_template"]     # ChatML, as Qwen3
    finally:
        cli.close()
        svc.stop()
        svc.client.close()
        srv.stop()


# ------------------------------------------------------------------------------------------------ block reference
def test_block_reference_sees_a_wrong_expert_and_a_wrong_width():
    """What the expert-table tests (tests/test_qwen3moe_gpu.py) can detect. The block on the CPU twin meets
    MB.BLOCK_TOL; a reference with two routed experts' weights swapped, or one that strides the experts by the dense
    FFN width (768) where the expert width (256) belongs, misses it by at least 10x.
    Measured (E 128, k 8, K 256, F 256, Q4_K gate|up, Q6_K down, T 3): block 1.4e-4 of the largest value; swapped
    experts 0.375 = 19x the bound; dense width 1.37 = 69x."""
    E, K, F, D, k, T = 128, 256, 256, 256, 8, 3
    ex = MB.Experts(E, K, F, D, GGMLType.Q4_K, GGMLType.Q6_K, "cpu", seed=11)
    g = torch.Generator().manual_seed(103)
    x = torch.zeros(64, K, dtype=ops.ACT_DTYPE)
    x[:T] = torch.randn(T, K, generator=g).to(ops.ACT_DTYPE)
    lg = torch.randn(T, E, generator=g)
    outs = []
    for table in (True, False):
        b = MB.buffers(E, T, k, F, D, "cpu")
        outs.append((MB.run_block(ex, x, lg, T, k, b, table=table), b))
    (out, b), (out8, b8) = outs
    assert torch.equal(out, out8) and torch.equal(b["yexp"], b8["yexp"]) and torch.equal(b["act"], b8["act"])
    assert bool((b["yexp"][T * k:] == MB.SENT).all()) and bool((b["act"][T * k:] == MB.SENT).all())
    ref, _ = MB.block_reference(ex, x, b["sel"], b["topw"], T, k)
    err = MB.rel_err(out, ref)
    sel = b["sel"].view(T, k)
    a = int(sel[0, 0])
    other = next(e for e in range(E) if e not in sel[0].tolist())
    swapped, _ = MB.block_reference(ex, x, b["sel"], b["topw"], T, k, swap=(a, other))
    wide, _ = MB.block_reference(ex, x, b["sel"], b["topw"], T, k, width=768)
    e_swap, e_wide = MB.rel_err(out, swapped), MB.rel_err(out, wide)
    print(f"block {err:.2e}, swapped experts {e_swap:.3f}, dense width {e_wide:.3f} (bound {MB.BLOCK_TOL})")
    assert err <= MB.BLOCK_TOL
    assert e_swap >= 10 * MB.BLOCK_TOL and e_wide >= 10 * MB.BLOCK_TOL
