"""Qwen3 dense models on the CPU path: config, the per-head Q/K RMSNorm + RoPE + KV-append op against an inline
float64 reference, the whole model against the fp32 oracle (and what that comparison can see), TP=2 and the service."""
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
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import SPECS, write_synthetic_gguf
from nats_llm_studio_amd.models.config import ModelConfig

MODEL_TOL = 0.02      # tests/test_model_cpu.py: max |logit error| < 0.02 * max |oracle logit|


@pytest.fixture(scope="module")
def qwen3_path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("qwen3") / "tiny-qwen3.gguf")
    write_synthetic_gguf(p, "tiny-qwen3", "Q4_K_M", seed=0)
    return p


def _prompt():
    """The prompt of test_model_cpu.test_cpu_prefill_matches_reference."""
    return list(np.random.default_rng(0).integers(0, 900, 24))


# ------------------------------------------------------------------------------------------------ config
def test_config(qwen3_path, tmp_path):
    r = GGUFReader(qwen3_path)
    cfg = ModelConfig.from_gguf(r.metadata, r.tensors.keys())
    assert (cfg.arch, cfg.head_dim, cfg.q_dim, cfg.kv_dim, cfg.d_model) == ("qwen3", 128, 1024, 256, 512)
    assert cfg.rope_neox and cfg.qk_norm and cfg.tied_embeddings and cfg.eps == pytest.approx(1e-6)
    assert r.tensors["blk.0.attn_q_norm.weight"].np_shape == (128,)
    assert "blk.0.attn_q.bias" not in r.tensors
    w = r.dequantized("blk.1.attn_k_norm.weight")
    assert w.min() > 0.2 and w.max() > 3.0 and 1.5 < float(np.median(w)) < 2.7      # wide, not near 1
    md = dict(r.metadata)
    md["qwen3.attention.value_length"] = 64
    with pytest.raises(NotImplementedError, match="128.*64"):
        ModelConfig.from_gguf(md, r.tensors.keys())
    md["general.architecture"] = "qwen3moe"
    with pytest.raises(NotImplementedError, match="qwen3moe"):
        ModelConfig.from_gguf(md)


def test_new_tensors_only_in_qwen3_plans():
    """The new tensors and the new init code appear in qwen3 plans only (every other spec draws what it drew)."""
    from nats_llm_studio_amd.gguf.synth import tensor_plan
    for name, spec in SPECS.items():
        plan = tensor_plan(spec, "Q4_K_M")
        qk = [t for t in plan if "attn_q_norm" in t[0] or "attn_k_norm" in t[0]]
        assert (len(qk) == 2 * spec.n_layer) == (spec.arch == "qwen3"), name
        assert all(t[3] == -4.0 for t in qk) and all(t[3] != -4.0 for t in plan if t not in qk)
        assert not (spec.arch == "qwen3" and any(t[0].endswith(".bias") for t in plan))
    assert SPECS["tiny-qwen2"].head_dim == 128 and SPECS["qwen3-0.6b"].head_dim == 128
    assert SPECS["qwen3-8b"].n_head * SPECS["qwen3-8b"].head_dim == 4096


def test_loading_is_supported(qwen3_path):
    """Fails without the feature: ModelConfig.from_gguf raised NotImplementedError for `qwen3`."""
    from nats_llm_studio_amd.models.llama import LlamaModel
    m = LlamaModel(GGUFReader(qwen3_path), "cpu")
    assert m.layers[0].q_norm.shape == (128,) and m.layers[1].k_norm.dtype == torch.float32
    assert m.layers[0].qkv_bias is None and m.layers[0].wo.K == 1024 and m.layers[0].qkv[0].w.rows == 1024


# ------------------------------------------------------------------------------------------------ the op
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


def _bf16_close(out, ref):
    """One bf16 ulp: |out - ref| <= 2^-7 |ref| + 1e-5 per element."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    bad = np.abs(out - ref) > 2.0 ** -7 * np.abs(ref) + 1e-5
    assert not bad.any(), (int(bad.sum()), float(np.abs(out - ref).max()))


@pytest.mark.parametrize("neox", [False, True])
@pytest.mark.parametrize("ks", [1, 3])
def test_cpu_twin_matches_float64_reference(neox, ks):
    g = torch.Generator().manual_seed(5 + ks)
    T, Hq, Hkv, D, eps = 5, 3, 2, 128, 1e-6
    ncol = (Hq + 2 * Hkv) * D
    ld = ncol + 8
    slabs = torch.randn(ks, T, ld, generator=g)
    qw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    kw = torch.exp(0.7 + 0.45 * torch.randn(D, generator=g))
    cs = ops.rope_table(64, D, 1e6, "cpu")
    pos = torch.tensor([0, 3, 6, 9, 63], dtype=torch.int32)
    slot = torch.tensor([4, -1, 0, 7, 2], dtype=torch.int32)
    SENT = -7.0
    q = torch.full((T, Hq * D + 8), SENT, dtype=torch.bfloat16)
    kc = torch.full((9, Hkv, D), SENT, dtype=torch.bfloat16)
    vc = kc.clone()
    ops.qk_norm_rope_kv(slabs.view(ks * T, ld), pos, slot, cs, q, kc, vc, T, Hq, Hkv, D, qw, kw, eps, neox,
                        ks=ks, slab=T * ld)
    rq, rk, rv = _ref_qknorm_rope(slabs.numpy(), pos.numpy(), cs.numpy(), qw.numpy(), kw.numpy(), eps, Hq, Hkv, D, neox)
    _bf16_close(q[:, :Hq * D].float().numpy().reshape(T, Hq, D), rq)
    assert bool((q[:, Hq * D:] == SENT).all())
    ok = slot.numpy() >= 0
    sl = slot.numpy()[ok]
    _bf16_close(kc[sl].float().numpy(), rk[ok])
    assert torch.equal(vc[sl], torch.from_numpy(rv[ok]).to(torch.bfloat16))
    rest = [i for i in range(9) if i not in set(sl.tolist())]
    assert bool((kc[rest] == SENT).all()) and bool((vc[rest] == SENT).all())


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


@pytest.mark.parametrize("permute", ["1", "0"])
def test_cpu_prefill_matches_reference(qwen3_path, monkeypatch, permute):
    """LlamaModel on the CPU path vs the oracle, with the NEOX row permutation (norm weights permuted with the
    single-head order) and without it (the NEOX rotation of the original rows)."""
    from nats_llm_studio_amd.models.reference import ReferenceModel
    monkeypatch.setenv("NLS_NEOX_PERMUTE", permute)
    ids = _prompt()
    m, lg = _model_logits(qwen3_path, ids)
    assert m.rope_neox == (permute == "0")
    rl = ReferenceModel(GGUFReader(qwen3_path)).logits(ids)
    err = (lg - rl).abs().max().item()
    assert err < MODEL_TOL * rl.abs().max().item(), err


def test_oracle_comparison_sees_the_qk_norm(qwen3_path):
    """What the model-vs-oracle tests can detect: three broken oracles on the model test's own prompt, each of which
    must move the logits by at least 3x that test's tolerance (0.02 * max |logit|).
    Measured (tiny-qwen3, Q4_K_M, seed 0; max |logit| 3.750, tolerance 0.0750):
      (a) norms skipped                    shift 3.850 = 51x the tolerance
      (b) norm weights replaced by ones    shift 3.525 = 47x
      (c) norm applied after the RoPE      shift 3.001 = 40x"""
    from nats_llm_studio_amd.models.reference import ReferenceModel

    class Skipped(ReferenceModel):
        def _qk_rope(self, q, k, pos, p):
            return self._rope(q, pos), self._rope(k, pos)

    class Ones(ReferenceModel):
        def w(self, name):
            t = super().w(name)
            return torch.ones_like(t) if name.endswith(("attn_q_norm.weight", "attn_k_norm.weight")) else t

    class AfterRope(ReferenceModel):
        def _qk_rope(self, q, k, pos, p):
            q, k = self._rope(q, pos), self._rope(k, pos)
            return (self._rms(q, self.w(p + "attn_q_norm.weight"), self.cfg.eps),
                    self._rms(k, self.w(p + "attn_k_norm.weight"), self.cfg.eps))

    ids = _prompt()
    r = GGUFReader(qwen3_path)
    rl = ReferenceModel(r).logits(ids)
    tol = MODEL_TOL * rl.abs().max().item()
    shifts = {}
    for cls in (Skipped, Ones, AfterRope):
        shifts[cls.__name__] = (cls(r).logits(ids) - rl).abs().max().item()
    print("max |logit|", rl.abs().max().item(), "tolerance", tol, "shifts", shifts)
    for name, s in shifts.items():
        assert s >= 3 * tol, (name, s, tol)


# ------------------------------------------------------------------------------------------------ TP
def test_tp2_matches_tp1(tmp_path):
    """Two gloo ranks (heads sharded whole, norm weights replicated) produce one rank's tokens."""
    from test_parallel import _engine, _free_port, _run, _worker
    spec = dataclasses.replace(SPECS["tiny-qwen3"], name="tp-qwen3", d_ff=1024)
    path = str(tmp_path / "tp-qwen3.gguf")
    write_synthetic_gguf(path, spec.name, "Q4_K_M", seed=1, spec=spec)
    ref_toks, ref_lg = _run(_engine(path))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, path, False, q)) for r in range(2)]
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
                    raise AssertionError(f"TP workers failed: {[p.exitcode for p in procs]}")
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
def test_service_lists_and_chats(qwen3_path, tmp_path):
    """list_models reports the architecture; a chat on the CPU engine backend is prompted through the file's ChatML
    template (its prompt token count is that of the ChatML-framed conversation) and answers 200."""
    from nats_llm_studio_amd.natsio import Client, EmbeddedServer
    from nats_llm_studio_amd.service.config import WorkerConfig
    from nats_llm_studio_amd.service.service import Service
    from nats_llm_studio_amd.tokenizer.bpe import tokenizer_from_metadata
    from nats_llm_studio_amd.tokenizer.chat_template import ChatTemplate
    d = tmp_path / "models" / "synthetic" / "tiny-qwen3-GGUF"
    d.mkdir(parents=True)
    shutil.copy(qwen3_path, d / "tiny-qwen3-Q4_K_M.gguf")
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
        entry = [m for m in lm["data"]["models"]["data"] if m["id"] == "tiny-qwen3"]
        assert len(entry) == 1 and entry[0]["arch"] == "qwen3", lm
        msgs = [{"role": "user", "content": "hello there"}]
        r = req("chat_model", {"model": "tiny-qwen3", "messages": msgs, "max_tokens": 6, "ignore_eos": True,
                               "temperature": 0}, timeout=120)
        assert r["ok"] and r["data"]["http_status"] == 200, r
        resp = r["data"]["response"]
        assert resp["model_info"]["arch"] == "qwen3"
        assert resp["usage"]["completion_tokens"] == 6
        assert isinstance(resp["choices"][0]["message"]["content"], str)
        md = GGUFReader(qwen3_path).metadata
        tok = tokenizer_from_metadata(md)
        prompt = ChatTemplate(md["tokenizer.chat_template"]).render(msgs, add_generation_prompt=True)
        assert prompt.endswith("<|im_start|>user\nhello there<|im_end|>\n<|im_start|>assistant\n")
        ids = tok.encode(prompt, add_bos=False)
        assert ids.count(tok.tokens.index("<|im_start|>")) == 3        # system, user, assistant: single tokens
        assert resp["usage"]["prompt_tokens"] == len(ids)
    finally:
        cli.close()
        svc.stop()
        svc.client.close()
        srv.stop()
