"""tiny-llama-d256 (4 / 2 heads of 256: G = 2, the rows form of the prefill kernel) and tiny-qwen3-d256 (8 / 2 heads:
G = 4, the quad form, with the Q/K norm and NEOX RoPE) through ModelConfig, LlamaModel and the fp32 oracle: a
40-token prompt through the flash-prefill kernel, then 4 decode steps with two flash-decoding splits."""
import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
from nats_llm_studio_amd.models.config import ModelConfig
from nats_llm_studio_amd.models.llama import LlamaModel
from nats_llm_studio_amd.models.reference import ReferenceModel

S, NDEC = 40, 4
IDS = [int(v) for v in np.random.default_rng(0).integers(0, 900, S + NDEC)]
MODELS = [("tiny-llama-d256", 4, 2), ("tiny-qwen3-d256", 8, 2)]


def test_d256_models_load(tmp_path, monkeypatch):
    for name, Hq, Hkv in MODELS:
        r = GGUFReader(write_synthetic_gguf(str(tmp_path / f"{name}.gguf"), name, "Q4_K_M", seed=0))
        cfg = ModelConfig.from_gguf(dict(r.metadata))
        assert cfg.head_dim == 256
        m = LlamaModel(r, "cpu")
        assert (m.Hq, m.Hkv, m.D) == (Hq, Hkv, 256)
        assert ops.attention_prefill_ok(Hq, Hkv, 256)
    monkeypatch.setattr(ops, "PREFILL_V1", True)
    assert not ops.attention_prefill_ok(8, 2, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _, _ in MODELS])
def test_gpu_prefill_and_decode_match_reference(gpu, tmp_path, name):
    """The bounds of test_prefill_logits_match_reference_g7: err < 0.05 max|ref|, arg-max agreement > 0.9."""
    r = GGUFReader(write_synthetic_gguf(str(tmp_path / f"{name}.gguf"), name, "Q4_K_M", seed=0))
    m = LlamaModel(r, gpu)
    rl = ReferenceModel(r).logits(IDS)
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.ids[:S] = torch.tensor(IDS[:S], dtype=torch.int32)
    b.pos[:S] = torch.arange(S)
    b.slot[:S] = torch.arange(S)
    b.tok_seq[:S] = 0
    b.ctx_len[:S] = torch.arange(S) + 1
    b.block_tables[0] = torch.arange(8)
    qb = ops.prefill_blocks(np.zeros(S, np.int32), np.arange(S, dtype=np.int32), S)
    m.forward(b, kc, vc, S, 16, n_split=2, qblocks=torch.from_numpy(qb).to(gpu), nqb=len(qb))
    bound = 0.05 * rl.abs().max().item()
    assert (b.logits[:S].cpu() - rl[:S]).abs().max().item() < bound
    assert (b.next_ids[:S].cpu() == rl[:S].argmax(1)).float().mean().item() > 0.9
    for p in range(S, S + NDEC):
        b.ids[:1] = IDS[p]
        b.pos[:1] = p
        b.slot[:1] = p
        b.ctx_len[:1] = p + 1
        m.forward(b, kc, vc, 1, 16, n_split=2)
        assert (b.logits[0].cpu() - rl[p]).abs().max().item() < bound, p
