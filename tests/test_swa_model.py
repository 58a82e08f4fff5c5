"""tiny-llama-swa (a 24-key window on layer 0 of 2, sinks on both layers) through ModelConfig, LlamaModel and the
fp32 oracle: a 60-token prompt (2.5 windows), then 8 decode steps on the GPU."""
import dataclasses

import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import SPECS, write_synthetic_gguf
from nats_llm_studio_amd.models.config import ModelConfig
from nats_llm_studio_amd.models.llama import LlamaModel
from nats_llm_studio_amd.models.reference import ReferenceModel

S, NDEC = 60, 8
IDS = [int(v) for v in np.random.default_rng(0).integers(0, 900, S + NDEC)]


@pytest.fixture(scope="module")
def swa(tmp_path_factory):
    """(tiny-llama-swa, the oracle's logits of IDS, the same for the same weights without the window key)."""
    d = tmp_path_factory.mktemp("swa")
    r = GGUFReader(write_synthetic_gguf(str(d / "swa.gguf"), "tiny-llama-swa", "Q4_K_M", seed=0))
    full = dataclasses.replace(SPECS["tiny-llama-swa"], sliding_window=0)
    r0 = GGUFReader(write_synthetic_gguf(str(d / "full.gguf"), "", "Q4_K_M", seed=0, spec=full))
    return r, ReferenceModel(r).logits(IDS), ReferenceModel(r0).logits(IDS)


def test_config_window_and_pattern(swa):
    md = dict(swa[0].metadata)
    cfg = ModelConfig.from_gguf(md)
    assert cfg.sliding_window == 24 and cfg.swa_layers == (True, False)
    assert [cfg.layer_window(i) for i in range(2)] == [24, 0]
    del md["llama.attention.sliding_window_pattern"]
    assert ModelConfig.from_gguf(md).swa_layers == (True, True)
    for bad in (np.asarray([True, False, True]), [1, 0], 2):
        md["llama.attention.sliding_window_pattern"] = bad
        with pytest.raises(NotImplementedError, match="sliding_window_pattern"):
            ModelConfig.from_gguf(md)


def _prefill(m, dev, qblocks):
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.ids[:S] = torch.tensor(IDS[:S], dtype=torch.int32)
    b.pos[:S] = torch.arange(S)
    b.slot[:S] = torch.arange(S)
    b.tok_seq[:S] = 0
    b.ctx_len[:S] = torch.arange(S) + 1
    b.block_tables[0] = torch.arange(8)
    qb = ops.prefill_blocks(np.zeros(S, np.int32), np.arange(S, dtype=np.int32), S)
    m.forward(b, kc, vc, S, 16, n_split=2, qblocks=torch.from_numpy(qb).to(dev) if qblocks else None, nqb=len(qb))
    return b, kc, vc


def test_cpu_logits_match_reference(swa):
    r, rl, rl_full = swa
    b, _, _ = _prefill(LlamaModel(r, "cpu"), "cpu", False)
    bound = 0.02 * rl.abs().max().item()                    # the bound of test_model_cpu
    assert (b.logits[:S] - rl[:S]).abs().max().item() < bound
    # the test can see the feature: past the window the oracle's logits depend on the metadata key
    assert (rl[S - 1] - rl_full[S - 1]).abs().max().item() > bound


@pytest.mark.gpu
def test_gpu_prefill_and_decode_match_reference(gpu, swa):
    """The prompt through the flash-prefill kernel, then 8 steps with two flash-decoding splits (bound: the G = 7 test's)."""
    r, rl, _ = swa
    m = LlamaModel(r, gpu)
    b, kc, vc = _prefill(m, gpu, True)
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
