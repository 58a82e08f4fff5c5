"""MFMA flash-prefill for GQA group sizes that are no multiple of 4 (attn_prefill_rows.hip: token-major query rows
packed 32 to a wave) against the fp64 reference, inputs and tolerance of test_attention_sensitivity.

Largest row ratio measured on the MI355X (non-census families; tolerance ROW_TOL = 0.034): 0.0067 .. 0.0091, worst at
(128, 14) fp8; the census families within 0.44 of their own tolerance (profiles/prefill_any_group.txt)."""
import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from test_attention_sensitivity import BS, F8, FAMILIES, ROW_TOL, _case, _judge


@pytest.mark.gpu
@pytest.mark.parametrize("kvt", [torch.bfloat16, F8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("D,G", [(128, 1), (128, 2), (128, 3), (128, 5), (128, 7), (64, 6), (64, 7), (128, 14)])
def test_prefill_families_any_group(gpu, D, G, kvt):
    """Every family through ops.attention_prefill at Hkv = 2: 1-token, ragged and mid-context chunks, and 64- / 130-token
    chunks whose wave and workgroup boundaries fall inside a token's heads."""
    Hkv, qt = 2, 64
    Hq = Hkv * G
    assert ops.attention_prefill_ok(Hq, Hkv, D)
    for fam in FAMILIES:
        c = _case("prefill", fam, D, G, Hkv, kvt, qt)
        T = c["T"]
        pos = np.concatenate([np.arange(p0, p0 + n) for _, p0, n in c["chunks"]]).astype(np.int32)
        tseq = np.concatenate([np.full(n, s) for s, _, n in c["chunks"]]).astype(np.int32)
        qb = ops.prefill_blocks(tseq, pos, T)
        assert int(qb[:, 1].max()) == qt and int(qb[:, 1].sum()) == T
        out = torch.full((T, Hq * D), 3.0, dtype=ops.ACT_DTYPE, device=gpu)
        ops.attention_prefill(c["q"].to(gpu), c["kc"].to(gpu), c["vc"].to(gpu), c["bt"].to(gpu),
                              torch.from_numpy(qb).to(gpu), len(qb), None, None, out, T, Hq, Hkv, D, BS, c["scale"])
        r = _judge(fam, out.cpu(), c["ref"], Hq, D)
        print(f"ATTN_RATIO prefill rows D{D} G{G} {fam} {float(r.max()) * (1 if fam.startswith('census') else ROW_TOL):.5f}")
        assert float(r.max()) <= 1.0, (fam, [(int(pos[i]), float(v)) for i, v in enumerate(r.amax(-1)) if v > 1][:8])


def test_prefill_ok_any_group(monkeypatch):
    monkeypatch.setattr(ops, "PREFILL_V1", False)
    for D in (64, 128):
        assert all(ops.attention_prefill_ok(2 * G, 2, D) for G in range(1, 17))
        assert not ops.attention_prefill_ok(34, 2, D)
    assert not ops.attention_prefill_ok(8, 2, 96) and not ops.attention_prefill_ok(7, 2, 128)
    monkeypatch.setattr(ops, "PREFILL_V1", True)
    for G in range(1, 18):
        assert ops.attention_prefill_ok(2 * G, 2, 128) == (G % 4 == 0)


@pytest.mark.gpu
def test_prefill_logits_match_reference_g7(gpu, tmp_path):
    """tiny-qwen2-g7 (14 / 2 heads of 128: QKV bias, NEOX RoPE, G = 7) against the fp32 oracle, as
    test_model_gpu.test_prefill_logits_match_reference compares tiny-qwen2, with the chunk's query blocks passed
    so that attention runs the prefill kernel as it does in the engine."""
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel
    from nats_llm_studio_amd.models.reference import ReferenceModel
    r = GGUFReader(write_synthetic_gguf(str(tmp_path / "tiny-qwen2-g7.gguf"), "tiny-qwen2-g7", "Q4_K_M", seed=0))
    m = LlamaModel(r, gpu)
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
    qb = ops.prefill_blocks(np.zeros(S, np.int32), np.arange(S, dtype=np.int32), S)
    m.forward(b, kc, vc, S, 16, n_split=2, qblocks=torch.from_numpy(qb).to(gpu), nqb=len(qb))
    rl = ReferenceModel(r).logits(ids)
    err = (b.logits[:S].cpu() - rl).abs().max().item()
    assert err < 0.05 * rl.abs().max().item(), err
    assert (b.next_ids[:S].cpu() == rl.argmax(1)).float().mean().item() > 0.9
