"""MXFP4 (ggml type 39) on the CPU: the codec's bit layout, the device tile-block re-pack (ops/transcode.py) and the
MoE models written as MXFP4_MOE on the CPU path."""
import os

import numpy as np
import pytest

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import FILE_TYPE_NAMES, GGMLType, tensor_nbytes
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
from nats_llm_studio_amd.models.reference import ReferenceModel
from nats_llm_studio_amd.ops import transcode

from test_qwen3moe import _model_logits

MAG = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float64)


def _e2m1(q):
    return np.where(q & 8, -1.0, 1.0) * MAG[q & 7]


@pytest.mark.parametrize("e", [114, 127, 140])
def test_bit_layout_and_grid_round_trip(e):
    """All 16 codes in both nibble positions: low nibbles 0..15 (values 0..15), high nibbles 15..0 (values 16..31)."""
    assert (int(GGMLType.MXFP4), FILE_TYPE_NAMES[38], tensor_nbytes(39, 64)) == (39, "MXFP4_MOE", 34)
    lo, hi = np.arange(16), 15 - np.arange(16)
    raw = np.concatenate([[e], lo | (hi << 4)]).astype(np.uint8)
    y = Q.dequantize(raw, GGMLType.MXFP4, (32,))
    ref = np.ldexp(np.concatenate([_e2m1(lo), _e2m1(hi)]), e - 127)
    assert y.dtype == np.float32 and np.array_equal(y.astype(np.float64), ref)
    assert np.array_equal(np.signbit(y), np.signbit(ref))                  # code 8 is -0
    assert Q.quantize(y, GGMLType.MXFP4).tobytes() == raw.tobytes()


def _decode_tiled(data: np.ndarray, rows: int, K: int) -> np.ndarray:
    """The documented MXFP4 tile-block read back with numpy: per (16-row tile, 256 values) 2176 bytes =
    e[r][8] | P_h[g][r][tt][j]: byte j of dword tt holds values k, k + 1 (low, high nibble) at
    k = 32 * (4h + tt) + 8g + 2j of row r, under the E8M0 byte e[r][4h + tt]."""
    T, nb = (rows + 15) // 16, K // 256
    tb = data.reshape(T, nb, 2176)
    e = tb[..., :128].reshape(T, nb, 16, 8).astype(np.int32)                # r, t
    P = tb[..., 128:].reshape(T, nb, 2, 4, 16, 4, 4)                        # h, g, r, tt, j
    q = np.stack([P & 15, P >> 4], axis=-1)                                 # ..., nibble
    v = _e2m1(q).transpose(0, 4, 1, 2, 5, 3, 6, 7).reshape(T, 16, nb, 8, 32)   # T, r, nb, t = 4h + tt, (g, j, nibble)
    return np.ldexp(v, e.transpose(0, 2, 1, 3)[..., None] - 127).reshape(T * 16, K)[:rows]


def test_tile_layout_is_a_permutation():
    rows, K = 40, 512
    raw = Q.random_blocks(GGMLType.MXFP4, rows * K, 0.05, np.random.default_rng(2))
    w = ops.QWeight(raw, GGMLType.MXFP4, rows, K, "cpu")
    assert (w.type, w.gtype, w.nbytes) == (transcode.QT_MXFP4, 39, 3 * 2 * 2176)
    ref = Q.dequantize(raw, GGMLType.MXFP4, (rows, K))
    assert (ref < 0).any() and (ref > 0).any()
    assert np.array_equal(_decode_tiled(w.data.numpy(), rows, K), ref.astype(np.float64))
    assert not w.data.numpy().reshape(3, 2, 2176)[2, :, :128].reshape(2, 16, 8)[:, 8:].any()    # padding rows: zeros
    assert np.array_equal(w.dense().numpy(), ref)                           # the CPU path decodes the original bytes
    assert ops.kernel_set([w.type]) == 5 and ops.kernel_set([w.type, 8]) is None
    with pytest.raises(NotImplementedError, match="MXFP4"):
        ops.QWeight(raw, GGMLType.MXFP4, rows, K, "cpu", layout="rows")


@pytest.mark.parametrize("name", ["tiny-mixtral", "tiny-qwen3moe"])
def test_cpu_prefill_mxfp4_moe(tmp_path, name):
    """The MoE models as MXFP4_MOE (experts MXFP4, the rest Q8_0): the reader reports the type and the file-type
    name, the model lists with it, and the CPU prefill logits match the fp32 oracle. The prompt is the first 20
    tokens of the GPU test's (tests/test_mxfp4_gpu.py: seed 2, chosen there by the oracle's router-logit gaps).
    Measured: 0.5 % of max |logit| for tiny-qwen3moe. Other prompts miss the 2 % through a flipped expert of the
    128: seed 1 gives 4.0 % -- and 2.2 % on the same model written as plain Q8_0, no MXFP4 in it."""
    from nats_llm_studio_amd.service.registry import Registry
    md = tmp_path / "synthetic" / f"{name}-MXFP4_MOE-GGUF"
    md.mkdir(parents=True)
    path = str(md / f"{name}-MXFP4_MOE.gguf")
    write_synthetic_gguf(path, name, "MXFP4_MOE", seed=0)
    r = GGUFReader(path)
    assert r.file_type_name == "MXFP4_MOE"
    assert {ti.ggml_type for n, ti in r.tensors.items() if n.endswith("_exps.weight")} == {int(GGMLType.MXFP4)}
    assert {ti.ggml_type for n, ti in r.tensors.items() if "attn_q." in n or n == "token_embd.weight"} == {8}
    entry = [e for e in Registry(str(tmp_path)).scan() if os.path.samefile(e.path, path)]
    assert len(entry) == 1 and entry[0].to_api(False)["quantization"] == "MXFP4_MOE"
    ids = list(np.random.default_rng(2).integers(0, 900, 40))[:20]
    m, lg = _model_logits(path, ids)
    lw = m.layers[0]
    assert {w.type for w in lw.exp_gateup + lw.exp_down} == {transcode.QT_MXFP4}
    rl = ReferenceModel(r).logits(ids)
    err = (lg - rl).abs().max().item()
    assert err < 0.02 * rl.abs().max().item(), err
