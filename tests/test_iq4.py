"""IQ4_NL / IQ4_XS (ggml's non-linear 4-bit types) on the CPU: the codec's bit layout, the quantisers, the device
tile layout (ops/transcode.py) and whole models on the CPU path."""
import os

import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import FILE_TYPE_NAMES, GGMLType, tensor_nbytes
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
from nats_llm_studio_amd.models.llama import LlamaModel
from nats_llm_studio_amd.models.reference import ReferenceModel
from nats_llm_studio_amd.ops import transcode

KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float32)
IQ4 = [GGMLType.IQ4_NL, GGMLType.IQ4_XS]
_QS = bytes(j | ((15 - j) << 4) for j in range(16))      # low nibbles 0..15, high nibbles 15..0


def test_type_ids_and_codebook():
    assert (int(GGMLType.IQ4_NL), int(GGMLType.IQ4_XS)) == (20, 23)
    assert (FILE_TYPE_NAMES[25], FILE_TYPE_NAMES[30]) == ("IQ4_NL", "IQ4_XS")
    assert Q.KVALUES_IQ4NL.astype(np.float32).tolist() == KV.tolist()


def test_iq4_nl_bit_layout():
    raw = np.frombuffer(bytes([0x00, 0x38]) + _QS, np.uint8)            # d = 0x3800 = 0.5
    y = Q.dequantize(raw, GGMLType.IQ4_NL, (32,))
    assert y[:16].tolist() == (0.5 * KV).tolist()
    assert y[16:].tolist() == (0.5 * KV[::-1]).tolist()


def test_iq4_xs_bit_layout():
    # d = 1.0, scales_h = 0xFEA4, scales_l = F0 10 0F FE: both nibbles of scales_l and every 2-bit field of scales_h
    ls = [0, 31, 32, 33, 47, 48, 62, 63]
    raw = np.frombuffer(bytes([0x00, 0x3C, 0xA4, 0xFE, 0xF0, 0x10, 0x0F, 0xFE]) + _QS * 8, np.uint8)
    assert raw.size == 136
    assert Q._unpack_iq4xs_scales(raw.reshape(1, 136))[0].tolist() == ls
    y = Q.dequantize(raw, GGMLType.IQ4_XS, (8, 32))
    for ib in range(8):
        assert y[ib, :16].tolist() == ((ls[ib] - 32) * KV).tolist(), ib
        assert y[ib, 16:].tolist() == ((ls[ib] - 32) * KV[::-1]).tolist(), ib
    assert not y[2].any()                                               # sub-block 2: scale 0
    assert Q._pack_iq4xs_scales(np.array([ls])).tobytes() == raw[2:8].tobytes()


def test_quantize_round_trip_and_sizes():
    """quantize -> dequantize of N(0, 0.05^2) data: relative rms error at most 1.1x that of the Q4_0 codec on the
    same data (a cap against a broken scale choice, not a quality target); deterministic."""
    x = (np.random.default_rng(0).standard_normal((256, 4096)) * 0.05).astype(np.float32)
    rms = float(np.sqrt(np.mean(x * x)))

    def rel(t):
        raw = Q.quantize(x, t)
        assert raw.size == tensor_nbytes(t, x.size) == 256 * ops.row_bytes(t, 4096)
        return float(np.sqrt(np.mean((Q.dequantize(raw, t, x.shape) - x) ** 2))) / rms, raw

    base, _ = rel(GGMLType.Q4_0)
    for t in IQ4:
        err, raw = rel(t)
        print(t.name, "relative rms error", err, "Q4_0", base)
        assert err <= 1.1 * base, (t.name, err, base)
        assert raw.tobytes() == Q.quantize(x, t).tobytes()
    assert tensor_nbytes(GGMLType.IQ4_NL, 4096) == 128 * 18 and ops.row_bytes(GGMLType.IQ4_NL, 4096) == 128 * 18
    assert tensor_nbytes(GGMLType.IQ4_XS, 4096) == 16 * 136 and ops.row_bytes(GGMLType.IQ4_XS, 4096) == 16 * 136


def test_quantize_zero_and_constant_blocks():
    for t in IQ4:
        x = np.zeros((2, 256), np.float32)
        x[1, 32:64] = 0.25
        y = Q.dequantize(Q.quantize(x, t), t, x.shape)
        assert np.isfinite(y).all() and not y[0].any()
        assert np.abs(y[1] - x[1]).max() <= 0.25 * 0.05


def _decode_tiled(data: np.ndarray, rows: int, K: int) -> np.ndarray:
    """The documented IQ4 tile layout read back with numpy: per (16-row tile, 256 values) 2304 bytes =
    [16 rows][8 f16 scales] | P_h[g][r][16]: bytes 8g..8g+7 of the 32-byte chunks 2h and 2h + 1, chunk c holding
    block 2c in its low nibbles and block 2c + 1 in its high ones."""
    T, nb = (rows + 15) // 16, K // 256
    tb = data.reshape(T, nb, 2304)
    sc = np.ascontiguousarray(tb[..., :256]).view(np.float16).reshape(T, nb, 16, 8).astype(np.float32)
    P = tb[..., 256:].reshape(T, nb, 2, 4, 16, 2, 8)                    # h, g, r, chunk of the piece, byte
    out = np.zeros((T, 16, nb, 8, 32), np.float32)
    for h in range(2):
        for c in range(2):
            for g in range(4):
                b = P[:, :, h, g, :, c, :].transpose(0, 2, 1, 3)          # [T, r, nb, 8]
                ch = 2 * h + c
                out[:, :, :, 2 * ch, 8 * g:8 * g + 8] = KV[b & 15]
                out[:, :, :, 2 * ch + 1, 8 * g:8 * g + 8] = KV[b >> 4]
    out *= sc.transpose(0, 2, 1, 3)[..., None]
    return out.reshape(T * 16, K)[:rows]


@pytest.mark.parametrize("t", IQ4)
def test_tile_layout(t):
    rows, K = 40, 512
    raw = Q.random_blocks(t, rows * K, 0.05, np.random.default_rng(2))
    w = ops.QWeight(raw, t, rows, K, "cpu")
    assert w.type == transcode.QT_IQ4 and w.gtype == int(t)
    assert w.nbytes == 3 * 2 * 2304
    got = _decode_tiled(w.data.numpy(), rows, K)
    ref = Q.dequantize(raw, t, (rows, K))
    assert np.abs(ref).max() > 0 and (ref < 0).any() and (ref > 0).any()
    if t == GGMLType.IQ4_NL:
        assert np.array_equal(got, ref)
    else:
        assert (np.abs(got - ref) <= 2.0 ** -10 * np.abs(ref)).all()
    # the padding rows of the last tile hold zeros
    assert not w.data.numpy().reshape(3, 2, 2304)[2, :, :256].reshape(2, 16, 16)[:, 8:].any()
    # the CPU path decodes the original bytes
    assert np.array_equal(w.dense().numpy(), ref)


@pytest.mark.parametrize("t", IQ4)
def test_rows_layout_is_q8_0(t):
    """Embedding tables become Q8_0 rows: qs = kv[q], the block scale d (IQ4_NL) or f16(d*(ls-32)) (IQ4_XS)."""
    rows, K = 6, 512
    raw = Q.random_blocks(t, rows * K, 0.05, np.random.default_rng(3))
    w = ops.QWeight(raw, t, rows, K, "cpu", layout="rows")
    assert w.type == int(GGMLType.Q8_0)
    d = w.data.numpy()
    qs = d[:rows * K].view(np.int8).reshape(rows, K // 32, 32).astype(np.float32)
    sc = d[rows * K:].view(np.float16).reshape(rows, K // 32).astype(np.float32)
    got = (qs * sc[..., None]).reshape(rows, K)
    ref = Q.dequantize(raw, t, (rows, K))
    if t == GGMLType.IQ4_NL:
        assert np.array_equal(got, ref)
    else:
        assert (np.abs(got - ref) <= 2.0 ** -10 * np.abs(ref)).all()


def test_kernel_set_and_tuning_never_pick_modes_2_3():
    from nats_llm_studio_amd.ops import tuning
    q = transcode.QT_IQ4
    assert ops.kernel_set([q, q, 13]) == 4 and ops.kernel_set([q, q, 14]) == 4 and ops.kernel_set([q, 8, 13, 14]) == 4
    assert ops.kernel_set([q, 12]) is None and ops.kernel_set([q, transcode.QT_Q51]) is None
    assert ops.kernel_set([q, 1]) is None
    assert ops.kernel_set([12, 14]) == 0 and ops.kernel_set([13, 8]) == 1 and ops.kernel_set([transcode.QT_Q51, 8]) == 3
    for rows, K in ((6144, 4096), (28672, 4096), (4096, 14336), (128256, 4096), (512, 512)):
        w = ops.QWeight.__new__(ops.QWeight)
        w.type, w.rows, w.K = q, rows, K
        for M in (1, 8, 16, 64, 65, 256, 512, 2048):
            assert tuning.select([ops.Seg(w)], M)[0] in (0, 1), (rows, K, M)


def test_other_iquants_fail_by_name():
    with pytest.raises(NotImplementedError, match="IQ2_XS"):
        tensor_nbytes(17, 256)


@pytest.fixture(scope="module")
def iq4_models(tmp_path_factory):
    d = tmp_path_factory.mktemp("iq4")
    out = {}
    for ft in ("IQ4_NL", "IQ4_XS"):
        md = d / "synthetic" / f"tiny-llama-{ft}-GGUF"
        md.mkdir(parents=True)
        out[ft] = str(md / f"tiny-llama-{ft}.gguf")
        write_synthetic_gguf(out[ft], "tiny-llama", ft, seed=0)
    return str(d), out


@pytest.mark.parametrize("ft", ["IQ4_NL", "IQ4_XS"])
def test_cpu_prefill_iq4_mixes(iq4_models, ft):
    """The whole model in the IQ4 mixes: opens (without the types the open fails with ValueError), lists with its
    ftype, and its prefill logits match the fp32 oracle."""
    from nats_llm_studio_amd.service.registry import Registry
    root, paths = iq4_models
    r = GGUFReader(paths[ft])
    assert r.file_type_name == ft and FILE_TYPE_NAMES[int(r.metadata["general.file_type"])] == ft
    types = {ti.ggml_type for ti in r.tensors.values()}
    assert int(GGMLType[ft]) in types and int(GGMLType.Q5_K) in types and int(GGMLType.Q6_K) in types
    entry = [e for e in Registry(root).scan() if os.path.samefile(e.path, paths[ft])]
    assert len(entry) == 1 and entry[0].quantization == ft and entry[0].to_api(False)["quantization"] == ft
    m = LlamaModel(r, "cpu")
    assert m.layers[0].qkv[0].w.type == transcode.QT_IQ4 and m.tok_embd.type == int(GGMLType.Q8_0)
    # a layer whose V is Q5_K keeps its quantised segments (one launch of kernel type-set 4), no f16 re-encoding
    assert [s.w.type for s in m.layers[1].qkv] == [transcode.QT_IQ4, transcode.QT_IQ4, int(GGMLType.Q5_K)]
    ref = ReferenceModel(r)
    S = 20
    ids = list(np.random.default_rng(1).integers(0, 900, S))
    b = m.step_buffers(64, 4, 8)
    kc, vc = m.kv_cache(8, 16)
    b.ids[:S] = torch.tensor(ids, dtype=torch.int32)
    b.pos[:S] = torch.arange(S)
    b.slot[:S] = torch.arange(S)
    b.tok_seq[:S] = 0
    b.ctx_len[:S] = torch.arange(S) + 1
    b.block_tables[0] = torch.arange(8)
    m.forward(b, kc, vc, S, 16)
    rl = ref.logits(ids)
    err = (b.logits[:S] - rl).abs().max().item()
    assert err < 0.02 * rl.abs().max().item(), err
