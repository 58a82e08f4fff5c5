"""Mode 14 (hgemm14.hip): the staggered dense f16 GEMM at 128 activation x 96 weight rows. Its yardstick is mode 4
(hgemm.hip): same operand roles, same K order, so every output -- store, add, f16, RoPE + KV append, split-K slabs --
is bit-identical to mode 4's on the same inputs and the same ks. Exact placement probes (identity activations,
one-hot weights) and a 50-launch determinism screen cover what a tolerance cannot: a misplaced fragment and a race in
the new barrier schedule."""
import functools

import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType

pytestmark = pytest.mark.gpu

M14 = (14, 8, 2)
M4S = [(4, 16, 2), (4, 8, 2)]          # both mode-4 instances at 128-row activation blocks


@functools.lru_cache(maxsize=None)
def _qw(rows, K, t, dev, seed=0):
    """(weight with its f16 copy, fp32 CPU dequantisation); shared by the cases, never written to."""
    rng = np.random.default_rng(seed)
    raw = Q.random_blocks(t, rows * K, 0.05, rng)
    cpu = ops.QWeight(raw, t, rows, K, "cpu")
    w = ops.QWeight(raw, t, rows, K, dev)
    w.expand_dense()
    return w, cpu.dense()


@functools.lru_cache(maxsize=None)
def _x(M, K, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    pad = (M + 63) // 64 * 64
    x = torch.zeros(pad, K, dtype=ops.ACT_DTYPE)
    x[:M] = torch.randn(M, K, generator=g).to(ops.ACT_DTYPE)
    return x.to(dev)


@functools.lru_cache(maxsize=None)
def _ref(M, rows, K, dev):
    return _x(M, K, dev)[:M].float().cpu() @ _qw(rows, K, GGMLType.Q4_K, dev)[1].t()


def _close(a, b, rtol=2e-2):
    err = (a.float().cpu() - b.float().cpu()).abs().max().item()
    scale = b.float().abs().max().item() + 1e-6
    assert err <= rtol * scale, f"max err {err} vs scale {scale}"


def _run(w, x, M, cfg, ks, epi, base=None):
    mode, waves, rt = cfg
    rows = w.rows
    if epi == "act":
        y = torch.zeros(x.shape[0], rows, dtype=ops.ACT_DTYPE, device=x.device)
    else:
        y = torch.zeros(x.shape[0], rows, device=x.device) if base is None else base.clone()
    ops.qgemv([ops.Seg(w)], x, y, M, alpha=0.5 if epi == "add" else 1.0, epi=epi, mode=mode, waves=waves, rt=rt, ks=ks)
    return y


@pytest.mark.parametrize("M", [1, 65, 128, 130, 300])
@pytest.mark.parametrize("K,ks", [(256, 2), (768, 1), (768, 3), (1536, 4), (1024, 1)])
def test_bit_equal_to_mode4(gpu, M, K, ks):
    """rows 264: two full 96-row weight tiles and a partial one of 72 rows; slices of 1, 6, 2, 3 (odd: the other
    ring parity at exit) and 8 K-tiles; M: clamped rows, the block edge, a partial last block. Store, add (alpha 0.5)
    and f16 store."""
    rows = 264
    w, _ = _qw(rows, K, GGMLType.Q4_K, gpu)
    x = _x(M, K, gpu)
    pad = x.shape[0]
    ref = _ref(M, rows, K, gpu)
    base = torch.randn(pad, rows, generator=torch.Generator().manual_seed(7)).to(gpu)
    for epi in ("f32", "add", "act"):
        b = base if epi == "add" else None
        y = _run(w, x, M, M14, ks, epi, b)
        for c4 in M4S:
            y4 = _run(w, x, M, c4, ks, epi, b)
            assert torch.equal(y, y4), (epi, c4, int((y != y4).sum()))
        if epi == "add":
            _close(y[:M], base[:M].cpu() + 0.5 * ref)
            assert torch.equal(y[M:], base[M:])
        else:
            _close(y[:M], ref)
            if M < pad:
                assert float(y[M:].float().abs().max().cpu()) == 0.0


@pytest.mark.parametrize("ks", [1, 2])
def test_exact_placement(gpu, ks):
    """No tolerance. x = I: y = W^T exactly, for every k position of both K-tiles and every activation row. Then
    one-hot weight rows against random x: y[m, n] = x[m, k(n)] exactly. Every other addend is an exact zero, so any
    misplaced fragment, chunk swizzle or k-step shows as a wrong entry."""
    rows, K, M = 264, 256, 256
    w0, _ = _qw(rows, K, GGMLType.Q4_K, gpu)
    eye = torch.eye(M, K, dtype=ops.ACT_DTYPE, device=gpu)
    y = _run(w0, eye, M, M14, ks, "f32")
    assert torch.equal(y, w0.d16.float().t())
    # one-hot rows: weight row n picks column k(n); 264 rows over 256 columns with an odd stride: every k is picked
    w = ops.QWeight.__new__(ops.QWeight)
    w.__dict__.update(w0.__dict__)
    kn = (torch.arange(rows) * 37 + 5) % K
    hot = torch.zeros(rows, K, dtype=torch.float16)
    hot[torch.arange(rows), kn] = 1.0
    w.d16 = hot.to(gpu)
    assert len(set(kn.tolist())) == K
    x = _x(M, K, gpu, seed=3)
    y = _run(w, x, M, M14, ks, "f32")
    assert torch.equal(y, x[:, kn.to(gpu)].float())


def _rope_launch(gpu, cfg, ks, M, bias, segs, x, Hq, Hkv, D):
    pad = x.shape[0]
    cs = ops.rope_table(4 * pad, D, 10000.0, gpu)
    pos = torch.arange(pad, dtype=torch.int32, device=gpu) * 3
    slot = torch.arange(pad, dtype=torch.int32, device=gpu)
    qkv = torch.zeros(pad, (Hq + 2 * Hkv) * D, device=gpu)
    q = torch.zeros(pad, Hq * D, dtype=torch.bfloat16, device=gpu)
    kc = torch.zeros(pad, Hkv, D, dtype=torch.bfloat16, device=gpu)
    vc = torch.zeros_like(kc)
    fz = ops._fuse_rope(ops._lib.NlsFuse(), pos, slot, cs, bias, q, kc, vc, Hq, Hkv, D)
    ok = ops._launch(segs, x, qkv, M, 1.0, "rope", (*cfg, ks), fz=fz, soft=True)
    return ok, q, kc, vc


@pytest.mark.parametrize("M", [65, 300])
@pytest.mark.parametrize("bias", [False, True])
def test_rope_epilogue_bit_equal_to_mode4(gpu, M, bias):
    """EPI_ROPE with the KV append on merged Q|K|V f16 copies (one launch segment): q_out, the K cache and the V
    cache are mode 4's bits; against the CPU rope of the fp32 product within mode 4's own tolerance; split-K with
    RoPE is refused."""
    Hq, Hkv, D, K = 4, 2, 64, 512
    rng = np.random.default_rng(21)
    ws, Wd = [], []
    for rows, t in ((Hq * D, GGMLType.Q4_K), (Hkv * D, GGMLType.Q4_K), (Hkv * D, GGMLType.Q6_K)):
        raw = Q.random_blocks(t, rows * K, 0.05, rng)
        ws.append(ops.QWeight(raw, t, rows, K, gpu))
        Wd.append(ops.QWeight(raw, t, rows, K, "cpu").dense())
    assert ops.QWeight.expand_dense_group(ws) == (Hq + 2 * Hkv) * D * K * 2
    segs = [ops.Seg(ws[0], 0), ops.Seg(ws[1], Hq * D), ops.Seg(ws[2], (Hq + Hkv) * D)]
    x = _x(M, K, gpu)
    bv = torch.randn((Hq + 2 * Hkv) * D, generator=torch.Generator().manual_seed(5)).to(gpu) if bias else None
    ok, q, kc, vc = _rope_launch(gpu, M14, 1, M, bv, segs, x, Hq, Hkv, D)
    assert ok
    for c4 in M4S:
        ok4, q4, kc4, vc4 = _rope_launch(gpu, c4, 1, M, bv, segs, x, Hq, Hkv, D)
        assert ok4 and torch.equal(q, q4) and torch.equal(kc, kc4) and torch.equal(vc, vc4), c4
    pad = x.shape[0]
    qc = torch.zeros(pad, Hq * D, dtype=torch.bfloat16)
    kcc = torch.zeros(pad, Hkv, D, dtype=torch.bfloat16)
    vcc = torch.zeros_like(kcc)
    ops.rope_kv(x[:M].float().cpu() @ torch.cat(Wd).t(), torch.arange(pad, dtype=torch.int32) * 3,
                torch.arange(pad, dtype=torch.int32), ops.rope_table(4 * pad, D, 10000.0, gpu).cpu(), qc, kcc, vcc, M,
                Hq, Hkv, D, bias=None if bv is None else bv.cpu())
    for a, b in ((q, qc), (kc, kcc), (vc, vcc)):
        _close(a[:M], b[:M], 3e-2)
    assert not _rope_launch(gpu, M14, 2, M, bv, segs, x, Hq, Hkv, D)[0]


def test_splitk_add_rmsnorm_bit_equal_to_mode4(gpu):
    """The o-projection path: ks 2 slabs into the fused reduce + residual + RMSNorm kernel. Hidden state and the
    normalised f16 output are mode 4's bits."""
    D, K, M = 512, 1024, 200
    w, Wd = _qw(D, K, GGMLType.Q4_K, gpu, 4)
    xin = _x(M, K, gpu)
    x0 = torch.randn(xin.shape[0], D, generator=torch.Generator().manual_seed(9)).to(gpu)
    nw = (torch.rand(D, generator=torch.Generator().manual_seed(10)) + 0.5).to(gpu)
    outs = []
    for cfg in (M14, *M4S):
        x = x0.clone()
        h = torch.zeros(xin.shape[0], D, dtype=ops.ACT_DTYPE, device=gpu)
        ops.qgemv_add_rmsnorm(ops.Seg(w), xin, x, nw, h, M, 1.0, 1e-5, cfg=(*cfg, 2))
        outs.append((x, h))
    for x, h in outs[1:]:
        assert torch.equal(outs[0][0], x) and torch.equal(outs[0][1], h)
    ref = x0[:M].cpu() + xin[:M].float().cpu() @ Wd.t()
    _close(outs[0][0][:M], ref)
    _close(outs[0][1][:M], ref * torch.rsqrt(ref.pow(2).mean(1, keepdim=True) + 1e-5) * nw.cpu(), 2e-2)


@pytest.mark.parametrize("rows,M", [(6144, 512), (2048, 256)])
def test_deterministic_when_the_chip_is_full(gpu, rows, M):
    """rows 6144 x M 512: 64 tiles x 4 blocks = 256 workgroups, one per CU (the flagship's Q|K|V grid); rows 2048 x
    M 256: 22 tiles, the last partial. 50 launches on the same inputs give the first launch's bits, which are mode
    4's."""
    K = 1024
    w, _ = _qw(rows, K, GGMLType.Q4_K, gpu, 11)
    x = _x(M, K, gpu, seed=12)
    ys = [_run(w, x, M, M14, 1, "f32") for _ in range(50)]
    y4 = _run(w, x, M, M4S[0], 1, "f32")
    torch.cuda.synchronize()
    assert all(torch.equal(ys[0], y) for y in ys[1:])
    assert torch.equal(ys[0], y4)
