"""Grid map of the dense f16 GEMMs (modes 4 / 5 / 10) under split-K (csrc/kernels/gemm_block.h dense_grid_pos): mode 10
with ks in {2, 4, 8} puts one k-slice on each XCD; every other ks, and modes 4 / 5, keep every k-slice of a weight tile
on one XCD. A map only moves workgroups, so every (tile, m-block, k-slice) must still be computed exactly once and land
in its own slab, whichever map a launch takes.

Shapes are the smallest at which the map can go wrong: K = 2048 is 32 K-tiles (ks 8: 4 per slice, ks 3: uneven
10 / 11 / 11); M = 300 is two m-blocks of 256 or three of 128, the last ragged; N = 384 is 3 tiles of 128 (fewer
tiles than groups at ks 2, no multiple of the group count), N = 688 ends in a ragged tile, N = 2304 is 18 tiles of 128
(more than 8, no multiple of 8). Reference: the fp32 product with the numpy ggml decode of the weight, bound as
test_production_gpu.py (max error <= 2e-2 of the reference's largest value). Outputs and the split-K workspace are
pre-filled with NaN, so a tile or a slab nobody wrote fails."""
import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType

pytestmark = pytest.mark.gpu

K, M, MPAD = 2048, 300, 320
NS = (384, 688, 2304)
KSS = (1, 2, 3, 4, 8)
# (mode, waves, rt): mode 10 at 256- and 128-row weight tiles; mode 4 with 8 and 16 waves (128- and 256-row
# activation blocks); mode 5 (256-row weight tiles)
KERNELS = [(10, 8, 1), (10, 8, 2), (4, 8, 2), (4, 16, 4), (5, 8, 4)]
RTOL = 2e-2


def _rows_of(w, r0, r1, own=False):
    """Rows [r0, r1) of a dense-expanded weight as a weight of their own (the dense modes read only the f16 copy);
    own: in a buffer of its own, so that a launch keeps it a segment."""
    v = ops.QWeight.__new__(ops.QWeight)
    v.__dict__.update(w.__dict__)
    v.rows = r1 - r0
    v.d16 = w.d16[r0:r1].clone() if own else w.d16[r0:r1]
    return v


@pytest.fixture(scope="module")
def case(gpu):
    """One random Q4_K weight [2304, 2048] with its f16 copy, activations [300, 2048], and the fp32 reference product
    (computed once, read-only); the smaller N are its leading rows."""
    rng = np.random.default_rng(7)
    n = max(NS)
    raw = Q.random_blocks(GGMLType.Q4_K, n * K, 0.05, rng)
    Wd = ops.QWeight(raw, GGMLType.Q4_K, n, K, "cpu").dense()
    w = ops.QWeight(raw, GGMLType.Q4_K, n, K, gpu)
    w.expand_dense()
    g = torch.Generator().manual_seed(11)
    x = torch.zeros(MPAD, K, dtype=ops.ACT_DTYPE)
    x[:M] = torch.randn(M, K, generator=g).to(ops.ACT_DTYPE)
    ref = (x[:M].float() @ Wd.t()).to(gpu)
    resid = torch.randn(M, n, generator=g).to(gpu)
    return dict(w=w, x=x.to(gpu), ref=ref, resid=resid)


def _nan_workspace(dev, ks, n):
    if ks > 1:
        ops._workspace(dev, ks * M * n)[:ks * M * n].fill_(float("nan"))


def _check(y, want, scale, what):
    err = (y - want).abs().max().item()     # NaN (an unwritten tile or slab) fails the comparison
    assert err <= RTOL * scale, f"{what}: err {err:.4g} vs {scale:.4g}"


@pytest.mark.parametrize("kern", KERNELS, ids=lambda k: "m%d_w%d_rt%d" % k)
def test_f32_and_add_epilogues(gpu, case, kern):
    mode, waves, rt = kern
    for n in NS:
        seg = [ops.Seg(_rows_of(case["w"], 0, n))]
        ref, resid = case["ref"][:, :n], case["resid"][:, :n]
        scale = ref.abs().max().item()
        for ks in KSS:
            what = f"mode {mode} waves {waves} rt {rt} ks {ks} N {n}"
            y = torch.full((MPAD, n), float("nan"), device=gpu)
            _nan_workspace(gpu, ks, n)
            ops.qgemv(seg, case["x"], y, M, mode=mode, waves=waves, rt=rt, ks=ks)
            _check(y[:M], ref, scale, what + " f32")
            y = torch.zeros(MPAD, n, device=gpu)
            y[:M] = resid
            _nan_workspace(gpu, ks, n)
            ops.qgemv(seg, case["x"], y, M, epi="add", mode=mode, waves=waves, rt=rt, ks=ks)
            _check(y[:M], resid + ref, scale, what + " add")


@pytest.mark.parametrize("kern", [(10, 8, 1), (10, 8, 2), (4, 16, 2), (5, 8, 4)], ids=lambda k: "m%d_w%d_rt%d" % k)
def test_slabs_into_add_rmsnorm(gpu, case, kern):
    """The production form of o / down: slabs -> fused reduce + residual add + RMSNorm. The residual stream against
    the reference product; the normalised f16 rows against the fp32 RMSNorm of the residual stream the kernel itself
    left (f16 rounding 2^-11 and the order of an fp32 sum: 2e-3 of the largest value)."""
    mode, waves, rt = kern
    eps = 1e-5
    for n in NS:
        seg = ops.Seg(_rows_of(case["w"], 0, n))
        ref, resid = case["ref"][:, :n], case["resid"][:, :n]
        scale = ref.abs().max().item()
        nw = torch.linspace(0.5, 1.5, n, device=gpu)
        for ks in (2, 3, 4, 8):
            what = f"mode {mode} waves {waves} rt {rt} ks {ks} N {n}"
            xr = torch.zeros(MPAD, n, device=gpu)
            xr[:M] = resid
            h = torch.full((MPAD, n), float("nan"), dtype=ops.ACT_DTYPE, device=gpu)
            _nan_workspace(gpu, ks, n)
            ops.qgemv_add_rmsnorm(seg, case["x"], xr, nw, h, M, 1.0, eps, cfg=(mode, waves, rt, ks))
            _check(xr[:M], resid + ref, scale, what + " residual")
            v = xr[:M]
            hr = v * torch.rsqrt(v.pow(2).mean(dim=1, keepdim=True) + eps) * nw
            herr = (h[:M].float() - hr).abs().max().item()
            assert herr <= 2e-3 * hr.abs().max().item(), f"{what} norm: err {herr:.4g}"


@pytest.mark.parametrize("kern", [(10, 8, 2), (4, 16, 2)], ids=lambda k: "m%d_w%d_rt%d" % k)
def test_three_segments_ks2(gpu, case, kern):
    """A Q|K|V-shaped launch: three segments (384 | 136 | 168 rows, the last two ending in ragged tiles), ks 2."""
    mode, waves, rt = kern
    cuts = (0, 384, 520, 688)
    segs = [ops.Seg(_rows_of(case["w"], a, b, own=True), a) for a, b in zip(cuts, cuts[1:])]
    y = torch.full((MPAD, cuts[-1]), float("nan"), device=gpu)
    _nan_workspace(gpu, 2, cuts[-1])
    ops.qgemv(segs, case["x"], y, M, mode=mode, waves=waves, rt=rt, ks=2)
    ref = case["ref"][:, :cuts[-1]]
    _check(y[:M], ref, ref.abs().max().item(), f"mode {mode} three segments ks 2")


@pytest.mark.parametrize("kern", [(10, 8, 2), (4, 16, 2)], ids=lambda k: "m%d_w%d_rt%d" % k)
def test_ks4_bits_do_not_depend_on_the_tile_placement(gpu, case, kern):
    """ks 4 at N = 688 and N = 2304 gives a 128-row tile different places in the grid (mode 10: group and XCD); the
    same tile launched alone, with the same ks, is always tile 0. Slices and slab sums are the same, so the outputs
    are bit-equal."""
    mode, waves, rt = kern
    for n in (688, 2304):
        y = torch.full((MPAD, n), float("nan"), device=gpu)
        ops.qgemv([ops.Seg(_rows_of(case["w"], 0, n))], case["x"], y, M, mode=mode, waves=waves, rt=rt, ks=4)
        for r0 in range(0, n, 128):
            r1 = min(r0 + 128, n)
            yt = torch.full((MPAD, r1 - r0), float("nan"), device=gpu)
            ops.qgemv([ops.Seg(_rows_of(case["w"], r0, r1))], case["x"], yt, M, mode=mode, waves=waves, rt=rt, ks=4)
            assert torch.equal(y[:M, r0:r1], yt[:M]), f"mode {mode} N {n}: rows {r0}..{r1} differ from the tile alone"
