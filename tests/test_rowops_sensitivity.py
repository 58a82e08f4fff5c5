"""The row kernels between the GEMMs and the attention -- the RoPE rotation with the paged K/V append (rope_kv_kernel,
the path-A GEMV epilogue, rope_store1 of hgemm.hip and hgemm10.hip, qknorm.hip), the RMSNorms and the residual adds
fused into them (rmsnorm, splitk_add_rmsnorm, moe_combine_norm) -- against fp64 references that are independent of ops
(tests/rowops.py), with inputs and a metric that notice ONE misplaced pair, row, slot, head or weight group.

What the older tests cannot see (test_old_inputs_cannot_see, on the CPU with their inputs and their metric, max err <=
rtol * max|ref|): with pos = 3 arange, base 1e4 and 3e-2, the last 8 pairs of every head taking the next pair's angle
moves the outputs by 0.028 of the maximum at M = 256 and passes; with slot = arange a kernel that writes K/V to its row
index computes the same caches; on unit rows with eps 1e-5 and 1e-2, dropping eps moves a norm by 3e-4 and eps times D
by 5e-3 of the maximum, and both pass. Here the same faults are rejected by 11466x, inf and 18504x / 1999x the bound.

Metric, per element and from the reference side only: |out - ref| <= round + ARITH * scale.
  round  half an ulp of a round-to-nearest store of ref: 2^-8 |ref| (bf16), 2^-11 |ref| with the subnormal floor 2^-25
         (f16), 2^-4 |ref| with the floor 2^-10 (e4m3, the reference clamped to +-448), 2^-24 |ref| (f32).
  ARITH  4 x EMU, EMU the largest ratio of a CPU emulation of the kernels' fp32 arithmetic against fp64 over this
         module's inputs (rowops: the references run in float32 -- fp32 products and sums, the slab order, the sum of
         squares as the kernels form it, 1 / sqrt of the fp32 mean), pinned by test_emulated_noise_bounds_tol:
           rotation  1.2e-7 of |x0 cos| + |x1 sin| (real 1.18, slabs 1.19, far 1.07, saturate 1.17, behind a GEMM 1.14)
           qk-norm   2.8e-7 of the same scale after the norm (tag 1.88, eps 2.71, real 2.51, saturate 2.65)
           norms     2.6e-7 of |ref| (scaled 1.73, eps 1.99, spike 2.23; after the add 2.01 / 2.01 / 2.52, integer 2.02)
         The factor 4 covers the summation order and rsqrtf. The scale of the rotation is |x0 cos| + |x1 sin|, so
         cancellation between the two products does not inflate it.
  The slab sum (order 0..ks-1) and the bias add are single fp32 additions, exactly defined: the references do them in
  fp32, so the slabs family (slabs 64x the size of their sum) is judged on the sum the kernel must have formed, and a
  bf16 V is asserted EQUAL to bf16 of that sum on every route with an exact projection.
  Everything that is no target keeps its sentinel exactly: unwritten slots, K/V of slot -1 rows, the columns past
  Hq*D of a wide q_out, rows past M, the columns past D of a strided norm output, the f32 qkv buffer of the fused
  routes. A truncating store fails the bound (test_truncating_store_fails_the_bound).
  Residual adds: the written-back x is within 2 fp32 roundings (MoE combine over k slots: 2k + 2) of its own size
  |x| + |update| and EQUAL on the integer family; h is then judged against the fp64 norm of the rows the kernel wrote,
  on the scale |ref| -- the two checks together are the operation, and h does not inherit a cancellation in x.
  Path A with the input norm fused in front: as test_weight_sensitivity.test_fused_norm_gemv_full, the projection of
  the fp64-normed, f16-rounded rows within 6.8e-4 of its own size B, carried through the rotation as B0 |cos| +
  B1 |sin|, plus the bf16 term. Its rows include mean squares of eps / 100, eps and 100 eps, its bias has the
  projection's size, and test_fused_norm_bound_still_rejects shows on the CPU that this wider bound still rejects the
  faults of the input norm (B1, B4, B5) and A2 - A8, A10 behind it by >= 10x.

Families. RoPE + append: tag (exact: a synthetic table whose entries are exact in the cache's format and name their
own (position, pair), heads of (2^e, 0) / (0, 2^e) with e naming row and head, V integer tags of (row, head, column),
bias and slabs on the same grid -- torch.equal on q, K and V; e4m3's 4 significant bits take a coarser table and two
passes), real (genuine tables: base 1e4, 5e5 with freq_factors, 1e6; unsorted and repeated positions with 0, 1 and the
last table row; one table of 131072 rows; Gaussian heads under a per-head log-uniform scale 2^-6 .. 2^6), saturate
(fp8: K and V at 447, 448, 449, 464, 480, 1e4 of both signs next to small values), slabs (ks 1..5, large slabs that
cancel), eps (qk-norm: heads with a mean square of eps / 100, eps, 100 eps for eps 1e-5 and 1e-6; norm weights of both
signs in every qk-norm case). Norms: scaled (rows under 2^-12 .. 2^12, weights of both signs, log-uniform 2^-3 .. 2^3,
another in every column), eps, spike (one element 2^12 times the rest, at column 0 and at column D - 1), integer
(integer base and slabs, alpha 1/2). GEMM-fused routes project {-1, 0, 1} activations with qblocks' integer weights: the
fp32 Q|K|V is exact in any split, the bound applies unchanged behind the GEMM.

Largest |out - ref| over the tolerance measured on the MI355X by the GPU tests below (bound: 1; a correct round-to-
nearest store alone reaches 1 at the bottom of a binade, the fp32 arithmetic adds about 1e-3 of it):

  route                                              bf16 cache                 fp8 cache
  rope_kv_kernel alone       real / slabs / tag      0.996 / 0.996 / equal      1.000 / 1.000 / equal, saturate 0.999
  qknorm.hip                 tag / eps / real        0.976 / 0.996 / 0.995      0.974 / 1.000 / 0.996, saturate 1.000
  path A epilogue            3 cfgs                  0.996                      (bf16 caches only)
  path A + norm (full rows)  3 cfgs                  0.936 each (the bound with the 6.8e-4 B term)
  path A + norm (partials)   M 1 / 3 / 16            0.657 / 0.635 / 0.797 (the same bound)
  dense epilogues            modes 4, 4, 5, 10, 10   0.996 each
  mode 14 (h14_rope)         copies / merged buffer  0.996 / 0.996 (three segments; one segment, the head and Q|K|V
                                                     boundaries inside a tile), 0.996 on DENSE's layouts
  split-K slabs              7 cfgs                  0.988 .. 0.996             0.988 .. 0.996
  rmsnorm f16 | f32          scaled / eps / spike    0.996 / 0.992 / 0.990 | 0.163 / 0.174 / 0.294
  splitk_add_rmsnorm         D 68 / 2052 / 8192      0.971 / 0.993 / 0.997 (h); x within 2 roundings, integer x equal
  qgemv_add_rmsnorm          9 split-K cfgs          x equal on all nine (modes 1, 2 and the dense 4, 4, 10, 14);
                                                     h 0.983 .. 0.996
  moe_combine_norm           k 1 / 2 / 3 / 8         0.998 / 0.997 / 0.996 / 0.997 (h); integer x equal

Bit-exact: tag on rope_kv_kernel for both cache types, all 60 + 120 cases (q, K and V); V = bf16 of the exact sum on
every bf16 route behind an exact projection (path A, dense epilogues, slabs, fallback); the integer x of
splitk_add_rmsnorm, qgemv_add_rmsnorm and moe_combine_norm. No kernel fault was found. Two faults of the CPU twins in
ops were: rope_kv and qk_norm_rope_kv did not saturate an e4m3 store (torch's cast gives NaN above 464 where kv_st4
gives +-448), and rope_kv could not take a bias with rows wider than their payload; both are fixed, and
test_cpu_twins_rope / test_cpu_twins_norms hold the twins to the same references, families and bounds as the kernels.

The GPU tests were also run once against two mutated builds: slot[t] replaced by the row index in rope_kv_kernel
failed all seven test_rope_kv_families cases and test_qkv_rope_fallback_is_seen, eps dropped in rmsnorm_kernel failed
test_rmsnorm_families[f16] and nothing else. Mode 14's own RoPE code was mutated the same way later (h14_rope: the row
index in place of slot[...]): test_qkv_rope_dense_epilogues[m14w8r2k1] and both test_qkv_rope_mode14_layouts cases
failed.

Route proof: every ops.qkv_rope_kv case hands in an f32 qkv buffer full of the sentinel; the epilogue and slab routes
must leave it untouched, the fallback (projection, then the RoPE kernel) must fill it with the exact product
(test_qkv_rope_fallback_is_seen: fuse_rope off, an fp8 cache on path A, NEOX pairing).

Fault models (test_fault_models_are_rejected, test_norm_fault_models_are_rejected: applied to the reference and stored
round-to-nearest; each is rejected by >= 10x the tolerance in at least one family -- the weakest: B3 first group
counted twice 599x, A7 bias omitted on V with the fp8 cache 1644x -- and changes the tag / integer outputs wherever it
changes the mathematical result):
  A1 one 4-column group, or the last 8 pairs of a head, with the next pair's angle   A2 table row p +- 1; the
  neighbouring token's position   A3 sin sign flipped; cos and sin exchanged   A4 the other pairing   A5 last K head
  not rotated; first V head rotated; K head written to head h ^ 1   A6 row index in place of slot[t]; the neighbouring
  row's slot; a slot -1 row written to slot 0, the last slot, its row index   A7 bias after the rotation; of the
  neighbouring pair; omitted on V   A8 a slab dropped; doubled; later slabs one row off   A9 fp8 without the clamp
  A10 Q written with stride Hq*D into a wider q_out
  B1 eps dropped; added after the root; times D   B2 mean over the width rounded up to 1024 / 2048   B3 last float4
  group left out of the sum; first counted twice   B4 weight of group i +- 4; no weight   B5 statistic of the
  neighbouring row   B6 slab dropped / doubled; alpha also on the base; alpha omitted; h from the row before the add; x
  not written back   B7 combine weight of the neighbouring slot; expert row of the neighbouring token; last slot dropped
(fault, route) pairs where no exact output can change: A9 on tag (its values stay below 448: the saturate family
rejects it, by inf); every A fault on the qk-norm route and on the path-A route with a fused input norm (the norm is not
exact: tag runs to the bound there, and the real / eps families reject by >= 10x); the rotation faults A1 - A4 behind a
GEMM (the projection decides x: no tag inputs, only V is exact -- they are rejected through the real tables); A5 head
h ^ 1 with one K head, A2 / A6 / A8 neighbouring rows at T = 1, A10 where q_out is not wider; B1 - B5 and B6 "h from the
row before the add" (no norm output is exact; they never touch x).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import qblocks as QB
import rowops as R
from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType

BF16, FP8, F16, F32, SENT = R.BF16, R.FP8, R.F16, R.F32, R.SENT
# largest emulated fp32-arithmetic ratios over this module's inputs (test_emulated_noise_bounds_tol)
EMU = {"rope": 1.2e-7, "qknorm": 2.8e-7, "norm": 2.6e-7}
ARITH = {k: 4 * v for k, v in EMU.items()}
NORM_GEMV_TOL = 6.8e-4          # test_weight_sensitivity.TOL["full"]: the bound of test_fused_norm_gemv_full

TS, HEADS, DS = (1, 3, 17, 70), ((4, 2), (5, 1)), (64, 96, 128)
TABLES = (dict(base=1e4), dict(base=5e5, ff=True), dict(base=1e6))
FAR = dict(fam="real", T=17, Hq=4, Hkv=2, D=128, base=5e5, ff=True, P=131072, seed=7)      # positions up to 131071


def _key(**kw):
    return tuple(sorted(kw.items()))


def alone_params(kv):
    """The cases of ops.rope_kv alone for one cache type: every (D, ks, neox, bias), T and the head split walking
    through them (test_case_lists_cover pins the pairs that occur); tag in every pass; the far table once."""
    out = []
    fams = ["tag", "real", "slabs"] + (["saturate", "tag"] if kv == FP8 else [])
    for f, fam in enumerate(fams):
        for i, (D, ks, neox, bias) in enumerate(itertools.product(DS, (1, 2, 3, 4, 5), (False, True), (False, True))):
            j = i + i // 4 + i // 20
            Hq, Hkv = HEADS[(i // 2 + i // 4 + i // 20) % 2]
            kw = dict(fam=fam, kv=kv, T=TS[j % 4], Hq=Hq, Hkv=Hkv, D=D, ks=ks, neox=neox, bias=bias, seed=f)
            if fam == "tag":
                kw["var"] = int(f > 0)
            elif fam != "saturate":
                kw.update(TABLES[i % 3])
            out.append(_key(**kw))
    out.append(_key(kv=kv, **FAR))
    return out


def qk_params(kv):
    """ops.qk_norm_rope_kv: what test_qwen3_gpu.py lacks -- tag tables, heads around eps, saturating K / V, weights
    of both signs (every case here)."""
    out = []
    fams = [("tag", 1e-6), ("eps", 1e-5), ("eps", 1e-6), ("real", 1e-6)] + ([("saturate", 1e-6)] if kv == FP8 else [])
    for f, (fam, eps) in enumerate(fams):
        for i, (D, neox, ks) in enumerate(itertools.product((64, 128), (False, True), (1, 5))):
            Hq, Hkv = HEADS[(i + i // 2) % 2]
            out.append(_key(fam=fam, kv=kv, T=(3, 17)[(i + i // 4) % 2], Hq=Hq, Hkv=Hkv, D=D, ks=ks, neox=neox, qk=eps,
                            seed=20 + f, base=1e6))
    return out


@functools.lru_cache(maxsize=None)
def _rope(key):
    """(case, fp64 reference) of one parameter set: built once, shared by the CPU and the GPU tests, never changed."""
    c = R.rope_case(**dict(key))
    return c, R.rope_ref(c)


# --------------------------------------------------------------------------------------------- GEMM-fused inputs

QKV_K = 512
QKV_TYPES = (GGMLType.Q4_K, GGMLType.Q4_K, GGMLType.Q6_K)


@functools.lru_cache(maxsize=None)
def _proj(Hq, Hkv, D):
    """Q | K | V weights of the integer family (raw blocks, rows, the exact dequantised matrix [ncol, K])."""
    rows = (Hq * D, Hkv * D, Hkv * D)
    raws = [QB.structured_blocks(t, r, QKV_K, "integer", np.random.default_rng(100 * Hq + D + i))
            for i, (t, r) in enumerate(zip(QKV_TYPES, rows))]
    W = np.concatenate([Q.dequantize(raw, t, (r, QKV_K)).astype(np.float64)
                        for raw, t, r in zip(raws, QKV_TYPES, rows)])
    return raws, rows, W


@functools.lru_cache(maxsize=None)
def _acts(pad, K=QKV_K, seed=3):
    return (torch.randint(0, 3, (pad, K), generator=torch.Generator().manual_seed(seed)) - 1).to(ops.ACT_DTYPE)


def _pad64(M):
    return (M + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _gemm(M, Hq, Hkv, D, bias, kv=BF16, table=0):
    """The rope case behind a GEMM: activations in {-1, 0, 1}, integer weights -- the fp32 Q|K|V is exact, so it
    stands as the single slab of the case; genuine table, unsorted positions, permuted slots, padding rows."""
    W = _proj(Hq, Hkv, D)[2]
    xd = _acts(_pad64(M))[:M].double().numpy()
    qkv = xd @ W.T
    assert float((np.abs(xd) @ np.abs(W).T).max()) * 8 < 2.0 ** 24          # unit 2^-3: every partial sum exact
    c = R.rope_case("real", kv, M, Hq, Hkv, D, bias=bias, seed=40 + table, **TABLES[table])
    ncol = (Hq + 2 * Hkv) * D
    c["slabs"] = torch.from_numpy(qkv.astype(np.float32))[None].contiguous()
    assert c["slabs"].shape == (1, M, ncol)
    if bias:
        c["bias"] = c["bias"] * float(qkv.std())          # a bias of the projection's own size
    return c, R.rope_ref(c)


def _normed_gemm(M, Hq, Hkv, D, xf, nw, eps, table=0, fault=None):
    """Path A with the input RMSNorm fused in front, judged as test_weight_sensitivity.test_fused_norm_gemv_full:
    the product of the fp64-normed, f16-rounded rows with the exact weights, every projection within NORM_GEMV_TOL
    of its own size B = |xn| @ |W|^T -- carried through the rotation as B0 |cos| + B1 |sin| (V: B itself)."""
    W = _proj(Hq, Hkv, D)[2]
    xn = torch.from_numpy(R.rms_ref(xf[:M].numpy(), nw.numpy(), eps, fault=fault)).to(ops.ACT_DTYPE).double().numpy()
    c = dict(R.rope_case("real", BF16, M, Hq, Hkv, D, bias=True, seed=50 + table, **TABLES[table]))
    c["slabs"] = torch.from_numpy((xn @ W.T).astype(np.float32))[None].contiguous()
    c["bias"] = c["bias"] * float(c["slabs"].std())        # a bias of the projection's own size
    ref = R.rope_ref(c)
    rb = R.rope_ref({**c, "slabs": torch.from_numpy((np.abs(xn) @ np.abs(W).T).astype(np.float32))[None].contiguous(),
                     "cs": c["cs"].abs(), "bias": None})
    ref["qs"], ref["ks"], ref["vs"] = rb["qs"], rb["ks"], np.where(rb["vw"], rb["v"], 0.0)
    return c, ref


# ------------------------------------------------------------------------------------------------- norm inputs

NORM_DS = (4, 68, 1024, 2048, 2052, 5120, 8192)


@functools.lru_cache(maxsize=None)
def _norm_case(fam, D, eps=1e-5, seed=0):
    """(x [M, D] f32, w [D] f32, eps, fp64 reference) of ops.rmsnorm."""
    g = torch.Generator().manual_seed(17 * D + seed)
    x, w = R.norm_rows(fam, D, g, eps), R.norm_weights(D, g)
    return x, w, eps, R.rms_ref(x.numpy(), w.numpy(), eps)


def _norm_keys():
    return [(fam, D, eps) for D in NORM_DS for fam, eps in (("scaled", 1e-5), ("eps", 1e-5), ("eps", 1e-6),
                                                            ("spike", 1e-6))]


@functools.lru_cache(maxsize=None)
def _add_case(fam, D, ks, eps=1e-5):
    """x += alpha sum_k slab_k, then the norm: base rows, ks slabs of the rows' own size, alpha, weights, and the
    reference residual with its size. The rows AFTER the add are the family's (their mean square for eps, the spike);
    integer: integer base and slabs, alpha 1/2 -- the written-back x is exact."""
    g = torch.Generator().manual_seed(31 * D + ks)
    w = R.norm_weights(D, g)
    if fam == "integer":
        base, alpha = R.norm_rows(fam, D, g), 0.5
        slabs = torch.randint(-500, 501, (ks, base.shape[0], D), generator=g).float()
    else:
        want, alpha = R.norm_rows(fam, D, g, eps), 0.7
        rms = want.pow(2).mean(1, keepdim=True).sqrt()
        slabs = torch.randn(ks, want.shape[0], D, generator=g) * rms
        base = (want.double() - alpha * slabs.double().sum(0)).float()
    xr, size = R.add_ref(base.numpy(), slabs.numpy(), alpha)
    return dict(fam=fam, base=base, slabs=slabs, alpha=alpha, w=w, eps=eps, x=xr, size=size)


ADD_KEYS = [(fam, D, ks, eps) for D in (68, 2052, 8192) for ks in (1, 2, 3, 4, 5)
            for fam, eps in (("scaled", 1e-5), ("eps", 1e-5), ("eps", 1e-6), ("spike", 1e-5), ("integer", 1e-5))]


@functools.lru_cache(maxsize=None)
def _moe_case(fam, T, k, D, eps=1e-5):
    """resid += alpha sum_j w_j y_j, then the norm. integer: integer rows, integer weights, alpha 1/2 (exact)."""
    g = torch.Generator().manual_seed(13 * D + 7 * k + T)
    nw = R.norm_weights(D, g)
    if fam == "integer":
        alpha = 0.5
        resid = torch.randint(-1000, 1001, (T, D), generator=g).float()
        y = torch.randint(-500, 501, (T * k, D), generator=g).float()
        wt = torch.randint(1, 5, (T, k), generator=g).float()
    else:
        want, alpha = R.norm_rows(fam, D, g, eps, M=T), 0.7
        T = want.shape[0]
        rms = want.pow(2).mean(1, keepdim=True).sqrt()
        y = (torch.randn(T, k, D, generator=g) * rms[:, None]).reshape(T * k, D)
        wt = torch.rand(T, k, generator=g) + 0.05 * torch.arange(1, k + 1)
        resid = (want.double() - alpha * (wt.double()[:, :, None] * y.double().view(T, k, D)).sum(1)).float()
    xr, size = R.moe_ref(resid.numpy(), y.numpy(), wt.numpy(), alpha)
    return dict(fam=fam, T=T, k=k, resid=resid, y=y, wt=wt, alpha=alpha, w=nw, eps=eps, x=xr, size=size)


MOE_KEYS = [(fam, T, k, D, eps) for k in (1, 2, 3, 8) for D in (68, 1024, 4100, 8192)
            for fam, T, eps in (("scaled", 1, 1e-5), ("scaled", 5, 1e-5), ("integer", 5, 1e-5), ("integer", 1, 1e-5),
                                ("eps", 3, 1e-6), ("spike", 2, 1e-5))]


def _judge_addnorm(what, x_out, h_out, c, nround, hdt=F16):
    """The written-back rows against the reference residual (integer: equal), and h against the fp64 norm of the
    rows the kernel wrote -- the two together are the operation, and neither inherits the other's cancellation."""
    M, D = c["x"].shape
    x_out, h_out = np.asarray(x_out, np.float64), np.asarray(h_out, np.float64)
    rx = R.x_ratio(x_out[:M, :D], c["x"], c["size"], 0 if c["fam"] == "integer" else nround)
    assert (x_out[M:] == SENT).all() and (x_out[:, D:] == SENT).all(), (what, "x past the rows was written")
    rh, where = R.rms_ratio(h_out, R.rms_ref(x_out[:M, :D], c["w"].numpy(), c["eps"]), hdt, ARITH["norm"])
    return rx, rh, where


# ------------------------------------------------------------------------------------------------------ CPU tests

def test_case_lists_cover():
    """The walk through (T, head split) against (D, ks, neox, bias) meets every pair the issue names."""
    for kv in (BF16, FP8):
        ps = [dict(k) for k in alone_params(kv)]
        for a, b, n in (("D", "T", 12), ("D", "Hq", 6), ("ks", "T", 20), ("ks", "D", 15), ("neox", "Hq", 4),
                        ("bias", "Hq", 4), ("T", "Hq", 8), ("neox", "D", 6), ("bias", "ks", 10)):
            for fam in {p["fam"] for p in ps}:
                assert len({(p[a], p.get(b, False)) for p in ps if p["fam"] == fam and "P" not in p}) == n, (fam, a, b)
        assert any(p.get("P") == 131072 for p in ps)
        for p in ps:
            c = _rope(_key(**p))[0]
            if p["T"] >= 3:
                assert int((c["slot"] < 0).sum()) == 2 and len(set(c["slot"].tolist())) == p["T"] - 1
            assert int(c["pos"][0]) == 0 and (p["T"] < 5 or int(c["pos"][3]) == c["cs"].shape[0] - 1)
    far = _rope(_key(kv=BF16, **FAR))[0]
    assert int(far["pos"].max()) == 131071
    for (Hq, Hkv), hd in itertools.product(HEADS14, (64, 128)):
        for edge in (Hq * hd, (Hq + Hkv) * hd):
            assert edge % 48, (Hq, Hkv, hd, edge)          # inside a wave's 48-row half, hence inside a 96-row tile


def test_tag_family_is_exact():
    """Every tag output is one table entry times a power of two, or an integer: exact in the cache's format (the
    stored reference IS the reference), inside e4m3's normal range for the fp8 cache, and neighbouring coordinates
    of the table differ."""
    n = 0
    for kv in (BF16, FP8):
        for key in alone_params(kv):
            if dict(key)["fam"] != "tag":
                continue
            c, r = _rope(key)
            st = R.rope_stored(r, kv)
            assert all(np.array_equal(st[m], r[m]) for m in "qkv"), dict(key)
            if kv == FP8:
                kk = np.abs(r["k"][r["kw"]])
                assert kk[kk > 0].min() >= 2.0 ** -6 and kk.max() <= 448
            n += 1
        cs = R.tag_table(kv, 128).numpy()
        assert (cs[1:] != cs[:-1]).any(-1).all() and (cs[:, 1:] != cs[:, :-1]).any(-1).all()
    assert n == 60 + 120


def _noise():
    rope = {}
    for key in alone_params(BF16) + alone_params(FP8):
        p = dict(key)
        if p["fam"] != "tag":
            name = "far" if "P" in p else p["fam"]
            rope[name] = max(rope.get(name, 0.0), R.rope_noise(_rope(key)[0]))
    for args in ((16, 4, 2, 128, True), (64, 5, 1, 64, True)):
        rope["gemm"] = max(rope.get("gemm", 0.0), R.rope_noise(_gemm(*args)[0]))
    qk = {}
    for key in qk_params(BF16) + qk_params(FP8):
        p = dict(key)
        qk[p["fam"]] = max(qk.get(p["fam"], 0.0), R.rope_noise(_rope(key)[0]))
    norm = {}

    def nz(fam, x, w, eps, ref):
        e = R.rms_ref(x, w, eps, np.float32)
        norm[fam] = max(norm.get(fam, 0.0), float((np.abs(e - ref) / np.abs(ref))[ref != 0].max()))

    for k in _norm_keys():
        x, w, eps, ref = _norm_case(*k)
        nz(k[0], x.numpy(), w.numpy(), eps, ref)
    for k in ADD_KEYS:
        c = _add_case(*k)
        x32 = c["x"].astype(np.float32)
        nz("add " + k[0], x32, c["w"].numpy(), c["eps"], R.rms_ref(x32, c["w"].numpy(), c["eps"]))
    return rope, qk, norm


def test_emulated_noise_bounds_tol():
    """EMU is the largest ratio of the emulated fp32 arithmetic (fp32 products and sums, the slab order, 1 / sqrt of
    the fp32 mean) against fp64 over this module's inputs, within a factor 2 below the constant: the measurement,
    not a guess. Scale: |x0 cos| + |x1 sin| for the rotation, |ref| for the norms."""
    rope, qk, norm = _noise()
    for name, per in (("rope", rope), ("qknorm", qk), ("norm", norm)):
        print(f"emulated noise {name}: " + " ".join(f"{k}={v:.2e}" for k, v in per.items()))
        worst = max(per.values())
        assert EMU[name] / 2 <= worst <= EMU[name], (name, worst)


def test_truncating_store_fails_the_bound():
    """The emulated fp32 result stored round-to-nearest is within the bound; the same result stored by truncation
    is not (bf16 Q and K of the rotation, f16 rows of the norm)."""
    for key in [k for k in alone_params(BF16) if dict(k)["fam"] == "real"][:12]:
        c, r = _rope(key)
        e = R.rope_ref(c, np.float32)
        assert R.rope_ratio(R.rope_stored(e, BF16), r, BF16, ARITH["rope"])[0] <= 1.0
        assert R.rope_ratio(R.rope_stored(e, BF16, trunc=True), r, BF16, ARITH["rope"])[0] > 1.0
    for k in _norm_keys()[4:12]:
        x, w, eps, ref = _norm_case(*k)
        e = R.rms_ref(x.numpy(), w.numpy(), eps, np.float32)
        assert R.rms_ratio(R.store(e, F16), ref, F16, ARITH["norm"])[0] <= 1.0
        assert R.rms_ratio(R.store(e, F16, trunc=True), ref, F16, ARITH["norm"])[0] > 1.0


def _fault_cases(kv):
    keys = [_key(fam="tag", kv=kv, T=17, Hq=4, Hkv=2, D=128, ks=3, neox=False, bias=True, var=0),
            _key(fam="tag", kv=kv, T=17, Hq=4, Hkv=2, D=64, ks=2, neox=True, bias=True, var=1),
            _key(fam="real", kv=kv, T=17, Hq=4, Hkv=2, D=128, ks=2, neox=False, bias=True, base=1e4),
            _key(fam="real", kv=kv, T=70, Hq=4, Hkv=2, D=96, ks=1, neox=True, bias=True, base=1e6),
            _key(fam="slabs", kv=kv, T=17, Hq=4, Hkv=2, D=64, ks=5, neox=False, bias=False, base=1e4),
            _key(fam="eps", kv=kv, T=17, Hq=4, Hkv=2, D=128, ks=2, neox=False, qk=1e-6, base=1e6),
            _key(kv=kv, **FAR)]
    if kv == FP8:
        keys.append(_key(fam="saturate", kv=kv, T=17, Hq=4, Hkv=2, D=128, ks=1, neox=False, bias=False))
    return keys


ROPE_FAULT_IDS = "A1 A2 A3 A4 A5 A6 A7 A8 A10".split()


@pytest.mark.parametrize("kv", [BF16, FP8], ids=["bf16", "fp8"])
def test_fault_models_are_rejected(kv):
    """Every RoPE / append fault model, applied to the reference and stored round-to-nearest: at least one family
    exceeds the tolerance by >= 10x, and on the tag cases the stored outputs differ wherever the mathematical result
    does -- using the reference alone."""
    res, tagged = {}, {}
    for key in _fault_cases(kv):
        c, r = _rope(key)
        arith = ARITH["qknorm" if c["qk"] is not None else "rope"]
        good = R.rope_stored(r, kv)
        assert R.rope_ratio(good, r, kv, arith)[0] <= 1.0
        for name, c2, kw, noclamp in R.rope_faults(c):
            f = R.rope_ref(c2, **kw)
            bad = R.rope_stored(f, kv, clamp=not noclamp)
            if c["fam"] == "tag":
                moved = any(not np.array_equal(f[m], r[m]) for m in "qkv")
                seen = any(not np.array_equal(bad[m], good[m], equal_nan=True) for m in "qkv")
                assert seen == moved, (name, dict(key))
                tagged[name] = tagged.get(name, False) or seen
            else:
                res[name] = max(res.get(name, 0.0), R.rope_ratio(bad, r, kv, arith)[0])
    assert sorted({n[:3].strip() for n in res}) == sorted(ROPE_FAULT_IDS + (["A9"] if kv == FP8 else []))
    for name, worst in res.items():
        print(f"{'bf16' if kv == BF16 else 'fp8'} {name}: rejected by {worst:.0f}x tolerance; changes tag outputs: "
              f"{tagged.get(name, False)}")
        assert worst >= 10.0, name
        assert tagged.get(name, False) or name.startswith("A9"), name       # A9: tag values stay below 448


def test_norm_fault_models_are_rejected():
    """B1 - B7 on the norm references: each is rejected by >= 10x the tolerance in at least one family (h, or the
    written-back x), and B6 / B7 change the integer family's x wherever they change the residual."""
    res = {}
    for fam, D, eps in _norm_keys():
        if D not in (68, 2052):
            continue
        x, w, _, ref = _norm_case(fam, D, eps)
        for f in R.RMS_FAULTS:
            bad = R.store(R.rms_ref(x.numpy(), w.numpy(), eps, fault=f), F16)
            res[f] = max(res.get(f, 0.0), R.rms_ratio(bad, ref, F16, ARITH["norm"])[0])
    ints = {}
    for k in ADD_KEYS:
        if k[1] != 2052 or k[2] not in (1, 3):
            continue
        c = _add_case(*k)
        base, w = c["base"].numpy(), c["w"].numpy()
        for f in R.ADD_FAULTS:
            xb = R.add_ref(base, c["slabs"].numpy(), c["alpha"], fault=f)[0].astype(np.float32).astype(np.float64)
            xo = base.astype(np.float64) if f == "B6 x not written back" else xb
            hb = R.store(R.rms_ref(base if f == "B6 h computed from the row before the add" else xb, w, c["eps"]), F16)
            rx, rh, _ = _judge_addnorm(f, xo, hb, c, 2)
            if c["fam"] == "integer":
                ints[f] = ints.get(f, False) or rx > 0
            else:
                res[f] = max(res.get(f, 0.0), rx, rh)
    for k in MOE_KEYS:
        if k[3] != 4100 or k[2] not in (2, 3):
            continue
        c = _moe_case(*k)
        for f in R.MOE_FAULTS:
            xb = R.moe_ref(c["resid"].numpy(), c["y"].numpy(), c["wt"].numpy(), c["alpha"], fault=f)[0]
            xb = xb.astype(np.float32).astype(np.float64)
            rx, rh, _ = _judge_addnorm(f, xb, R.store(R.rms_ref(xb, c["w"].numpy(), c["eps"]), F16), c, 2 * c["k"] + 2)
            if c["fam"] == "integer":
                ints[f] = ints.get(f, False) or rx > 0
            else:
                res[f] = max(res.get(f, 0.0), rx, rh)
    assert sorted(res) == sorted(R.RMS_FAULTS + R.ADD_FAULTS + R.MOE_FAULTS)
    for f, worst in res.items():
        print(f"{f}: rejected by {worst:.0f}x tolerance" + (f"; changes integer x: {ints[f]}" if f in ints else ""))
        assert worst >= 10.0, f
    assert all(v for f, v in ints.items() if f != "B6 h computed from the row before the add"), ints


def test_fused_norm_bound_still_rejects():
    """Path A with the input norm in front is judged on the wider bound of test_fused_norm_gemv_full (6.8e-4 of the
    projection's own size B, through the rotation): faults of the input norm (eps, weight group, the neighbouring row's
    statistic) and of the rotation and the append behind it are still rejected by >= 10x."""
    M, Hq, Hkv, D, eps = 16, 4, 2, 128, 1e-5
    xf, nw = _norm_inputs(eps, 60)
    c, ref = _normed_gemm(M, Hq, Hkv, D, xf, nw, eps)
    assert R.rope_ratio(R.rope_stored(ref, BF16), ref, BF16, NORM_GEMV_TOL)[0] <= 1.0
    for f in ("B1 eps dropped", "B1 eps times D", "B1 eps added after the root", "B4 no weight",
              "B4 weight of the neighbouring group (i + 4)", "B5 statistic of the neighbouring row"):
        bad = R.rope_stored(_normed_gemm(M, Hq, Hkv, D, xf, nw, eps, fault=f)[1], BF16)
        r = R.rope_ratio(bad, ref, BF16, NORM_GEMV_TOL)[0]
        print(f"fused norm, {f}: rejected by {r:.0f}x tolerance")
        assert r >= 10.0, f
    seen = set()
    for name, c2, kw, _ in R.rope_faults(c):
        r = R.rope_ratio(R.rope_stored(R.rope_ref(c2, **kw), BF16), ref, BF16, NORM_GEMV_TOL)[0]
        print(f"fused norm, {name}: rejected by {r:.0f}x tolerance")
        if r >= 10.0:
            seen.add(name[:3].strip())
    assert seen >= {"A2", "A3", "A4", "A5", "A6", "A7", "A8", "A10"}, seen


def test_old_inputs_cannot_see():
    """The gap these families close, on the CPU with the existing tests' inputs and metric (max err <= rtol * max|ref|):
    test_kernels_gpu._qkv_rope_case (pos = 3 arange, base 1e4, D = 128, slot = arange, 3e-2) passes A1 on the last 8
    pairs at M = 256 and cannot tell slot[t] from t; test_rmsnorm_embed (D = 1024, eps 1e-5, unit rows, 1e-2) passes
    eps dropped and eps times D."""
    M, Hq, Hkv, D = 256, 4, 2, 128
    g = torch.Generator().manual_seed(0)
    c = dict(fam="old", kv=BF16, T=M, Hq=Hq, Hkv=Hkv, D=D, ks=1, neox=False, qk=None, qw=None, kw=None, bias=None,
             slabs=1.1 * torch.randn(1, M, (Hq + 2 * Hkv) * D, generator=g), pos=3 * torch.arange(M, dtype=torch.int32),
             slot=torch.arange(M, dtype=torch.int32), cs=R.real_table(4 * M, D, 1e4), nslot=M, ldq=Hq * D)
    r = R.rope_ref(c)
    faults = {n: (c2, kw) for n, c2, kw, _ in R.rope_faults(c)}
    seen = 0
    for name in ("A1 last 8 pairs of a head take the next pair's angle", "A6 row index in place of slot[t]"):
        c2, kw = faults[name]
        f = R.rope_stored(R.rope_ref(c2, **kw), BF16)
        old = max(np.abs(f[m] - r[m]).max() / np.abs(r[m]).max() for m in "qkv")
        print(f"old inputs, {name}: {old:.4f} of the largest value (limit 0.03); new metric "
              f"{R.rope_ratio(f, r, BF16, ARITH['rope'])[0]:.1f}x tolerance")
        assert old <= 3e-2, name
        seen += 1
    assert np.array_equal(R.rope_ref(faults["A6 row index in place of slot[t]"][0])["k"], r["k"])
    x = torch.randn(5, 1024, generator=g).numpy()
    w = torch.randn(1024, generator=g).numpy()
    ref = R.rms_ref(x, w, 1e-5)
    for f in ("B1 eps dropped", "B1 eps times D"):
        old = np.abs(R.store(R.rms_ref(x, w, 1e-5, fault=f), F16) - ref).max() / np.abs(ref).max()
        print(f"old inputs, {f}: {old:.2e} of the largest value (limit 0.01)")
        assert old <= 1e-2, f
        seen += 1
    assert seen == 4


def _outs(q, kc, vc, T):
    return dict(q=q[:T].cpu().float().double().numpy(), k=kc.cpu().float().double().numpy(),
                v=vc.cpu().float().double().numpy())


def _bufs(c, dev, rows=None):
    q = torch.full((rows or c["T"], c["ldq"]), SENT, dtype=torch.bfloat16, device=dev)
    kc = torch.full((c["nslot"], c["Hkv"], c["D"]), SENT, device=dev).to(c["kv"])
    return q, kc, kc.clone()


def _judge_rope(what, c, out, ref, arith, worst=None, exact_x=True):
    r, where = R.rope_ratio(out, ref, c["kv"], arith)
    if worst is not None:
        worst[0] = max(worst[0], r)
    assert r <= 1.0, (what, f"{r:.3f} of the tolerance at {where}")
    if c["fam"] == "tag" and c["qk"] is None:
        for m in "qkv":
            assert np.array_equal(out[m], ref[m]), (what, "tag outputs must be EQUAL", m,
                                                    np.argwhere(out[m] != ref[m])[:4].tolist())
    if c["kv"] == BF16 and exact_x:         # V is a plain store of the fp32 sum: bf16(x), wherever x is exact
        assert np.array_equal(out["v"], R.store(ref["v"], BF16)), (what, "V is not bf16 of the fp32 sum")


@pytest.mark.parametrize("kv", [BF16, FP8], ids=["bf16", "fp8"])
def test_cpu_twins_rope(kv):
    """The CPU twins ops.rope_kv (ks = 1: it takes no slabs) and ops.qk_norm_rope_kv against the same references,
    families and bound as the kernels; tag equal; saturating values clamp as kv_st4 does."""
    n = 0
    for key in alone_params(kv) + qk_params(kv):
        c, ref = _rope(key)
        if c["ks"] > 1 and c["qk"] is None or c["cs"].shape[0] > 4096:
            continue
        q, kc, vc = _bufs(c, "cpu")
        s = c["slabs"]
        if c["qk"] is None:
            ops.rope_kv(s[0], c["pos"], c["slot"], c["cs"], q, kc, vc, c["T"], c["Hq"], c["Hkv"], c["D"], c["neox"],
                        c["bias"])
        else:
            ops.qk_norm_rope_kv(s.view(-1, s.shape[2]), c["pos"], c["slot"], c["cs"], q, kc, vc, c["T"], c["Hq"],
                                c["Hkv"], c["D"], c["qw"], c["kw"], c["qk"], c["neox"], ks=c["ks"],
                                slab=c["T"] * s.shape[2])
        _judge_rope(dict(key), c, _outs(q, kc, vc, c["T"]), ref, ARITH["qknorm" if c["qk"] is not None else "rope"])
        n += 1
    assert n >= 40


def test_cpu_twins_norms():
    """ops.rmsnorm and ops.moe_combine_norm on the CPU against the same references, families and bounds."""
    for k in _norm_keys():
        x, w, eps, ref = _norm_case(*k)
        for dt in (F16, F32):
            out = torch.full((x.shape[0] + 2, x.shape[1]), SENT, dtype=dt)
            ops.rmsnorm(x, w, out, x.shape[0], eps)
            r, where = R.rms_ratio(out.double().numpy(), ref, dt, ARITH["norm"])
            assert r <= 1.0, (k, dt, r, where)
    for k in MOE_KEYS:
        c = _moe_case(*k)
        x = torch.full((c["T"] + 1, c["x"].shape[1]), SENT)
        x[:c["T"]] = c["resid"]
        h = torch.full(x.shape, SENT, dtype=F16)
        ops.moe_combine_norm(c["y"], c["wt"].reshape(-1), c["T"], c["k"], x, c["alpha"], c["w"], c["eps"], h)
        rx, rh, where = _judge_addnorm(k, x.double().numpy(), h.double().numpy(), c, 2 * c["k"] + 2)
        assert rx <= 1.0 and rh <= 1.0, (k, rx, rh, where)


# ------------------------------------------------------------------------------------------------------ GPU tests

_TABLES = {}


def _dev_table(c, dev):
    k = id(c["cs"])
    if k not in _TABLES:
        _TABLES[k] = (c["cs"], c["cs"].to(dev))          # the host tensor is kept so that its id stays its own
    return _TABLES[k][1]


def _launch_rope(c, dev):
    """One case straight into the stand-alone kernels: nls_rope_kv[8] (through ops.rope_kv at ks = 1) or
    ops.qk_norm_rope_kv; strided slab rows, a q_out wider than Hq * D."""
    T, Hq, Hkv, D = c["T"], c["Hq"], c["Hkv"], c["D"]
    q, kc, vc = _bufs(c, dev)
    s = c["slabs"].to(dev)
    ks, ld = s.shape[0], s.shape[2]
    pos, slot, cs = c["pos"].to(dev), c["slot"].to(dev), _dev_table(c, dev)
    bias = None if c["bias"] is None else c["bias"].to(dev)
    if c["qk"] is not None:
        ops.qk_norm_rope_kv(s.view(ks * T, ld), pos, slot, cs, q, kc, vc, T, Hq, Hkv, D, c["qw"].to(dev),
                            c["kw"].to(dev), c["qk"], c["neox"], ks=ks, slab=T * ld)
    elif ks == 1:
        ops.rope_kv(s[0], pos, slot, cs, q, kc, vc, T, Hq, Hkv, D, c["neox"], bias)
    else:
        ops._lib.check(ops._kv_fn("nls_rope_kv", kc)(s.data_ptr(), ld, ks, T * ld, ops._p(bias), pos.data_ptr(),
                                                     slot.data_ptr(), cs.data_ptr(), q.data_ptr(), q.stride(0),
                                                     kc.data_ptr(), vc.data_ptr(), T, Hq, Hkv, D, int(c["neox"]),
                                                     ops._stream_ptr(s)), "nls_rope_kv")
    return _outs(q, kc, vc, T)


def _fams(params):
    return sorted({dict(k)["fam"] for k in params})


@pytest.mark.gpu
@pytest.mark.parametrize("kv,fam", [(kv, f) for kv in (BF16, FP8) for f in _fams(alone_params(kv))],
                         ids=lambda v: v if isinstance(v, str) else ("bf16" if v == BF16 else "fp8"))
def test_rope_kv_families(gpu, kv, fam):
    """rope_kv_kernel alone: ks 1..5 (5: the run-time loop; the fp8 kernel always), both pairings, bias, D 64 / 96 /
    128, both head splits, T 1 .. 70, strided rows, a wide q_out, permuted slots with two padding rows."""
    worst = [0.0]
    for key in alone_params(kv):
        if dict(key)["fam"] == fam:
            c, ref = _rope(key)
            _judge_rope(dict(key), c, _launch_rope(c, gpu), ref, ARITH["rope"], worst)
    print(f"RO_RATIO rope_kv {'bf16' if kv == BF16 else 'fp8'} {fam} {worst[0]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kv", [BF16, FP8], ids=["bf16", "fp8"])
def test_qk_norm_rope_kv_families(gpu, kv):
    """qknorm.hip on what test_qwen3_gpu.py lacks: the tag table (to the bound: the norm is not exact), heads with a
    mean square around eps, saturating K / V, norm weights of both signs."""
    worst = {}
    for key in qk_params(kv):
        c, ref = _rope(key)
        w = [worst.get(c["fam"], 0.0)]
        _judge_rope(dict(key), c, _launch_rope(c, gpu), ref, ARITH["qknorm"], w)
        worst[c["fam"]] = w[0]
    print(f"RO_RATIO qknorm {'bf16' if kv == BF16 else 'fp8'} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


class _Proj:
    """Device copies of the integer Q | K | V weights of one head layout (dense: with their f16 copies)."""

    def __init__(self, dev):
        self.dev, self._w, self._keep = dev, {}, []

    def segs(self, Hq, Hkv, D, dense=False):
        """dense: True -- per-matrix f16 copies; "copies" -- the same, and no copy starts where the previous one ends
        (a launch merges copies that happen to be adjacent in memory: this keeps them three launch segments);
        "merged" -- the copies as consecutive rows of one buffer (QWeight.expand_dense_group: one launch segment,
        the Q|K and K|V boundaries inside its tiles)."""
        key = (Hq, Hkv, D, dense)
        if key not in self._w:
            raws, rows, _ = _proj(Hq, Hkv, D)
            ws = [ops.QWeight(raw, t, r, QKV_K, self.dev) for raw, t, r in zip(raws, QKV_TYPES, rows)]
            if dense == "merged":
                assert ops.QWeight.expand_dense_group(ws) == sum(rows) * QKV_K * 2
            elif dense:
                for w in ws:
                    w.expand_dense()
                for a, b in zip(ws, ws[1:]) if dense == "copies" else ():
                    if b.d16.data_ptr() == a.d16.data_ptr() + a.d16.numel() * 2:
                        self._keep.append(b.d16)          # stays allocated, so the clone lies elsewhere
                        b.d16 = b.d16.clone()
            self._w[key] = ws
        ws = self._w[key]
        return [ops.Seg(ws[0], 0), ops.Seg(ws[1], Hq * D), ops.Seg(ws[2], (Hq + Hkv) * D)]


@pytest.fixture(scope="module")
def proj(gpu):
    return _Proj(gpu)


def _run_qkv(dev, c, ref, segs, cfg, route, arith=None, norm=None, worst=None, **kw):
    """ops.qkv_rope_kv on one case. The f32 qkv buffer proves the route: the epilogue and the slab routes never touch
    it (it keeps its sentinel), the fallback (projection, then the RoPE kernel) fills it with the exact product."""
    M, Hq, Hkv, D = c["T"], c["Hq"], c["Hkv"], c["D"]
    pad, ncol = _pad64(M), (Hq + 2 * Hkv) * D
    x = torch.zeros(pad, QKV_K, dtype=ops.ACT_DTYPE, device=dev) if norm is not None else _acts(pad).to(dev)
    qkv = torch.full((pad, ncol), SENT, device=dev)
    q, kc, vc = _bufs(c, dev, rows=pad)
    pos = torch.zeros(pad, dtype=torch.int32)
    slot = torch.full((pad,), -1, dtype=torch.int32)
    pos[:M], slot[:M] = c["pos"], c["slot"]
    bias = None if c["bias"] is None else c["bias"].to(dev)
    ops.qkv_rope_kv(segs, x, qkv, pos.to(dev), slot.to(dev), _dev_table(c, dev), q, kc, vc, M, Hq, Hkv, D, c["neox"],
                    cfg=cfg, bias=bias, norm=norm, **kw)
    what = (route, cfg, M, Hq, Hkv, D)
    kept = bool((qkv == SENT).all())
    if route == "fallback":
        assert not kept and np.array_equal(qkv[:M].cpu().numpy(), c["slabs"][0].numpy()), (what, "fallback not taken")
        assert bool((qkv[M:] == SENT).all()), what
    else:
        assert kept, (what, "the f32 qkv buffer was written: not the route this case names")
    assert bool((q[M:].float() == SENT).all()), (what, "q rows past M were written")
    _judge_rope(what, c, _outs(q, kc, vc, M), ref, ARITH["rope"] if arith is None else arith, worst,
                exact_x=norm is None)


PATH_A = [(0, 4, 1, 1), (0, 8, 2, 1), (0, 8, 1, 1)]          # the mode-0 cfgs of test_qkv_rope_kv_fused


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", PATH_A, ids=lambda c: "m%dw%dr%dk%d" % c)
def test_qkv_rope_path_a(gpu, proj, cfg):
    """Path A, RoPE + append in the GEMV epilogue, behind an exact projection: M 1 .. 64, D 64 / 128, both head
    splits, with and without bias, three tables."""
    worst = [0.0]
    for i, (M, D, (Hq, Hkv), bias) in enumerate(itertools.product((1, 3, 16, 64), (64, 128), HEADS, (False, True))):
        c, ref = _gemm(M, Hq, Hkv, D, bias, BF16, i % 3)
        _run_qkv(gpu, c, ref, proj.segs(Hq, Hkv, D), cfg, "epilogue", worst=worst)
    print(f"RO_RATIO pathA m%dw%dr%dk%d {worst[0]:.3f}" % cfg)


@pytest.mark.gpu
def test_qkv_rope_fallback_is_seen(gpu, proj):
    """The route proof works: where the dispatcher cannot fuse (NEOX pairing, an fp8 cache or fuse_rope off on path
    A) the same call takes the projection + RoPE kernel, the f32 qkv buffer holds the exact product, and the outputs
    are still within the bound."""
    c, ref = _gemm(16, 4, 2, 128, True, BF16, 0)
    _run_qkv(gpu, c, ref, proj.segs(4, 2, 128), PATH_A[0], "fallback", fuse_rope=False)
    c8, ref8 = _gemm(16, 4, 2, 128, True, FP8, 0)
    _run_qkv(gpu, c8, ref8, proj.segs(4, 2, 128), PATH_A[0], "fallback")
    cn = {**c, "neox": True}
    _run_qkv(gpu, cn, R.rope_ref(cn), proj.segs(4, 2, 128), PATH_A[0], "fallback")


def _norm_inputs(eps, seed):
    """16 residual rows for the fused input norm: even rows with a mean square of eps, eps / 100, 100 eps (row 0: eps,
    so M = 1 sees it), odd rows under a log-uniform scale; weights of both signs, another in every column."""
    g = torch.Generator().manual_seed(seed)
    xf = torch.randn(16, QKV_K, generator=g)
    xf = xf / xf.pow(2).mean(1, keepdim=True).sqrt()
    ms = torch.where(torch.arange(16) % 2 == 0, eps * 10.0 ** (2.0 * ((torch.arange(16) // 2 + 1) % 3 - 1)),
                     4.0 ** (torch.rand(16, generator=g) * 8 - 4))
    return xf * ms.sqrt()[:, None], R.norm_weights(QKV_K, g)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", PATH_A, ids=lambda c: "m%dw%dr%dk%d" % c)
def test_qkv_rope_path_a_fused_norm(gpu, proj, cfg):
    """The decode hot path's first half: qkv_rope_kv(norm=(x, w, eps)) -- the input RMSNorm from the full rows, the
    path-A GEMV, the RoPE + append epilogue in one launch."""
    worst = [0.0]
    for i, (M, D, (Hq, Hkv)) in enumerate(itertools.product((1, 3, 16), (64, 128), HEADS)):
        eps = (1e-5, 1e-6)[i % 2]
        xf, nw = _norm_inputs(eps, 60 + i)
        c, ref = _normed_gemm(M, Hq, Hkv, D, xf, nw, eps, i % 3)
        _run_qkv(gpu, c, ref, proj.segs(Hq, Hkv, D), cfg, "epilogue", arith=NORM_GEMV_TOL, worst=worst,
                 norm=(xf.to(gpu), nw.to(gpu), eps))
    print(f"RO_RATIO pathA+norm m%dw%dr%dk%d {worst[0]:.3f}" % cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 3, 16])
def test_qkv_rope_path_a_split_norm(gpu, proj, M):
    """The decode hot path as _forward_fused_norm runs it: ops.qgemv_add_ssq leaves the residual rows and their
    partial sums of squares (integer weights, alpha 1/2: the rows are exact), then qkv_rope_kv(norm=(x, w, eps,
    ssq, ldss, parts)) normalises from the partials, projects, rotates and appends in one launch."""
    Hq, Hkv, D, K2 = 4, 2, 128, 256
    rng = np.random.default_rng(77)
    raw = QB.structured_blocks(GGMLType.Q4_K, QKV_K, K2, "integer", rng)
    Wo = Q.dequantize(raw, GGMLType.Q4_K, (QKV_K, K2)).astype(np.float64)
    wo = ops.QWeight(raw, GGMLType.Q4_K, QKV_K, K2, gpu)
    pad = _pad64(M)
    xin = _acts(pad, K2, seed=9)
    base = torch.randint(-200, 201, (pad, QKV_K), generator=torch.Generator().manual_seed(M)).float()
    base = base * 2.0 ** (torch.arange(pad) % 5)[:, None]          # rows whose statistics differ by factors of 2
    x = base.to(gpu)
    ldss = QKV_K // 16
    ssq = torch.full((pad * ldss,), float("nan"), device=gpu)
    parts = ops.qgemv_add_ssq(ops.Seg(wo), xin.to(gpu), x, M, 0.5, ssq, ldss, cfg=(0, 8, 1, 1))
    assert parts == QKV_K // 16, "the producer did not run on path A"
    xr = base[:M].double().numpy() + 0.5 * (xin[:M].double().numpy() @ Wo.T)
    assert np.array_equal(x[:M].cpu().double().numpy(), xr), "integer residual rows must be exact"
    tot = ssq.view(-1, ldss)[:M, :parts].double().sum(1).cpu().numpy()
    assert np.allclose(tot, (xr * xr).sum(1), rtol=2.0 ** -20, atol=0)
    nw = R.norm_weights(QKV_K, torch.Generator().manual_seed(M + 5))
    worst = [0.0]
    for cfg in PATH_A:
        c, ref = _normed_gemm(M, Hq, Hkv, D, torch.from_numpy(xr).float(), nw, 1e-5)
        _run_qkv(gpu, c, ref, proj.segs(Hq, Hkv, D), cfg, "epilogue", arith=NORM_GEMV_TOL, worst=worst,
                 norm=(x, nw.to(gpu), 1e-5, ssq, ldss, parts))
    print(f"RO_RATIO pathA+ssq M={M} {worst[0]:.3f}")


# test_qkv_rope_kv_dense, ks 1; and mode 14, the production Q|K|V path with its own hoisted RoPE (h14_rope)
DENSE = [(4, 16, 2, 1), (4, 16, 4, 1), (5, 8, 4, 1), (10, 8, 1, 1), (10, 8, 2, 1), (14, 8, 2, 1)]
# head layouts whose Q|K and K|V boundaries (Hq D, (Hq + Hkv) D) fall inside a 96-row tile of the merged buffer and
# inside a wave's 48-row half of it, at D 64 and 128 (test_case_lists_cover)
HEADS14 = ((5, 2), (7, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", DENSE, ids=lambda c: "m%dw%dr%dk%d" % c)
def test_qkv_rope_dense_epilogues(gpu, proj, cfg):
    """Modes 4 / 5 (rope_store1 behind a lane shuffle), 10 (in-lane) and 14 (its own hoisted h14_rope) on the f16
    copies: a partial tile and several m0 chunks (M 70 / 300 / 520), D 64 / 128."""
    worst = [0.0]
    for i, (M, D) in enumerate(itertools.product((70, 300, 520), (64, 128))):
        Hq, Hkv = HEADS[i % 2]
        c, ref = _gemm(M, Hq, Hkv, D, bool(i % 3), BF16, i % 3)
        _run_qkv(gpu, c, ref, proj.segs(Hq, Hkv, D, dense=True), cfg, "epilogue", worst=worst)
    print(f"RO_RATIO dense m%dw%dr%dk%d {worst[0]:.3f}" % cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("dense", ["copies", "merged"])
def test_qkv_rope_mode14_layouts(gpu, proj, dense):
    """Mode 14's hoisted RoPE epilogue on per-matrix copies (three segments, a partial 96-row tile at each end) and
    on one merged buffer (one segment: head and Q|K|V boundaries inside a tile and inside a wave's 48 rows), with
    unsorted positions, permuted slots, slot -1 rows, a wide q_out and a bias: M 70 / 300 (several m0), D 64 / 128."""
    worst = [0.0]
    for i, (M, D, (Hq, Hkv)) in enumerate(itertools.product((70, 300), (64, 128), HEADS14 + HEADS[:1])):
        c, ref = _gemm(M, Hq, Hkv, D, bool((i + 1) % 3), BF16, i % 3)
        segs = proj.segs(Hq, Hkv, D, dense=dense)
        assert len(ops._merge_dense(segs)) == (1 if dense == "merged" else 3)
        _run_qkv(gpu, c, ref, segs, (14, 8, 2, 1), "epilogue", worst=worst)
    print(f"RO_RATIO dense m14 {'merged' if dense == 'merged' else 'copies'} {worst[0]:.3f}")


SLABS = [((1, 8, 1, 2), 3, False), ((1, 8, 1, 3), 16, False), ((1, 4, 2, 2), 70, False), ((2, 8, 4, 2), 70, False),
         ((2, 8, 2, 2), 300, False), ((10, 8, 1, 2), 70, True), ((4, 16, 2, 2), 300, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,M,dense", SLABS, ids=lambda c: "m%dw%dr%dk%d" % c if isinstance(c, tuple) else str(c))
@pytest.mark.parametrize("kv", [BF16, FP8], ids=["bf16", "fp8"])
def test_qkv_rope_split_k_slabs(gpu, proj, cfg, M, dense, kv):
    """Split-K projections (mode 1, mode 2, dense) leave their slabs to the RoPE kernel: integer partial sums add
    exactly in any split, so the same exact reference holds."""
    worst = [0.0]
    for D, (Hq, Hkv) in ((128, HEADS[0]), (64, HEADS[1])):
        c, ref = _gemm(M, Hq, Hkv, D, D == 128, kv, 1)
        _run_qkv(gpu, c, ref, proj.segs(Hq, Hkv, D, dense=dense), cfg, "slabs", worst=worst)
    print(f"RO_RATIO slabs m%dw%dr%dk%d {'bf16' if kv == BF16 else 'fp8'} {worst[0]:.3f}" % cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_rmsnorm_families(gpu, dt):
    """ops.rmsnorm: D 4 .. 8192, strided rows in and out, every family; rows and columns past the targets keep the
    sentinel."""
    worst = {}
    for k in _norm_keys():
        x, w, eps, ref = _norm_case(*k)
        M, D = x.shape
        xs = torch.randn(M, D + 8, generator=torch.Generator().manual_seed(D))
        xs[:, :D] = x
        out = torch.full((M + 2, D + 12), SENT, dtype=dt, device=gpu)
        ops.rmsnorm(xs.to(gpu)[:, :D], w.to(gpu), out[:, :D], M, eps)
        r, where = R.rms_ratio(out.cpu().double().numpy(), ref, dt, ARITH["norm"])
        worst[k[0]] = max(worst.get(k[0], 0.0), r)
        assert r <= 1.0, (k, f"{r:.3f} of the tolerance at {where}")
    print(f"RO_RATIO rmsnorm {'f16' if dt == F16 else 'f32'} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1022, 8196])
def test_rmsnorm_rejects_other_widths(gpu, D):
    """A width that is no multiple of 4, or past the 8192 the single pass holds, is the usual error, not a launch."""
    x = torch.randn(2, D, device=gpu)
    out = torch.full((2, D), SENT, dtype=F16, device=gpu)
    with pytest.raises(RuntimeError):
        ops.rmsnorm(x, torch.ones(D, device=gpu), out, 2, 1e-5)
    torch.cuda.synchronize()
    assert bool((out.float() == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("D", [68, 2052, 8192])
def test_splitk_add_rmsnorm_families(gpu, D):
    """nls_splitk_add_rmsnorm on synthetic slabs, ks 1..5 (5: the run-time loop): the written-back rows, then h
    against the fp64 norm of those rows; strided x and h."""
    worst = {}
    for k in ADD_KEYS:
        if k[1] != D:
            continue
        c = _add_case(*k)
        ks, M = c["slabs"].shape[0], c["base"].shape[0]
        x = torch.full((M + 1, D + 8), SENT, device=gpu)
        x[:M, :D] = c["base"].to(gpu)
        h = torch.full((M + 1, D + 12), SENT, dtype=ops.ACT_DTYPE, device=gpu)
        ws, w = c["slabs"].contiguous().to(gpu), c["w"].to(gpu)
        rc = ops._lib.lib().nls_splitk_add_rmsnorm(ws.data_ptr(), ks, M, c["alpha"], x.data_ptr(), x.stride(0),
                                                   w.data_ptr(), h.data_ptr(), h.stride(0), D, c["eps"],
                                                   ops._stream_ptr(x))
        ops._lib.check(rc, "nls_splitk_add_rmsnorm")
        rx, rh, where = _judge_addnorm(k, x.cpu().double().numpy(), h.cpu().double().numpy(), c, 2)
        worst[k[0]] = max(worst.get(k[0], 0.0), rh)
        assert rx <= 1.0 and rh <= 1.0, (k, f"x {rx:.3f}, h {rh:.3f} of the tolerance at {where}")
    print(f"RO_RATIO splitk_add_rmsnorm D={D} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# the last four: the o projection's real route, a dense split-K launch into splitk_add_rmsnorm (K = 1024)
ADDNORM_CFGS = [(5, (1, 8, 1, 4)), (64, (1, 4, 1, 2)), (200, (1, 8, 1, 3)), (256, (2, 8, 4, 4)), (130, (2, 8, 2, 2)),
                (130, (4, 16, 2, 2)), (200, (4, 8, 2, 3)), (258, (10, 8, 2, 2)), (130, (14, 8, 2, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("M,cfg", ADDNORM_CFGS, ids=lambda c: "m%dw%dr%dk%d" % c if isinstance(c, tuple) else str(c))
def test_qgemv_add_rmsnorm_integer(gpu, M, cfg):
    """ops.qgemv_add_rmsnorm with the split-K cfgs of test_qgemv_add_rmsnorm_fused, and dense split-K launches on the
    f16 copy, on integer weights: integer base, alpha 1/2 -- the written-back residual must EQUAL the reference, h is
    within the bound of its fp64 norm."""
    dense = cfg[0] in ops.DENSE_MODES
    D, K = 512, 1024 if dense else 768
    raw = QB.structured_blocks(GGMLType.Q4_K, D, K, "integer", np.random.default_rng(11))
    W = Q.dequantize(raw, GGMLType.Q4_K, (D, K)).astype(np.float64)
    pad = _pad64(M)
    xin = _acts(pad, K, seed=4)
    base = torch.full((pad, D), SENT)
    base[:M] = torch.randint(-1000, 1001, (M, D), generator=torch.Generator().manual_seed(M)).float()
    nw = R.norm_weights(D, torch.Generator().manual_seed(M + 1))
    x = base.to(gpu)
    h = torch.full((pad, D), SENT, dtype=ops.ACT_DTYPE, device=gpu)
    w = ops.QWeight(raw, GGMLType.Q4_K, D, K, gpu)
    if dense:
        w.expand_dense()
    ops.qgemv_add_rmsnorm(ops.Seg(w), xin.to(gpu), x, nw.to(gpu), h, M, 0.5, 1e-5, cfg=cfg)
    xr = base[:M].double().numpy() + 0.5 * (xin[:M].double().numpy() @ W.T)
    c = dict(fam="integer", x=xr, size=np.abs(xr), w=nw, eps=1e-5)
    rx, rh, where = _judge_addnorm((M, cfg), x.cpu().double().numpy(), h.cpu().double().numpy(), c, 0)
    print(f"RO_RATIO qgemv_add_rmsnorm M={M} m%dw%dr%dk%d x exact={rx == 0} h {rh:.3f}" % cfg)
    assert rx == 0 and rh <= 1.0, (M, cfg, rx, rh, where)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_moe_combine_norm_families(gpu, k):
    """ops.moe_combine_norm: both KMAX instantiations (k <= 2, k <= 8), D 68 .. 8192 (4100, 8192: a second pass of
    the 4096-column loop), T 1 / 5."""
    worst = {}
    for key in MOE_KEYS:
        if key[2] != k:
            continue
        c = _moe_case(*key)
        T, D = c["x"].shape
        x = torch.full((T + 1, D + 8), SENT, device=gpu)
        x[:T, :D] = c["resid"].to(gpu)
        h = torch.full((T + 1, D + 12), SENT, dtype=ops.ACT_DTYPE, device=gpu)
        ops.moe_combine_norm(c["y"].to(gpu), c["wt"].reshape(-1).to(gpu), T, k, x[:, :D], c["alpha"], c["w"].to(gpu),
                             c["eps"], h[:, :D])
        rx, rh, where = _judge_addnorm(key, x.cpu().double().numpy(), h.cpu().double().numpy(), c, 2 * k + 2)
        worst[key[0]] = max(worst.get(key[0], 0.0), rh)
        assert rx <= 1.0 and rh <= 1.0, (key, f"x {rx:.3f}, h {rh:.3f} of the tolerance at {where}")
    print(f"RO_RATIO moe_combine_norm k={k} " + " ".join(f"{f}={v:.3f}" for f, v in worst.items()))
