"""Cases and digests of tests/test_gemm_digests_gpu.py: every large-M GEMM instance (modes 2, 3, 4 / 5 / 6, 9, 10, 14)
launched once per case, a sha256 of every output buffer (padding rows included), "refused" where the dispatcher's plan
does not take the launch. The digests in tests/golden/gemm_digests.json were recorded with this module on the commit
before the kernels' workgroup prologue, epilogues and launcher moved into csrc/kernels/gemm_block.h; the code around
the K loops may be reorganised, the bits may not change.

    python tests/gemm_digest_cases.py tests/golden/gemm_digests.json

Outputs are deterministic: split-K slabs are summed in slice order, the arg-max is an atomicMax on keys, `add` is a
read-modify-write with one writer per element. Shapes are the smallest at which the shared code can go wrong: weight
rows 2 * tile + 48 (two full tiles and a partial one), M = BM + 2 (the second m-block holds two rows) and 1, K = 768
with ks 1 and 3 (mode 14 also K 1536 / ks 3: whole 128-column K-tiles per slice; mode 10 also K 1024 / ks 2: the
slice-per-XCD map), two segments with a gap between their output columns, mapped two-expert launches (modes 2 - 6) and
the expert table (mode 2).

Paths A and B (modes 0 and 1, qgemv_impl.h) have groups of their own, recorded in tests/golden/gemv_digests.json on the
commit before path B moved onto the shared workgroup prologue and the kernels' type switches onto one table:

    python tests/gemm_digest_cases.py tests/golden/gemv_digests.json gemv

The activation rows M pick the (waves, rt, mt) instance there, so each M is a group: M = 1 (path B: the staged
instance, and the 7-wave one that exists only there), 18, 35, 64 (mt 2, 3, 4) and, path B, 130 (mt 8, two m-blocks,
the second of two rows). The mapped two-expert and expert-table launches give the experts M rows between them (at
M = 1 three: the unstaged one-tile instance); at M = 130 with (8, 2) their counts reach the 2- and 8-tile forms of the
active-tile dispatch. One sha256 per case over all its buffers."""
import functools
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType as T

EPIS = ("f32", "add", "act", "swiglu", "rope", "rope_bias", "argmax", "f32_argmax", "slabs")
D = 16                                   # head size of the RoPE cases
HKV = 4


def instances():
    """(group id, (mode, waves, rt), tile rows, BM, weight type, dense) of every instance."""
    out = []
    for t in (T.Q4_K, T.Q5_K):           # kernel type-sets 0 and 1
        for wm in (4, 2, 1):
            out.append((f"m2w8r{wm}-{t.name}", (2, 8, wm), 128, 64 * wm, t, False))
        for mt in (16, 8, 6, 4):
            out.append((f"m3w4r{mt}-{t.name}", (3, 4, mt), 128, 16 * mt, t, False))
    for mode, waves, rt in [(m, w, r) for m in (4, 5) for w in (8, 16) for r in (4, 2)] + [(6, 8, 2)]:
        out.append((f"m{mode}w{waves}r{rt}", (mode, waves, rt), 256 if mode == 5 else 128, 64 * rt, T.Q4_K, True))
    for waves, rt in ((4, 2), (8, 2), (8, 1)):
        for t in (T.Q4_K, T.Q5_K, T.Q5_1, T.IQ4_XS):     # one type of each of the type-sets 0, 1, 3, 4
            out.append((f"m9w{waves}r{rt}-{t.name}", (9, waves, rt), 16 * waves * rt, 256, t, False))
    for rt in (1, 2):
        out.append((f"m10w8r{rt}", (10, 8, rt), 256 // rt, 256, T.Q4_K, True))
    out.append(("m14w8r2", (14, 8, 2), 96, 128, T.Q4_K, True))
    return out


GROUPS = [i[0] for i in instances()]


def gemv_instances():
    """(group id, (mode, waves, rt), tile rows, M, weight type) of every path-A / path-B group."""
    out = []
    for waves, rt in ((4, 1), (4, 2), (8, 1), (8, 2), (7, 1)):
        # (8, 1): one type of every kernel type-set; the others Q4_K
        types = (T.Q4_K, T.Q5_K, T.F16, T.Q5_1, T.IQ4_XS) if (waves, rt) == (8, 1) else (T.Q4_K,)
        for t in types:
            for M in ((1,) if waves == 7 else (1, 18, 35, 64, 130)):
                out.append((f"m1w{waves}r{rt}-{t.name}-M{M}", (1, waves, rt), 16 * waves * rt, M, t))
    for waves, rt in ((4, 1), (4, 2), (8, 1), (8, 2)):
        for M in (1, 18, 35, 64):
            # (rows as path B's 4-wave instances: the RoPE cases need more columns than the K / V heads take)
            out.append((f"m0w{waves}r{rt}-M{M}", (0, waves, rt), 64 * rt, M, T.Q4_K))
    return out


GEMV_GROUPS = [i[0] for i in gemv_instances()]


@functools.lru_cache(maxsize=None)
def _w(t, rows, K, dev, dense, seed=0):
    """A random weight (with its f16 copy for the dense modes); shared by the cases, never written to."""
    rng = np.random.default_rng(1000 * int(t) + rows + K + seed)
    w = ops.QWeight(Q.random_blocks(t, rows * K, 0.05, rng), t, rows, K, dev)
    if dense:
        w.expand_dense()
    return w


@functools.lru_cache(maxsize=None)
def _x(rows, K, dev):
    g = torch.Generator().manual_seed(rows + K)
    return torch.randn(rows, K, generator=g).to(ops.ACT_DTYPE).to(dev)


@functools.lru_cache(maxsize=None)
def _base(rows, cols, dev):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(7 + cols)).to(dev)


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _pad(M):
    return (M + 63) // 64 * 64


def _plain(dev, cfg, ks, M, K, segs, cols, epi):
    """One launch over unmapped segments that end at output column `cols`; digests or "refused"."""
    pad = _pad(M)
    x = _x(pad, K, dev)
    keys = torch.zeros(pad, dtype=torch.int64, device=dev) if "argmax" in epi else None
    if epi in ("rope", "rope_bias"):
        hq = cols // D - 2 * HKV
        cs = ops.rope_table(4 * pad, D, 10000.0, dev)
        pos = torch.arange(pad, dtype=torch.int32, device=dev) * 3
        slot = torch.arange(pad, dtype=torch.int32, device=dev)
        bias = _base(1, cols, dev)[0].contiguous() if epi == "rope_bias" else None
        y = torch.zeros(pad, cols, device=dev)
        q = torch.zeros(pad, hq * D, dtype=torch.bfloat16, device=dev)
        kc = torch.zeros(pad, HKV, D, dtype=torch.bfloat16, device=dev)
        vc = torch.zeros_like(kc)
        fz = ops._fuse_rope(ops._lib.NlsFuse(), pos, slot, cs, bias, q, kc, vc, hq, HKV, D)
        if not ops._launch(segs, x, y, M, 1.0, "rope", (*cfg, ks), fz=fz, soft=True):
            return "refused"
        return [_sha(q), _sha(kc), _sha(vc)]
    if epi == "swiglu":
        y = torch.zeros(pad, cols // 2, dtype=ops.ACT_DTYPE, device=dev)
    elif epi == "act":
        y = torch.zeros(pad, cols, dtype=ops.ACT_DTYPE, device=dev)
    elif epi == "add":
        y = _base(pad, cols, dev).clone()
    else:
        y = torch.zeros(pad, cols, device=dev)
    name = {"f32_argmax": "f32"}.get(epi, epi)
    if not ops._launch(segs, x, y, M, 0.5 if epi == "add" else 1.0, name, (*cfg, ks), argmax=keys, soft=True):
        return "refused"
    if epi == "slabs":
        return [_sha(ops._WS[x.device][:ops._ws_floats(segs, M, cfg[0], ks)])]
    if epi == "argmax":
        return [_sha(keys)]
    return [_sha(y)] + ([_sha(keys)] if keys is not None else [])


def _mapped(dev, cfg, ks, bm, K, rows, t, dense, counts, table=False, epi="f32"):
    """Two experts over row lists (the MoE down shape: gather and scatter through the same list, f32 store into
    sentinel rows; ks 2: the mapped split-K form). counts: the experts' device-side row counts."""
    cap = bm + 2
    ws = [_w(t, rows, K, dev, dense, seed=e + 1) for e in range(2)]
    x = _x(_pad(cap), K, dev)
    perm = np.random.default_rng(cap).permutation(cap)     # expert 0 from its front, expert 1 from its back: disjoint
    lists = torch.from_numpy(np.concatenate([perm, perm[::-1]]).astype(np.int32)).to(dev)
    assert sum(counts) <= cap
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    if epi == "swiglu":
        y = torch.full((_pad(cap), rows // 2), 5.0, dtype=ops.ACT_DTYPE, device=dev)
    else:
        y = torch.full((_pad(cap), rows), 5.0, device=dev)
    fz = None
    if table:
        tab = ops.ExpertTable(ws)
        segs = [ops.Seg(ws[0], 0, lists, lists, cnt)]
        fz = ops._lib.NlsFuse()
        fz.tab, fz.tab_n, fz.tab_cap = tab.ptrs.data_ptr(), 2, cap
    else:
        segs = [ops.Seg(ws[e], 0, lists[e * cap:], lists[e * cap:], cnt[e:e + 1]) for e in range(2)]
    n = ops._ws_floats(segs, cap, cfg[0], ks)
    if n:       # the reduce of mapped split-K reads every y row's slabs, also those of rows no expert was given
        ops._workspace(dev, n)[:n].zero_()
    if not ops._launch(segs, x, y, cap, 1.0, epi, (*cfg, ks), fz=fz, soft=True):
        return "refused"
    return [_sha(y)]


def run_group(dev, inst):
    """{case id: digests or "refused"} of one instance."""
    gid, cfg, tile, bm, t, dense = inst
    rows = 2 * tile + 48
    out = {}
    shapes = [(768, 1), (768, 3)] + ([(1536, 3)] if cfg[0] == 14 else []) + ([(1024, 2)] if cfg[0] == 10 else [])
    for K, ks in shapes:
        segs = [ops.Seg(_w(t, rows, K, dev, dense))]
        for M in (bm + 2, 1):
            for epi in EPIS:
                out[f"{gid}/K{K}ks{ks}/M{M}/{epi}"] = _plain(dev, cfg, ks, M, K, segs, rows, epi)
        # two segments, a gap of 16 output columns between them: the tile_begin lookup, ycol, tile_begin_col
        w2 = _w(t if dense else T.Q6_K, tile + 48, K, dev, dense, seed=3)
        for epi, h in (("f32", 1), ("swiglu", 2)):      # SwiGLU halves the output columns, ycol included
            two = [ops.Seg(_w(t, rows, K, dev, dense), 0), ops.Seg(w2, rows // h + 16)]
            out[f"{gid}/K{K}ks{ks}/M{bm + 2}/two_segments/{epi}"] = _plain(dev, cfg, ks, bm + 2, K, two,
                                                                          (rows // h + 16 + w2.rows // h) * h, epi)
    if cfg[0] <= 6:
        for name, counts in (("short", (5, 0)), ("two_blocks", (bm + 1, 1))):
            for ks in (1, 2):
                out[f"{gid}/mapped_{name}/ks{ks}"] = _mapped(dev, cfg, ks, bm, 768, rows, t, dense, counts)
    if cfg[0] == 2:
        for epi in ("f32", "swiglu"):
            out[f"{gid}/table/{epi}"] = _mapped(dev, cfg, 1, bm, 768, rows, t, dense, (bm + 1, 1), table=True, epi=epi)
    return out


def run_gemv_group(dev, inst):
    """{case id: digest or "refused"} of one path-A / path-B group."""
    gid, cfg, tile, M, t = inst
    rows = 2 * tile + 48
    out = {}
    for ks in ((1,) if cfg[0] == 0 else (1, 3)):        # (path A has no split-K)
        segs = [ops.Seg(_w(t, rows, 768, dev, False))]
        for epi in EPIS:
            out[f"{gid}/ks{ks}/{epi}"] = _plain(dev, cfg, ks, M, 768, segs, rows, epi)
        w2 = _w(t if t == T.F16 else T.Q6_K, tile + 48, 768, dev, False, seed=3)   # (no Q6_K in the float set)
        for epi, h in (("f32", 1), ("swiglu", 2)):
            two = [ops.Seg(_w(t, rows, 768, dev, False), 0), ops.Seg(w2, rows // h + 16)]
            out[f"{gid}/ks{ks}/two_segments/{epi}"] = _plain(dev, cfg, ks, M, 768, two,
                                                            (rows // h + 16 + w2.rows // h) * h, epi)
    if cfg[1] != 7:
        bm = max(M - 2, 1)
        for name, counts in (("short", (min(5, bm + 1), 0)), ("two_blocks", (bm + 1, 1))):
            for ks in ((1,) if cfg[0] == 0 else (1, 2)):
                out[f"{gid}/mapped_{name}/ks{ks}"] = _mapped(dev, cfg, ks, bm, 768, rows, t, False, counts)
        for epi in ("f32", "swiglu"):
            out[f"{gid}/table/{epi}"] = _mapped(dev, cfg, 1, bm, 768, rows, t, False, (bm + 1, 1), table=True, epi=epi)
    return {k: v if v == "refused" else hashlib.sha256("".join(v).encode()).hexdigest() for k, v in out.items()}


def run_all(dev):
    out = {}
    for inst in instances():
        out.update(run_group(dev, inst))
    return out


if __name__ == "__main__":
    if sys.argv[2:] == ["gemv"]:
        res = {}
        for inst in gemv_instances():
            res.update(run_gemv_group(torch.device("cuda:0"), inst))
    else:
        res = run_all(torch.device("cuda:0"))
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(res), "cases,", sum(v == "refused" for v in res.values()), "refused")
