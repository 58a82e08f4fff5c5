#!/usr/bin/env python3
"""Batch-1 decode attention latency in isolation (Llama-3-8B heads: 32 q / 8 kv, D = 128, 16-token blocks),
captured in a hipGraph: the attention launch alone, a trivial launch alone (the boundary floor), and the two
interleaved (attention after another kernel, as in a decode layer). Per-launch microseconds, one JSON line per
context length. The production split policy and chunk are used (models/llama.py attn_splits, _MIN_CHUNK).
    python tools/attn_b1_probe.py [--ctx 128,512,2048] [--kv bf16|fp8] [--window W] [--head-dim 64|128|256]
                                  [--heads HQ,HKV] [--batch B]
(--head-dim 256 --heads 16,4 moves the K/V bytes and the Hq * D of the default 32 / 8 heads of 128. --batch B: B rows
of the same context, each with its own block table over the shared 64K-slot pool; REPS launches per graph stay.)
(NLS_ATTN_MFMA_WAVES=4|8 selects the workgroup size per process.)"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.models import llama

REPS = 64


def timed(fn, iters=7):
    fn(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(REPS):
            fn(i)
    best = math.inf
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / REPS)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", default="128,512,2048")
    ap.add_argument("--kv", default="bf16")
    ap.add_argument("--splits", type=int, default=0, help="override the split count (0: the production policy)")
    ap.add_argument("--window", type=int, default=0, help="sliding window of the layer (0: none)")
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--heads", default="32,8", help="query heads, kv heads")
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kvt = torch.bfloat16 if a.kv == "bf16" else torch.float8_e4m3fn
    (Hq, Hkv), D, bs, B = [int(v) for v in a.heads.split(",")], a.head_dim, 16, a.batch
    nblk = 4096
    kc = (torch.randn(nblk * bs, Hkv, D, device=dev) * 0.5).to(kvt)
    vc = (torch.randn(nblk * bs, Hkv, D, device=dev) * 0.5).to(kvt)
    q = torch.randn(B, Hq * D, device=dev).to(torch.bfloat16)
    out = torch.zeros(B, Hq * D, dtype=ops.ACT_DTYPE, device=dev)
    ts = torch.arange(B, dtype=torch.int32, device=dev)
    dummy = torch.zeros(256, device=dev)
    ns = a.splits or llama.LlamaModel.attn_splits(B, Hkv)
    ws = torch.zeros(B * Hq * ns * (D + 2), dtype=torch.float32, device=dev)
    cnt = torch.zeros(B * Hkv, dtype=torch.int32, device=dev)
    for ctx in [int(c) for c in a.ctx.split(",")]:
        bt = torch.stack([torch.randperm(nblk, device=dev)[: (ctx + bs - 1) // bs] for _ in range(B)]).to(torch.int32)
        cl = torch.full((B,), ctx, dtype=torch.int32, device=dev)

        def attn(i):
            ops.attention(q, kc, vc, bt, ts, cl, out, B, Hq, Hkv, D, bs, D ** -0.5, chunk=-llama._MIN_CHUNK,
                          n_split=ns, workspace=ws, counters=cnt, window=a.window)

        def triv(i):
            dummy.add_(1.0)

        def both(i):
            triv(i)
            attn(i)
        t_attn, t_triv, t_both = timed(attn), timed(triv), timed(both)
        print(json.dumps(dict(ctx=ctx, D=D, heads=a.heads, batch=B, kv=a.kv, n_split=ns, window=a.window, waves_env=os.environ.get("NLS_ATTN_MFMA_WAVES"),
                              mfma_env=os.environ.get("NLS_ATTN_MFMA"),
                              attn_us=round(t_attn, 2), trivial_us=round(t_triv, 2), pair_us=round(t_both, 2),
                              attn_after_kernel_us=round(t_both - t_triv, 2))), flush=True)


if __name__ == "__main__":
    main()
