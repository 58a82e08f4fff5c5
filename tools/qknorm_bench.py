#!/usr/bin/env python3
"""Launch time of the per-head Q/K norm + RoPE + KV-append kernel (csrc/kernels/qknorm.hip) next to nls_rope_kv on
identical inputs: Hq 32, Hkv 8, D 128 (Llama-3-8B / Qwen3-8B), T in {1, 64, 512}, split-K slabs ks in {1, 2}.
Device events around N back-to-back launches replayed as one hipGraph (as the decode steps run them; no host
enqueue time in the window) after a warm-up, the two kernels alternating over several rounds (median and range).
Both kernels read ks * T * 6144 floats and write T * 6144 bf16, so us -> GB/s is the same formula for both.
python tools/qknorm_bench.py [--out FILE]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.ops import _lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    Hq, Hkv, D, eps = 32, 8, 128, 1e-6
    ncol = (Hq + 2 * Hkv) * D
    L = _lib.lib()
    lines = [f"# {torch.cuda.get_device_name(0)}; Hq {Hq} Hkv {Hkv} D {D}; {a.launches} launches per event pair, "
             f"{a.rounds} alternating rounds, median (min..max) us per launch",
             "#   T ks neox | rope_kv us            | qknorm_rope_kv us      | ratio | qknorm GB/s"]
    cs = ops.rope_table(4096, D, 1e6, dev)
    qw = torch.exp(0.7 + 0.45 * torch.randn(D, device=dev))
    kw = torch.exp(0.7 + 0.45 * torch.randn(D, device=dev))
    for T in (1, 64, 512):
        for ks in (1, 2):
            for neox in (0, 1):
                slabs = torch.randn(ks * T, ncol, device=dev)
                pos = (torch.arange(T, dtype=torch.int32, device=dev) * 3) % 4096
                slot = torch.arange(T, dtype=torch.int32, device=dev)
                q = torch.zeros(T, Hq * D, dtype=torch.bfloat16, device=dev)
                kc = torch.zeros(T, Hkv, D, dtype=torch.bfloat16, device=dev)
                vc = torch.zeros_like(kc)
                st = torch.cuda.current_stream().cuda_stream

                def rope(st=st):
                    return L.nls_rope_kv(slabs.data_ptr(), ncol, ks, T * ncol, None, pos.data_ptr(), slot.data_ptr(),
                                         cs.data_ptr(), q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), T, Hq,
                                         Hkv, D, neox, st)

                def qkn(st=st):
                    return L.nls_qknorm_rope_kv(slabs.data_ptr(), ncol, ks, T * ncol, qw.data_ptr(), kw.data_ptr(), eps,
                                                pos.data_ptr(), slot.data_ptr(), cs.data_ptr(), q.data_ptr(),
                                                q.stride(0), kc.data_ptr(), vc.data_ptr(), T, Hq, Hkv, D, neox, st)

                def captured(fn):      # the launches as one hipGraph: no host enqueue cost in the timed window
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        cst = torch.cuda.current_stream().cuda_stream
                        for _ in range(a.launches):
                            assert fn(cst) == 0
                    return g

                def timed(g):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / a.launches

                for fn in (rope, qkn):
                    for _ in range(20):
                        assert fn() == 0
                torch.cuda.synchronize()
                gr, gq = captured(rope), captured(qkn)
                for g in (gr, gq):
                    g.replay()
                torch.cuda.synchronize()
                res = {"rope": [], "qkn": []}
                for _ in range(a.rounds):
                    res["rope"].append(timed(gr))
                    res["qkn"].append(timed(gq))
                m = {k: statistics.median(v) for k, v in res.items()}
                gbs = (ks * T * ncol * 4 + T * ncol * 2) / (m["qkn"] * 1e-6) / 1e9
                lines.append(f"{T:5d} {ks:2d} {neox:4d} "
                             f"| {m['rope']:7.2f} ({min(res['rope']):.2f}..{max(res['rope']):.2f}) "
                             f"| {m['qkn']:7.2f} ({min(res['qkn']):.2f}..{max(res['qkn']):.2f}) "
                             f"| {m['qkn'] / m['rope']:5.2f} | {gbs:8.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
