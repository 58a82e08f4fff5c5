#!/usr/bin/env python3
"""What the un-fused Q/K norm + RoPE launch costs a decode step, measured on ONE model so that nothing else differs:
Llama-3-8B (Qwen3-8B's Q|K|V and o shapes) decoding with
  fused   its own path: RoPE + KV append in the Q|K|V GEMV / GEMM epilogue (5 launches per layer at batch 1)
  rope    the projection, then nls_rope_kv as a launch of its own (fuse_rope=False)
  qknorm  the projection, then nls_qknorm_rope_kv with all-ones norm weights -- the launches Qwen3 runs (6 per layer)
One variant per process (the decode hipGraphs are captured with the variant in place); a run script alternates them.
python tools/qkv_launch_cost.py --variant qknorm --concurrency 1 [--steps 200] [--model-dir DIR]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import SamplingParams
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
from nats_llm_studio_amd.models.llama import LlamaModel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("fused", "rope", "qknorm"), required=True)
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--concurrency", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--model-dir", default=os.environ.get("NLS_BENCH_DIR", "/tmp/nls_bench"))
    ap.add_argument("--device", choices=("cuda", "cpu"), default="cuda", help="cpu: rehearsal of the script only")
    a = ap.parse_args()
    cuda = a.device == "cuda"
    if cuda and not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a CPU timing says nothing about the launches")
    dev = torch.device("cuda:0" if cuda else "cpu")
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    path = os.path.join(a.model_dir, f"{a.model}-Q4_K_M.gguf")
    if not os.path.exists(path):
        os.makedirs(a.model_dir, exist_ok=True)
        write_synthetic_gguf(path, a.model, "Q4_K_M", seed=0)
    model = LlamaModel(GGUFReader(path), dev)
    if any(lw.q_norm is not None or lw.qkv_bias is not None for lw in model.layers):
        raise SystemExit("pick a family without a Q/K norm or QKV bias: the variants replace its RoPE path")
    orig = ops.qkv_rope_kv
    ones = torch.ones(model.D, device=dev)
    if a.variant == "rope":
        ops.qkv_rope_kv = lambda *p, **k: orig(*p, **{**k, "fuse_rope": False})
    elif a.variant == "qknorm":
        ops.qkv_rope_kv = lambda *p, **k: orig(*p, **{**k, "qk_norm": (ones, ones, model.cfg.eps)})
    B = a.concurrency
    gen = a.warmup + a.steps + (B * a.prompt_len + 2047) // 2048 + 8
    eng = Engine(model, None, max_batch=B, use_graphs=cuda, ctx=max(a.prompt_len + gen + 16, 512),
                 num_blocks=None if cuda else B * ((a.prompt_len + gen + 15) // 16 + 1))
    eng.capture_all()
    rng = np.random.default_rng(0)
    for _ in range(B):
        ids = list(rng.integers(0, min(model.cfg.vocab, 100000), a.prompt_len))
        eng.submit(GenRequest(ids, SamplingParams(max_tokens=gen, ignore_eos=True)))
    while any(s.n_prefilled < s.n_target for s in eng.running) or eng.waiting:
        eng.step()
    for _ in range(a.warmup):
        eng.step()
    assert len(eng.running) == B
    sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        eng.step()
    sync()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    print(json.dumps({"device": a.device, "model": a.model, "variant": a.variant, "concurrency": B, "steps": a.steps,
                      "ms_per_step": round(ms, 4), "us_per_layer": round(ms * 1e3 / model.cfg.n_layer, 2)}))


if __name__ == "__main__":
    main()
