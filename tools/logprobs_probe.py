#!/usr/bin/env python3
"""Cost of per-token logprobs (csrc/kernels/sample.hip logprob_kernel / logprob_pick_kernel).

1. The two launches on random fp32 logits of V = 128256 at 64 and 512 rows (n_top 20 on every row), against
   two existing kernels on the same tensor: nls_argmax (one read pass over the rows) and nls_sample with
   top_k = 40. Each figure is the median over --repeats windows of --iters back-to-back launches between device
   events, the kernels alternating window by window; min / max show the spread. The acceptance bar of the main
   launch is 4x the nls_argmax time at both row counts, on random logits. The worst case is measured next to it:
   all-equal rows, whose survivors overflow the LDS list and take the k exact passes over the row.
2. ms/step of a B = 64 greedy decode of the synthetic tiny Llama through the engine (hipGraphs), with and
   without `logprobs` (top_logprobs 20) on every row, and where the engine thread spent it (Engine.host_ms:
   "wait" is blocked on the GPU step, "tokens" digests the ids and records, "launch" builds and launches a step).

    python tools/logprobs_probe.py [--rows 64,512] [--vocab 128256] [--iters 50] [--repeats 7]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nats_llm_studio_amd import ops  # noqa: E402
from nats_llm_studio_amd.engine.sampling import HIST, SamplingParams  # noqa: E402
from nats_llm_studio_amd.ops import _lib  # noqa: E402


def _window(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us per launch


def kernels(rows: int, V: int, iters: int, repeats: int, dev) -> dict:
    g = torch.Generator(device="cpu").manual_seed(rows)
    lg = (torch.randn(rows, V, generator=g) * 4).to(dev)
    L = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    nt = torch.full((rows,), ops.LP_TOP, dtype=torch.int32, device=dev)
    rec = torch.zeros(rows, ops.LP_REC, dtype=torch.int32, device=dev)
    ids = torch.zeros(rows, dtype=torch.int32, device=dev)
    p = SamplingParams(temperature=0.8, top_k=40)
    raw = bytearray(ops.sample_params_bytes(p))
    sp = _lib.SampleParams.from_buffer(raw)
    sp.u = 0.37
    params = torch.from_numpy(np.frombuffer(bytes(raw) * rows, dtype=np.uint8).reshape(rows, -1).copy()).to(dev)
    hist = torch.full((rows, HIST), -1, dtype=torch.int32, device=dev)
    fns = {
        "nls_argmax": lambda: _lib.check(L.nls_argmax(lg.data_ptr(), lg.stride(0), rows, V, ids.data_ptr(), st), "argmax"),
        "nls_sample top_k=40": lambda: _lib.check(L.nls_sample(lg.data_ptr(), lg.stride(0), rows, V, params.data_ptr(),
                                                               hist.data_ptr(), HIST, ids.data_ptr(), st), "sample"),
        "nls_logprobs n_top=20": lambda: ops.token_logprobs(lg, rows, nt, rec, V=V),
        "nls_logprobs n_top=0": None,
        "nls_logprobs_pick": lambda: ops.token_logprobs_pick(lg, rows, nt, ids, rec, V=V),
    }
    nt0 = torch.zeros(rows, dtype=torch.int32, device=dev)
    fns["nls_logprobs n_top=0"] = lambda: ops.token_logprobs(lg, rows, nt0, rec, V=V)
    eq = torch.full_like(lg, 0.375)
    fns["nls_logprobs all-equal rows"] = lambda: ops.token_logprobs(eq, rows, nt, rec, V=V)
    for fn in fns.values():                         # warm every kernel
        fn()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(_window(fn, iters))
    return times


def decode_ms_per_step(logprobs: bool, dev, batch: int = 64, tokens: int = 160):
    """(ms/step, host ms/step by Engine.host_ms bucket) of the best of three passes."""
    from nats_llm_studio_amd.engine.engine import Engine, GenRequest
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tiny-llama.gguf")
        write_synthetic_gguf(path, "tiny-llama", "Q4_K_M", seed=0)
        m = LlamaModel(GGUFReader(path), dev)
        eng = Engine(m, None, max_batch=batch, use_graphs=True, ctx=512)
        best, best_host = None, {}
        for _ in range(3):                          # the first pass captures the graphs
            p = SamplingParams(max_tokens=tokens, ignore_eos=True, logprobs=logprobs,
                               top_logprobs=ops.LP_TOP if logprobs else 0)
            futs = [eng.submit(GenRequest([3 + i, 7, 11, 13 + i], p)) for i in range(batch)]
            eng.step()                              # admission + prefill + the first decode launch
            torch.cuda.synchronize(dev)
            s0, t0, h0 = eng.counters["steps"], time.perf_counter(), dict(eng.host_ms)
            while not all(f.done() for f in futs):
                eng.step()
            torch.cuda.synchronize(dev)
            steps = max(1, eng.counters["steps"] - s0)
            ms = (time.perf_counter() - t0) * 1e3 / steps
            if best is None or ms < best:
                best = ms
                best_host = {k: (v - h0.get(k, 0.0)) / steps for k, v in eng.host_ms.items()}
            if logprobs:
                assert all(len(f.result().logprobs) == tokens for f in futs)
        eng.shutdown()
        return best, best_host


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="64,512")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-engine", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprobs_probe: needs the GPU (no CPU fallback for a timing)")
    dev = torch.device("cuda:0")
    print(f"# logprobs cost, V = {a.vocab}, fp32 logits randn * 4, {a.iters} launches per window, "
          f"{a.repeats} windows, us per launch: median (min - max)")
    for rows in (int(v) for v in a.rows.split(",")):
        t = kernels(rows, a.vocab, a.iters, a.repeats, dev)
        base = statistics.median(t["nls_argmax"])
        mb = rows * a.vocab * 4 / 1e6
        print(f"rows = {rows} ({mb:.0f} MB of logits)")
        for k, v in t.items():
            med = statistics.median(v)
            print(f"  {k:28s} {med:9.1f} ({min(v):.1f} - {max(v):.1f})  {med / base:5.2f}x nls_argmax  "
                  f"{mb / med:6.2f} TB/s (bytes of the logits over the launch time)")
        ratio = statistics.median(t["nls_logprobs n_top=20"]) / base
        print(f"  main launch / nls_argmax = {ratio:.2f} (bar: <= 4): {'met' if ratio <= 4 else 'MISSED'}")
    if not a.no_engine:
        off, h_off = decode_ms_per_step(False, dev)
        on, h_on = decode_ms_per_step(True, dev)
        print(f"tiny-llama B = 64 greedy decode, hipGraphs, best of 3 passes: {off:.3f} ms/step without logprobs, "
              f"{on:.3f} ms/step with logprobs + top_logprobs 20 on every row (+{on - off:.3f} ms)")
        for name, h in (("without", h_off), ("with", h_on)):
            print(f"  engine thread, ms/step {name} logprobs: " + ", ".join(
                f"{k} {h.get(k, 0.0):.3f}" for k in ("wait", "tokens", "launch", "schedule", "prefill")))


if __name__ == "__main__":
    main()
