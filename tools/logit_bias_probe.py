#!/usr/bin/env python3
"""Cost of chat_model `logit_bias` in the in-graph sampler (csrc/kernels/sample.hip sample_decode_kernel).

1. Requests without logit_bias pay nothing: nls_sample_decode (the entry without tables) at 64 and 512 rows, V =
   128256, temperature 0.8 / top-k 40 on every row, of this tree's library against a library built from the parent
   commit (--parent PATH/_kernels.so). The two alternate window by window; the parent is timed twice per round (before
   and after this tree's window), and the distance of its two medians is its own run-to-run spread -- the bar this
   tree's median is held to. Without --parent only this tree is timed.
2. What a biased row costs: nls_sample_decode_bias with 0, 1, 64 and 300 entries on EVERY row (values in [-8, 8] on
   random ids), against its own 0-entry figure. Reported, not gated.
Each figure is the median over --repeats windows of --iters back-to-back launches between device events; min / max show
the spread. The launches of a window are identical (same rows, positions and seeds; the kernel leaves the logits raw).
The current shader clock is read before and after (rocm-smi, if present).

    python tools/logit_bias_probe.py [--parent /path/to/parent/_kernels.so] [--rows 64,512] [--iters 30] [--repeats 9]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nats_llm_studio_amd import ops  # noqa: E402
from nats_llm_studio_amd.engine.sampling import HIST, LOGIT_BIAS_MAX, SamplingParams  # noqa: E402
from nats_llm_studio_amd.ops import _lib  # noqa: E402


def _window(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us per launch


def _clock() -> str:
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return "; ".join(ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln)[:300] or "not reported"
    except Exception as e:           # the tool is optional
        return f"not read ({type(e).__name__})"


def _fmt(v) -> str:
    return f"{statistics.median(v):9.1f} ({min(v):.1f} - {max(v):.1f})"


def probe(rows: int, V: int, iters: int, repeats: int, parent, dev):
    g = torch.Generator(device="cpu").manual_seed(rows)
    lg = (torch.randn(rows, V, generator=g) * 4).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = SamplingParams(temperature=0.8, top_k=40)
    seeds = torch.arange(1, rows + 1, dtype=torch.int64, device=dev)
    pos = torch.full((rows,), 100, dtype=torch.int32, device=dev)
    ctx = pos + 1
    hist = torch.full((rows, HIST), -1, dtype=torch.int32, device=dev)
    nxt = torch.zeros(rows, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(rows)
    ids = np.stack([rng.permutation(V)[:LOGIT_BIAS_MAX] for _ in range(rows)]).astype(np.int32)
    val = (rng.integers(-64, 65, ids.shape) / 8.0).astype(np.float32)
    bi, bv = torch.from_numpy(ids).to(dev), torch.from_numpy(val).to(dev)

    def params(nb):
        raw = ops.sample_params_bytes(p, n_bias=nb)
        return torch.from_numpy(np.frombuffer(raw * rows, dtype=np.uint8).reshape(rows, -1).copy()).to(dev)

    par = {nb: params(nb) for nb in (0, 1, 64, LOGIT_BIAS_MAX)}

    def old_entry(L):
        return lambda: _lib.check(L.nls_sample_decode(lg.data_ptr(), lg.stride(0), rows, V, par[0].data_ptr(),
                                                      seeds.data_ptr(), pos.data_ptr(), ctx.data_ptr(), hist.data_ptr(),
                                                      HIST, nxt.data_ptr(), st), "nls_sample_decode")

    fns = {}
    if parent is not None:
        fns["parent (a)  nls_sample_decode"] = old_entry(parent)
    fns["this tree   nls_sample_decode"] = old_entry(_lib.lib())
    if parent is not None:
        fns["parent (b)  nls_sample_decode"] = old_entry(parent)
    for nb in par:
        fns[f"this tree   nls_sample_decode_bias, {nb:3d} entries / row"] = (
            lambda nb=nb: ops.sample_decode(lg, rows, par[nb], seeds, pos, ctx, hist, nxt, bi, bv))
    before = lg.clone()
    toks = {}
    for k, fn in fns.items():                       # warm every variant; same draws from the same rows
        fn()
        toks[k] = nxt.clone()
    torch.cuda.synchronize(dev)
    same = [k for k in fns if "entries" not in k or "  0 entries" in k]
    assert all(torch.equal(toks[k], toks[same[0]]) for k in same), "unbiased launches disagree"
    assert torch.equal(lg.view(torch.int32), before.view(torch.int32)), "a launch left the logits changed"
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(_window(fn, iters))
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=None, help="_kernels.so built from the parent commit")
    ap.add_argument("--rows", default="64,512")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logit_bias_probe: needs the GPU (no CPU fallback for a timing)")
    dev = torch.device("cuda:0")
    parent = None
    if a.parent:
        parent = ctypes.CDLL(a.parent)
        parent.nls_sample_decode.argtypes = _lib._SIGS["nls_sample_decode"]
        parent.nls_sample_decode.restype = ctypes.c_int
    print(f"# logit_bias cost, V = {a.vocab}, fp32 logits randn * 4, temperature 0.8 / top-k 40 on every row, "
          f"{a.iters} launches per window, {a.repeats} windows, us per launch: median (min - max)")
    print(f"# {torch.cuda.get_device_name(dev)}; clocks before: {_clock()}")
    for rows in (int(v) for v in a.rows.split(",")):
        t = probe(rows, a.vocab, a.iters, a.repeats, parent, dev)
        print(f"rows = {rows} ({rows * a.vocab * 4 / 1e6:.0f} MB of logits)")
        for k, v in t.items():
            print(f"  {k:58s} {_fmt(v)}")
        med = {k: statistics.median(v) for k, v in t.items()}
        this = med["this tree   nls_sample_decode"]
        if parent is not None:
            pa, pb = med["parent (a)  nls_sample_decode"], med["parent (b)  nls_sample_decode"]
            spread = abs(pa - pb)
            lo, hi = min(pa, pb), max(pa, pb)
            verdict = "inside" if lo - spread <= this <= hi + spread else "OUTSIDE"
            print(f"  without logit_bias: parent {pa:.1f} / {pb:.1f} us (its own spread {spread:.1f} us, "
                  f"{100 * spread / lo:.2f} %), this tree {this:.1f} us ({100 * (this / ((pa + pb) / 2) - 1):+.2f} % "
                  f"of the parent's mean): {verdict} the parent's two medians widened by their distance")
        zero = med[f"this tree   nls_sample_decode_bias, {0:3d} entries / row"]
        print("  a biased row: " + ", ".join(
            f"{nb} entries {med[k] - zero:+.1f} us ({100 * (med[k] / zero - 1):+.2f} %)"
            for nb in (1, 64, LOGIT_BIAS_MAX)
            for k in [f"this tree   nls_sample_decode_bias, {nb:3d} entries / row"]) + " against 0 entries")
    print(f"# clocks after: {_clock()}")


if __name__ == "__main__":
    main()
