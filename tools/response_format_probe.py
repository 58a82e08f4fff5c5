#!/usr/bin/env python3
"""Cost of chat_model `response_format` (the sampler's allowed-token mask stage, the host matcher, the engine step).

(a) Requests without a response_format pay nothing in the shared wrapper: nls_sample and nls_sample_decode without
    masks, V = 128256, temperature 0.8 / top-k 40 on every row, 64 and 512 rows, of this tree's library against a
    library built from the parent commit (--parent PATH/_kernels.so). The two alternate window by window; the parent
    is timed twice per round (before and after this tree's window); the range of its 2 x --repeats windows is the
    spread of its own repeated runs -- the bar this tree's median is held to. Without --parent only this tree is
    timed.
(b) What the mask stage adds: nls_sample_mask with EVERY row masked (1 %, 50 %, 99 % of the tokens allowed) against
    nls_sample on the same rows, which already hold -inf at the disallowed ids (so both sample the same kept sets and
    the difference is the stage: ceil(V/32) mask words read, the -inf stores, one barrier).
(c) The host: fill_mask at V = 128256 cold and from the mask cache, native and pure-Python matcher, for four kinds of
    state: start of an object, inside a key, inside an unbounded string, after a value; on the synthetic Llama-3
    vocabulary (a few hundred tokens with bytes) and on a dense one (a byte string for every id).
(d) --engine: ms per decode step of the synthetic Llama-3-8B with 64 requests in flight (temperature 0.8 / top-k 40,
    seeded), 0, 1 and 64 of them constrained to a JSON string they cannot close (the closing tokens carry a -100
    logit_bias), so every step of the window has the same rows.
Each kernel figure is the median over --repeats windows of --iters back-to-back launches between device events; min /
max show the spread.

    python tools/response_format_probe.py [--parent /path/to/parent/_kernels.so] [--engine] [--rows 64,512]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nats_llm_studio_amd import ops  # noqa: E402
from nats_llm_studio_amd.engine import grammar as G  # noqa: E402
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


def _fmt(v) -> str:
    return f"{statistics.median(v):9.1f} ({min(v):.1f} - {max(v):.1f})"


def kernels(rows: int, V: int, iters: int, repeats: int, parent, dev):
    g = torch.Generator(device="cpu").manual_seed(rows)
    lg = (torch.randn(rows, V, generator=g) * 4).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = SamplingParams(temperature=0.8, top_k=40)
    raw = ops.sample_params_bytes(p)
    par = torch.from_numpy(np.frombuffer(raw * rows, dtype=np.uint8).reshape(rows, -1).copy()).to(dev)
    seeds = torch.arange(1, rows + 1, dtype=torch.int64, device=dev)
    pos = torch.full((rows,), 100, dtype=torch.int32, device=dev)
    ctx = pos + 1
    hist = torch.full((rows, HIST), -1, dtype=torch.int32, device=dev)
    nxt = torch.zeros(rows, dtype=torch.int32, device=dev)

    def host(L, buf=lg):
        return lambda: _lib.check(L.nls_sample(buf.data_ptr(), buf.stride(0), rows, V, par.data_ptr(), hist.data_ptr(),
                                               HIST, nxt.data_ptr(), st), "nls_sample")

    def graph(L):
        return lambda: _lib.check(L.nls_sample_decode(lg.data_ptr(), lg.stride(0), rows, V, par.data_ptr(),
                                                      seeds.data_ptr(), pos.data_ptr(), ctx.data_ptr(), hist.data_ptr(),
                                                      HIST, nxt.data_ptr(), st), "nls_sample_decode")

    fns = {}
    for name, mk in (("nls_sample", host), ("nls_sample_decode", graph)):
        if parent is not None:
            fns[f"parent (a)  {name}"] = mk(parent)
        fns[f"this tree   {name}"] = mk(_lib.lib())
        if parent is not None:
            fns[f"parent (b)  {name}"] = mk(parent)
    # (b): every row masked, the rows pre-masked as well
    rng = np.random.default_rng(rows)
    nw = (V + 31) // 32
    rowid = torch.arange(rows, dtype=torch.int32, device=dev)
    for pct in (1, 50, 99):
        ok = rng.random((rows, V)) < pct / 100.0
        ok[np.arange(rows), rng.integers(0, V, rows)] = True
        bits = np.zeros((rows, nw * 32), np.uint8)
        bits[:, :V] = ok
        words = torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.int32)).to(dev)
        pre = lg.clone()
        pre[torch.from_numpy(~ok).to(dev)] = float("-inf")
        fns[f"this tree   nls_sample, rows pre-masked to {pct:2d} %"] = host(_lib.lib(), pre)
        fns[f"this tree   nls_sample_mask, {pct:2d} % allowed"] = (
            lambda pre=pre, words=words: _lib.check(_lib.lib().nls_sample_mask(
                pre.data_ptr(), pre.stride(0), rows, V, par.data_ptr(), hist.data_ptr(), HIST, None, None, 0,
                words.data_ptr(), nw, rowid.data_ptr(), rows, nxt.data_ptr(), st), "nls_sample_mask"))
    toks = {}
    for k, fn in fns.items():                       # warm every variant
        fn()
        toks[k] = nxt.clone()
    torch.cuda.synchronize(dev)
    for name in ("nls_sample", "nls_sample_decode"):
        same = [k for k in fns if k.endswith(name)]
        assert all(torch.equal(toks[k], toks[same[0]]) for k in same), "unmasked launches disagree"
    for pct in (1, 50, 99):
        a, b = (k for k in fns if f"{pct:2d} %" in k)
        assert torch.equal(toks[a], toks[b]), "the mask stage changed a token of pre-masked rows"
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(_window(fn, iters))
    return times


def report_kernels(rows, t, parent):
    for k, v in t.items():
        print(f"  {k:58s} {_fmt(v)}")
    med = {k: statistics.median(v) for k, v in t.items()}
    if parent is not None:
        for name in ("nls_sample", "nls_sample_decode"):
            pa, pb, this = med[f"parent (a)  {name}"], med[f"parent (b)  {name}"], med[f"this tree   {name}"]
            runs = t[f"parent (a)  {name}"] + t[f"parent (b)  {name}"]      # the parent's own repeated runs
            lo, hi = min(runs), max(runs)
            verdict = "inside" if lo <= this <= hi else "OUTSIDE"
            print(f"  (a) {name} without masks: parent medians {pa:.1f} / {pb:.1f} us, its {len(runs)} windows "
                  f"{lo:.1f} - {hi:.1f} us ({100 * (hi - lo) / lo:.2f} %); this tree's median {this:.1f} us "
                  f"({100 * (this / ((pa + pb) / 2) - 1):+.2f} % of the parent's mean): {verdict} the spread of the "
                  f"parent's own windows")
    for pct in (1, 50, 99):
        a, b = (k for k in t if f"{pct:2d} %" in k)
        print(f"  (b) mask stage, {pct:2d} % allowed: {med[b] - med[a]:+.1f} us per launch of {rows} rows "
              f"({100 * (med[b] / med[a] - 1):+.2f} %)")


def synthetic_vocab(n: int):
    from nats_llm_studio_amd.tokenizer.bpe import ByteLevelBPE
    from nats_llm_studio_amd.tokenizer.synthetic import bytelevel_vocab
    toks, types, merges, ids = bytelevel_vocab(n)
    eog = [ids["<|eot_id|>"], ids["<|end_of_text|>"]]
    return G.GrammarVocab.from_tokenizer(ByteLevelBPE(toks, merges, types), eog, n), eog


def dense_vocab(n: int):
    """A vocabulary with a byte string for (nearly) every id, as a trained 128K vocabulary has: the 256 bytes, then
    seeded random words of 2 to 9 bytes (letters mostly, with and without a leading space, some digits and JSON
    punctuation). The synthetic Llama-3 vocabulary holds a few hundred merges and placeholders for the rest, so its
    trie is small; this one shows what the walk costs at full size."""
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxzETAOINSHRDLU", dtype=np.uint8)
    other = np.frombuffer(b"0123456789 _-.,:;{}[]\"'/\\()=+*<>\n", dtype=np.uint8)
    toks = {bytes([b]) for b in range(256)}
    while len(toks) < n - 2:
        k = int(rng.integers(2, 10))
        w = bytes(rng.choice(letters, k)) if rng.random() < 0.85 else bytes(rng.choice(other, min(k, 4)))
        toks.add(b" " + w[:-1] if rng.random() < 0.4 else w)
    tb = sorted(toks)[:n - 2] + [b"", b""]
    return G.GrammarVocab(tb, [n - 2, n - 1], n)


def host_masks(V: int):
    for name, vocab in (("synthetic Llama-3 vocabulary", synthetic_vocab(V)[0]), ("dense vocabulary", dense_vocab(V))):
        print(f" {name}")
        _host_masks(vocab, V)


def _host_masks(vocab, V: int):
    schema = {"type": "object", "properties": {"name": {"type": "string"}, "n": {"type": "integer"}}, "required": ["name"]}
    one = {bs: t for t, bs in enumerate(vocab.token_bytes) if len(bs) == 1}
    t0 = time.perf_counter()
    vocab.trie
    t1 = time.perf_counter()
    vocab.native()
    t2 = time.perf_counter()
    print(f"  byte trie of the vocabulary ({sum(1 for b in vocab.token_bytes if b)} tokens with bytes of {V}): "
          f"pure Python {1e3 * (t1 - t0):.1f} ms, native {1e3 * (t2 - t1):.1f} ms, once per loaded model")
    for kind, g in (("start of an object", b""), ("inside a key", b'{"na'), ("inside an unbounded string", b'{"name":"ab'),
                    ("after a value", b'{"name":"ab"')):
        for native in (True, False):
            cg = G.CompiledGrammar(G.compile_schema(schema), vocab)      # (a fresh mask cache)
            m = cg.matcher(native=native)
            for b in g:
                assert m.advance(one[bytes([b])])
            t0 = time.perf_counter()
            mask = m.fill_mask()
            t1 = time.perf_counter()
            for _ in range(100):
                m.fill_mask()
            t2 = time.perf_counter()
            n = int(np.unpackbits(mask.view(np.uint8)).sum())
            print(f"  {kind:28s} {'native' if native else 'python'}: cold {1e3 * (t1 - t0):8.3f} ms, cached "
                  f"{1e6 * (t2 - t1) / 100:6.1f} us, {n} tokens allowed")


def engine_steps(model_name: str, ftype: str, model_dir: str, B: int, warm: int, steps: int, dev):
    from nats_llm_studio_amd.engine.engine import Engine, GenRequest
    from nats_llm_studio_amd.gguf.reader import GGUFReader
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.models.llama import LlamaModel
    path = os.path.join(model_dir, f"{model_name}-{ftype}.gguf")
    if not os.path.exists(path):
        os.makedirs(model_dir, exist_ok=True)
        write_synthetic_gguf(path, model_name, ftype, seed=0)
    model = LlamaModel(GGUFReader(path), dev)
    vocab, eog = synthetic_vocab(model.cfg.vocab)
    cg = G.parse_response_format({"type": "json_schema", "json_schema": {"schema": {"type": "string"}}}, vocab)
    ban = tuple(sorted((t, -100.0) for t, bs in enumerate(vocab.token_bytes) if b'"' in bs))
    assert 0 < len(ban) <= 300
    rng = np.random.default_rng(0)
    for k in (0, 1, B):
        eng = Engine(model, None, max_batch=B, max_prefill_tokens=4096, use_graphs=True, ctx=1024, num_blocks=2048)
        eng.eos.update(eog)
        total = warm + steps + 40
        futs = []
        for i in range(B):
            kw = dict(temperature=0.8, top_k=40, seed=i + 1, max_tokens=total)
            sp = (SamplingParams(response_format=cg, logit_bias=ban, **kw) if i < k
                  else SamplingParams(ignore_eos=True, **kw))
            futs.append(eng.submit(GenRequest([int(v) for v in rng.integers(10, min(5000, model.cfg.vocab), 32)], sp)))
        while eng.waiting or any(s.n_prefilled < s.n_target for s in eng.running):
            eng.step()
        for _ in range(warm):
            eng.step()
        eng._drain()
        torch.cuda.synchronize(dev)
        c0, t0 = dict(eng.counters), time.perf_counter()
        for _ in range(steps):
            eng.step()
        eng._drain()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        assert len(eng.running) == B and not any(f.done() for f in futs), "a request ended inside the window"
        c = {key: eng.counters[key] - c0[key] for key in ("steps", "decode_tokens", "constrained_steps",
                                                          "device_sampled_steps", "graph_replays")}
        print(f"  {k:2d} of {B} constrained: {1e3 * dt / steps:7.3f} ms / step ({steps} steps; {c}; "
              f"mask ms {eng.stats()['grammar_mask_ms']})")
        while not all(f.done() for f in futs):
            eng.step()
        del eng


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=None, help="_kernels.so built from the parent commit")
    ap.add_argument("--rows", default="64,512")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--engine", action="store_true", help="also (d): the synthetic model's ms per step")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--ftype", default="Q4_K_M")
    ap.add_argument("--model-dir", default=os.environ.get("NLS_BENCH_DIR", "/tmp/nls_bench"))
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("response_format_probe: needs the GPU (no CPU fallback for a timing)")
    dev = torch.device("cuda:0")
    parent = None
    if a.parent:
        parent = ctypes.CDLL(a.parent)
        for name in ("nls_sample", "nls_sample_decode"):
            getattr(parent, name).argtypes = _lib._SIGS[name]
            getattr(parent, name).restype = ctypes.c_int
    print(f"# response_format cost, V = {a.vocab}, fp32 logits randn * 4, temperature 0.8 / top-k 40 on every row, "
          f"{a.iters} launches per window, {a.repeats} windows, us per launch: median (min - max)")
    print(f"# {torch.cuda.get_device_name(dev)}")
    for rows in (int(v) for v in a.rows.split(",")):
        print(f"rows = {rows} ({rows * a.vocab * 4 / 1e6:.0f} MB of logits)")
        report_kernels(rows, kernels(rows, a.vocab, a.iters, a.repeats, parent, dev), parent)
    print(f"(c) fill_mask on the host, V = {a.vocab}")
    host_masks(a.vocab)
    if a.engine:
        print(f"(d) {a.model} {a.ftype}, 64 requests in flight, prompts of 32 tokens")
        engine_steps(a.model, a.ftype, a.model_dir, 64, 20, a.steps, dev)


if __name__ == "__main__":
    main()
