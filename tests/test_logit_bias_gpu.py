"""chat_model `logit_bias` on the MI355X: the bias stage of csrc/kernels/sample.hip (sample_one_biased) through the
host-driven entry nls_sample_bias and the in-graph entry nls_sample_decode_bias, the logprob kernels around it, and
the engine. Inputs: tests/logit_bias_ref.py (5 rows per launch -- plain, history overlap, exact tie, -inf, NaN -- with
0 / 1 / 63 / 64 / 65 / 300 entries mixed over the rows, V = 19 / 1025 / 128256, row pitch V and V + 24);
tests/test_logit_bias.py shows that this case list notices each fault of the stage.

The oracle has no tolerance: the biased call on the raw logits returns exactly the tokens of the existing, unbiased
entry on a copy whose biased entries were pre-added in float32 on the host. Afterwards the raw buffer is bit-equal to
its input, except at the history ids of penalised rows (rewritten in place, as always)."""
import glob
import os

import numpy as np
import pytest
import torch

import logit_bias_ref as B
import sampler_ref as S
from nats_llm_studio_amd import ops
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import HIST, SamplingParams
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.models.llama import LlamaModel

pytestmark = pytest.mark.gpu

SENT = -7
PADV = np.float32(1e30)
GUARD = 64
CASES = [(V, pad, v) for V in B.VS for pad in (0, 24) for v in range(len(B.COUNTS))]


def _L():
    from nats_llm_studio_amd.ops import _lib
    return _lib.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _buffer(rows, pad):
    """Rows at pitch V + pad, 1e30 in the padding columns and in a guard band behind the last row."""
    n, V = rows.shape
    ld = V + pad
    buf = np.full(n * ld + GUARD, PADV, np.float32)
    for r in range(n):
        buf[r * ld: r * ld + V] = rows[r]
    return buf, ld


def _params(c, dev, decode, nb=None):
    from nats_llm_studio_amd.ops import _lib
    raw = b""
    for r, p in enumerate(c.params):
        u, nh = (0.0, 0) if decode else (c.us[r], len(c.hists[r]))
        raw += bytes(_lib.SampleParams(p["temperature"], p["top_p"], p["min_p"], p["repeat_penalty"],
                                       p["presence_penalty"], p["frequency_penalty"], u, int(p["top_k"]), nh,
                                       c.nb[r] if nb is None else nb))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)


def _hist(c, dev):
    h = np.full((len(c.nb), HIST), -1, np.int32)
    for r, hh in enumerate(c.hists):
        h[r, :len(hh)] = hh
    return torch.from_numpy(h).to(dev)


def _tables(c, dev):
    return torch.from_numpy(c.ids.copy()).to(dev), torch.from_numpy(c.vals.copy()).to(dev)


def _sample(dev, buf, ld, V, pb, hd, tabs=None):
    """nls_sample (tabs None) or nls_sample_bias on a device copy of buf: (tokens, buffer afterwards, device buffer)."""
    d = buf if torch.is_tensor(buf) else torch.from_numpy(buf.copy()).to(dev)
    n = hd.shape[0]
    out = torch.full((n,), SENT, dtype=torch.int32, device=dev)
    if tabs is None:
        rc = _L().nls_sample(d.data_ptr(), ld, n, V, pb.data_ptr(), hd.data_ptr(), HIST, out.data_ptr(), _stream(dev))
    else:
        rc = _L().nls_sample_bias(d.data_ptr(), ld, n, V, pb.data_ptr(), hd.data_ptr(), HIST, tabs[0].data_ptr(),
                                  tabs[1].data_ptr(), tabs[0].shape[1], out.data_ptr(), _stream(dev))
    assert rc == 0
    return out.cpu().numpy().tolist(), d.cpu().numpy(), d


def _check_buffer(c, before, after, ld, windows, where):
    """Bit-equal to the input outside the penalised history ids of penalised rows; padding and guard band intact."""
    diff = np.flatnonzero(before.view(np.int32) != after.view(np.int32))
    allowed = set()
    for r in range(len(c.nb)):
        allowed |= {r * ld + t for t in B.penalised_ids(c, r, windows[r])}
    assert set(diff.tolist()) <= allowed, (where, sorted(set(diff.tolist()) - allowed)[:6])
    mask = np.ones(len(before), bool)
    for r in range(len(c.nb)):
        mask[r * ld: r * ld + c.V] = False
    assert (after[mask] == PADV).all(), where


@pytest.mark.parametrize("V,pad,variant", CASES)
def test_host_entry_equals_prebiased(gpu, V, pad, variant):
    c = B.launch(V, variant)
    raw, ld = _buffer(c.logits, pad)
    pre, _ = _buffer(B.prebiased(c), pad)
    hd, tabs = _hist(c, gpu), _tables(c, gpu)
    want, _, _ = _sample(gpu, pre, ld, V, _params(c, gpu, False, nb=0), hd)
    got, after, d = _sample(gpu, raw, ld, V, _params(c, gpu, False), hd, tabs)
    print(c.name, "pad", pad, "n_bias", c.nb, "tokens", got, "pre-biased", want)
    assert got == want
    assert all(0 <= t < V for t in got)
    _check_buffer(c, raw, after, ld, c.hists, c.name)
    # once more on the same buffer: a row without penalties is as it was, so its token is too
    again, _, _ = _sample(gpu, d, ld, V, _params(c, gpu, False), hd, tabs)
    unpen = [r for r in range(len(c.nb)) if not S.penal(c.params[r])]
    assert [again[r] for r in unpen] == [got[r] for r in unpen]
    # the same params (n_bias > 0) through the old entry: null tables, the bias is not applied and nothing is read
    if variant == 0:
        plain, _, _ = _sample(gpu, raw, ld, V, _params(c, gpu, False), hd)
        zero, _, _ = _sample(gpu, raw, ld, V, _params(c, gpu, False, nb=0), hd)
        assert plain == zero


def _decode(dev, buf, ld, c, pb, ctx, tabs=None):
    d = torch.from_numpy(buf.copy()).to(dev)
    n = len(c.nb)
    rg = torch.from_numpy(c.ring.copy()).to(dev)
    seeds = torch.from_numpy(np.array(c.seed, dtype=np.uint64).view(np.int64)).to(dev)
    pos = torch.tensor(c.pos, dtype=torch.int32, device=dev)
    cx = torch.tensor(ctx, dtype=torch.int32, device=dev)
    nxt = torch.full((n,), SENT, dtype=torch.int32, device=dev)
    if tabs is None:
        rc = _L().nls_sample_decode(d.data_ptr(), ld, n, c.V, pb.data_ptr(), seeds.data_ptr(), pos.data_ptr(),
                                    cx.data_ptr(), rg.data_ptr(), HIST, nxt.data_ptr(), _stream(dev))
    else:
        rc = _L().nls_sample_decode_bias(d.data_ptr(), ld, n, c.V, pb.data_ptr(), seeds.data_ptr(), pos.data_ptr(),
                                         cx.data_ptr(), rg.data_ptr(), HIST, tabs[0].data_ptr(), tabs[1].data_ptr(),
                                         tabs[0].shape[1], nxt.data_ptr(), _stream(dev))
    assert rc == 0
    return nxt.cpu().numpy().tolist(), d.cpu().numpy(), rg.cpu().numpy()


@pytest.mark.parametrize("V,pad,variant", CASES)
def test_graph_entry_equals_prebiased(gpu, V, pad, variant):
    """nls_sample_decode_bias on the rings, positions and seeds of the launch. Expected tokens: the old in-graph entry
    on the pre-biased copy, for every row it draws; it skips a temperature-0 row without penalties, which the new
    entry must NOT skip when the row has a bias -- there (and for every row) the old host-driven entry on the
    pre-biased copy, given the same window and the same variate uniform01(seed, position), is the witness."""
    c = B.launch(V, variant)
    n = len(c.nb)
    raw, ld = _buffer(c.logits, pad)
    pre, _ = _buffer(B.prebiased(c), pad)
    tabs = _tables(c, gpu)
    live = [p + 1 for p in c.pos]
    got, after, ring = _decode(gpu, raw, ld, c, _params(c, gpu, True), live, tabs)
    old_pre, _, _ = _decode(gpu, pre, ld, c, _params(c, gpu, True, nb=0), live)
    old_raw, _, _ = _decode(gpu, raw, ld, c, _params(c, gpu, True, nb=0), live)
    windows = [B.decode_window(c, r) for r in range(n)]
    host = c._replace(hists=[tuple(w) for w in windows], us=[S.uniform01(c.seed[r], c.pos[r]) for r in range(n)])
    want, _, _ = _sample(gpu, pre, ld, V, _params(host, gpu, False, nb=0), _hist(host, gpu))
    print(c.name, "pad", pad, "n_bias", c.nb, "tokens", got, "host on pre-biased", want, "old entry", old_pre)
    for r in range(n):
        greedy = c.params[r]["temperature"] <= 0.0 and not S.penal(c.params[r])
        if greedy and c.nb[r] == 0:
            assert got[r] == SENT and old_pre[r] == SENT
            continue
        assert got[r] == want[r], (r, got, want)
        if not greedy:
            assert got[r] == old_pre[r], (r, got, old_pre)
        if c.nb[r] == 0:
            assert got[r] == old_raw[r]
    exp = c.ring.copy()
    for r in range(n):
        if got[r] != SENT:
            exp[r, (c.pos[r] + 1) % HIST] = got[r]
    assert np.array_equal(ring, exp)
    _check_buffer(c, raw, after, ld, windows, c.name)
    # padding rows (ctx_len 0, -3) write nothing, biased or not
    dead = [0 if r % 2 else -3 for r in range(n)]
    got0, after0, ring0 = _decode(gpu, raw, ld, c, _params(c, gpu, True), dead, tabs)
    assert got0 == [SENT] * n and np.array_equal(ring0, c.ring)
    assert np.array_equal(after0.view(np.int32), raw.view(np.int32))


def test_entries_refuse_null_tables(gpu):
    """Null tables, or a stride outside [1, 1024], with n_bias > 0 in the params: -1, nothing launched."""
    c = B.launch(1025, 1)
    raw, ld = _buffer(c.logits, 0)
    d = torch.from_numpy(raw.copy()).to(gpu)
    n, L, st = len(c.nb), _L(), _stream(gpu)
    pb, pbd, hd = _params(c, gpu, False), _params(c, gpu, True), _hist(c, gpu)
    ti, tv = _tables(c, gpu)
    out = torch.full((n,), SENT, dtype=torch.int32, device=gpu)
    seeds = torch.zeros(n, dtype=torch.int64, device=gpu)
    pos = torch.tensor(c.pos, dtype=torch.int32, device=gpu)
    ctx = pos + 1
    rg = torch.from_numpy(c.ring.copy()).to(gpu)
    for ids, val, stride in ((None, None, 300), (ti.data_ptr(), None, 300), (None, tv.data_ptr(), 300),
                             (ti.data_ptr(), tv.data_ptr(), 0), (ti.data_ptr(), tv.data_ptr(), 1025)):
        assert L.nls_sample_bias(d.data_ptr(), ld, n, c.V, pb.data_ptr(), hd.data_ptr(), HIST, ids, val, stride,
                                 out.data_ptr(), st) == -1
        assert L.nls_sample_decode_bias(d.data_ptr(), ld, n, c.V, pbd.data_ptr(), seeds.data_ptr(), pos.data_ptr(),
                                        ctx.data_ptr(), rg.data_ptr(), HIST, ids, val, stride, out.data_ptr(),
                                        st) == -1
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [SENT] * n and np.array_equal(rg.cpu().numpy(), c.ring)
    assert np.array_equal(d.cpu().numpy().view(np.int32), raw.view(np.int32))
    with pytest.raises(TypeError):
        ops.sample_decode(d[:n * ld].view(n, ld), n, pbd, seeds, pos, ctx, rg, out, bias_ids=ti)


@pytest.mark.parametrize("penalised", [False, True])
def test_biased_row_reports_the_raw_logprob(gpu, penalised):
    """token_logprobs -> biased sample_decode -> token_logprobs_pick on one buffer: the top-n entries are bit-equal to
    the unbiased run's, the chosen entry is the raw log-probability of the token actually drawn (a token that only
    its +100 bias makes likely; with `penalised` it sits in the penalty window as well)."""
    V, n, ps = 1000, 3, 100
    g = torch.Generator().manual_seed(5)
    host = torch.randn(n, V, generator=g)
    tok = [321, 654, 17]
    hist = torch.randint(0, V, (n, HIST), generator=g, dtype=torch.int32)
    for r in range(n):
        hist[r][hist[r] == tok[r]] = (tok[r] + 1) % V
        host[r, tok[r]] = -3.0                          # unlikely by itself
        if penalised:
            hist[r, 5] = tok[r]
    p = SamplingParams(temperature=1.0, top_k=1, **(dict(repeat_penalty=1.3, presence_penalty=0.5) if penalised else {}))
    pb = [dataclass_replace(p, logit_bias=((tok[r], 100.0), (0, -1.0))) for r in range(n)]
    ids = torch.full((n, 300), -1, dtype=torch.int32)
    val = torch.zeros(n, 300)
    for r in range(n):
        ids[r, :2] = torch.tensor([tok[r], 0], dtype=torch.int32)
        val[r, :2] = torch.tensor([100.0, -1.0])

    def run(params, tabs):
        par = torch.from_numpy(np.frombuffer(b"".join(ops.sample_params_bytes(q) for q in params), dtype=np.uint8)
                               .reshape(n, -1).copy()).to(gpu)
        seeds = torch.tensor([3, 4, 5], dtype=torch.int64, device=gpu)
        pos = torch.full((n,), ps, dtype=torch.int32, device=gpu)
        ctx = pos + 1
        lg, hd = host.to(gpu), hist.to(gpu)
        nt = torch.tensor([3, 0, 20], dtype=torch.int32, device=gpu)
        rec = torch.zeros(n, ops.LP_REC, dtype=torch.int32, device=gpu)
        stash = ops.logprob_stash(n, HIST, gpu)
        nxt = torch.zeros(n, dtype=torch.int32, device=gpu)
        ops.token_logprobs(lg, n, nt, rec, ctx_len=ctx, params=par, pos=pos, hist=hd, stash=stash)
        ops.sample_decode(lg, n, par, seeds, pos, ctx, hd, nxt, *tabs)
        ops.token_logprobs_pick(lg, n, nt, nxt, rec, ctx_len=ctx, stash=stash)
        return nxt.cpu().tolist(), rec.cpu().numpy(), nt.cpu().tolist()

    plain_tok, plain, nt = run([p] * n, ())
    got_tok, got, _ = run(pb, (ids.to(gpu), val.to(gpu)))
    assert got_tok == tok and all(a != b for a, b in zip(plain_tok, tok))
    assert np.array_equal(got[:, 2:], plain[:, 2:])                    # top-n logprobs and ids: bit-equal
    for r in range(n):
        raw = torch.log_softmax(host[r].double(), 0)
        tid, lp, top = ops.logprob_record(got[r], nt[r])
        assert tid == tok[r] and abs(lp - float(raw[tok[r]])) <= 1e-4, (r, lp, float(raw[tok[r]]))
        assert lp < -5.0                                                # the raw one: -3 against a thousand N(0, 1)


def dataclass_replace(p, **kw):
    import dataclasses
    return dataclasses.replace(p, **kw)


# ------------------------------------------------------------------ engine
PROMPT = [5, 17, 99, 3, 250, 7, 81, 12]
MOD = tuple((3 * j + 1, (j % 17 - 8) * 0.75 or 0.5) for j in range(300))       # 300 moderate entries


def _mix(banned):
    ban = tuple((t, -100.0) for t in sorted(banned))
    return [
        (PROMPT, dict(max_tokens=40)),
        (PROMPT[:5], dict(max_tokens=14, temperature=0.9, top_k=40, seed=5)),
        (PROMPT, dict(max_tokens=16, logit_bias=ban)),
        (PROMPT[2:], dict(max_tokens=14, temperature=1.1, top_k=40, seed=7, repeat_penalty=1.3, presence_penalty=0.5,
                          logit_bias=MOD)),
        (PROMPT[1:], dict(max_tokens=12, temperature=0.8, top_k=20, seed=9, logit_bias=MOD[:65] + ((1000, 6.0),),
                          logprobs=True, top_logprobs=5)),
        (PROMPT[:3], dict(max_tokens=10, temperature=0.9, top_k=40, seed=11, logit_bias=((777, 100.0),))),
    ]


def _run(m, reqs, graphs, stagger=2, **kw):
    eng = Engine(m, None, max_batch=8, use_graphs=graphs, **kw)
    futs, pending, steps = [], list(reqs), 0
    while pending or not all(f.done() for f in futs):
        if pending and steps % stagger == 0:
            ids, p = pending.pop(0)
            futs.append(eng.submit(GenRequest(list(ids), SamplingParams(ignore_eos=True, **p))))
        eng.step()
        steps += 1
        assert steps < 2000
    return [f.result() for f in futs], eng


@pytest.fixture(scope="module")
def mixed(gpu, tiny_models, tmp_path_factory):
    """The mixed batch (greedy, sampled, biased greedy, biased sampled + penalties, biased + logprobs, forced) with
    decode graphs on and off and with the host-driven sampler, and the unbiased batch for comparison. Prompts are
    prefilled eagerly in all of them (the padded prefill graph rounds differently: tests/test_logprobs_gpu.py)."""
    from nats_llm_studio_amd.engine import engine as E
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), gpu)
    old, E._PREFILL_GRAPHS = E._PREFILL_GRAPHS, False
    mp = pytest.MonkeyPatch()
    dumps = {k: str(tmp_path_factory.mktemp(f"dump_{k}")) for k in ("plain", "biased")}
    try:
        base = _run(m, [(PROMPT, dict(max_tokens=16))], False)[0][0].token_ids
        mix = _mix(set(base))
        plain = [(ids, {k: v for k, v in p.items() if k != "logit_bias"}) for ids, p in mix]
        out = {"mix": mix, "banned": set(base), "dumps": dumps}
        mp.setenv("NLS_GRAPH_DUMP", dumps["plain"])
        out["plain"] = _run(m, plain, True)
        mp.setenv("NLS_GRAPH_DUMP", dumps["biased"])
        out[True] = _run(m, mix, True)
        mp.delenv("NLS_GRAPH_DUMP")
        out[False] = _run(m, mix, False)
        mp.setenv("NLS_DEVICE_SAMPLING", "0")
        out["host"] = _run(m, mix, True)
    finally:
        mp.undo()
        E._PREFILL_GRAPHS = old
    return out


def test_engine_same_tokens_on_every_path(mixed):
    (on, _), (off, _), (host, heng), (plain, _) = mixed[True], mixed[False], mixed["host"], mixed["plain"]
    assert not heng.device_sampling and heng.counters["device_sampled_steps"] == 0
    for (ids, p), a, b, c, d in zip(mixed["mix"], on, off, host, plain):
        print(p.get("logit_bias", ())[:2], a.token_ids)
        assert a.token_ids == b.token_ids == c.token_ids and len(a.token_ids) == p["max_tokens"]
        assert a.logprobs == b.logprobs == c.logprobs
        if "logit_bias" in p:
            assert a.token_ids != d.token_ids
        else:
            assert a.token_ids == d.token_ids                              # the neighbours of biased rows: untouched
    assert not set(on[2].token_ids) & mixed["banned"]
    assert on[5].token_ids == [777] * 10
    assert on[4].logprobs is not None and [e[0] for e in on[4].logprobs] == on[4].token_ids


def test_engine_biased_rows_stay_on_the_chained_graph_path(mixed):
    """Biased rows are drawn in the decode graph, which is the graph of the same batch without biases: the same keys
    and, per key, the same kernel-node list (NLS_GRAPH_DUMP)."""
    (_, eng), (_, base) = mixed[True], mixed["plain"]
    c = eng.counters
    assert c["device_sampled_steps"] > 0 and c["graph_replays"] > 0
    assert c["device_sampled_steps"] == base.counters["device_sampled_steps"]
    assert c["steps"] == base.counters["steps"] and c["graph_replays"] == base.counters["graph_replays"]
    assert set(eng.graphs) == set(base.graphs) and any(len(k) >= 3 and k[2] for k in eng.graphs)
    names = {}
    for k, d in mixed["dumps"].items():
        for f in glob.glob(os.path.join(d, "*dsamp1*.nodes")):
            with open(f) as fh:
                names[k, os.path.basename(f)] = [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]
    files = {f for k, f in names if k == "biased"}
    assert files and files == {f for k, f in names if k == "plain"}
    for f in files:
        assert names["biased", f] == names["plain", f] and len(names["plain", f]) > 0, f
        assert sum("sample_decode_kernel" in x for x in names["plain", f]) == 1, f


def test_engine_recycled_row_forgets_the_bias(gpu, tiny_models):
    """One decode row: a request with 300 entries, then requests with fewer and with none in the same slot."""
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), gpu)
    kw = dict(max_tokens=10, temperature=0.9, top_k=40, seed=3, ignore_eos=True)
    fresh = lambda **k: Engine(m, None, max_batch=1, use_graphs=True).generate(list(PROMPT), SamplingParams(**dict(kw, **k)))
    want, want1 = fresh().token_ids, fresh(logit_bias=MOD[:1]).token_ids
    eng = Engine(m, None, max_batch=1, use_graphs=True)
    full = eng.generate(list(PROMPT), SamplingParams(logit_bias=MOD, **kw)).token_ids
    assert full == fresh(logit_bias=MOD).token_ids and full != want
    assert eng.generate(list(PROMPT), SamplingParams(logit_bias=MOD[:1], **kw)).token_ids == want1
    assert eng.generate(list(PROMPT), SamplingParams(**kw)).token_ids == want
    assert eng.counters["device_sampled_steps"] > 0
    g = SamplingParams(max_tokens=10, ignore_eos=True)
    assert eng.generate(list(PROMPT), g).token_ids == Engine(m, None, max_batch=1).generate(list(PROMPT), g).token_ids


def test_tp2_one_gpu_biased_requests(gpu, tmp_path):
    """Two ranks on the one GPU (parallel/rehearsal.py) with the driver's logit_bias requests: ban (greedy, -100 on
    the tokens of the first greedy request), force (+100) and a seeded top-k row with penalties and 300 entries.
    Their steps are host-driven on the gathered full logits (Engine._cand_ok) and draw what TP=1 draws in its
    decode graph."""
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.parallel import rehearsal
    path = write_synthetic_gguf(str(tmp_path / "llama-3-70b-2layer-Q4_K_M.gguf"), "llama-3-70b-2layer", "Q4_K_M", seed=3)
    os.environ["NLS_REHEARSAL_LOGIT_BIAS"] = "1"
    try:
        r = rehearsal.run(path, world=2, new_tokens=8, timeout=300)
    finally:
        os.environ.pop("NLS_REHEARSAL_LOGIT_BIAS", None)
    for v in (r["ref"], r["tp"], r["followers"][0]):
        assert "exception" not in v, v
    ref, tp = r["ref"]["bias"], r["tp"]["bias"]
    print("TP=1", ref, "TP=2", tp)
    assert ref["device_sampled_steps"] > 0                              # TP=1: in the decode graph
    assert tp["device_sampled_steps"] == 0 and tp["candidate_sampled"] == 0, tp
    assert not set(tp["tokens"][0]) & set(tp["banned"]) and tp["tokens"][1] == [tp["forced"]] * 8
    assert tp["tokens"] == ref["tokens"], (tp["tokens"], ref["tokens"])
    assert r["tp"]["oneshot_resets"] == 0
