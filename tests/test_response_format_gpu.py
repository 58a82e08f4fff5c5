"""chat_model `response_format` on the GPU: the sampler's allowed-token mask stage through nls_sample_mask (cases and
twin: tests/mask_ref.py; the oracle is the existing entry on a pre-masked copy, no tolerance), its refusals, the engine
on tiny-llama, and one two-rank rehearsal."""
import json
import os

import numpy as np
import pytest
import torch

import grammar_ref as R
import mask_ref as M
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import HIST, SamplingParams, sample_rows_gpu
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.models.llama import LlamaModel
from nats_llm_studio_amd.tokenizer.bpe import tokenizer_from_metadata

pytestmark = pytest.mark.gpu

SENT = -7
PADV = np.float32(1e30)
GUARD = 64
CASES = [(V, pad, v) for V in M.VS for pad in (0, 24) for v in M.VARIANTS]


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


def _params(c, dev, bias=True):
    from nats_llm_studio_amd.ops import _lib
    raw = b""
    for r, p in enumerate(c.params):
        raw += bytes(_lib.SampleParams(p["temperature"], p["top_p"], p["min_p"], p["repeat_penalty"],
                                       p["presence_penalty"], p["frequency_penalty"], c.us[r], int(p["top_k"]),
                                       len(c.hists[r]), len(c.bias.get(r, ())) if bias else 0))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)


def _hist(c, dev):
    h = np.full((len(c.params), HIST), -1, np.int32)
    for r, hh in enumerate(c.hists):
        h[r, :len(hh)] = hh
    return torch.from_numpy(h).to(dev)


def _bias(c, dev, width=4):
    ids = np.full((len(c.params), width), -1, np.int32)
    val = np.zeros((len(c.params), width), np.float32)
    for r, ent in c.bias.items():
        ids[r, :len(ent)] = [t for t, _ in ent]
        val[r, :len(ent)] = [v for _, v in ent]
    return torch.from_numpy(ids).to(dev), torch.from_numpy(val).to(dev)


def _old(dev, buf, ld, V, pb, hd, tabs):
    """The existing entries on a device copy of buf: (tokens, buffer afterwards)."""
    d = torch.from_numpy(buf.copy()).to(dev)
    n = hd.shape[0]
    out = torch.full((n,), SENT, dtype=torch.int32, device=dev)
    if tabs is None:
        rc = _L().nls_sample(d.data_ptr(), ld, n, V, pb.data_ptr(), hd.data_ptr(), HIST, out.data_ptr(), _stream(dev))
    else:
        rc = _L().nls_sample_bias(d.data_ptr(), ld, n, V, pb.data_ptr(), hd.data_ptr(), HIST, tabs[0].data_ptr(),
                                  tabs[1].data_ptr(), tabs[0].shape[1], out.data_ptr(), _stream(dev))
    assert rc == 0
    return out.cpu().numpy().tolist(), d.cpu().numpy()


def _new(dev, buf, ld, V, pb, hd, tabs, mask, rows):
    d = torch.from_numpy(buf.copy()).to(dev)
    n = hd.shape[0]
    out = torch.full((n,), SENT, dtype=torch.int32, device=dev)
    md = torch.from_numpy(mask.view(np.int32).copy()).to(dev)
    rd = torch.from_numpy(np.asarray(rows, np.int32).copy()).to(dev)
    rc = _L().nls_sample_mask(d.data_ptr(), ld, n, V, pb.data_ptr(), hd.data_ptr(), HIST,
                              tabs[0].data_ptr() if tabs else None, tabs[1].data_ptr() if tabs else None,
                              tabs[0].shape[1] if tabs else 0, md.data_ptr(), md.shape[1], rd.data_ptr(), md.shape[0],
                              out.data_ptr(), _stream(dev))
    assert rc == 0
    return out.cpu().numpy().tolist(), d.cpu().numpy()


@pytest.mark.parametrize("V,pad,variant", CASES)
def test_mask_entry_equals_premasked(gpu, V, pad, variant):
    c = M.launch(V, variant, 3 if pad else 0)                # (the padded pitch also takes a table wider than needed)
    raw, ld = _buffer(c.logits, pad)
    pre, _ = _buffer(M.premasked(c), pad)
    hd = _hist(c, gpu)
    eff = M.effective(c)
    for bias in (True, False):                               # without entries: null bias tables
        tabs = _bias(c, gpu) if bias else None
        pb = _params(c, gpu, bias)
        want, left = _old(gpu, pre, ld, V, pb, hd, tabs)
        got, after = _new(gpu, raw, ld, V, pb, hd, tabs, c.mask, c.mask_rows)
        print(c.name, "pad", pad, "bias", bias, "tokens", got, "pre-masked", want)
        assert got == want
        assert all(0 <= t < V and eff[r, t] for r, t in enumerate(got))
        assert got[0] == int(np.argmin(c.logits[0]))         # the one allowed token, the row's minimum
        # the whole buffer is bit-equal to what the existing entry leaves of the pre-masked copy: -inf at the
        # disallowed ids, the existing contract at the allowed ones (bias taken off, penalised history ids
        # rewritten), padding and guard band untouched
        assert np.array_equal(after.view(np.int32), left.view(np.int32))
        rows = after[:len(c.params) * ld].reshape(-1, ld)
        assert np.isneginf(rows[:, :V][~eff]).all()
        pen = {t for t in c.hists[4] if 0 <= t < V}
        keep = eff.copy()
        keep[4, sorted(pen)] = False
        assert np.array_equal(rows[:, :V][keep].view(np.int32), c.logits[keep].view(np.int32))
        outside = np.ones(len(raw), bool)
        for r in range(len(c.params)):
            outside[r * ld: r * ld + V] = False
        assert (after[outside] == PADV).all()
        # the -1 row and the all-ones row: bit-equal to what the existing entry leaves of the RAW rows
        _, plain = _old(gpu, raw, ld, V, pb, hd, tabs)
        for r in (1, 3):
            assert np.array_equal(after[r * ld: r * ld + V].view(np.int32), plain[r * ld: r * ld + V].view(np.int32))


def test_entry_refusals(gpu):
    c = M.launch(1025, 1)
    raw, ld = _buffer(c.logits, 0)
    d = torch.from_numpy(raw.copy()).to(gpu)
    n, L, st = len(c.params), _L(), _stream(gpu)
    pb, hd, (bi, bv) = _params(c, gpu), _hist(c, gpu), _bias(c, gpu)
    md = torch.from_numpy(c.mask.view(np.int32).copy()).to(gpu)
    rd = torch.from_numpy(c.mask_rows.copy()).to(gpu)
    out = torch.full((n,), SENT, dtype=torch.int32, device=gpu)
    need = (c.V + 31) // 32
    for mask, stride, rows, nm, bids, bval in (
            (None, need, rd.data_ptr(), 4, bi.data_ptr(), bv.data_ptr()),           # null mask, rows given
            (md.data_ptr(), need - 1, rd.data_ptr(), 4, bi.data_ptr(), bv.data_ptr()),   # short stride
            (md.data_ptr(), need, rd.data_ptr(), 0, bi.data_ptr(), bv.data_ptr()),   # n_masks 0
            (md.data_ptr(), need, None, 4, bi.data_ptr(), bv.data_ptr()),            # mask without rows
            (md.data_ptr(), need, rd.data_ptr(), 4, bi.data_ptr(), None)):           # half a bias table
        assert L.nls_sample_mask(d.data_ptr(), ld, n, c.V, pb.data_ptr(), hd.data_ptr(), HIST, bids, bval, 4, mask,
                                 stride, rows, nm, out.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [SENT] * n
    assert np.array_equal(d.cpu().numpy().view(np.int32), raw.view(np.int32))


def test_sample_rows_gpu_routes_masks(gpu):
    """engine.sampling.sample_rows_gpu: masks -> nls_sample_mask (with and without bias entries), the tokens of the
    pre-masked rows;
    no mask -> the entries it always took."""
    for c in (M.launch(1025, 1), M.launch(33, 6)):
        for bias in (True, False):
            ps = [SamplingParams(temperature=p["temperature"], top_k=p["top_k"], repeat_penalty=p["repeat_penalty"],
                                 presence_penalty=p["presence_penalty"], frequency_penalty=p["frequency_penalty"],
                                 logit_bias=tuple(sorted((int(t), float(v)) for t, v in c.bias.get(r, ()))) if bias else ())
                  for r, p in enumerate(c.params)]
            masks = [c.mask[tr] if tr >= 0 else None for tr in c.mask_rows]
            lg = torch.from_numpy(c.logits.copy()).to(gpu)
            got = sample_rows_gpu(lg, ps, [list(h) for h in c.hists], list(c.us), masks)
            pre = torch.from_numpy(M.premasked(c)).to(gpu)
            assert got == sample_rows_gpu(pre, ps, [list(h) for h in c.hists], list(c.us))
            assert torch.isneginf(lg[0]).sum().item() == c.V - 1         # left -inf in the buffer it was given
            free = sample_rows_gpu(torch.from_numpy(c.logits.copy()).to(gpu), ps, [list(h) for h in c.hists], list(c.us))
            assert free == sample_rows_gpu(torch.from_numpy(c.logits.copy()).to(gpu), ps, [list(h) for h in c.hists],
                                           list(c.us), [None] * 5)
            assert free != got


# ------------------------------------------------------------------ engine
PROMPT = [5, 17, 99, 3, 250, 7, 81, 12]
FINITE = {"type": "object", "properties": {"k": {"enum": ["a", "b"]}, "f": {"type": "boolean"}},
          "required": ["k", "f"]}
RF = {"type": "json_schema", "json_schema": {"schema": FINITE}}
CAP = R.longest_sentence_bytes(FINITE) + 1


@pytest.fixture(scope="module")
def model(gpu, tiny_models):
    r = GGUFReader(tiny_models["tiny-llama"])
    return LlamaModel(r, gpu), tokenizer_from_metadata(r.metadata)


def _engine(model, **kw):
    return Engine(model[0], model[1], max_batch=8, use_graphs=True, **kw)


def _p(eng, **req):
    return SamplingParams.from_request(req, vocab=eng.cfg.vocab, grammar_vocab=eng.grammar_vocab)


def _run(eng, reqs, stagger=2):
    futs, pending, steps = [], list(reqs), 0
    while pending or not all(f.done() for f in futs):
        if pending and steps % stagger == 0:
            ids, p = pending.pop(0)
            futs.append(eng.submit(GenRequest(list(ids), p)))
        eng.step()
        steps += 1
        assert steps < 3000
    return [f.result() for f in futs]


def _content(eng, res):
    return b"".join(eng.tok.token_bytes(t) for t in res.token_ids if t not in eng.eos)


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.9, seed=7)])
def test_engine_finite_schema(model, sampling, monkeypatch):
    eng = _engine(model)
    res = eng.generate(PROMPT, _p(eng, response_format=RF, max_tokens=CAP, **sampling))
    print(sampling, res.token_ids, _content(eng, res))
    assert res.finish_reason == "stop" and res.error is None, res
    assert len(res.token_ids) <= CAP and res.token_ids[-1] in eng.eos
    content = _content(eng, res)
    assert R.is_sentence(FINITE, content) and R.validate(FINITE, json.loads(content))
    assert eng.counters["constrained_steps"] > 0
    monkeypatch.setenv("NLS_DEVICE_SAMPLING", "0")
    host = _engine(model)
    assert not host.device_sampling
    assert host.generate(PROMPT, _p(host, response_format=RF, max_tokens=CAP, **sampling)).token_ids == res.token_ids


def test_engine_unconstrained_rows_and_graphs(model):
    free = [(PROMPT, dict(temperature=0, max_tokens=150, ignore_eos=True)),
            ([9, 8, 7, 6], dict(temperature=0.8, seed=3, top_k=40, max_tokens=150, ignore_eos=True))]
    cons = [([4, 4, 2], dict(temperature=0.9, seed=1, max_tokens=CAP, response_format=RF)),
            ([3, 1, 4, 1, 5], dict(temperature=0, max_tokens=CAP, response_format=RF))]
    base = _engine(model)
    alone = _run(base, [(ids, _p(base, **kw)) for ids, kw in free])
    assert base.counters["constrained_steps"] == 0
    eng = _engine(model)
    solo = [_engine(model).generate(ids, _p(eng, **kw)) for ids, kw in cons]
    mix = _run(eng, [(ids, _p(eng, **kw)) for ids, kw in free + cons])
    assert [r.token_ids for r in mix[:2]] == [r.token_ids for r in alone]
    assert [r.token_ids for r in mix[2:]] == [r.token_ids for r in solo]
    assert all(r.finish_reason == "stop" and R.is_sentence(FINITE, _content(eng, r)) for r in mix[2:])
    assert eng.counters["constrained_steps"] > 0 and eng.counters["graph_replays"] > 0
    # steps without constrained rows run the graphs they ran: the chained-step graphs are those of the run with no
    # constrained request, and the constrained steps' graphs are the plain logits variant (no new node)
    chained = lambda e: {k for k in e.graphs if not k[1]}
    assert chained(eng) == chained(base) and chained(base)
    assert all(k == (k[0], True) for k in set(eng.graphs) - chained(eng))
    assert all(r is None for r in eng.rows) and eng._inflight is None


def test_engine_logprobs_are_the_models_own(model):
    eng = _engine(model)
    kw = dict(temperature=0, max_tokens=4, logprobs=True, top_logprobs=5)
    plain = eng.generate(PROMPT, _p(eng, ignore_eos=True, **kw))
    cons = eng.generate(PROMPT, _p(eng, response_format=RF, **kw))
    (t0, lp0, top0), (t1, lp1, top1) = plain.logprobs[0], cons.logprobs[0]
    assert top0 == top1
    assert t1 == cons.token_ids[0] and eng.tok.token_bytes(t1)[:1] == b"{" and t1 != t0 and lp1 < lp0


def test_tp2_one_gpu_constrained_requests(gpu, tmp_path):
    """Two ranks on the one GPU (parallel/rehearsal.py) with the driver's response_format requests: their steps are
    host-driven on the gathered full logits (Engine._cand_ok) and draw what TP=1 draws."""
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    from nats_llm_studio_amd.parallel import rehearsal
    path = write_synthetic_gguf(str(tmp_path / "llama-3-70b-2layer-Q4_K_M.gguf"), "llama-3-70b-2layer", "Q4_K_M", seed=3)
    os.environ["NLS_REHEARSAL_RESPONSE_FORMAT"] = "1"
    try:
        r = rehearsal.run(path, world=2, new_tokens=8, timeout=300)
    finally:
        os.environ.pop("NLS_REHEARSAL_RESPONSE_FORMAT", None)
    for v in (r["ref"], r["tp"], r["followers"][0]):
        assert "exception" not in v, v
    ref, tp = r["ref"]["constrained"], r["tp"]["constrained"]
    print("TP=1", ref, "TP=2", tp)
    assert tp["tokens"] == ref["tokens"], (tp["tokens"], ref["tokens"])
    assert tp["finish"] == ["stop", "stop", "length"]
    for text in tp["content"]:
        assert R.is_sentence(FINITE, text.encode()) and R.validate(FINITE, json.loads(text))
    assert tp["constrained_steps"] > 0 and tp["candidate_sampled"] == 0, tp
    assert r["tp"]["oneshot_resets"] == 0
