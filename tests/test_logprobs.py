"""Per-token logprobs on CPU: request fields, the CPU twin of the logprob kernels, the engine's records on the
chained and the synchronous decode path (first tokens, stops, preemption) against the fp32 oracle, and the
chat_model response / stream shape.

The log-probabilities are those of the model's own distribution: log_softmax of the raw logits at temperature 1,
before penalties and truncation; top entries by descending logit, ties by lower id."""
import json
import math
import shutil
import threading

import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import RequestError, SamplingParams
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.models.llama import LlamaModel


# ------------------------------------------------------------------ request fields
def test_from_request_accepts_and_rejects():
    S = SamplingParams.from_request
    p = S({"temperature": 0})
    assert p.logprobs is False and p.top_logprobs == 0
    p = S({"logprobs": True})
    assert p.logprobs is True and p.top_logprobs == 0
    for n in (0, 1, 5, 20):
        p = S({"logprobs": True, "top_logprobs": n})
        assert p.logprobs and p.top_logprobs == n
    assert S({"logprobs": False, "top_logprobs": 0}).top_logprobs == 0
    assert S({"logprobs": None, "top_logprobs": None}).logprobs is False
    for bad, field in (({"logprobs": True, "top_logprobs": 21}, "top_logprobs"),
                       ({"logprobs": True, "top_logprobs": -1}, "top_logprobs"),
                       ({"logprobs": True, "top_logprobs": 2.5}, "top_logprobs"),
                       ({"logprobs": True, "top_logprobs": True}, "top_logprobs"),
                       ({"top_logprobs": 3}, "top_logprobs"),
                       ({"logprobs": False, "top_logprobs": 3}, "top_logprobs"),
                       ({"logprobs": 1}, "logprobs"),
                       ({"logprobs": "true"}, "logprobs")):
        with pytest.raises(RequestError) as e:
            S(bad)
        assert field in str(e.value), (bad, str(e.value))
    assert issubclass(RequestError, ValueError)


def test_greedy_is_unaffected_by_logprobs():
    S = SamplingParams.from_request
    assert S({"logprobs": True, "top_logprobs": 20}).greedy
    assert S({"temperature": 0, "logprobs": True}).greedy
    assert not S({"temperature": 0.7, "logprobs": True}).greedy
    assert SamplingParams(logprobs=True, top_logprobs=5).greedy
    assert not SamplingParams(logprobs=True, repeat_penalty=1.1).greedy


# ------------------------------------------------------------------ CPU twin
def _twin(logits, n_top, chosen):
    n = logits.shape[0]
    rec = torch.zeros(n, ops.LP_REC, dtype=torch.int32)
    nt = torch.tensor(n_top, dtype=torch.int32)
    ops.token_logprobs(logits, n, nt, rec)
    ops.token_logprobs_pick(logits, n, nt, torch.tensor(chosen, dtype=torch.int32), rec)
    return [ops.logprob_record(rec[i].numpy(), n_top[i]) if n_top[i] >= 0 else None for i in range(n)]


def test_cpu_twin_hand_case():
    pr = [0.1, 0.2, 0.3, 0.4]
    lg = torch.log(torch.tensor([pr, pr, pr]))
    a, b, c = _twin(lg, [2, 0, 4], [1, 3, 0])
    assert a[0] == 1 and abs(a[1] - math.log(0.2)) < 1e-6
    assert [i for i, _ in a[2]] == [3, 2]
    assert all(abs(v - math.log(pr[i])) < 1e-6 for i, v in a[2])
    assert b[0] == 3 and abs(b[1] - math.log(0.4)) < 1e-6 and b[2] == []
    assert [i for i, _ in c[2]] == [3, 2, 1, 0] and abs(c[1] - math.log(0.1)) < 1e-6


def test_cpu_twin_ties_masks_and_skipped_rows():
    eq = torch.full((1, 50), 0.25)
    (r,) = _twin(eq, [5], [7])
    assert [i for i, _ in r[2]] == [0, 1, 2, 3, 4]
    assert all(abs(v + math.log(50)) < 1e-6 for _, v in r[2]) and abs(r[1] + math.log(50)) < 1e-6
    # only 3 finite entries (one -inf mask, NaNs): 3 pairs, the rest is padding dropped on the host
    lg = torch.full((1, 16), float("-inf"))
    lg[0, 5], lg[0, 2], lg[0, 9], lg[0, 11], lg[0, 0] = 1.0, 3.0, 2.0, float("nan"), float("nan")
    (r,) = _twin(lg, [5], [9])
    assert [i for i, _ in r[2]] == [2, 9, 5]
    want = torch.log_softmax(torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64), 0).tolist()
    assert all(abs(v - w) < 1e-6 for (_, v), w in zip(r[2], want)) and abs(r[1] - want[1]) < 1e-6
    # a skipped row (-1) keeps its record; columns past V (vocab padding) never count
    lg = torch.tensor([[0.0, 1.0, 9.0, 9.0], [0.0, 1.0, 9.0, 9.0]])
    rec = torch.full((2, ops.LP_REC), 77, dtype=torch.int32)
    nt = torch.tensor([-1, 2], dtype=torch.int32)
    ops.token_logprobs(lg, 2, nt, rec, V=2)
    ops.token_logprobs_pick(lg, 2, nt, torch.tensor([0, 0], dtype=torch.int32), rec, V=2)
    assert bool((rec[0] == 77).all())
    tid, lp, top = ops.logprob_record(rec[1].numpy(), 2)
    assert tid == 0 and [i for i, _ in top] == [1, 0]
    assert abs(lp - math.log(1 / (1 + math.e))) < 1e-6


# ------------------------------------------------------------------ engine
# Admitted one every second step, finishing in the reverse order (request i: 2 * i + max_tokens decreases): every
# sequence keeps its decode row and rows free up from the top, so the synchronous and the chained engine run the
# same batches step for step and their records can be compared exactly (the CPU GEMMs round differently for
# different batch shapes: the reason test_engine_pressure.py compares tokens up to near-ties).
PROMPTS = [
    ([1, 2, 3, 4, 5], dict(max_tokens=30)),
    ([1, 2, 3, 4, 5], dict(max_tokens=27, logprobs=True, top_logprobs=1)),
    ([9, 8, 7, 6, 5, 4, 3, 2, 1, 11, 12, 13, 14, 15, 16, 17, 18], dict(max_tokens=24, logprobs=True, top_logprobs=20)),
    ([42] * 30, dict(max_tokens=21)),
    ([5, 6], dict(max_tokens=18, logprobs=True, top_logprobs=0)),
    ([3, 1, 4, 1, 5, 9, 2, 6], dict(max_tokens=15, logprobs=True, top_logprobs=20)),
    ([9, 8, 7], dict(max_tokens=1, logprobs=True)),
]


def _engine(m, async_decode, **kw):
    args = dict(max_batch=8, max_prefill_tokens=64, num_blocks=128, use_graphs=False, ctx=256)
    args.update(kw)
    return Engine(m, None, async_decode=async_decode, **args)


def _run(eng, reqs, stagger=2):
    futs, pending, steps = [], list(reqs), 0
    while pending or not all(f.done() for f in futs):
        if pending and steps % stagger == 0:
            ids, kw = pending.pop(0)
            futs.append(eng.submit(GenRequest(list(ids), SamplingParams(ignore_eos=True, **kw))))
        eng.step()
        steps += 1
        assert steps < 5000
    return [f.result() for f in futs]


@pytest.fixture(scope="module")
def runs(tiny_models):
    """One pass of the mixed batch per decode mode, plus the same batch without logprobs (shared, read-only)."""
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), "cpu")
    plain = [(ids, {k: v for k, v in kw.items() if k not in ("logprobs", "top_logprobs")}) for ids, kw in PROMPTS]
    out = {"model": m, "plain": _run(_engine(m, True), plain)}
    for mode in (False, True):
        eng = _engine(m, mode)
        out[mode] = _run(eng, PROMPTS)
        assert all(r is None for r in eng.rows) and eng._inflight is None
    return out


@pytest.mark.parametrize("mode", [False, True])
def test_engine_records(runs, mode):
    for (ids, kw), r, p in zip(PROMPTS, runs[mode], runs["plain"]):
        assert r.token_ids == p.token_ids and len(r.token_ids) == kw["max_tokens"]
        if not kw.get("logprobs"):
            assert r.logprobs is None
            continue
        n = kw.get("top_logprobs", 0)
        assert len(r.logprobs) == len(r.token_ids)
        assert [e[0] for e in r.logprobs] == r.token_ids
        for tid, lp, top in r.logprobs:
            assert len(top) == n and lp <= 0.0
            if n:                                           # greedy: the chosen token leads the list
                assert top[0][0] == tid and top[0][1] == lp
            vals = [v for _, v in top]
            assert vals == sorted(vals, reverse=True)
            assert len({i for i, _ in top}) == len(top)
            assert sum(math.exp(v) for v in vals) <= 1 + 1e-6


def test_engine_records_same_on_both_decode_paths(runs):
    for a, b in zip(runs[False], runs[True]):
        assert a.token_ids == b.token_ids and a.logprobs == b.logprobs


def test_engine_records_match_the_oracle(runs, tiny_models):
    """Teacher-forced fp32 oracle (models/reference.py), fp64 log_softmax. The CPU engine runs the dequantised
    fp32 model: the chosen-token logprobs agree with the oracle's within the bound that
    test_prefill_logits_match_reference applies to logits, 5 % of the oracle's largest |logit|."""
    from nats_llm_studio_amd.models.reference import ReferenceModel
    ref = ReferenceModel(GGUFReader(tiny_models["tiny-llama"]))
    checked = 0
    for (ids, kw), r in zip(PROMPTS, runs[True]):
        if not kw.get("logprobs"):
            continue
        seq = list(ids) + list(r.token_ids)
        rl = ref.logits(seq[:-1]).double()
        bound = 0.05 * float(rl.abs().max())
        lsm = torch.log_softmax(rl, -1)
        for j, (tid, lp, top) in enumerate(r.logprobs):
            row = lsm[len(ids) - 1 + j]
            assert abs(lp - float(row[tid])) <= bound, (j, tid, lp, float(row[tid]), bound)
            if top and tid == int(row.argmax()):
                assert top[0][0] == int(row.argmax())
            checked += 1
    assert checked == 27 + 24 + 18 + 15 + 1


def test_callback_receives_records(tiny_models):
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), "cpu")
    eng = _engine(m, True)
    seen, plain = [], []
    f = eng.submit(GenRequest([1, 2, 3], SamplingParams(max_tokens=4, ignore_eos=True, logprobs=True, top_logprobs=2),
                              on_token=plain.append, on_token_logprobs=lambda t, rec: seen.append((t, rec))))
    g = eng.submit(GenRequest([1, 2, 3], SamplingParams(max_tokens=2, ignore_eos=True),
                              on_token_logprobs=lambda t, rec: seen.append((t, rec))))
    while not (f.done() and g.done()):
        eng.step()
    r = f.result()
    assert plain == r.token_ids
    assert [x for x in seen if x[1] is not None] == [(e[0], e) for e in r.logprobs]
    assert [t for t, rec in seen if rec is None] == g.result().token_ids and g.result().logprobs is None


def test_stop_token_and_eos_entries(tiny_models):
    """The token that ends a generation (a stop id, known one step late on the chained path) has its entry."""
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), "cpu")
    base = _run(_engine(m, False), [([1, 2, 3, 4, 5], dict(max_tokens=12))])[0]
    stop = base.token_ids[4]
    for mode in (False, True):
        eng = _engine(m, mode)
        f = eng.submit(GenRequest([1, 2, 3, 4, 5], SamplingParams(max_tokens=12, ignore_eos=True, logprobs=True,
                                                                  top_logprobs=3, stop_token_ids=[stop])))
        while not f.done():
            eng.step()
        r = f.result()
        assert r.stop_reason == "stopTokenFound" and r.token_ids == base.token_ids[:len(r.token_ids)]
        assert r.token_ids[-1] == stop and [e[0] for e in r.logprobs] == r.token_ids


def test_sampled_request_with_penalties_on_the_host_path(tiny_models):
    """A seeded sampled request (host-driven sampler on CPU) draws the same tokens with and without logprobs,
    and its records are those of the RAW distribution: equal to a greedy request's over the same context."""
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), "cpu")
    kw = dict(max_tokens=8, temperature=0.9, top_k=20, seed=11, repeat_penalty=1.3, presence_penalty=0.5)
    a = _run(_engine(m, True), [([7, 7, 8, 9], kw)])[0]
    b = _run(_engine(m, True), [([7, 7, 8, 9], dict(kw, logprobs=True, top_logprobs=4))])[0]
    assert a.token_ids == b.token_ids and [e[0] for e in b.logprobs] == b.token_ids
    # the first token comes out of the same prefill chunk as a greedy request's: the same top list, to the bit
    c = _run(_engine(m, True), [([7, 7, 8, 9], dict(max_tokens=1, logprobs=True, top_logprobs=4))])[0]
    assert c.logprobs[0][2] == b.logprobs[0][2]
    # every entry against the fp32 oracle's raw distribution (bound: test_engine_records_match_the_oracle)
    from nats_llm_studio_amd.models.reference import ReferenceModel
    rl = ReferenceModel(GGUFReader(tiny_models["tiny-llama"])).logits([7, 7, 8, 9] + b.token_ids[:-1]).double()
    bound, lsm = 0.05 * float(rl.abs().max()), torch.log_softmax(rl, -1)
    for j, (tid, lp, top) in enumerate(b.logprobs):
        assert abs(lp - float(lsm[3 + j, tid])) <= bound
        assert all(abs(v - float(lsm[3 + j, i])) <= bound for i, v in top)


def test_preemption_keeps_one_entry_per_token(tiny_models):
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), "cpu")
    rng = np.random.default_rng(11)
    reqs = [([int(v) for v in rng.integers(20, 200, int(rng.integers(4, 14)))],
             dict(max_tokens=int(rng.integers(60, 100)), logprobs=bool(i % 2 == 0), top_logprobs=2 if i % 2 == 0 else 0))
            for i in range(6)]
    tight = Engine(m, None, max_batch=8, max_prefill_tokens=32, num_blocks=16, use_graphs=False, ctx=256,
                   async_decode=True)
    futs = [tight.submit(GenRequest(list(t), SamplingParams(ignore_eos=True, **kw))) for t, kw in reqs]
    steps = 0
    while not all(f.done() for f in futs):
        tight.gen_ratio = 0.05            # as optimistic as on-demand admission: the pool runs dry mid-decode
        tight.step()
        steps += 1
        assert steps < 5000
    assert tight.counters["preemptions"] > 0, tight.stats()
    for (t, kw), f in zip(reqs, futs):
        r = f.result()
        assert len(r.token_ids) == kw["max_tokens"]
        if kw["logprobs"]:
            assert len(r.logprobs) == len(r.token_ids) and [e[0] for e in r.logprobs] == r.token_ids
            assert all(e[2][0][0] == e[0] for e in r.logprobs)
        else:
            assert r.logprobs is None
    assert tight.alloc.n_free == tight.num_blocks and tight._inflight is None


# ------------------------------------------------------------------ tokenizer + service
def test_sentencepiece_token_bytes():
    from nats_llm_studio_amd.tokenizer.bpe import SentencePieceBPE
    toks = ["<unk>", "<s>", "</s>", "<0xE2>", "<0x82>", "<0xAC>", "▁hi", "▁", "a"]
    types = [2, 3, 3, 6, 6, 6, 1, 1, 1]
    t = SentencePieceBPE(toks, [0.0] * len(toks), types, add_space_prefix=False)
    assert t.token_bytes(3) == b"\xe2" and t.token_bytes(6) == b" hi" and t.token_bytes(8) == b"a"
    ids = [6, 3, 4, 5, 8]
    assert b"".join(t.token_bytes(i) for i in ids).decode() == t.decode(ids) == " hi€a"


@pytest.fixture(scope="module")
def chat_env(tmp_path_factory, tiny_models):
    from nats_llm_studio_amd.natsio import Client, EmbeddedServer
    from nats_llm_studio_amd.service.config import WorkerConfig
    from nats_llm_studio_amd.service.service import Service
    root = tmp_path_factory.mktemp("lp_models")
    md = root / "synthetic" / "tiny-llama-GGUF"
    md.mkdir(parents=True)
    shutil.copy(tiny_models["tiny-llama"], md / "tiny-llama-Q4_K_M.gguf")
    srv = EmbeddedServer().start()
    cfg = WorkerConfig(nats_url=srv.url, models_dir=str(root), backend="engine", device="cpu", max_batch=8,
                       max_ctx=256)
    svc = Service(cfg).start()
    cli = Client().connect(srv.url)
    yield srv, svc, cli
    cli.close()
    svc.stop()
    svc.client.close()
    srv.stop()


def _chat(cli, **kw):
    body = {"model": "tiny-llama", "messages": [{"role": "user", "content": "Hello!"}], "max_tokens": 6,
            "temperature": 0}
    body.update(kw)
    out = json.loads(cli.request("lmstudio.chat_model", json.dumps(body).encode(), 120).data)
    assert out["ok"], out
    return out["data"]["http_status"], out["data"]["response"]


def test_chat_response_shape(chat_env, tiny_models):
    from nats_llm_studio_amd.tokenizer.bpe import tokenizer_from_metadata
    _, _, cli = chat_env
    st, plain = _chat(cli)
    assert st == 200 and plain["choices"][0]["logprobs"] is None
    st, resp = _chat(cli, logprobs=True, top_logprobs=3)
    assert st == 200
    ch = resp["choices"][0]
    assert ch["message"]["content"] == plain["choices"][0]["message"]["content"]
    content = ch["logprobs"]["content"]
    assert len(content) == resp["usage"]["completion_tokens"] > 0
    tok = tokenizer_from_metadata(GGUFReader(tiny_models["tiny-llama"]).metadata)
    text = bytearray()
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert e["token"] == bytes(e["bytes"]).decode("utf-8", errors="replace") and e["logprob"] <= 0
        assert len(e["top_logprobs"]) == 3 and e["top_logprobs"][0]["bytes"] == e["bytes"]
        assert e["top_logprobs"][0]["logprob"] == e["logprob"]
        assert all(set(t) == {"token", "logprob", "bytes"} for t in e["top_logprobs"])
        tid = tok.vocab.get(e["token"])
        if tid is None or not tok.is_control(tid):      # control tokens carry their name, the text skips them
            text += bytes(e["bytes"])
    assert bytes(text) == ch["message"]["content"].encode("utf-8")
    st, resp = _chat(cli, logprobs=True)
    assert st == 200 and all(e["top_logprobs"] == [] for e in resp["choices"][0]["logprobs"]["content"])


@pytest.mark.parametrize("bad,field", [({"logprobs": True, "top_logprobs": 21}, "top_logprobs"),
                                       ({"top_logprobs": 2}, "top_logprobs"),
                                       ({"logprobs": "yes"}, "logprobs")])
def test_chat_bad_fields_are_400(chat_env, bad, field):
    _, _, cli = chat_env
    st, resp = _chat(cli, **bad)
    assert st == 400 and field in resp["error"], resp


def test_chat_stream_chunks_carry_the_entries(chat_env):
    from nats_llm_studio_amd.natsio import Client
    srv, _, cli = chat_env
    sub = Client().connect(srv.url)
    chunks, lock = [], threading.Lock()

    def on_msg(msg):
        with lock:
            chunks.append(json.loads(msg.data))
    sub.subscribe("lp.stream.1", cb=on_msg)
    sub.flush()
    try:
        st, resp = _chat(cli, logprobs=True, top_logprobs=2, stream=True, stream_subject="lp.stream.1", max_tokens=8)
        assert st == 200
        sub.flush()
        final = resp["choices"][0]["logprobs"]["content"]
        assert len(final) == resp["usage"]["completion_tokens"]
        import time
        t_end = time.time() + 5
        got = []
        while time.time() < t_end:
            with lock:
                got = [e for c in chunks for e in (c["choices"][0].get("logprobs") or {"content": []})["content"]]
            if len(got) >= len(final):
                break
            time.sleep(0.01)
        assert got == final
        with lock:
            assert all(c["object"] == "chat.completion.chunk" for c in chunks)
            assert "".join(c["choices"][0]["delta"]["content"] for c in chunks) == resp["choices"][0]["message"]["content"]
    finally:
        sub.close()
