"""chat_model `logit_bias` without a GPU: request validation, the 400 of the service, the CPU sampler, the CPU engine,
tensor parallelism over gloo, and the self-test of the inputs that tests/test_logit_bias_gpu.py runs on the device
(tests/logit_bias_ref.py: the case list and a fault-switchable numpy twin of the kernel's bias stage).

The oracle has no tolerance: a biased call on raw logits returns exactly the tokens of the unbiased call on a copy whose
biased entries were pre-added in float32."""
import dataclasses
import json
import math
import shutil

import numpy as np
import pytest
import torch

import logit_bias_ref as B
import sampler_ref as S
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import (LOGIT_BIAS_MAX, RequestError, SamplingParams, bias_tables,
                                                 sample_rows)
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.models.llama import LlamaModel


# ------------------------------------------------------------------ validation
BAD = [
    [[1, 2.0]],                                   # llama.cpp's array form
    "{}", 3, True, [],                            # not an object
    {"-1": 1}, {"+1": 1}, {"01": 1}, {" 1": 1}, {"1 ": 1}, {"1.0": 1}, {"": 1}, {"abc": 1}, {"١": 1}, {"1e2": 1},
    {"1": True}, {"1": False}, {"1": "2"}, {"1": None}, {"1": [1]},
    {"1": float("nan")}, {"1": float("inf")}, {"1": -float("inf")}, {"1": 100.5}, {"1": -101}, {"1": 10 ** 400},
    {"99999999999": 1},                           # past any vocabulary, with or without `vocab`
    {str(i): 1 for i in range(LOGIT_BIAS_MAX + 1)},
]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b)[:24] for b in BAD])
def test_from_request_rejects(bad):
    with pytest.raises(RequestError) as e:
        SamplingParams.from_request({"logit_bias": bad})
    assert "'logit_bias'" in str(e.value)


def test_from_request_accepts():
    F = SamplingParams.from_request
    plain = F({"temperature": 0.7})
    for none in ({}, {"logit_bias": None}, {"logit_bias": {}}, {"logit_bias": {"5": 0}, }, {"logit_bias": {"5": 0.0}}):
        assert F(dict(none, temperature=0.7)) == plain
    assert plain.logit_bias == () and F({}).greedy
    p = F({"logit_bias": {"7": -100, "0": 100, "12": 0, "3": 1.5}})
    assert p.logit_bias == ((0, 100.0), (3, 1.5), (7, -100.0))          # sorted, zero dropped, floats
    assert not p.greedy and p.temperature == 0.0                        # temperature 0 + bias: the sampler's arg-max
    full = {str(i): 1 for i in range(LOGIT_BIAS_MAX)}
    assert len(F({"logit_bias": full}).logit_bias) == LOGIT_BIAS_MAX
    with pytest.raises(RequestError):
        F({"logit_bias": dict(full, **{"1000": 1})})
    # the vocabulary bounds the ids only when it is given
    assert F({"logit_bias": {"5000": 1}}).logit_bias == ((5000, 1.0),)
    assert F({"logit_bias": {"999": 1}}, vocab=1000).logit_bias == ((999, 1.0),)
    with pytest.raises(RequestError) as e:
        F({"logit_bias": {"1000": 1}}, vocab=1000)
    assert "'logit_bias'" in str(e.value) and "1000" in str(e.value)


def test_bias_tables():
    ps = [SamplingParams(), SamplingParams(logit_bias=((3, 1.0), (9, -2.0))), SamplingParams(logit_bias=((1, 4.0),))]
    assert bias_tables(ps[:1]) is None
    ids, val = bias_tables(ps)
    assert ids.dtype == np.int32 and val.dtype == np.float32
    assert ids.tolist() == [[-1, -1], [3, 9], [1, -1]] and val.tolist() == [[0, 0], [1, -2], [4, 0]]
    assert bias_tables(ps, 5)[0].shape == (3, 5)


# ------------------------------------------------------------------ service
@pytest.fixture(scope="module")
def chat_env(tmp_path_factory, tiny_models):
    from nats_llm_studio_amd.natsio import Client, EmbeddedServer
    from nats_llm_studio_amd.service.config import WorkerConfig
    from nats_llm_studio_amd.service.service import Service
    root = tmp_path_factory.mktemp("lb_models")
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


@pytest.mark.parametrize("bad", [[[1, 2.0]], {"x": 1}, {"1": 101}, {"1024": 1}, {"1": True}],
                         ids=["array", "key", "range", "vocab", "bool"])
def test_chat_bad_logit_bias_is_400(chat_env, bad):
    """The engine backend answers an illegal logit_bias as it answers an illegal top_logprobs: http_status 400 and an
    error that names the field ({"1024": 1}: the loaded model has 1024 tokens, the backend passes its vocabulary)."""
    _, _, cli = chat_env
    st, resp = _chat(cli, logit_bias=bad)
    assert st == 400 and "'logit_bias'" in resp["error"], resp


def test_chat_applies_logit_bias(chat_env):
    _, _, cli = chat_env
    st, plain = _chat(cli)
    st2, same = _chat(cli, logit_bias={})
    st3, forced = _chat(cli, logit_bias={"1023": 100}, logprobs=True)
    assert st == st2 == st3 == 200
    assert same["choices"][0]["message"]["content"] == plain["choices"][0]["message"]["content"]
    ents = forced["choices"][0]["logprobs"]["content"]
    assert len(ents) == 6 and len({e["token"] for e in ents}) == 1
    assert forced["choices"][0]["message"]["content"] != plain["choices"][0]["message"]["content"]


# ------------------------------------------------------------------ CPU sampler
def _sp(p, lb=()):
    return SamplingParams(logit_bias=tuple(sorted(lb)), **p)


CPU_PARAMS = B.PARAMS + (S.P(temperature=0.9, top_k=S.KFAST), S.P(temperature=0.7, top_p=0.9, min_p=0.05))


def test_sample_rows_equals_prebiased():
    """engine.sampling.sample_rows with logit_bias against itself on the pre-biased copy: every launch of the case
    list below 100000 tokens, each row under every parameter set (temperature 0, top-k below, at and above KFAST,
    top-p / min-p, penalties whose window holds biased ids)."""
    n = 0
    for c in B.launches(big=False):
        pre = torch.from_numpy(B.prebiased(c))
        raw = torch.from_numpy(c.logits.copy())
        for p in CPU_PARAMS:
            ps = [_sp(p, [(int(t), float(v)) for t, v in zip(c.ids[r, :c.nb[r]], c.vals[r, :c.nb[r]])])
                  for r in range(len(c.nb))]
            got = sample_rows(raw, ps, [list(h) for h in c.hists], list(c.us))
            want = sample_rows(pre, [_sp(p)] * len(ps), [list(h) for h in c.hists], list(c.us))
            assert got == want, (c.name, p, got, want)
            n += len(got)
        assert torch.equal(raw.view(torch.int32), torch.from_numpy(c.logits).view(torch.int32))    # rows untouched
    assert n == 12 * 5 * len(CPU_PARAMS)


def test_sample_rows_matches_the_twin():
    """... and against the definition (the numpy twin over tests/sampler_ref.py), so the pre-biased copy is not the
    only witness. The twin's variates are not placed away from the CDF steps here: a token may differ only where
    the variate lies within 8e-7 of a step of the reference's CDF (sampler_ref.accepted)."""
    for c in B.launches(big=False):
        ps = [_sp(c.params[r], [(int(t), float(v)) for t, v in zip(c.ids[r, :c.nb[r]], c.vals[r, :c.nb[r]])])
              for r in range(len(c.nb))]
        got = sample_rows(torch.from_numpy(c.logits.copy()), ps, [list(h) for h in c.hists], list(c.us))
        pre = B.prebiased(c)
        for r, t in enumerate(got):
            ref = S.ref_row(pre[r], c.params[r], c.hists[r])
            assert S.accepted(ref, c.us[r], t, 8e-7), (c.name, r, t, S.draw(ref, c.us[r]))
        assert B.twin(c, calls=1)[0][0] == [S.draw(S.ref_row(pre[r], c.params[r], c.hists[r]), c.us[r]) or 0
                                            for r in range(len(got))]


# ------------------------------------------------------------------ the GPU inputs notice each fault
def test_case_list_notices_each_fault():
    """Each fault of the twin changes a token of the case list of tests/test_logit_bias_gpu.py (host-driven inputs,
    in-graph inputs, second call on the same buffer; the 128256-token launches are left to variants 0 and 3 here, for
    run time) -- and the twin without a fault restores every row and repeats its tokens."""
    seen = {f: 0 for f in B.FAULTS}
    for c in B.launches():
        if c.V > 100000 and c.name[-1] not in "03":
            continue
        unpen = [r for r in range(len(c.nb)) if not S.penal(c.params[r])]
        for decode in (False, True):
            good, after = B.twin(c, decode)
            assert np.array_equal(after.view(np.int32), c.logits.view(np.int32))
            assert [good[0][r] for r in unpen] == [good[1][r] for r in unpen]
            for f in B.FAULTS:
                if f == "skip0" and not decode:
                    continue
                bad, _ = B.twin(c, decode, fault=f)
                seen[f] += sum(a != b for a, b in zip(good[0], bad[0]))
                seen[f] += sum(good[1][r] != bad[1][r] for r in unpen)
    print("tokens changed per fault:", seen)
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------ CPU engine
PROMPT = [5, 17, 99, 3, 250, 7, 81, 12]


def _engine(m, **kw):
    args = dict(max_batch=4, max_prefill_tokens=64, num_blocks=64, use_graphs=False, ctx=256)
    args.update(kw)
    return Engine(m, None, **args)


def _gen(eng, prompt, **kw):
    return eng.generate(list(prompt), SamplingParams(ignore_eos=True, **kw))


@pytest.fixture(scope="module")
def model(tiny_models):
    return LlamaModel(GGUFReader(tiny_models["tiny-llama"]), "cpu")


@pytest.mark.parametrize("async_decode", [False, True])
def test_engine_bans_and_forces(model, async_decode):
    eng = _engine(model, async_decode=async_decode)
    base = _gen(eng, PROMPT, max_tokens=12)
    banned = sorted(set(base.token_ids))
    r = _gen(eng, PROMPT, max_tokens=12, logit_bias=tuple((t, -100.0) for t in banned))
    assert len(r.token_ids) == 12 and not set(r.token_ids) & set(banned), (r.token_ids, banned)
    tok = 777
    assert tok not in base.token_ids
    for kw in (dict(), dict(temperature=0.9, top_k=40, seed=3), dict(temperature=1.0, seed=4, repeat_penalty=1.3)):
        r = _gen(eng, PROMPT, max_tokens=8, logit_bias=((tok, 100.0),), **kw)
        assert r.token_ids == [tok] * 8, (kw, r.token_ids)               # the first token too
    # logprobs stay those of the model's own distribution: the forced token's are far below the raw arg-max's
    r = _gen(eng, PROMPT, max_tokens=3, logit_bias=((tok, 100.0),), logprobs=True, top_logprobs=2)
    b = _gen(eng, PROMPT, max_tokens=1, logprobs=True, top_logprobs=2)
    assert r.logprobs[0][0] == tok and r.logprobs[0][2] == b.logprobs[0][2]     # same context: the same top list
    assert r.logprobs[0][1] < b.logprobs[0][1] and all(e[0] == tok and e[1] < e[2][0][1] for e in r.logprobs)


def test_engine_recycled_row_forgets_the_bias(model):
    """One decode row: a biased request, then an unbiased one in the same slot, which reproduces a fresh engine's."""
    want = _gen(_engine(model, max_batch=1), PROMPT, max_tokens=10, temperature=0.9, top_k=40, seed=3).token_ids
    eng = _engine(model, max_batch=1)
    biased = _gen(eng, PROMPT, max_tokens=10, temperature=0.9, top_k=40, seed=3,
                  logit_bias=tuple((t, -100.0) for t in sorted(set(want))))
    assert not set(biased.token_ids) & set(want)
    assert _gen(eng, PROMPT, max_tokens=10, temperature=0.9, top_k=40, seed=3).token_ids == want
    assert _gen(eng, PROMPT, max_tokens=10).token_ids == _gen(_engine(model), PROMPT, max_tokens=10).token_ids


# ------------------------------------------------------------------ tensor parallel
def test_cand_ok_is_false_with_a_biased_row(model):
    eng = _engine(model)
    eng.tp = object()                           # (_cand_ok only asks whether there is a group)
    seq = lambda **kw: type("Q", (), {"req": type("R", (), {"params": SamplingParams(**kw)})})
    ok = [seq(temperature=0.8, top_k=40), seq()]
    assert eng._cand_ok(ok)
    assert not eng._cand_ok(ok + [seq(temperature=0.8, top_k=40, logit_bias=((3, -1.0),))])
    assert not eng._cand_ok(ok + [seq(logit_bias=((3, 5.0),))])


def test_tp2_gloo_matches_tp1(tmp_path):
    """The rehearsal driver on gloo with its logit_bias requests (ban / force / 300 moderate entries on a seeded
    top-k row with penalties): two ranks draw what TP=1 draws (host-driven there on the CPU), on the gathered full
    logits -- no candidate draw, no in-step draw for those steps."""
    import os
    from nats_llm_studio_amd.gguf.synth import SPECS, write_synthetic_gguf
    from nats_llm_studio_amd.parallel import rehearsal
    spec = dataclasses.replace(SPECS["tiny-llama"], name="tp-llama", d_ff=1024)
    path = str(tmp_path / "tp-llama.gguf")
    write_synthetic_gguf(path, spec.name, "Q4_K_M", seed=4, spec=spec)
    os.environ["NLS_REHEARSAL_LOGIT_BIAS"] = "1"
    try:
        r = rehearsal.run(path, world=2, new_tokens=5, timeout=240, device="cpu")
    finally:
        os.environ.pop("NLS_REHEARSAL_LOGIT_BIAS", None)
    for v in (r["ref"], r["tp"], r["followers"][0]):
        assert "exception" not in v, v
    ref, tp = r["ref"]["bias"], r["tp"]["bias"]
    assert tp["tokens"] == ref["tokens"], (tp["tokens"], ref["tokens"])
    assert not set(tp["tokens"][0]) & set(tp["banned"]) and tp["tokens"][1] == [tp["forced"]] * 5
    assert tp["device_sampled_steps"] == 0 and tp["candidate_sampled"] == 0, tp
    assert r["tp"]["tokens"] == r["ref"]["tokens"]
