"""Logprobs under tensor parallelism on the GPU: the shard-partial and merge kernels of csrc/kernels/sample.hip
against the fp64 reference (single process, torch.cat standing in for the gather), and the records of the real
engine with 2 ranks sharing the one GPU (parallel/rehearsal.py, tensor and expert parallel): partials, gather and
merge inside the captured decode graphs of every rank. (No rehearsal with 8 ranks: profiles/tp_logprobs.txt,
section 3; eight partials are merged by the kernel test.)"""
import pytest
import torch

import lp_shards as S
from nats_llm_studio_amd import ops

pytestmark = pytest.mark.gpu


def _sharded(gpu, V, W, n):
    """One case through shard_logprobs per column slice, torch.cat, merge_logprobs: (case, buffer, records,
    partials as numpy words)."""
    host, n_top, chosen, ctx, kinds = S.make_case(V, W, n)
    buf = S.padded(host, W)
    per, bounds = S.shard_bounds(V, W)
    lg = buf.to(gpu)
    nt = torch.tensor(n_top, dtype=torch.int32, device=gpu)
    nxt = torch.tensor(chosen, dtype=torch.int32, device=gpu)
    cl = torch.tensor(ctx, dtype=torch.int32, device=gpu)
    parts = []
    for lo, valid in bounds:                               # slice starts are unaligned on purpose (odd row stride)
        part = torch.full((n, ops.LP_REC), S.SENTINEL, dtype=torch.int32, device=gpu)
        ops.shard_logprobs(lg[:, lo:lo + per], n, nt, nxt, lo, valid, part, ctx_len=cl)
        parts.append(part)
    allp = torch.cat(parts, dim=1)
    rec = torch.full((n, ops.LP_REC), S.SENTINEL, dtype=torch.int32, device=gpu)
    ops.merge_logprobs(allp, n, W, nt, nxt, rec, ctx_len=cl)
    torch.cuda.synchronize()
    assert torch.equal(lg.cpu(), buf)                      # the kernels only read the logits
    return (host, n_top, chosen, ctx, kinds), lg, rec.cpu().numpy(), allp.cpu().numpy()


@pytest.mark.parametrize("W", S.WS)
@pytest.mark.parametrize("V", S.VS)
def test_shard_and_merge_kernels_match_reference(gpu, V, W):
    """ids exact, logprobs within 1e-4 absolute of the fp64 log_softmax of the whole row -- the bound
    test_logprobs_gpu._check applies to the single-GPU pair. Skipped rows keep the sentinel in records and partials."""
    for n in S.NS:
        (host, n_top, chosen, ctx, kinds), lg, words, parts = _sharded(gpu, V, W, n)
        hn = host.numpy()
        for r in range(n):
            what = (V, W, n, r, kinds[r], n_top[r], chosen[r])
            if n_top[r] < 0 or ctx[r] <= 0:
                assert (words[r] == S.SENTINEL).all() and (parts[r] == S.SENTINEL).all(), what
                continue
            assert (words[r, 2 + 2 * ops.LP_TOP:] == S.SENTINEL).all(), what       # the record's two pad words
            want = S.reference(hn[r], V, n_top[r], chosen[r])
            tid, lp, top = ops.logprob_record(words[r], n_top[r])
            assert tid == chosen[r], what
            bad = S.mismatch((lp, [i for i, _ in top], [v for _, v in top]), want, 1e-4)
            assert bad is None, (what, bad)
            k = len(want[1])                               # entries past the finite count: (-1, -inf)
            assert (words[r, 2 + ops.LP_TOP + k:2 + 2 * ops.LP_TOP] == -1).all(), what
            assert (words[r, 2 + k:2 + ops.LP_TOP] == -8388608).all(), what          # 0xFF800000: -inf
        if W > 1:
            continue
        # one shard: the merged record against the single-GPU pair on the same rows; each side is within 1e-4 of
        # the same fp64 value
        nt = torch.tensor(n_top, dtype=torch.int32, device=gpu)
        cl = torch.tensor(ctx, dtype=torch.int32, device=gpu)
        rec = torch.full((n, ops.LP_REC), S.SENTINEL, dtype=torch.int32, device=gpu)
        ops.token_logprobs(lg, n, nt, rec, V=V, ctx_len=cl)
        ops.token_logprobs_pick(lg, n, nt, torch.tensor(chosen, dtype=torch.int32, device=gpu), rec, V=V, ctx_len=cl)
        single = rec.cpu().numpy()
        for r in range(n):
            if n_top[r] < 0 or ctx[r] <= 0:
                continue
            a, b = ops.logprob_record(words[r], n_top[r]), ops.logprob_record(single[r], n_top[r])
            bad = S.mismatch((a[1], [i for i, _ in a[2]], [v for _, v in a[2]]),
                             (b[1], [i for i, _ in b[2]], [v for _, v in b[2]]), 2e-4)
            assert a[0] == b[0] and bad is None, (V, n, r, kinds[r], bad)


def test_partial_layout(gpu):
    """The words of a shard partial as the merge (and a reader of the gathered block) relies on them: the raw top
    logits with GLOBAL ids, (-inf, -1) past the finite count, the owner flag with the chosen logit bit for bit, and
    the empty shard's (-inf, 0) with no candidate."""
    V, W, n = 19, 8, 3
    (host, n_top, chosen, ctx, kinds), _, _, parts = _sharded(gpu, V, W, n)
    per, bounds = S.shard_bounds(V, W)
    f = parts.view("float32")
    for r in range(n):
        if n_top[r] < 0 or ctx[r] <= 0:
            continue
        for p, (lo, valid) in enumerate(bounds):
            w, fw = parts[r, 44 * p:44 * p + 44], f[r, 44 * p:44 * p + 44]
            want = S.ref_partial(host[r].numpy()[lo:lo + valid], lo, valid, n_top[r], chosen[r])
            k = len(want["ids"])
            assert w[22:22 + k].tolist() == want["ids"] and (w[22 + k:42] == -1).all(), (r, p, w[22:42])
            assert fw[2:2 + k].tolist() == want["vals"] and (w[2 + k:22] == -8388608).all(), (r, p)
            assert int(w[43]) == int(want["own"]) and (not want["own"] or fw[42] == want["raw"]), (r, p)
            if want["z"] > 0:
                assert fw[0] == want["m"] and abs(fw[1] - want["z"]) <= 1e-5 * want["z"], (r, p, fw[:2], want)
            else:
                assert fw[0] == float("-inf") and fw[1] == 0 and k == 0, (r, p, fw[:2])
    assert bounds[7][1] == 0                               # the empty tail shard was among them


# ------------------------------------------------------------------ the engine, ranks sharing the GPU
@pytest.fixture(autouse=True)
def _epx_checksums(monkeypatch):
    monkeypatch.setenv("NLS_EPX_CHECK", "1")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
    d = tmp_path_factory.mktemp("tp_lp_models")
    out = {}
    for name, ft in (("llama-3-70b-2layer", "Q4_K_M"), ("mixtral-8x7b-1layer", "Q5_K_M")):
        out[name] = write_synthetic_gguf(str(d / f"{name}-{ft}.gguf"), name, ft, seed=3)
    return out


N_TOP = 5
# worst |logprob(TP) - logprob(TP=1)| over the chosen tokens of the greedy rows: logits under TP differ from TP=1 in
# their last bits (the row-parallel sums add in rank order), no bound can be derived; twice the measured worst,
# rounded up to one significant digit (profiles/tp_logprobs.txt: measured 2.387e-3 and 6.127e-4). The runs are
# deterministic per build; the margin covers a re-tune that picks other kernels.
TP_VS_REF = {("llama-3-70b-2layer", 2): 5e-3, ("mixtral-8x7b-1layer", 2): 2e-3}


def _rehearse(monkeypatch, path, world, ep, dump, ref=True, env=()):
    from nats_llm_studio_amd.parallel import rehearsal
    with monkeypatch.context() as mp:                      # (spawned ranks inherit; the caller's values come back)
        mp.setenv("NLS_REHEARSAL_LOGPROBS", str(N_TOP))
        mp.setenv("NLS_GRAPH_DUMP", str(dump))
        for k, v in env:
            mp.setenv(k, v)
        return rehearsal.run(path, world=world, ep=ep, new_tokens=8, ref=ref, timeout=300)


def _check_in_graph(r, world, name):
    """The in-graph run: no exception on any rank, tokens equal TP=1, lp graphs on leader and followers, no RCCL or
    PyTorch node in any captured graph, record structure; returns the worst greedy chosen-logprob distance to TP=1
    (printed; the caller asserts its bound last)."""
    from nats_llm_studio_amd.parallel import rehearsal
    ref, tp = r["ref"], r["tp"]
    ranks = [("ref", ref), ("rank 0", tp)] + [(f"rank {i + 1}", f) for i, f in enumerate(r["followers"])]
    for who, v in ranks:                                   # every rank's report first: the first to fail is the cause
        if v is None or "exception" in v:
            print(f"{who}: {v and v['exception']}\n{v and v.get('tb')}")
    for who, v in ranks:
        assert v is not None and "exception" not in v, (who, v)
    n = len(rehearsal.PROMPTS)
    assert tp["tokens"][:n] == ref["tokens"][:n], (tp["tokens"], ref["tokens"])          # greedy
    diff = [i for i in range(n, len(ref["tokens"])) if tp["tokens"][i] != ref["tokens"][i]]
    assert not diff, (diff, tp["tokens"], ref["tokens"])                                 # seeded top-k
    c = tp["counters"]
    assert c["logprob_steps"] > 0 and c["graph_replays"] > 0 and c["candidate_sampled_steps"] == 0, c
    for fol in r["followers"]:
        assert fol["counters"]["logprob_steps"] == c["logprob_steps"], (fol["counters"], c)
        assert sorted(map(tuple, fol["graphs"])) == sorted(map(tuple, tp["graphs"]))
    assert any(len(k) == 4 for k in tp["graphs"]), tp["graphs"]
    dumps = {f: v for f, v in r["graph_dump"].items() if f.startswith(f"w{world}_")}
    assert {f.split("_")[1] for f in dumps} == {f"r{i}" for i in range(world)}, sorted(r["graph_dump"])
    assert any("_lp1" in f for f in dumps), sorted(dumps)
    for f, v in dumps.items():
        assert v["nodes"] > 0 and v["rccl_nodes"] == 0 and v["torch_nodes"] == 0, (f, v["kernels"])
    assert tp["oneshot_resets"] == 0
    assert tp["comm"].get("gather_words", 0) > 0, tp["comm"]
    reqs = rehearsal._requests(8)
    for i, (_, sp) in enumerate(reqs):
        S.check_structure(tp["tokens"][i], tp["lps"][i], N_TOP, sp.greedy)
        S.check_structure(ref["tokens"][i], ref["lps"][i], N_TOP, sp.greedy)
    worst = max(abs(a[1] - b[1]) for i in range(n) for a, b in zip(tp["lps"][i], ref["lps"][i]))
    print(f"{name} world {world}: worst |logprob(TP) - logprob(TP=1)| over greedy chosen tokens {worst:.3e}")
    return worst


def test_tp2_records_in_graph_and_host_driven(gpu, models, tmp_path, monkeypatch):
    """World 2, Llama-70B 2-layer: the in-graph run, then the same requests with NLS_DEVICE_SAMPLING=0 and
    NLS_TP_CANDIDATES=0 -- every step host-driven: full-logit gather plus the single-GPU kernels on rank 0. Both
    compute on the same rank-ordered logits and each is within 1e-4 of their fp64 value: same tokens, same ids,
    logprobs within 2e-4."""
    name = "llama-3-70b-2layer"
    r = _rehearse(monkeypatch, models[name], 2, False, tmp_path)
    vs_ref = _check_in_graph(r, 2, name)
    h = _rehearse(monkeypatch, models[name], 2, False, tmp_path / "host", ref=False,
                  env=(("NLS_DEVICE_SAMPLING", "0"), ("NLS_TP_CANDIDATES", "0")))
    tp, ht = r["tp"], h["tp"]
    for v in [ht] + h["followers"]:
        assert v is not None and "exception" not in v, v
    assert ht["counters"]["logprob_steps"] == 0 and ht["counters"]["device_sampled_steps"] == 0, ht["counters"]
    assert ht["tokens"] == tp["tokens"]
    worst = 0.0
    for a, b in zip(tp["lps"], ht["lps"]):
        for (ta, la, pa), (tb, lb, pb) in zip(a, b):
            assert ta == tb and [i for i, _ in pa] == [i for i, _ in pb], (a, b)
            worst = max([worst, abs(la - lb)] + [abs(x[1] - y[1]) for x, y in zip(pa, pb)])
    print(f"in-graph (shard partials + merge) vs host-driven (full logits): worst logprob difference {worst:.3e}")
    assert worst <= 2e-4
    assert vs_ref <= TP_VS_REF[(name, 2)], vs_ref


def test_ep2_records_in_graph(gpu, models, tmp_path, monkeypatch):
    name = "mixtral-8x7b-1layer"
    r = _rehearse(monkeypatch, models[name], 2, True, tmp_path)
    vs_ref = _check_in_graph(r, 2, name)
    assert r["tp"]["comm"].get("ep_exchange", 0) > 0, r["tp"]["comm"]
    assert vs_ref <= TP_VS_REF[(name, 2)], vs_ref
