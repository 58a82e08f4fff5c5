"""Logprobs under tensor parallelism on the CPU: the fp64 twins of the shard-partial / merge ops, the self-test of
the kernel test's inputs (every fault of the merge they must notice), the gloo TP=2 engine against TP=1 and a chat
request with logprobs on a TP=2 worker."""
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

import lp_shards as S
from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf.synth import write_synthetic_gguf
from test_parallel import _TP_SPECS, _engine, _free_port, _tp_worker_main


def _twins(host, W, n_top, chosen, ctx):
    n, V = host.shape
    buf = S.padded(host, W)
    per, bounds = S.shard_bounds(V, W)
    nt = torch.tensor(n_top, dtype=torch.int32)
    nxt = torch.tensor(chosen, dtype=torch.int32)
    cl = torch.tensor(ctx, dtype=torch.int32)
    parts = []
    for lo, valid in bounds:
        part = torch.full((n, ops.LP_REC), S.SENTINEL, dtype=torch.int32)
        ops.shard_logprobs(buf[:, lo:lo + per], n, nt, nxt, lo, valid, part, ctx_len=cl)
        parts.append(part)
    rec = torch.full((n, ops.LP_REC), S.SENTINEL, dtype=torch.int32)
    ops.merge_logprobs(torch.cat(parts, dim=1), n, W, nt, nxt, rec, ctx_len=cl)
    return rec.numpy()


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("V", [19, 1000, 1025])
def test_twins_match_reference(V, W):
    """The CPU twins over W column slices of width ceil(V / W) against the fp64 log_softmax of the whole row: ids
    exact, logprobs within 1e-6. A record holds f32 logprobs, so the rows are those whose logprobs stay below 16 in
    magnitude (an f32 there is within 4.8e-7 of the fp64 value; the partial's f32 sum adds 6e-8): the chosen token is
    one of the 50 most likely. Larger magnitudes are the kernel test's, at its 1e-4.

    The rows with a dead shard (an empty partial), with shard maxima 1e4 apart (a rescale that underflows to 0) and
    with the top 20 in one shard are here too, under the same rule: their chosen token, and every top entry that is
    compared, lies in the shard that stayed up (far_maxima and, at V = 19, top_in_one ask for one top entry: the
    second would be 1e4, or 40, below)."""
    g = torch.Generator().manual_seed(31 * V + W)
    kinds = ("randn", "masked", "shift_up", "equal", "cut_ties", "top_spread", "shard_ties", "shift_down", "dead_shard",
             "far_maxima", "top_in_one")
    n = len(kinds)
    host = torch.stack([S.shard_row(k, V, W, r % W, g) for r, k in enumerate(kinds)])
    n_top = [S.N_TOPS[r % len(S.N_TOPS)] for r in range(7)] + [20, 5, 1, 20 if V >= 1000 else 1]
    ctx = [1 + r for r in range(n)]
    ctx[3] = 0
    _, bounds = S.shard_bounds(V, W)
    lim = []
    for r, k in enumerate(kinds):
        up = bounds[r % W][1]                              # the columns of the shard the kind singles out
        if k == "top_spread":                              # (lifts its 21 largest entries 40 above the rest)
            lim.append(min(20, V))
        elif k in ("far_maxima", "top_in_one") and up:
            lim.append(min(20, up))
        else:
            lim.append(min(50, V, int((host[r] > float("-inf")).sum())))
    chosen = [int(torch.topk(host[r], lim[r]).indices[(7 * r + W) % lim[r]]) for r in range(n)]
    chosen[2] = -1
    words = _twins(host, W, n_top, chosen, ctx)
    for r in range(n):
        if n_top[r] < 0 or ctx[r] <= 0:
            assert (words[r] == S.SENTINEL).all()
            continue
        want = S.reference(host[r].numpy(), V, n_top[r], chosen[r])
        tid, lp, top = ops.logprob_record(words[r], n_top[r])
        assert tid == chosen[r]
        bad = S.mismatch((lp, [i for i, _ in top], [v for _, v in top]), want, 1e-6)
        assert bad is None, (V, W, r, kinds[r], bad)


def test_twins_on_a_row_with_no_finite_entry():
    """What the single-GPU pair writes for such a row: no top entry, the chosen entry is the raw logit."""
    host = torch.full((2, 10), float("-inf"))
    host[1, 4] = float("nan")
    n_top, chosen, ctx = [3, 3], [2, 4], [1, 1]
    a = _twins(host, 2, n_top, chosen, ctx)
    rec = torch.full((2, ops.LP_REC), S.SENTINEL, dtype=torch.int32)
    nt = torch.tensor(n_top, dtype=torch.int32)
    ops.token_logprobs(host, 2, nt, rec)
    ops.token_logprobs_pick(host, 2, nt, torch.tensor(chosen, dtype=torch.int32), rec)
    for r in range(2):
        x, y = ops.logprob_record(a[r], 3), ops.logprob_record(rec.numpy()[r], 3)
        assert x[0] == y[0] and x[2] == y[2] == []
        assert x[1] == y[1] or (math.isnan(x[1]) and math.isnan(y[1]))


def _cases():
    for V in S.VS:
        for W in S.WS:
            for n in S.NS:
                yield V, W, n


def test_kernel_test_inputs_reject_every_merge_fault():
    """The inputs of test_shard_and_merge_kernels_match_reference against an fp64 reference of the partial / merge
    pair: the faultless pair is within 1e-9 of the row's log_softmax on every case, and each fault is noticed on some
    row -- an id mismatch, or an error of at least 10x the kernel test's 1e-4 bound."""
    left = set(S.MUTANTS)
    for V, W, n in _cases():
        host, n_top, chosen, ctx, kinds = S.make_case(V, W, n)
        buf = S.padded(host, W).numpy()
        want = [None if n_top[r] < 0 or ctx[r] <= 0 else S.reference(buf[r], V, n_top[r], chosen[r]) for r in range(n)]
        if V <= 1025 or n == 3:                            # (the large vocabularies: one launch size is enough)
            for r, got in enumerate(S.ref_rows(buf, V, W, n_top, chosen, ctx)):
                assert (got is None) == (want[r] is None)
                if got is not None:
                    bad = S.mismatch(got, want[r], 1e-9 * max(1.0, abs(want[r][0]) if math.isfinite(want[r][0]) else 1))
                    assert bad is None, (V, W, n, r, kinds[r], bad)
        for m in sorted(left):
            got = S.ref_rows(buf, V, W, n_top, chosen, ctx, mutant=m)
            if any(g is not None and S.mismatch(g, w, 1e-3) is not None for g, w in zip(got, want)):
                left.discard(m)
    assert not left, f"faults that no input of the kernel test notices: {sorted(left)}"


@pytest.mark.parametrize("W", S.WS)
@pytest.mark.parametrize("V", S.VS)
def test_kernel_test_inputs_hold_every_case(V, W):
    """What the computed rows of the kernel test's launches hold at every (V, W), so that no case is only named:
    every row kind; a cross-shard tie across the cut of n_top 1, 5 and 20 in a row that asks for exactly that n_top
    (where the row has the cut + 2 entries it takes); the chosen token owned by every rank that holds an id, and by
    every such rank with a token outside the top 20 (where there are more than 20); chosen = -1, a chosen id past
    the vocabulary, the arg-max."""
    c = S.coverage(V, W)
    _, bounds = S.shard_bounds(V, W)
    live = {p for p, (_, valid) in enumerate(bounds) if valid}
    assert c["kinds"] == set(S.ALL_KINDS), set(S.ALL_KINDS) - c["kinds"]
    assert c["cuts"] == ({a for a in (1, 5, 20) if a + 2 <= V} if W > 1 else set()), c["cuts"]
    assert c["owners"] == live, live - c["owners"]
    assert V <= 20 or c["low_owners"] == live, live - c["low_owners"]
    assert c["chosen"]["none"] and c["chosen"]["tail"] and c["chosen"]["argmax"], c["chosen"]
    assert len(c["chosen"]["own"]) >= 6, c["chosen"]       # the chosen token is not tied to a few kinds
    # every expected logprob fits the record's f32 with most of the kernel test's 1e-4 left for the kernels
    assert c["f32_err"] <= 1e-5, c["f32_err"]


# ------------------------------------------------------------------ gloo TP=2 engine
PROMPTS = [[1, 5, 9, 200, 31, 7, 77], [1, 300, 301, 302], [1, 17, 400, 23, 9]]


def _lp_run(eng):
    """Greedy + top_logprobs 20, seeded top-k + top_logprobs 5 and a short repeat_penalty 0.7 row: while that one
    runs every TP step is host-driven (full-logit gather); once it is done the other two chain again."""
    from nats_llm_studio_amd.engine.engine import GenRequest
    from nats_llm_studio_amd.engine.sampling import SamplingParams
    ps = [SamplingParams(max_tokens=10, ignore_eos=True, logprobs=True, top_logprobs=20),
          SamplingParams(max_tokens=10, temperature=0.9, top_k=20, seed=11, ignore_eos=True, logprobs=True,
                         top_logprobs=5),
          SamplingParams(max_tokens=4, temperature=0.8, top_k=10, repeat_penalty=0.7, seed=22, ignore_eos=True,
                         logprobs=True, top_logprobs=3)]
    futs = [eng.submit(GenRequest(list(p), sp)) for p, sp in zip(PROMPTS, ps)]
    while not all(f.done() for f in futs):
        eng.step()
    return [(f.result().token_ids, f.result().logprobs) for f in futs], dict(eng.counters)


def _lp_worker(rank, world, port, path, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    from nats_llm_studio_amd.models.llama import ShardSpec
    from nats_llm_studio_amd.parallel.comm import init_distributed
    import torch.distributed as dist
    comm = init_distributed("cpu")
    try:
        eng = _engine(path, ShardSpec(rank, world, False), comm)
        if rank == 0:
            try:
                res = _lp_run(eng)
            finally:
                eng.stop_followers()
            out.put((res, dict(comm.stats)))
        else:
            eng.follow()
            out.put(("follower", dict(eng.counters)))
    finally:
        dist.destroy_process_group()


def test_tp2_engine_records_match_tp1(tmp_path):
    import queue
    import time
    spec = _TP_SPECS["llama"]
    path = str(tmp_path / f"{spec.name}.gguf")
    write_synthetic_gguf(path, spec.name, "Q4_K_M", seed=1, spec=spec)
    ref, ref_ctr = _lp_run(_engine(path))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_lp_worker, args=(r, 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    got, t0 = [], time.time()
    try:
        while len(got) < 2:
            try:
                got.append(q.get(timeout=2))
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs) or time.time() - t0 > 300:
                    raise AssertionError(f"TP workers failed: {[p.exitcode for p in procs]}")
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    (res, ctr), stats = next(g[0] for g in got if g[0] != "follower"), next(g[1] for g in got if g[0] != "follower")
    fol = next(g[1] for g in got if g[0] == "follower")
    assert ctr["logprob_steps"] > 0 and fol["logprob_steps"] == ctr["logprob_steps"], (ctr, fol)
    assert ctr["device_sampled_steps"] > 0 and stats.get("gather_words", 0) >= ctr["logprob_steps"], (ctr, stats)
    for (toks, lps), (rtoks, rlps), n_top, greedy in zip(res, ref, (20, 5, 3), (True, False, False)):
        assert toks == rtoks
        S.check_structure(toks, lps, n_top, greedy)
        for (tid, lp, top), (_, rlp, rtop) in zip(lps, rlps):
            # logits under TP differ from TP=1 in their last bits: ids are compared where TP=1's neighbouring values
            # are more than 1e-3 apart
            rv = [v for _, v in rtop]
            for j, ((i, _), (ri, _)) in enumerate(zip(top, rtop)):
                apart = all(abs(rv[j] - rv[k]) > 1e-3 for k in (j - 1, j + 1) if 0 <= k < len(rv))
                assert i == ri or not apart, (j, top, rtop)


# ------------------------------------------------------------------ NATS
def test_tp_worker_serves_chat_with_logprobs(tmp_path):
    import json
    import signal
    import time
    from nats_llm_studio_amd.natsio import Client, EmbeddedServer
    spec = _TP_SPECS["llama"]
    d = tmp_path / "models" / "synthetic" / "tp-llama-GGUF"
    d.mkdir(parents=True)
    write_synthetic_gguf(str(d / "tp-llama-Q4_K_M.gguf"), spec.name, "Q4_K_M", seed=2, spec=spec)
    srv = EmbeddedServer().start()
    argv = ["--nats-url", srv.url, "--models-dir", str(tmp_path / "models"), "--tp", "2", "--model", "tp-llama",
            "--max-batch", "4", "--max-ctx", "256", "--device", "cpu"]
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker_main, args=(r, 2, port, argv)) for r in range(2)]
    for p in procs:
        p.start()
    cli = Client().connect(srv.url)
    try:
        deadline = time.time() + 120
        r = None
        while time.time() < deadline:
            try:
                r = json.loads(cli.request("lmstudio.health", b"{}", 2).data)
                break
            except Exception:
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
                time.sleep(0.5)
        assert r and r["ok"] and r["data"]["models_loaded"] == ["tp-llama"]
        body = {"model": "tp-llama", "messages": [{"role": "user", "content": "hello there"}], "max_tokens": 5,
                "temperature": 0, "logprobs": True, "top_logprobs": 3}
        r = json.loads(cli.request("lmstudio.chat_model", json.dumps(body).encode(), 120).data)
        assert r["ok"] is True and r["data"]["http_status"] == 200, r
        resp = r["data"]["response"]
        content = resp["choices"][0]["logprobs"]["content"]
        assert len(content) == resp["usage"]["completion_tokens"] >= 1
        assert all(len(e["top_logprobs"]) == 3 and e["logprob"] <= 0 for e in content), content
    finally:
        cli.close()
        os.kill(procs[0].pid, signal.SIGTERM)
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
        srv.stop()
    assert [p.exitcode for p in procs] == [0, 0]
