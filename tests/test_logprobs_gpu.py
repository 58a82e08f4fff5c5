"""Per-token logprobs on the GPU: the two kernels of csrc/kernels/sample.hip against an fp64 reference, the
penalised row whose drawn token the sampler has rewritten, and the engine's records with and without hipGraphs."""
import math

import numpy as np
import pytest
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import HIST, SamplingParams
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.models.llama import LlamaModel

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
N_TOPS = (20, 5, 1, 0, -1)          # -1: a skipped row, its record stays untouched
KINDS = ("randn", "masked", "shift_up", "shift_down", "equal", "cut_ties")


def _row(kind: str, V: int, g: torch.Generator) -> torch.Tensor:
    x = torch.randn(V, generator=g) * 4
    if kind == "masked":
        x[1::2] = float("-inf")                        # every other entry
    elif kind == "shift_up":
        x += 1e4                                       # the online rescale must not overflow
    elif kind == "shift_down":
        x -= 1e4
    elif kind == "equal":
        x[:] = 0.375                                   # pins the tie order: lowest ids first
    elif kind == "cut_ties":
        # exact ties across the cut of n_top 1, 5 and 20 (ranks a, a + 1). Where the row is long enough the tied
        # pair is moved to ids (1024 j - 1, 1024 j): the kernel's thread 1023 holds the lower id and thread 0 the
        # higher one, which a 1024-thread sweep meets first
        for j, a in enumerate((0, 4, 19)):
            if a + 1 >= V:
                continue
            order = torch.sort(x, descending=True, stable=True).indices
            p, q = int(order[a]), int(order[a + 1])
            lo, hi = 1024 * (j + 1) - 1, 1024 * (j + 1)
            if hi < V and not ({lo, hi} & {int(i) for i in order[:21]}):
                x[[p, lo]] = x[[lo, p]]
                x[[q, hi]] = x[[hi, q]]
                p, q = lo, hi
            x[q] = x[p]
    return x


def _reference(row: np.ndarray, n_top: int, chosen: int):
    """fp64 log_softmax over the finite entries and a stable sort on (-logit, id) of the same fp32 values."""
    ids = np.nonzero(row > -np.inf)[0]                 # drops -inf and NaN
    x = row[ids].astype(np.float64)
    m = x.max()
    lse = m + math.log(np.exp(x - m).sum())
    order = np.lexsort((ids, -x))[:max(n_top, 0)]
    return float(row[chosen]) - lse, [int(i) for i in ids[order]], [float(v) for v in x[order] - lse]


def _check(gpu, V, pad, kinds, n_top, g):
    """One launch pair over len(kinds) rows against the reference: ids exact, logprobs within 1e-4."""
    n = len(kinds)
    host = torch.full((n, V + pad), 1e30)              # the padding columns would win every comparison
    for r in range(n):
        host[r, :V] = _row(kinds[r], V, g)
    chosen = []
    for r in range(n):
        fin = torch.nonzero(host[r, :V] > float("-inf")).flatten()
        chosen.append(int(host[r, :V].argmax()) if r % 2 else int(fin[int(torch.randint(len(fin), (1,), generator=g))]))
    # an unaligned row start: the rows begin one float into the allocation when the stride is padded
    buf = torch.empty(n * (V + pad) + 1, dtype=torch.float32, device=gpu)
    lg = buf[1 if pad else 0:][:n * (V + pad)].view(n, V + pad)
    lg.copy_(host)
    rec = torch.full((n, ops.LP_REC), SENTINEL, dtype=torch.int32, device=gpu)
    nt = torch.tensor(n_top, dtype=torch.int32, device=gpu)
    ops.token_logprobs(lg, n, nt, rec, V=V)
    ops.token_logprobs_pick(lg, n, nt, torch.tensor(chosen, dtype=torch.int32, device=gpu), rec, V=V)
    words = rec.cpu().numpy()
    assert torch.equal(lg.cpu(), host)                 # the kernels only read the logits
    for r in range(n):
        if n_top[r] < 0:
            assert (words[r] == SENTINEL).all(), (V, pad, n, r)
            continue
        lp, ids, lps = _reference(host[r, :V].numpy(), n_top[r], chosen[r])
        tid, got_lp, top = ops.logprob_record(words[r], n_top[r])
        what = (V, pad, n, r, kinds[r], n_top[r])
        assert tid == chosen[r], what
        assert abs(got_lp - lp) <= 1e-4, (what, got_lp, lp)
        assert [i for i, _ in top] == ids, (what, top, ids)
        assert all(abs(a - b) <= 1e-4 for (_, a), b in zip(top, lps)), (what, top, lps)
        # entries past the finite count are (-1, -inf) padding on the device
        k = len(ids)
        assert (words[r, 2 + ops.LP_TOP + k:2 + 2 * ops.LP_TOP][:max(0, n_top[r] - k)] == -1).all(), what


VS = [1, 19, 64, 1000, 1025, 32000, 128256]


@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("V", VS)
def test_kernel_matches_reference(gpu, V, pad):
    g = torch.Generator().manual_seed(1000 * V + pad)
    for n in (1, 3, 17):
        kinds = [KINDS[r % len(KINDS)] for r in range(n)]
        n_top = [N_TOPS[(r + n) % len(N_TOPS)] for r in range(n)]
        if n == 1:
            n_top = [20]
        _check(gpu, V, pad, kinds, n_top, g)


@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("V", VS)
def test_kernel_ties_at_every_cut(gpu, V, pad):
    """The rows with exact ties -- across the cut of n_top 1, 5 and 20 (the 20th and 21st values equal), and the
    all-equal row -- with every n_top: the lower id wins, whichever thread meets it first."""
    g = torch.Generator().manual_seed(7000 * V + pad)
    kinds = [k for k in ("cut_ties", "equal") for _ in (20, 5, 1, 0)]
    _check(gpu, V, pad, kinds, [20, 5, 1, 0] * 2, g)
    if V > 3072:                                       # the tied pairs did move to the stride boundaries
        x = _row("cut_ties", V, torch.Generator().manual_seed(1))
        top = torch.sort(x, descending=True, stable=True).indices[:21].tolist()
        assert {1023, 1024, 2047, 2048, 3071, 3072} <= set(top), top


@pytest.mark.parametrize("slot", ["middle", "recycled"])
def test_penalised_row_reports_the_raw_logprob(gpu, slot):
    """The sampler divides / shifts the logits of the history window in place and overwrites the oldest ring
    slot with its draw. The drawn token is in that window (in the very slot that is recycled, for "recycled"):
    its logprob is still that of the raw distribution."""
    V, n, ps = 1000, 2, 100
    g = torch.Generator().manual_seed(5)
    host = torch.randn(n, V, generator=g)
    tok = [321, 654]
    recycled = (ps + 1) % HIST
    hist = torch.randint(0, V, (n, HIST), generator=g, dtype=torch.int32)
    for r in range(n):
        hist[r][hist[r] == tok[r]] = (tok[r] + 1) % V
        host[r, tok[r]] = 8.0                          # 8 / 1.3 - 0.5 = 5.65: still the arg-max after penalties
        hist[r, recycled if slot == "recycled" else 5] = tok[r]
    p = SamplingParams(temperature=1.0, top_k=1, repeat_penalty=1.3, presence_penalty=0.5)
    params = torch.from_numpy(np.frombuffer(ops.sample_params_bytes(p) * n, dtype=np.uint8).reshape(n, -1).copy()).to(gpu)
    seeds = torch.tensor([3, 4], dtype=torch.int64, device=gpu)
    pos = torch.full((n,), ps, dtype=torch.int32, device=gpu)
    ctx = torch.full((n,), ps + 1, dtype=torch.int32, device=gpu)
    lg, hd = host.to(gpu), hist.to(gpu)
    nt = torch.tensor([3, 0], dtype=torch.int32, device=gpu)
    rec = torch.zeros(n, ops.LP_REC, dtype=torch.int32, device=gpu)
    stash = ops.logprob_stash(n, HIST, gpu)
    nxt = torch.zeros(n, dtype=torch.int32, device=gpu)
    ops.token_logprobs(lg, n, nt, rec, ctx_len=ctx, params=params, pos=pos, hist=hd, stash=stash)
    ops.sample_decode(lg, n, params, seeds, pos, ctx, hd, nxt)
    ops.token_logprobs_pick(lg, n, nt, nxt, rec, ctx_len=ctx, stash=stash)
    assert nxt.cpu().tolist() == tok
    after = lg.cpu()
    assert all(abs(float(after[r, tok[r]]) - (8.0 / 1.3 - 0.5)) < 1e-5 for r in range(n))   # rewritten in place
    assert all(int(hd[r, recycled]) == tok[r] for r in range(n))
    words = rec.cpu().numpy()
    for r in range(n):
        raw = torch.log_softmax(host[r].double(), 0)
        tid, lp, top = ops.logprob_record(words[r], int(nt[r]))
        assert tid == tok[r] and abs(lp - float(raw[tok[r]])) <= 1e-4, (r, lp, float(raw[tok[r]]))
        assert abs(lp - float(torch.log_softmax(after[r].double(), 0)[tok[r]])) > 0.5     # not the penalised one
        if r == 0:
            want = torch.sort(-host[r].double(), stable=True).indices[:3].tolist()
            assert [i for i, _ in top] == want and top[0] == (tid, lp)


# ------------------------------------------------------------------ engine
PROMPT = [5, 17, 99, 3, 250, 7, 81, 12]


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


MIX = [
    (PROMPT, dict(max_tokens=60)),
    (PROMPT[:5], dict(max_tokens=14, logprobs=True, top_logprobs=20)),
    (PROMPT[2:], dict(max_tokens=12, logprobs=True, top_logprobs=0)),
    (PROMPT, dict(max_tokens=12, logprobs=True, top_logprobs=5, temperature=1.1, top_k=40, seed=7, repeat_penalty=1.3,
                  presence_penalty=0.5)),
]


@pytest.fixture(scope="module")
def mixed(gpu, tiny_models):
    """The mixed batch with decode graphs on and off, and without logprobs (shared, read-only). Prompts are
    prefilled eagerly in all three: the captured single-prompt prefill graph pads the prompt to a token bucket,
    its GEMMs then round differently from the eager chunk's and leave slightly different KV behind (measured on
    this batch: same tokens and top ids, logprobs up to 4.9e-4 apart between graphs on and off; bit-equal once
    both prefill eagerly), so records could only be compared to that. test_first_token_entries covers that
    graph."""
    from nats_llm_studio_amd.engine import engine as E
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), gpu)
    plain = [(ids, {k: v for k, v in p.items() if k not in ("logprobs", "top_logprobs")}) for ids, p in MIX]
    old, E._PREFILL_GRAPHS = E._PREFILL_GRAPHS, False
    try:
        out = {"plain": _run(m, plain, True)}
        for graphs in (False, True):
            out[graphs] = _run(m, MIX, graphs)
    finally:
        E._PREFILL_GRAPHS = old
    out["prefill_graphs"] = _run(m, MIX, True)
    return out


def test_engine_graphs_on_and_off(mixed):
    (on, eng), (off, _), (plain, _) = mixed[True], mixed[False], mixed["plain"]
    for (ids, p), a, b, c in zip(MIX, on, off, plain):
        assert a.token_ids == b.token_ids == c.token_ids and len(a.token_ids) == p["max_tokens"]
        for j, (e, f) in enumerate(zip(a.logprobs or [], b.logprobs or [])):
            if e != f:
                print("graphs on / off differ:", a.request_id, j, e, f)
        assert a.logprobs == b.logprobs
        if not p.get("logprobs"):
            assert a.logprobs is None
            continue
        assert [e[0] for e in a.logprobs] == a.token_ids
        for tid, lp, top in a.logprobs:
            assert len(top) == p["top_logprobs"] and lp <= 0
            vals = [v for _, v in top]
            assert vals == sorted(vals, reverse=True) and sum(math.exp(v) for v in vals) <= 1 + 1e-6
            if top and p.get("temperature", 0) <= 0:
                assert top[0] == (tid, lp)


def test_engine_graphs_on_with_prefill_graphs(mixed):
    """Every graph on (the captured single-prompt prefill graphs too) against no graphs at all: the same tokens and
    the same top ids; the logprobs agree to 1e-3. The padded prefill graph's GEMMs sum in another order, which
    moves fp16-rounded activations by an ulp (2^-11 relative) here and there; on logits of magnitude <= 2 that is
    a few 1e-4 (measured: up to 4.9e-4), and 1e-3 is one fp16 ulp at that magnitude."""
    (on, eng), (off, _) = mixed["prefill_graphs"], mixed[False]
    assert eng.counters["prefill_graph_replays"] + len(eng.pf_graphs) > 0
    worst = 0.0
    for a, b in zip(on, off):
        assert a.token_ids == b.token_ids
        for (ta, la, pa), (tb, lb, pb) in zip(a.logprobs or [], b.logprobs or []):
            assert ta == tb and [i for i, _ in pa] == [i for i, _ in pb]
            worst = max([worst, abs(la - lb)] + [abs(x[1] - y[1]) for x, y in zip(pa, pb)])
    print(f"graphs on (prefill graphs too) vs off: worst logprob difference {worst:.6f}")
    assert worst <= 1e-3


def test_engine_stays_on_the_chained_graph_path(mixed):
    """The mixed batch (greedy, greedy + logprobs, seeded sampled + logprobs) is drawn in the decode graph; once the
    logprobs rows are done the remaining greedy row replays the graphs an engine without the feature has."""
    (res, eng), (_, base) = mixed[True], mixed["plain"]
    c = eng.counters
    assert c["device_sampled_steps"] > 0 and c["graph_replays"] > 0 and c["logprob_steps"] > 0
    # the long greedy request decodes alone for some 40 steps after the last logprobs row has finished
    assert c["logprob_steps"] < c["steps"] - 20
    lp_keys = {k for k in eng.graphs if len(k) == 4}
    assert lp_keys and all(k[3] is True for k in lp_keys)
    assert {k for k in eng.graphs if len(k) < 4} <= set(base.graphs)
    assert (1, False) in eng.graphs and (1, False) in base.graphs
    assert base.counters["logprob_steps"] == 0 and not {k for k in base.graphs if len(k) == 4}


def test_engine_records_match_the_oracle(mixed, tiny_models):
    """Chosen-token (and top-entry) logprobs against the teacher-forced fp32 oracle, within the bound that
    test_prefill_logits_match_reference applies to logits: 5 % of the oracle's largest |logit|."""
    from nats_llm_studio_amd.models.reference import ReferenceModel
    ref = ReferenceModel(GGUFReader(tiny_models["tiny-llama"]))
    res, _ = mixed[True]
    for (ids, p), r in zip(MIX, res):
        if not p.get("logprobs"):
            continue
        rl = ref.logits((list(ids) + list(r.token_ids))[:-1]).double()
        bound, lsm = 0.05 * float(rl.abs().max()), torch.log_softmax(rl, -1)
        worst = max(abs(lp - float(lsm[len(ids) - 1 + j][tid])) for j, (tid, lp, _) in enumerate(r.logprobs))
        print(f"oracle: {r.request_id} worst chosen-logprob error {worst:.5f}, bound {bound:.5f}")
        for j, (tid, lp, top) in enumerate(r.logprobs):
            row = lsm[len(ids) - 1 + j]
            assert abs(lp - float(row[tid])) <= bound, (j, tid, lp, float(row[tid]), bound)
            assert all(abs(v - float(row[i])) <= bound for i, v in top)


def test_first_token_entries(gpu, tiny_models):
    """Token 0 comes out of prefill: through the captured single-prompt graph (<= 64 tokens; the second request of
    a bucket replays it) and through an eager chunk (> 64 tokens)."""
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), gpu)
    eng = Engine(m, None, max_batch=8, use_graphs=True, prefix_cache=False)
    long_prompt = [int(v) for v in np.random.default_rng(2).integers(3, 900, 100)]
    outs = []
    for prompt in (PROMPT, PROMPT[::-1], long_prompt):
        outs.append(eng.generate(prompt, SamplingParams(max_tokens=3, ignore_eos=True, logprobs=True, top_logprobs=4)))
        plain = eng.generate(prompt, SamplingParams(max_tokens=3, ignore_eos=True))
        assert plain.token_ids == outs[-1].token_ids and plain.logprobs is None
    assert eng.counters["prefill_graph_replays"] > 0
    for r in outs:
        assert len(r.logprobs) == 3 and [e[0] for e in r.logprobs] == r.token_ids
        tid, lp, top = r.logprobs[0]
        assert len(top) == 4 and top[0] == (tid, lp) and lp <= 0


def test_host_driven_path_gives_the_same_records(gpu, tiny_models, monkeypatch):
    """NLS_DEVICE_SAMPLING=0: a sampled request leaves the chained path, every step is drawn by the host-driven
    batched sampler, and the two logprob kernels run eagerly around it -- same seed, same tokens, same records as
    in the decode graph."""
    m = LlamaModel(GGUFReader(tiny_models["tiny-llama"]), gpu)
    reqs = [(PROMPT, dict(max_tokens=10, logprobs=True, top_logprobs=5, temperature=1.1, top_k=40, seed=7,
                          repeat_penalty=1.3, presence_penalty=0.5))]
    (dev_res,), eng = _run(m, reqs, True)
    assert eng.counters["device_sampled_steps"] > 0
    monkeypatch.setenv("NLS_DEVICE_SAMPLING", "0")
    (host_res,), eng = _run(m, reqs, True)
    assert eng.counters["device_sampled_steps"] == 0 and not eng.device_sampling
    assert host_res.token_ids == dev_res.token_ids
    assert [e[0] for e in host_res.logprobs] == host_res.token_ids
    assert host_res.logprobs == dev_res.logprobs
