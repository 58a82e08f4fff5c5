"""The decode step's variant value (graph keys, graph-dump tags) and the tensor-parallel control header (wire order).

Both are interfaces: bench.py, the GPU logprobs / logit_bias tests and parallel/rehearsal.py read Engine.graphs by key,
and a follower rank must understand the header words a rank 0 of another build sends."""
from nats_llm_studio_amd.engine import engine as E
from nats_llm_studio_amd.engine.engine import StepVariant


def test_variant_keys_and_dump_tags():
    Bp = 48
    want = {
        (False, False, False): ((48, False), "logits0_dsamp0"),
        (True, False, False): ((48, True), "logits1_dsamp0"),
        (False, True, False): ((48, False, True), "logits0_dsamp1"),
        (True, True, False): ((48, True, True), "logits1_dsamp1"),
        (False, False, True): ((48, False, False, True), "logits0_dsamp0_lp1"),
        (True, False, True): ((48, True, False, True), "logits1_dsamp0_lp1"),
        (False, True, True): ((48, False, True, True), "logits0_dsamp1_lp1"),
        (True, True, True): ((48, True, True, True), "logits1_dsamp1_lp1"),
    }
    assert len(want) == 8
    for flags, (key, tag) in want.items():
        v = StepVariant(*flags)
        assert (v.need_logits, v.dsamp, v.lp) == flags
        k = v.key(Bp)
        assert k == key and len(k) == len(key) and all(type(a) is type(b) for a, b in zip(k, key)), (flags, k)
        assert v.tag == tag, (flags, v.tag)
    assert StepVariant() == StepVariant(False, False, False)       # the plain greedy step
    assert StepVariant(dsamp=True).key(1) == (1, False, True)


def test_control_header_round_trip():
    # ten distinct words, in the order they travel: op | T | nrows | need_logits | nseq | pad | candidate mode |
    # in-graph sampling | sampling rows | lp (bit 0) + n_top pairs (the rest)
    words = [2, 48, 3, 11, 5, 1024, 6, 7, 8, 1 | 4 << 1]
    assert len(set(words)) == 10 and E._HDR == 10
    h, v, nlp = E._Header.unpack(words + [77, 78])     # (the logit rows that follow the header are not its part)
    assert tuple(h) == tuple(words) and h._fields == ("op", "T", "nrows", "need_logits", "nseq", "pad", "cand", "dsamp",
                                                      "nsrows", "lpw")
    assert nlp == 4 and v == StepVariant(True, True, True)
    assert h.pack() == [2, 48, 3, 11, 5, 1024, 6, 7, 8, 9]
    # a chained decode step: lp = 1 with 4 (row, n_top) pairs, 2 sampling rows, candidate mode on
    v = StepVariant(True, False, True)
    h = E._Header(op=E._OP_DECODE, T=48, need_logits=v.need_logits, nseq=48, pad=1024, cand=True, dsamp=v.dsamp,
                  nsrows=2, lpw=v.lp | 4 << 1)
    assert h.pack() == [2, 48, 0, 1, 48, 1024, 1, 0, 2, 9] and all(type(w) is int for w in h.pack())
    back, bv, bn = E._Header.unpack(h.pack())
    assert back.pack() == h.pack() and bv == v and bn == 4 and back.nsrows == 2 and back.cand == 1
    h = E._Header(op=E._OP_CAPTURE, T=16, dsamp=True)
    assert h.pack() == [3, 16, 0, 0, 0, 0, 0, 1, 0, 0] and E._Header.unpack(h.pack())[1:] == (StepVariant(dsamp=True), 0)
    assert E._Header(E._OP_STOP).pack() == [0] * 10
