"""chat_model `response_format` on the CPU: the request field, the grammar matcher against an independent reference
parser (tests/grammar_ref.py) over whole vocabularies, completability, the engine (tiny-llama, random weights), and
the mask stage's numpy twin (tests/mask_ref.py) with its fault list."""
import json
import random

import numpy as np
import pytest
import torch

import grammar_ref as R
import mask_ref as M
from nats_llm_studio_amd.engine import grammar as G
from nats_llm_studio_amd.engine.engine import Engine, GenRequest
from nats_llm_studio_amd.engine.sampling import RequestError, SamplingParams, mask_tables, sample_rows
from nats_llm_studio_amd.gguf.reader import GGUFReader
from nats_llm_studio_amd.models.llama import LlamaModel
from nats_llm_studio_amd.tokenizer.bpe import ByteLevelBPE, SentencePieceBPE, tokenizer_from_metadata
from nats_llm_studio_amd.tokenizer.synthetic import bytelevel_vocab, spm_vocab


# ---- vocabularies -------------------------------------------------------------------------------------------------
def _bytelevel(n=1024):
    toks, types, merges, ids = bytelevel_vocab(n)
    tok = ByteLevelBPE(toks, merges, types)
    return G.GrammarVocab.from_tokenizer(tok, [ids["<|eot_id|>"], ids["<|end_of_text|>"]])


def _spm(n=1024):
    toks, types, scores = spm_vocab(n)
    tok = SentencePieceBPE(toks, scores, types)
    return G.GrammarVocab.from_tokenizer(tok, [2])


@pytest.fixture(scope="module")
def vocabs():
    return {"bytelevel": _bytelevel(), "spm": _spm()}


def _allowed(mask):
    return set(np.flatnonzero(np.unpackbits(mask.view(np.uint8), bitorder="little")).tolist())


# ---- the request field --------------------------------------------------------------------------------------------
FINITE = {"type": "object", "properties": {"k": {"enum": ["a", "b"]}, "f": {"type": "boolean"}},
          "required": ["k", "f"]}

ACCEPTED = [
    {"type": "json_object"},
    {"type": "json_schema", "json_schema": {"schema": FINITE}},
    {"type": "json_schema", "json_schema": {"name": "x", "strict": True, "schema": {"type": "integer"}}},
    {"type": "json_schema", "json_schema": {"schema": {"type": ["string", "null"], "minLength": 1, "maxLength": 4}}},
    {"type": "json_schema", "json_schema": {"schema": {"enum": [1, "a", None, {"b": [1.5]}]}}},
    {"type": "json_schema", "json_schema": {"schema": {"const": {"a": 1}}}},
    {"type": "json_schema", "json_schema": {"schema": {
        "title": "t", "description": "d", "default": 1, "examples": [1], "$schema": "s", "$id": "i", "type": "object",
        "properties": {"a": {"type": "array", "items": {"type": "number"}, "minItems": 1, "maxItems": 2},
                       "b": {"oneOf": [{"type": "null"}, {"$ref": "#/definitions/b"}]}},
        "required": ["a"], "additionalProperties": False, "definitions": {"b": {"type": "boolean"}}}}},
    {"type": "json_schema", "json_schema": {"schema": {"type": "object", "additionalProperties": True}}},
    {"type": "json_schema", "json_schema": {"schema": {"type": "array"}}},
    {"type": "json_schema", "json_schema": {"schema": {
        "$defs": {"n": {"type": "object", "properties": {"next": {"anyOf": [{"type": "null"}, {"$ref": "#/$defs/n"}]}},
                        "required": ["next"]}}, "$ref": "#/$defs/n"}}},
]


def _js(schema):
    return {"type": "json_schema", "json_schema": {"schema": schema}}


REJECTED = [(_js({"type": "string", kw: v}), kw) for kw, v in (
    ("pattern", "a+"), ("format", "date"))] + [(_js({"type": "number", kw: 1}), kw) for kw in (
        "minimum", "maximum", "exclusiveMinimum", "exclusiveMaximum", "multipleOf")] + [
    (_js({"type": "array", "prefixItems": [{}]}), "prefixItems"),
    (_js({"allOf": [{"type": "integer"}]}), "allOf"),
    (_js({"not": {"type": "integer"}}), "not"),
    (_js({"if": {}, "then": {}, "else": {}}), "if"),
    (_js({"type": "object", "patternProperties": {"a": {}}}), "patternProperties"),
    (_js({"type": "object", "propertyNames": {}}), "propertyNames"),
    (_js({"type": "object", "dependentRequired": {}}), "dependentRequired"),
    (_js({"type": "object", "dependentSchemas": {}}), "dependentSchemas"),
    (_js({"$ref": "http://example.com/s.json"}), "$ref"),
    (_js({"$ref": "#/properties/a"}), "$ref"),
    (_js({"$ref": "#/$defs/missing"}), "$ref"),
    (_js({"type": "array", "minItems": 3, "maxItems": 2}), "maxItems"),
    (_js({"type": "string", "minLength": 3, "maxLength": 2}), "maxLength"),
    (_js({"type": "string", "minLength": -1}), "minLength"),
    (_js({"enum": []}), "enum"),
    (_js({"type": "object", "properties": {"a": {}}, "required": ["b"]}), "required"),
    (_js({"type": "object", "additionalProperties": {"type": "integer"}}), "additionalProperties"),
    (_js({"type": "object", "properties": {"a": {"type": "strin"}}}), "type"),
    (_js({"type": "array", "items": [{"type": "integer"}]}), "items"),
    (_js({"$defs": {"a": {"$ref": "#/$defs/a"}}, "$ref": "#/$defs/a"}), "response_format"),
    (_js({"$defs": {"a": {"type": "object", "properties": {"n": {"$ref": "#/$defs/a"}}, "required": ["n"]}},
          "$ref": "#/$defs/a"}), "response_format"),
    ("json", "response_format"), (["json_object"], "response_format"), ({"type": "grammar"}, "type"),
    ({}, "type"), ({"type": "json_schema"}, "json_schema"),
    ({"type": "json_schema", "json_schema": {"name": "x"}}, "schema"),
    ({"type": "json_schema", "json_schema": {"schema": [1]}}, "schema"),
]


@pytest.mark.parametrize("rf", ACCEPTED, ids=lambda r: json.dumps(r)[:40])
def test_from_request_accepts(vocabs, rf):
    p = SamplingParams.from_request({"response_format": rf}, grammar_vocab=vocabs["bytelevel"])
    assert isinstance(p.response_format, G.CompiledGrammar) and not p.greedy
    again = SamplingParams.from_request({"response_format": json.loads(json.dumps(rf))}, grammar_vocab=vocabs["bytelevel"])
    assert again.response_format is p.response_format          # compiled once per canonical schema and vocabulary
    m = p.response_format.matcher()
    assert _allowed(m.fill_mask()) and not m.is_complete()


@pytest.mark.parametrize("rf,word", REJECTED, ids=lambda r: json.dumps(r)[:50] if not isinstance(r, str) else r)
def test_from_request_rejects(vocabs, rf, word):
    with pytest.raises(RequestError) as e:
        SamplingParams.from_request({"response_format": rf}, grammar_vocab=vocabs["bytelevel"])
    assert "'response_format'" in str(e.value) and word in str(e.value)


def test_rejection_names_the_path(vocabs):
    rf = _js({"type": "object", "properties": {"a": {"type": "array", "items": {"type": "string", "pattern": "x"}}}})
    with pytest.raises(RequestError) as e:
        SamplingParams.from_request({"response_format": rf}, grammar_vocab=vocabs["bytelevel"])
    assert "'pattern'" in str(e.value) and "#/properties/a/items" in str(e.value)


def test_text_forms_change_nothing(vocabs):
    base = {"temperature": 0.7, "seed": 3, "max_tokens": 9, "top_k": 5}
    want = SamplingParams.from_request(dict(base))
    for rf in ({}, {"response_format": None}, {"response_format": {"type": "text"}}):
        assert SamplingParams.from_request(dict(base, **rf)) == want
        assert SamplingParams.from_request(dict(base, **rf), grammar_vocab=vocabs["spm"]) == want
    assert want.response_format is None and SamplingParams().greedy


def test_ignore_eos_is_refused(vocabs):
    with pytest.raises(RequestError) as e:
        SamplingParams.from_request({"response_format": {"type": "json_object"}, "ignore_eos": True},
                                    grammar_vocab=vocabs["spm"])
    assert "'ignore_eos'" in str(e.value) and "'response_format'" in str(e.value)
    with pytest.raises(RequestError):                       # no tokenizer, no grammar
        SamplingParams.from_request({"response_format": {"type": "json_object"}})


# ---- the matcher against the reference ------------------------------------------------------------------------------
LIST = {"$defs": {"n": {"type": "object", "properties": {"v": {"type": "integer"},
                                                          "next": {"anyOf": [{"type": "null"}, {"$ref": "#/$defs/n"}]}},
                        "required": ["next"]}}, "$ref": "#/$defs/n"}
SCHEMAS = {
    "integer": {"type": "integer"},
    "number": {"type": "number"},
    "boolean": {"type": "boolean"},
    "null": {"type": "null"},
    "string": {"type": "string"},
    "nested": {"type": "object", "properties": {
        "a": {"type": "integer"},
        "b": {"type": "object", "properties": {"c": {"type": "boolean"}, "d": {"type": "null"}}, "required": ["d"]},
        "e": {"enum": ["x", 1]}}, "required": ["b"]},
    "int|num": {"anyOf": [{"type": "integer"}, {"type": "number"}]},
    "str|null": {"type": ["string", "null"]},
    "enum": {"enum": ["ab", "abc", "b"]},
    "const": {"const": "żó€𝄞"},
    "arr0-3": {"type": "array", "items": {"type": "boolean"}, "minItems": 0, "maxItems": 3},
    "arr2-3": {"type": "array", "items": {"enum": [1, 10]}, "minItems": 2, "maxItems": 3},
    "len0": {"type": "string", "maxLength": 0},
    "len1": {"type": "string", "maxLength": 1},
    "len3": {"type": "string", "minLength": 2, "maxLength": 3},
    "list": LIST,
    "finite": FINITE,
    "typed-enum": {"type": ["string", "integer"], "enum": ["a", 1, 2.0, 2.5, None, "ab", [1]]},
    "json_object": {"type": "object"},
}
FINITE_NAMES = ("typed-enum", "boolean", "null", "nested", "enum", "const", "arr0-3", "arr2-3", "len0", "len1", "len3", "finite",
                "integer", "number", "int|num")
PATHS, STEPS = 200, 12


class _RefMasks:
    """{t : is_prefix(g + bytes(t))} over the WHOLE vocabulary by the reference parser, memoised by g (the walks of
    one schema share their first steps). The tokens are visited along a byte trie of the test's own and a branch ends
    at the first byte string that is no prefix: by the definition of a prefix no longer one can be."""

    def __init__(self, schema, vocab):
        self.schema, self.vocab, self.memo = schema, vocab, {}
        self.root = {}
        for t, bs in enumerate(vocab.token_bytes):
            node = self.root
            for b in bs:
                node = node.setdefault(b, {})
            if bs:
                node.setdefault("ids", []).append(t)

    def __call__(self, g: bytes):
        got = self.memo.get(g)
        if got is None:
            got, work = set(), [(self.root, g)]
            while work:
                node, text = work.pop()
                for b, kid in node.items():
                    if b != "ids" and R.is_prefix(self.schema, text + bytes([b])):
                        got.update(kid.get("ids", ()))
                        work.append((kid, text + bytes([b])))
            if R.is_sentence(self.schema, g):
                got |= set(self.vocab.eog)
            self.memo[g] = got
        return got


def _walks(schema, vocab, paths=PATHS, steps=STEPS, seed=0):
    """Seeded random allowed-token paths: yields (matcher, g) at every state, the start included."""
    cg = G.CompiledGrammar(G.compile_schema(schema), vocab)
    for i in range(paths):
        rng = random.Random(1000 * seed + i)
        m, g = cg.matcher(native=False), b""
        nm = cg.matcher(native=True)                         # (not built: an error, never a quiet fallback)
        for _ in range(steps):
            # the native matcher and this one: bit for bit
            assert np.array_equal(nm.fill_mask(), m.fill_mask()) and nm.is_complete() == m.is_complete(), g
            yield m, g
            allowed = sorted(_allowed(m.fill_mask()))
            # (half of the draws among the shortest tokens: a uniform draw inside a string almost never leaves it)
            t = rng.choice(allowed if rng.random() < 0.5 else sorted(allowed, key=lambda t: len(vocab.token_bytes[t])
                                                                       if t not in vocab.eog else 0)[:8])
            assert m.advance(t), (g, t)
            assert nm.advance(t), (g, t)
            if t in vocab.eog:
                assert m.is_complete() and R.is_sentence(schema, g)
                break
            g += vocab.token_bytes[t]


@pytest.mark.parametrize("kind", ["bytelevel", "spm"])
@pytest.mark.parametrize("name", list(SCHEMAS))
def test_masks_equal_the_reference(vocabs, kind, name):
    schema, vocab = SCHEMAS[name], vocabs[kind]
    ref = _RefMasks(schema, vocab)
    seen = set()
    for m, g in _walks(schema, vocab):
        key = (g, m.state_key())
        if key in seen:
            continue
        seen.add(key)
        got, want = _allowed(m.fill_mask()), ref(g)
        assert got == want, (g, sorted(got - want)[:8], sorted(want - got)[:8])
        assert got, g                                                   # a mask is never empty
        assert m.is_complete() == R.is_sentence(schema, g)
        assert (set(vocab.eog) <= got) if m.is_complete() else not (set(vocab.eog) & got)
    assert len(seen) >= 3


def test_depth_64_is_the_last_opener(vocabs):
    vocab = vocabs["bytelevel"]
    one = {bs: t for t, bs in enumerate(vocab.token_bytes) if len(bs) == 1}
    for schema in (LIST, {"type": "array"}):
        m, g = G.CompiledGrammar(G.compile_schema(schema), vocab).matcher(), b""
        unit = b'{"next":' if schema is LIST else b"["
        for depth in range(64):
            for b in unit:
                assert m.advance(one[bytes([b])]), (depth, g)
            g += unit
        opener = one[unit[:1]]
        got = _allowed(m.fill_mask())
        assert opener not in got and got == _RefMasks(schema, vocab)(g)
        assert not m.advance(opener)
        closing = b"null" + b"}" * 64 if schema is LIST else b"]" * 64
        for b in closing:
            assert m.advance(one[bytes([b])])
        assert m.is_complete() and R.is_sentence(schema, g + closing)


@pytest.mark.parametrize("kind", ["bytelevel", "spm"])
@pytest.mark.parametrize("name", FINITE_NAMES)
def test_every_state_can_be_completed(vocabs, kind, name):
    """From every state of the walks of test_masks_equal_the_reference (the same seeds, paths and vocabularies)."""
    schema, vocab = SCHEMAS[name], vocabs[kind]
    bound = R.longest_sentence_bytes(schema) + 1
    proven = set()
    for m, g in _walks(schema, vocab):
        if m.state_key() in proven:
            continue
        proven.add(m.state_key())
        w = m.cg.matcher(native=False)
        w.state, w.ended = m.state, m.ended
        n = 0
        while not w.ended:
            t = min(_allowed(w.fill_mask()))
            assert w.advance(t)
            n += 1
            assert n <= bound, (g, n, bound)
        assert n <= bound - len(g)


def test_real_size_vocabulary():
    """The synthetic Llama-3 vocabulary at its real size, 8 states, the full mask against the reference over all ids."""
    vocab = _bytelevel(128256)
    assert vocab.n_vocab == 128256 and vocab.n_words == 4008
    one = {bs: t for t, bs in enumerate(vocab.token_bytes) if len(bs) == 1}
    schema = SCHEMAS["nested"]
    cg = G.CompiledGrammar(G.compile_schema(schema), vocab)
    ref = _RefMasks(schema, vocab)
    for g in (b"", b"{", b'{"', b'{"a":1', b'{"a":12,\n  "b', b'{"b":{"d":null', b'{"b":{"d":null}, "e":"', b'{"b":{"d":null}}'):
        for native in (False, True):
            m = cg.matcher(native=native)
            for b in g:
                assert m.advance(one[bytes([b])])
            mask = m.fill_mask()
            assert mask.shape == (4008,) and mask.dtype == np.uint32
            assert _allowed(mask) == ref(g), (g, native)
    free = G.CompiledGrammar(G.compile_schema({"type": "object"}), vocab).matcher()
    for b in b'{"key':
        assert free.advance(one[bytes([b])])
    assert _allowed(free.fill_mask()) == _RefMasks({"type": "object"}, vocab)(b'{"key')
    k = free.state_key()
    assert free.advance(one[b"x"]) and free.state_key() == k        # a string interior repeats its state
    hits = free.cg.mask_hits
    free.fill_mask()
    assert free.cg.mask_hits == hits + 1


def test_end_of_generation_ids_have_no_bytes(vocabs):
    """An end-of-generation id of NORMAL type (SentencePiece "</s>" in some GGUFs) ends the request and is never
    allowed by its bytes, in both matchers: inside a string its text would otherwise be a legal continuation."""
    tb = [bytes([b]) for b in range(256)] + [b"</s>", b"ab"]
    vocab = G.GrammarVocab(tb, [256])
    assert vocab.token_bytes[256] == b"" and vocab.token_bytes[257] == b"ab"
    cg = G.CompiledGrammar(G.compile_schema({"type": "string"}), vocab)
    for native in (False, True):
        m = cg.matcher(native=native)
        assert m.advance(ord('"')) and m.advance(ord("x"))
        got = _allowed(m.fill_mask())
        assert 256 not in got and 257 in got and not m.advance(256)
        assert m.advance(ord('"')) and _allowed(m.fill_mask()) == {256} and m.advance(256)
    assert all(vocabs[k].token_bytes[e] == b"" for k in vocabs for e in vocabs[k].eog)


def test_enum_and_const_keep_the_values_of_the_type(vocabs):
    lits = lambda schema: sorted(G.compile_schema(schema).lits[n[1]] for n in G.compile_schema(schema).nodes
                                 if n[0] == "lit")
    assert lits({"type": "string", "enum": [1, "a"]}) == [b'"a"']
    assert lits({"type": "integer", "enum": [1, 2.0, 2.5, True, "1"]}) == [b"1", b"2.0"]
    assert lits({"type": ["null", "boolean"], "enum": [0, None, False]}) == [b"false", b"null"]
    assert lits({"enum": [1, 2], "const": 2}) == [b"2"]
    for bad, word in (({"type": "string", "enum": [1]}, "enum"), ({"type": "null", "const": 0}, "const"),
                      ({"enum": [1], "const": 2}, "enum"), ({"type": "strin", "enum": [1]}, "type")):
        with pytest.raises(RequestError) as e:
            SamplingParams.from_request({"response_format": _js(bad)}, grammar_vocab=vocabs["spm"])
        assert "'response_format'" in str(e.value) and f"'{word}'" in str(e.value)


def test_grammar_cache_under_concurrent_requests(vocabs):
    """from_request runs on service threads: more distinct schemas than the cache holds, from several threads."""
    import threading
    vocab, errors = _spm(600), []

    def work(k):
        try:
            for i in range(120):
                rf = _js({"type": "string", "maxLength": (7 * i + k) % 90})
                assert SamplingParams.from_request({"response_format": rf}, grammar_vocab=vocab).response_format
        except Exception as e:          # (reported below: an exception in a thread fails nothing by itself)
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and len(vocab._grammars) <= G.GRAMMAR_CACHE


def test_native_matcher_is_built():
    """build() compiles csrc/tokcore/grammar.cpp into the tokenizer module; the engine then matches natively."""
    from nats_llm_studio_amd.tokenizer import _tokcore as tc          # (missing: the build is broken, no skip)
    assert hasattr(tc, "GrammarMatcher") and G.native_available()
    cg = G.CompiledGrammar(G.compile_schema(FINITE), _bytelevel())
    assert isinstance(cg.matcher(), G.NativeMatcher) and isinstance(cg.matcher(native=False), G.Matcher)
    with pytest.raises(ValueError):
        tc.Grammar([[0, 99]], [b"x"], [0], 0, list(range(10)))          # a malformed table is refused, not followed


def _fnv(mask):
    h = 1469598103934665603
    for b in np.ascontiguousarray(mask, dtype="<u4").tobytes():
        h = ((h ^ b) * 1099511628211) & ((1 << 64) - 1)
    return h


def test_standalone_matcher_under_sanitizers(tmp_path, vocabs):
    """csrc/tools/grammar_check.cpp (its own main, grammar.cpp linked in, no Python) built with ASAN + UBSAN replays
    node tables and token paths from a file: clean exit, and the checksums of the pure-Python matcher's masks."""
    import os
    import shutil
    import subprocess
    from nats_llm_studio_amd import build
    assert shutil.which("g++") is not None, "g++, which build() itself compiles the tokenizer module with, is missing"
    vocab = vocabs["bytelevel"]
    hx = lambda bs: bs.hex() if bs else "-"
    lines = [f"V {vocab.n_vocab} {len(vocab.token_bytes)} {len(vocab.eog)}", " ".join(map(str, vocab.eog))]
    lines += [hx(bs) for bs in vocab.token_bytes]
    want = []
    for name in ("nested", "int|num", "const", "len3", "arr2-3", "list", "json_object", "str|null"):
        schema = SCHEMAS[name]
        g = G.compile_schema(schema)
        cg = G.CompiledGrammar(g, vocab)
        paths, sums = [], []
        for i in range(6):
            rng = random.Random(77 + i)
            m, path, cs = cg.matcher(native=False), [], []
            for _ in range(24):
                mask = m.fill_mask()
                cs.append(_fnv(mask))
                t = rng.choice(sorted(_allowed(mask)))
                assert m.advance(t)
                path.append(t)
                if t in vocab.eog:
                    break
            cs.append(_fnv(m.fill_mask()))
            paths.append(path)
            sums.append((cs, m.is_complete()))
        rows = []
        for n in g.nodes:
            flat = [x for mem in n[1] for x in mem] if n[0] == "obj" else list(n[1]) if n[0] == "alt" else list(n[1:])
            rows.append(" ".join(map(str, [G.Grammar._KINDS[n[0]], *map(int, flat)])))
        punct = [g.q, g.colon, g.comma, g.lb, g.rb, g.lc, g.rc, *g.words]
        lines += [f"G {len(g.nodes)} {len(g.lits)} {g.root} {len(paths)}", " ".join(map(str, punct)),
                  " ".join(map(str, g.mind))] + rows + [hx(l) for l in g.lits]
        lines += [f"{len(p)} " + " ".join(map(str, p)) for p in paths]
        want += sums
    f = tmp_path / "replay.txt"
    f.write_text("\n".join(lines) + "\n")
    exe = build.build_grammar_check(extra=("-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"),
                                    out_dir=str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want)
    for line, (cs, complete) in zip(got, want):
        parts = line.split()
        assert [int(x, 16) for x in parts[:-2]] == cs and parts[-2] == ("complete" if complete else "open")
    bad = tmp_path / "bad.txt"                               # a malformed table ends it with status 1, no fault
    bad.write_text("V 4 1 0\n\n61\nG 1 1 0 0\n" + " ".join(["0"] * 10) + "\n0\n0 7\n61\n")
    r = subprocess.run([exe, str(bad)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 1 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


# ---- the engine ---------------------------------------------------------------------------------------------------
PROMPT = [5, 17, 99, 3, 250, 7, 81, 12]


@pytest.fixture(scope="module")
def model(tiny_models):
    r = GGUFReader(tiny_models["tiny-llama"])
    return LlamaModel(r, "cpu"), tokenizer_from_metadata(r.metadata)


def _engine(model, **kw):
    args = dict(max_batch=8, max_prefill_tokens=64, num_blocks=128, use_graphs=False, ctx=256)
    args.update(kw)
    return Engine(model[0], model[1], **args)


def _params(eng, **req):
    return SamplingParams.from_request(req, vocab=eng.cfg.vocab, grammar_vocab=eng.grammar_vocab)


def _run(eng, reqs, stagger=1):
    futs, pending, steps = [], list(reqs), 0
    while pending or not all(f.done() for f in futs):
        if pending and steps % stagger == 0:
            ids, p = pending.pop(0)
            futs.append(eng.submit(GenRequest(list(ids), p)))
        eng.step()
        steps += 1
        assert steps < 5000
    return [f.result() for f in futs]


def _content(eng, res):
    return b"".join(eng.tok.token_bytes(t) for t in res.token_ids if t not in eng.eos)


@pytest.mark.parametrize("sampling", [dict(temperature=0), dict(temperature=0.9, seed=7), dict(temperature=0.9, seed=8)])
@pytest.mark.parametrize("async_decode", [False, True])
def test_engine_finite_schema(model, sampling, async_decode):
    eng = _engine(model, async_decode=async_decode)
    cap = R.longest_sentence_bytes(FINITE) + 1
    p = _params(eng, response_format=_js(FINITE), max_tokens=cap, **sampling)
    res = eng.generate(PROMPT, p)
    assert res.finish_reason == "stop" and res.error is None, res
    assert len(res.token_ids) <= cap and res.token_ids[-1] in eng.eos
    content = _content(eng, res)
    assert R.is_sentence(FINITE, content) and R.validate(FINITE, json.loads(content))
    assert json.loads(res.text) == json.loads(content)
    assert eng.counters["constrained_steps"] > 0
    assert eng.stats()["grammar_mask_ms"]["count"] >= len(res.token_ids)


def test_engine_json_object(model):
    eng = _engine(model)
    for sampling in (dict(temperature=0), dict(temperature=1.0, seed=5, top_k=0)):
        res = eng.generate(PROMPT, _params(eng, response_format={"type": "json_object"}, max_tokens=48, **sampling))
        content = _content(eng, res)
        assert R.is_prefix({"type": "object"}, content), content
        assert res.finish_reason in ("stop", "length")
        if res.finish_reason == "stop":
            assert isinstance(json.loads(content), dict)
        else:
            assert len(res.token_ids) == 48


def test_engine_unconstrained_rows_are_untouched(model):
    free = [(PROMPT, dict(temperature=0, max_tokens=20, ignore_eos=True)),
            ([9, 8, 7, 6], dict(temperature=0.8, seed=3, top_k=40, max_tokens=20, ignore_eos=True))]
    cons = [([4, 4, 2], dict(temperature=0.9, seed=1, max_tokens=40, response_format=_js(FINITE))),
            ([3, 1, 4, 1, 5], dict(temperature=0, max_tokens=30, response_format={"type": "json_object"}))]
    for async_decode in (False, True):
        eng = _engine(model, async_decode=async_decode)
        solo = [_run(_engine(model, async_decode=async_decode), [(ids, _params(eng, **kw))])[0] for ids, kw in free + cons]
        mix = _run(eng, [(ids, _params(eng, **kw)) for ids, kw in (free[0], cons[0], free[1], cons[1])])
        assert [r.token_ids for r in mix] == [solo[i].token_ids for i in (0, 2, 1, 3)]
        assert eng.counters["constrained_steps"] > 0
        assert all(r is None for r in eng.rows) and eng._inflight is None


def test_engine_logprobs_are_the_models_own(model):
    eng = _engine(model)
    kw = dict(temperature=0, max_tokens=4, logprobs=True, top_logprobs=5)
    plain = eng.generate(PROMPT, _params(eng, ignore_eos=True, **kw))
    cons = eng.generate(PROMPT, _params(eng, response_format=_js(FINITE), **kw))
    (t0, lp0, top0), (t1, lp1, top1) = plain.logprobs[0], cons.logprobs[0]
    assert top0 == top1                                   # raw logits: the list may hold disallowed tokens
    assert t1 == cons.token_ids[0] and eng.tok.token_bytes(t1)[:1] == b"{"
    assert t1 != t0 and lp1 < lp0


def test_engine_preemption_keeps_the_matcher(model):
    rng = np.random.default_rng(11)
    eng0 = _engine(model)
    reqs = []
    for i in range(6):
        ids = [int(v) for v in rng.integers(20, 200, int(rng.integers(4, 14)))]
        if i % 2:
            reqs.append((ids, _params(eng0, temperature=0.9, seed=i, max_tokens=90, response_format={"type": "json_object"})))
        else:
            reqs.append((ids, _params(eng0, temperature=0, max_tokens=80, ignore_eos=True)))
    roomy = _run(_engine(model, num_blocks=256), reqs, stagger=1)
    tight = Engine(model[0], model[1], max_batch=8, max_prefill_tokens=32, num_blocks=16, use_graphs=False, ctx=256,
                   async_decode=True)
    futs = [tight.submit(GenRequest(list(t), p)) for t, p in reqs]
    steps = 0
    while not all(f.done() for f in futs):
        tight.gen_ratio = 0.05            # as optimistic as on-demand admission: the pool runs dry mid-decode
        tight.step()
        steps += 1
        assert steps < 5000
    assert tight.counters["preemptions"] > 0, tight.stats()
    got = [f.result() for f in futs]
    assert [r.error for r in got] == [None] * 6
    # (the constrained ones: a recomputed free-running greedy row may flip a near-tie, as it always could)
    assert [r.token_ids for r in got[1::2]] == [r.token_ids for r in roomy[1::2]]
    for r in got[1::2]:
        assert R.is_prefix({"type": "object"}, _content(tight, r))


def test_engine_rejected_token_fails_the_request(model):
    eng = _engine(model)
    p = _params(eng, response_format=_js(FINITE), max_tokens=8, temperature=0)
    fut = eng.submit(GenRequest(list(PROMPT), p))
    s = eng.waiting[0]
    eng._append(s, 0)                                        # a token outside the grammar never decodes on
    res = fut.result(timeout=1)
    assert res.finish_reason == "error" and "response_format" in res.error


# ---- the mask stage --------------------------------------------------------------------------------------------------
def _sp(p, bias=()):
    return SamplingParams(temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], min_p=p["min_p"],
                          repeat_penalty=p["repeat_penalty"], presence_penalty=p["presence_penalty"],
                          frequency_penalty=p["frequency_penalty"],
                          logit_bias=tuple(sorted((int(t), float(v)) for t, v in bias)))


def _rows(c):
    return [c.mask[tr] if tr >= 0 else None for tr in c.mask_rows]


def test_sample_rows_applies_the_masks():
    """engine.sampling.sample_rows with masks: the twin's tokens, and its own on the pre-masked copy."""
    for c in M.launches(big=False) + [M.launch(128256, 3)]:
        ps = [_sp(p, c.bias.get(r, ())) for r, p in enumerate(c.params)]
        hists, us = [list(h) for h in c.hists], list(c.us)
        got = sample_rows(torch.from_numpy(c.logits.copy()), ps, hists, us, _rows(c))
        assert got == sample_rows(torch.from_numpy(M.premasked(c)), ps, hists, us), c.name
        assert got == M.twin(c)[0], c.name
        eff = M.effective(c)
        assert all(eff[r, t] for r, t in enumerate(got)), c.name
        assert got[0] == int(np.argmin(c.logits[0]))


def test_mask_tables():
    c = M.launch(33, 2)
    words, rows = mask_tables(_rows(c), 5, 33)
    assert words.shape == (4, 2) and words.dtype == np.uint32 and rows.tolist() == [0, -1, 1, 2, 3]
    assert mask_tables([None] * 5, 5, 33) is None and mask_tables(None, 5, 33) is None
    short, _ = mask_tables([np.array([5], np.uint32)], 1, 70)     # words a short mask lacks: nothing allowed there
    assert short.tolist() == [[5, 0, 0]]


def test_case_list_notices_each_fault():
    cases = M.launches(big=False)
    for fault in M.FAULTS:
        seen = 0
        for c in cases:
            for ld in (c.V, c.V + 24):
                good, bad = M.twin(c, ld=ld), M.twin(c, fault, ld=ld)
                seen += good[0] != bad[0] or good[1].tobytes() != bad[1].tobytes()
        assert seen > 0, fault
    c = M.launch(33, 0)                     # bits at t >= V honoured: a write past V, visible in the buffer alone
    good, bad = M.twin(c, ld=33 + 24), M.twin(c, "pastv", ld=33 + 24)
    assert good[1].tobytes() != bad[1].tobytes()


# ---- tensor parallel --------------------------------------------------------------------------------------------------
def test_cand_ok_is_false_with_a_constrained_row(model, vocabs):
    eng = _engine(model)
    eng.tp = object()                           # (_cand_ok only asks whether there is a group)
    cg = G.parse_response_format({"type": "json_object"}, vocabs["bytelevel"])
    seq = lambda **kw: type("Q", (), {"req": type("R", (), {"params": SamplingParams(**kw)})})
    ok = [seq(temperature=0.8, top_k=40), seq()]
    assert eng._cand_ok(ok)
    assert not eng._cand_ok(ok + [seq(temperature=0.8, top_k=40, response_format=cg)])
    assert not eng._cand_ok(ok + [seq(response_format=cg)])


def test_tp2_gloo_matches_tp1(tmp_path):
    """The rehearsal driver on gloo with its response_format requests: two ranks draw what TP=1 draws, on the
    gathered full logits -- no candidate draw for those steps -- and the values are sentences of the schema."""
    import dataclasses
    import os
    from nats_llm_studio_amd.gguf.synth import SPECS, write_synthetic_gguf
    from nats_llm_studio_amd.parallel import rehearsal
    spec = dataclasses.replace(SPECS["tiny-llama"], name="tp-llama", d_ff=1024)
    path = str(tmp_path / "tp-llama.gguf")
    write_synthetic_gguf(path, spec.name, "Q4_K_M", seed=4, spec=spec)
    os.environ["NLS_REHEARSAL_RESPONSE_FORMAT"] = "1"
    try:
        r = rehearsal.run(path, world=2, new_tokens=5, timeout=240, device="cpu")
    finally:
        os.environ.pop("NLS_REHEARSAL_RESPONSE_FORMAT", None)
    for v in (r["ref"], r["tp"], r["followers"][0]):
        assert "exception" not in v, v
    ref, tp = r["ref"]["constrained"], r["tp"]["constrained"]
    assert tp["tokens"] == ref["tokens"], (tp["tokens"], ref["tokens"])
    assert tp["finish"] == ["stop", "stop", "length"]
    for text in tp["content"]:
        assert R.is_sentence(FINITE, text.encode()) and R.validate(FINITE, json.loads(text))
    assert tp["constrained_steps"] > 0 and tp["candidate_sampled"] == 0, tp
    assert r["tp"]["tokens"] == r["ref"]["tokens"]


# ---- service ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chat_env(tmp_path_factory, tiny_models):
    import shutil
    from nats_llm_studio_amd.natsio import Client, EmbeddedServer
    from nats_llm_studio_amd.service.config import WorkerConfig
    from nats_llm_studio_amd.service.service import Service
    root = tmp_path_factory.mktemp("rf_models")
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


def test_chat_returns_a_value_of_the_schema(chat_env):
    _, _, cli = chat_env
    cap = R.longest_sentence_bytes(FINITE) + 1
    for extra in (dict(), dict(temperature=0.9, seed=4)):
        st, resp = _chat(cli, response_format=_js(FINITE), max_tokens=cap, **extra)
        choice = resp["choices"][0]
        assert st == 200 and choice["finish_reason"] == "stop", resp
        assert R.validate(FINITE, json.loads(choice["message"]["content"]))
    st, plain = _chat(cli)
    st2, text = _chat(cli, response_format={"type": "text"})
    assert st == st2 == 200 and text["choices"][0]["message"]["content"] == plain["choices"][0]["message"]["content"]


@pytest.mark.parametrize("rf,word", [("json", "response_format"), ({"type": "gbnf"}, "type"),
                                     (_js({"type": "string", "pattern": "a"}), "'pattern'")])
def test_chat_bad_response_format_is_400(chat_env, rf, word):
    _, _, cli = chat_env
    st, resp = _chat(cli, response_format=rf)
    assert st == 400 and "'response_format'" in resp["error"] and word in resp["error"], resp
    st, resp = _chat(cli, response_format={"type": "json_object"}, ignore_eos=True)
    assert st == 400 and "'ignore_eos'" in resp["error"]
