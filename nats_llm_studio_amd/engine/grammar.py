"""chat_model `response_format`: JSON-schema constrained decoding on the host.

Three layers:

  parse_response_format / compile_schema   validate the request field and lower the schema to a small node table;
                                           every 400 of the field comes from here (RequestError names
                                           'response_format', the keyword and its JSON-pointer path)
  GrammarVocab                             the tokens' exact bytes (b"" for tokens that are never allowed), the
                                           end-of-generation ids and a byte trie of the vocabulary, built once
  Matcher                                  a byte-level pushdown matcher over the node table that keeps a SET of
                                           alternative stacks (`anyOf: [integer, number]` is ambiguous byte by
                                           byte): advance(token) / is_complete() / fill_mask() / state_key()

The language L(schema) is byte-exact (README, "chat_model response_format"):
  * strings are RFC 8259 strings in well-formed UTF-8 (no raw byte < 0x20, the nine escapes); minLength / maxLength
    count one per raw character and one per escape (a \\uXXXX escape is one, so an escaped surrogate pair is two);
  * numbers are RFC 8259 numbers of at most 16 integer, 16 fraction and 3 exponent digits;
  * enum / const values and property names are spelled as json.dumps(v, ensure_ascii=False, separators=(",", ":"));
  * whitespace stands only after { [ , : and before } ], each place holding nothing, one space, or one newline and at
    most 16 spaces (an empty container has two adjacent places);
  * at most 64 containers are open at once. A value that cannot be finished inside that bound is never begun, so
    every state the matcher reaches can be completed.

A matcher state is a frozenset of stacks; a stack is a tuple of frames, top last:
  ("L", literal id, offset)            the rest of a literal
  ("S", state, count, min, max)        inside a string, behind its opening quote
  ("N", state, digits, integer?)       inside a number
  ("W", k)                             a whitespace place: k = -1 nothing read yet, else spaces behind the newline
  ("V", node)                          a value of a node, not begun
  ("O", node, next member, first?)     an object with properties, between members
  ("F", first?)                        a free-form object, between members
  ("A", node, items so far)            an array, between items
Only L / S / N / W read bytes; the others are rewritten (expanded) until one of those is on top.

csrc/tokcore/grammar.cpp is the same matcher in C++ (bound in _tokcore); CompiledGrammar.matcher() takes it when the
native module is built, and the pure-Python Matcher below gives the same masks without it.
"""
from __future__ import annotations

import json
import threading
from collections import OrderedDict
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from .sampling import RequestError

try:
    from ..tokenizer import _tokcore
    if not hasattr(_tokcore, "GrammarMatcher"):
        _tokcore = None
except ImportError:          # not built: the pure-Python matcher below gives the same masks
    _tokcore = None

MAX_DEPTH = 64
MAX_INT_DIGITS, MAX_FRAC_DIGITS, MAX_EXP_DIGITS = 16, 16, 3
MAX_INDENT = 16
_INF = 1 << 30
ANY, ANY_ARRAY, ANY_OBJECT = 0, 1, 2      # nodes every grammar begins with: any value, an array / object of any values

_TYPES = ("object", "array", "string", "number", "integer", "boolean", "null")
_ANNOTATIONS = ("title", "description", "default", "examples", "$schema", "$id")
_KNOWN = set(_ANNOTATIONS) | {"type", "enum", "const", "properties", "required", "additionalProperties", "items",
                              "minItems", "maxItems", "minLength", "maxLength", "anyOf", "oneOf", "$ref", "$defs",
                              "definitions"}
_FIELD = "'response_format'"
# chat requests are parsed on service threads: the caches of compiled grammars and the lazily built native objects and
# tries are filled under this lock (a matcher and its mask cache belong to the one engine thread)
_LOCK = threading.RLock()


def _bad(msg: str):
    raise RequestError(f"{_FIELD}: {msg}")


def _bad_kw(kw: str, path: str, why: str = "is not supported"):
    raise RequestError(f"{_FIELD}: schema keyword '{kw}' at '{path or '#'}' {why}")


def _is_type(v, t: str) -> bool:
    """A parsed JSON value against a JSON-schema type name (1.0 is an integer, true is no number)."""
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t == "string":
        return isinstance(v, str)
    if t == "array":
        return isinstance(v, list)
    if t == "object":
        return isinstance(v, dict)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return False
    return t == "number" or isinstance(v, int) or v.is_integer()


def spell(v) -> bytes:
    """The one spelling of an enum / const value or a property name."""
    try:
        return json.dumps(v, ensure_ascii=False, separators=(",", ":"), allow_nan=False).encode("utf-8")
    except (TypeError, ValueError) as e:
        raise RequestError(f"{_FIELD}: a value that JSON cannot spell ({e})")


class Grammar:
    """A lowered schema. nodes[i] is one of
         ("lit", literal id) / ("alt", (node, ...)) / ("str", min, max) / ("num", integer?) /
         ("obj", ((key literal id, node, required?), ...)) / ("fobj",) / ("arr", item node, min, max) / ("any",)
       with max = -1 for "unbounded"; lits[i] the literals' bytes; root the root node; mind[i] the containers a value
       of node i needs open at least (the depth bound is checked against it before a value is begun)."""

    def __init__(self, nodes: List[tuple], lits: List[bytes], root: int):
        self.nodes, self.lits, self.root = nodes, lits, root
        self.mind = self._min_depths()
        self._check_cycles()
        if self.mind[root] > MAX_DEPTH:
            _bad(f"the schema admits no value within {MAX_DEPTH} nested containers")
        self.q, self.colon, self.comma = self.lit(b'"'), self.lit(b":"), self.lit(b",")
        self.lb, self.rb, self.lc, self.rc = self.lit(b"["), self.lit(b"]"), self.lit(b"{"), self.lit(b"}")
        self.words = [self.lit(w) for w in (b"true", b"false", b"null")]
        self._trans: Dict[tuple, frozenset] = {}
        self._native = None

    _KINDS = {"lit": 0, "alt": 1, "str": 2, "num": 3, "obj": 4, "fobj": 5, "arr": 6, "any": 7}

    def native(self):
        """The node table as the native module's Grammar (built once)."""
        with _LOCK:
            if self._native is not None:
                return self._native
            rows = []
            for n in self.nodes:
                k = n[0]
                if k == "alt":
                    rows.append([1, *n[1]])
                elif k == "obj":
                    rows.append([4, *[int(x) for m in n[1] for x in m]])
                else:
                    rows.append([self._KINDS[k], *[int(x) for x in n[1:]]])
            punct = [self.q, self.colon, self.comma, self.lb, self.rb, self.lc, self.rc, *self.words]
            self._native = _tokcore.Grammar(rows, list(self.lits), list(self.mind), self.root, punct)
            return self._native

    def lit(self, b: bytes) -> int:
        try:
            return self.lits.index(b)
        except ValueError:
            self.lits.append(b)
            return len(self.lits) - 1

    def _min_depths(self) -> List[int]:
        md = [_INF] * len(self.nodes)
        changed = True
        while changed:
            changed = False
            for i, n in enumerate(self.nodes):
                k = n[0]
                if k in ("lit", "str", "num", "any"):
                    v = 0
                elif k == "alt":
                    v = min((md[j] for j in n[1]), default=_INF)
                elif k == "obj":
                    v = 1 + max((md[m[1]] for m in n[1] if m[2]), default=0)
                elif k == "fobj":
                    v = 1
                else:
                    v = 1 + (md[n[1]] if n[2] > 0 else 0)
                v = min(v, _INF)
                if v < md[i]:
                    md[i], changed = v, True
        return md

    def _check_cycles(self):
        """alt -> alt chains must end: a `$ref` / anyOf loop that opens no container would never read a byte."""
        state = [0] * len(self.nodes)

        def visit(i):
            if state[i] == 1:
                _bad_kw("$ref", "#", "refers to itself without a value in between")
            if state[i] == 2 or self.nodes[i][0] != "alt":
                return
            state[i] = 1
            for j in self.nodes[i][1]:
                visit(j)
            state[i] = 2
        for i in range(len(self.nodes)):
            visit(i)

    # ---- the automaton -------------------------------------------------------------------------------------------
    def start(self) -> frozenset:
        out: set = set()
        self._expand((("V", self.root),), out)
        return frozenset(out)

    @staticmethod
    def _depth(stack: tuple) -> int:
        return sum(1 for f in stack if f[0] in "OFA")

    def _value(self, node: int, depth: int) -> List[tuple]:
        """The frame runs (pushed bottom first) a value of `node` may begin with, `depth` containers being open."""
        if depth + self.mind[node] > MAX_DEPTH:
            return []
        n = self.nodes[node]
        k = n[0]
        if k == "lit":
            return [(("L", n[1], 0),)]
        if k == "alt":
            return [r for j in n[1] for r in self._value(j, depth)]
        if k == "str":
            return [(("S", 0, 0, n[1], n[2]), ("L", self.q, 0))]
        if k == "num":
            return [(("N", 0, 0, n[1]),)]
        if k == "obj":
            return [(("O", node, 0, True), ("W", -1), ("L", self.lc, 0))]
        if k == "fobj":
            return [(("F", True), ("W", -1), ("L", self.lc, 0))]
        if k == "arr":
            return [(("A", node, 0), ("W", -1), ("L", self.lb, 0))]
        out = [(("S", 0, 0, 0, -1), ("L", self.q, 0)), (("N", 0, 0, False),)]      # any
        out += [(("L", w, 0),) for w in self.words]
        return out + self._value(ANY_ARRAY, depth) + self._value(ANY_OBJECT, depth)

    def _expand(self, stack: tuple, out: set):
        if not stack:
            out.add(stack)
            return
        f = stack[-1]
        k = f[0]
        if k == "L" or k == "S":
            out.add(stack)
        elif k == "N":
            out.add(stack)
            if f[1] in (2, 3, 5, 8):
                self._expand(stack[:-1], out)
        elif k == "W":
            out.add(stack)
            self._expand(stack[:-1], out)
        elif k == "V":
            base = stack[:-1]
            for run in self._value(f[1], self._depth(base)):
                self._expand(base + run, out)
        else:
            base = stack[:-1]
            depth = self._depth(stack)             # this container included
            sep = () if (f[-1] if k != "A" else f[2] == 0) else (("W", -1), ("L", self.comma, 0))
            if k == "O":
                members = self.nodes[f[1]][1]
                i = f[2]
                for j in range(i, len(members)):
                    key, node, req = members[j]
                    if depth + self.mind[node] <= MAX_DEPTH:
                        self._expand(base + (("O", f[1], j + 1, False), ("V", node), ("W", -1),
                                             ("L", self.colon, 0), ("L", key, 0)) + sep, out)
                    if req:
                        break
                else:
                    self._expand(base + (("L", self.rc, 0), ("W", -1)), out)
            elif k == "F":
                self._expand(base + (("L", self.rc, 0), ("W", -1)), out)
                self._expand(base + (("F", False), ("V", ANY), ("W", -1), ("L", self.colon, 0),
                                     ("S", 0, 0, 0, -1), ("L", self.q, 0)) + sep, out)
            else:
                item, mn, mx = self.nodes[f[1]][1:]
                n = f[2]
                if n >= mn:
                    self._expand(base + (("L", self.rb, 0), ("W", -1)), out)
                if (mx < 0 or n < mx) and depth + self.mind[item] <= MAX_DEPTH:
                    nn = n + 1 if mx >= 0 else min(n + 1, max(mn, 1))      # unbounded: the count saturates
                    self._expand(base + (("A", f[1], nn), ("V", item)) + sep, out)

    def _consume(self, stack: tuple, b: int) -> Optional[tuple]:
        """The stack behind byte b (its top frame reads bytes), or None."""
        f = stack[-1]
        base = stack[:-1]
        k = f[0]
        if k == "L":
            lit = self.lits[f[1]]
            if lit[f[2]] != b:
                return None
            return base if f[2] + 1 == len(lit) else base + (("L", f[1], f[2] + 1),)
        if k == "W":
            if b == 0x20:
                if f[1] < 0:
                    return base
                return base + (("W", f[1] + 1),) if f[1] < MAX_INDENT else None
            if b == 0x0A and f[1] < 0:
                return base + (("W", 0),)
            return None
        if k == "N":
            st, cnt, integer = f[1], f[2], f[3]
            digit = 0x30 <= b <= 0x39
            nxt = None
            if st == 0 and b == 0x2D:
                nxt = (1, 0)
            elif st in (0, 1):
                if b == 0x30:
                    nxt = (2, 1)
                elif digit:
                    nxt = (3, 1)
            elif st in (2, 3, 5) and not integer and b in (0x65, 0x45):
                nxt = (6, 0)
            elif st in (2, 3) and not integer and b == 0x2E:
                nxt = (4, 0)
            elif st == 3 and digit:
                nxt = (3, cnt + 1) if cnt < MAX_INT_DIGITS else None
            elif st in (4, 5) and digit:
                nxt = (5, cnt + 1) if st == 4 or cnt < MAX_FRAC_DIGITS else None
            elif st == 6 and b in (0x2B, 0x2D):
                nxt = (7, 0)
            elif st in (6, 7, 8) and digit:
                nxt = (8, cnt + 1) if st != 8 or cnt < MAX_EXP_DIGITS else None
            return None if nxt is None else base + (("N", nxt[0], nxt[1], integer),)
        # k == "S"
        st, cnt, mn, mx = f[1], f[2], f[3], f[4]
        if st == 0:
            if b == 0x22:
                return base if cnt >= mn else None
            if b < 0x20 or (mx >= 0 and cnt >= mx):
                return None
            cnt = min(cnt + 1, mn) if mx < 0 else cnt + 1       # unbounded: the count saturates at min
            if b == 0x5C:
                ns = 1
            elif b < 0x80:
                ns = 0
            elif 0xC2 <= b <= 0xDF:
                ns = 21
            elif b == 0xE0:
                ns = 30
            elif b == 0xED:
                ns = 31
            elif 0xE1 <= b <= 0xEF:
                ns = 22
            elif b == 0xF0:
                ns = 32
            elif 0xF1 <= b <= 0xF3:
                ns = 23
            elif b == 0xF4:
                ns = 33
            else:
                return None
        elif st == 1:
            if b == 0x75:
                ns = 14
            elif b in b'"\\/bfnrt':
                ns = 0
            else:
                return None
        elif 11 <= st <= 14:
            if not (0x30 <= b <= 0x39 or 0x41 <= b <= 0x46 or 0x61 <= b <= 0x66):
                return None
            ns = st - 1 if st > 11 else 0
        elif 21 <= st <= 23:
            if not 0x80 <= b <= 0xBF:
                return None
            ns = st - 1 if st > 21 else 0
        else:
            lo, hi, ns = {30: (0xA0, 0xBF, 21), 31: (0x80, 0x9F, 21), 32: (0x90, 0xBF, 22), 33: (0x80, 0x8F, 22)}[st]
            if not lo <= b <= hi:
                return None
        return base + (("S", ns, cnt, mn, mx),)

    def step(self, state: frozenset, b: int) -> frozenset:
        """The state behind byte b (empty: b is rejected). Memoised: a string interior steps to itself."""
        key = (state, b)
        nxt = self._trans.get(key)
        if nxt is None:
            out: set = set()
            for stack in state:
                if stack:
                    ns = self._consume(stack, b)
                    if ns is not None:
                        self._expand(ns, out)
            nxt = frozenset(out)
            if len(self._trans) > 200000:
                self._trans.clear()
            self._trans[key] = nxt
        return nxt


_EMPTY = frozenset()


class _Lower:
    """Schema -> Grammar nodes, with the validation."""

    def __init__(self, root_schema):
        self.root_schema = root_schema
        self.nodes: List[tuple] = []
        self.lits: List[bytes] = []
        self.refs: Dict[str, int] = {}
        self.any = self.add(("any",))
        self.add(("arr", ANY, 0, -1))
        self.add(("fobj",))

    def add(self, n: tuple) -> int:
        self.nodes.append(n)
        return len(self.nodes) - 1

    def lit(self, b: bytes) -> int:
        if b not in self.lits:
            self.lits.append(b)
        return self.lits.index(b)

    def alt(self, ids: Sequence[int]) -> int:
        ids = list(dict.fromkeys(ids))
        return ids[0] if len(ids) == 1 else self.add(("alt", tuple(ids)))

    def bound(self, s: dict, kw: str, path: str, default: int) -> int:
        v = s.get(kw)
        if v is None:
            return default
        if isinstance(v, float) and v.is_integer():
            v = int(v)
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            _bad_kw(kw, path, "must be a non-negative integer")
        return v

    def ref(self, target, path: str) -> int:
        if not isinstance(target, str) or not (target.startswith("#/$defs/") or target.startswith("#/definitions/")):
            _bad_kw("$ref", path, f"must point into '#/$defs/...' or '#/definitions/...' (got {target!r})")
        if target in self.refs:
            return self.refs[target]
        cur = self.root_schema
        for part in target[2:].split("/"):
            part = part.replace("~1", "/").replace("~0", "~")
            if not isinstance(cur, dict) or part not in cur:
                _bad_kw("$ref", path, f"points to {target!r}, which the schema does not hold")
            cur = cur[part]
        nid = self.refs[target] = self.add(("alt", ()))          # placeholder: recursion refers to it
        self.nodes[nid] = ("alt", (self.schema(cur, target),))
        return nid

    def schema(self, s, path: str) -> int:
        if s is True:
            return self.any
        if not isinstance(s, dict):
            _bad(f"the schema at '{path or '#'}' must be an object")
        for kw in s:
            if kw not in _KNOWN:
                _bad_kw(str(kw), path)
        for kw in ("$defs", "definitions"):
            if kw in s and not isinstance(s[kw], dict):
                _bad_kw(kw, path, "must be an object")
        if "$ref" in s:
            for kw in s:
                if kw not in _ANNOTATIONS and kw not in ("$ref", "$defs", "definitions"):
                    _bad_kw(kw, path, "cannot stand next to '$ref'")
            return self.ref(s["$ref"], path)
        if "const" in s or "enum" in s:
            # `type` next to them keeps the values of that type (none left: an error, as an empty enum); a `const`
            # next to an `enum` must be one of its values
            kw = "enum" if "enum" in s else "const"
            values = s["enum"] if "enum" in s else [s["const"]]
            if not isinstance(values, list) or not values:
                _bad_kw("enum", path, "must be a non-empty list")
            if "enum" in s and "const" in s:
                values = [v for v in values if spell(v) == spell(s["const"])]
            if s.get("type") is not None:
                types = s["type"] if isinstance(s["type"], list) else [s["type"]]
                if not types or any(not isinstance(x, str) or x not in _TYPES for x in types):
                    _bad_kw("type", path, f"must be one of {', '.join(_TYPES)}, or a list of them")
                values = [v for v in values if any(_is_type(v, x) for x in types)]
            if not values:
                _bad_kw(kw, path, "leaves no value of the schema's 'type'" if s.get("type") is not None
                        else "leaves no value")
            return self.alt([self.add(("lit", self.lit(b))) for b in dict.fromkeys(spell(v) for v in values)])
        for kw in ("anyOf", "oneOf"):
            if kw in s:
                if not isinstance(s[kw], list) or not s[kw]:
                    _bad_kw(kw, path, "must be a non-empty list of schemas")
                for other in s:
                    if other not in _ANNOTATIONS and other not in (kw, "$defs", "definitions"):
                        _bad_kw(other, path, f"cannot stand next to '{kw}'")
                return self.alt([self.schema(x, f"{path}/{kw}/{i}") for i, x in enumerate(s[kw])])
        t = s.get("type")
        if t is None:
            if "properties" in s or "required" in s or "additionalProperties" in s:
                t = "object"
            elif "items" in s or "minItems" in s or "maxItems" in s:
                t = "array"
            elif "minLength" in s or "maxLength" in s:
                t = "string"
            else:
                return self.any
        types = t if isinstance(t, list) else [t]
        if not types or any(not isinstance(x, str) or x not in _TYPES for x in types):
            _bad_kw("type", path, f"must be one of {', '.join(_TYPES)}, or a list of them")
        return self.alt([self.typed(x, s, path) for x in dict.fromkeys(types)])

    def typed(self, t: str, s: dict, path: str) -> int:
        if t == "null":
            return self.add(("lit", self.lit(b"null")))
        if t == "boolean":
            return self.alt([self.add(("lit", self.lit(b"true"))), self.add(("lit", self.lit(b"false")))])
        if t in ("number", "integer"):
            return self.add(("num", t == "integer"))
        if t == "string":
            mn, mx = self.bound(s, "minLength", path, 0), self.bound(s, "maxLength", path, -1)
            if 0 <= mx < mn:
                _bad_kw("maxLength", path, f"({mx}) is below 'minLength' ({mn})")
            return self.add(("str", mn, mx))
        if t == "array":
            mn, mx = self.bound(s, "minItems", path, 0), self.bound(s, "maxItems", path, -1)
            if 0 <= mx < mn:
                _bad_kw("maxItems", path, f"({mx}) is below 'minItems' ({mn})")
            if "items" in s:
                if not isinstance(s["items"], dict):
                    _bad_kw("items", path, "must be one schema")
                item = self.schema(s["items"], path + "/items")
            else:
                item = self.any
            return self.add(("arr", item, mn, mx))
        ap = s.get("additionalProperties")
        if ap is not None and not isinstance(ap, bool):
            _bad_kw("additionalProperties", path, "given as a schema is not supported (use true or false)")
        props, req = s.get("properties"), s.get("required", [])
        if props is not None and not isinstance(props, dict):
            _bad_kw("properties", path, "must be an object")
        if not isinstance(req, list) or any(not isinstance(r, str) for r in req):
            _bad_kw("required", path, "must be a list of names")
        for r in req:
            if props is None or r not in props:
                _bad_kw("required", path, f"names {r!r}, which 'properties' does not hold")
        if props is None:
            return ANY_OBJECT
        nid = self.add(("obj", ()))
        self.nodes[nid] = ("obj", tuple((self.lit(spell(str(k))), self.schema(v, f"{path}/properties/{k}"), k in req)
                                        for k, v in props.items()))
        return nid


def compile_schema(schema) -> Grammar:
    lo = _Lower(schema)
    root = lo.schema(schema, "#")
    return Grammar(lo.nodes, lo.lits, root)


def json_object_grammar() -> Grammar:
    return compile_schema({"type": "object"})


# ---- vocabulary ---------------------------------------------------------------------------------------------------
class GrammarVocab:
    """What the matcher knows of a vocabulary: token_bytes[t] (b"": never allowed by its bytes -- control, unused and
    unknown-type tokens and the end-of-generation ids themselves), the end-of-generation ids, the mask width, and the byte trie (children dict and token list per node), built on first use."""

    def __init__(self, token_bytes: Sequence[bytes], eog: Iterable[int], n_vocab: Optional[int] = None):
        self.token_bytes = list(token_bytes)
        self.n_vocab = max(len(self.token_bytes), n_vocab or 0)
        self.eog = sorted(int(e) for e in set(eog) if 0 <= int(e) < self.n_vocab)
        for e in self.eog:          # an end-of-generation id ends the request, whatever its type: never by its bytes
            if e < len(self.token_bytes):
                self.token_bytes[e] = b""
        self.n_words = (self.n_vocab + 31) // 32
        self._trie = None
        self._native = None
        self._grammars: "OrderedDict[str, CompiledGrammar]" = OrderedDict()

    @classmethod
    def from_tokenizer(cls, tok, eog: Iterable[int], n_vocab: Optional[int] = None) -> "GrammarVocab":
        from ..tokenizer.bpe import TOKEN_TYPE_CONTROL, TOKEN_TYPE_UNKNOWN, TOKEN_TYPE_UNUSED
        skip = (TOKEN_TYPE_CONTROL, TOKEN_TYPE_UNKNOWN, TOKEN_TYPE_UNUSED)
        tb = [b"" if tok.token_types[i] in skip else tok.token_bytes(i) for i in range(tok.n_vocab)]
        return cls(tb, eog, n_vocab)

    def native(self):
        """The native module's vocabulary (its byte trie is built once per loaded model)."""
        with _LOCK:
            if self._native is None:
                self._native = _tokcore.GrammarVocab(self.token_bytes, self.eog, self.n_vocab)
            return self._native

    @property
    def trie(self):
        if self._trie is None:
            with _LOCK:
                if self._trie is None:
                    self._trie = self._build_trie()
        return self._trie

    def _build_trie(self):
        kids: List[dict] = [{}]
        toks: List[list] = [[]]
        for t, bs in enumerate(self.token_bytes):
            if not bs:
                continue
            n = 0
            for b in bs:
                c = kids[n].get(b)
                if c is None:
                    c = len(kids)
                    kids[n][b] = c
                    kids.append({})
                    toks.append([])
                n = c
            toks[n].append(t)
        return kids, toks


GRAMMAR_CACHE = 64     # compiled grammars kept per vocabulary
MASK_CACHE = 256       # masks kept per compiled grammar


class CompiledGrammar:
    """A grammar bound to a vocabulary, with its mask cache (LRU keyed by the matcher state: a string interior
    repeats its state on every step). SamplingParams.response_format holds one."""

    def __init__(self, grammar: Grammar, vocab: GrammarVocab, key: str = ""):
        self.grammar, self.vocab, self.key = grammar, vocab, key
        self.masks: "OrderedDict[frozenset, np.ndarray]" = OrderedDict()
        self.mask_hits = self.mask_misses = 0

    def matcher(self, native: Optional[bool] = None):
        """A matcher at the start of the grammar: the native one when the module is built (native=None), or the one
        asked for. Both give the same masks; their state keys differ, so a compiled grammar caches them apart."""
        if native is None:
            native = _tokcore is not None
        return NativeMatcher(self) if native else Matcher(self)

    def __repr__(self):
        return f"CompiledGrammar({self.key[:60]!r})"

    def mask_of(self, state, fill=None) -> np.ndarray:
        """The mask of a matcher state, from the cache or from `fill()` (default: the pure-Python trie walk)."""
        m = self.masks.get(state)
        if m is not None:
            self.masks.move_to_end(state)
            self.mask_hits += 1
            return m
        self.mask_misses += 1
        m = self._fill(state) if fill is None else fill()
        m.setflags(write=False)
        self.masks[state] = m
        if len(self.masks) > MASK_CACHE:
            self.masks.popitem(last=False)
        return m

    def _fill(self, state: frozenset) -> np.ndarray:
        """The trie walk: a branch is cut at its first rejected byte."""
        g, v = self.grammar, self.vocab
        kids, toks = v.trie
        allowed: List[int] = []
        work = [(0, state)]
        step = g.step
        while work:
            n, st = work.pop()
            for b, c in kids[n].items():
                ns = step(st, b)
                if ns:
                    if toks[c]:
                        allowed.extend(toks[c])
                    if kids[c]:
                        work.append((c, ns))
        if () in state:
            allowed.extend(v.eog)
        bits = np.zeros(v.n_words * 32, dtype=np.uint8)
        bits[np.asarray(allowed, dtype=np.int64)] = 1
        return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


class Matcher:
    """One request's position in its grammar: a function of the tokens generated so far."""

    def __init__(self, cg: CompiledGrammar):
        self.cg = cg
        self.state = cg.grammar.start()
        self.ended = False

    def advance(self, token_id: int) -> bool:
        """Feed a generated token; False (state unchanged) when the grammar rejects it."""
        v = self.cg.vocab
        t = int(token_id)
        if self.ended:
            return False
        if t in v.eog:
            if () not in self.state:
                return False
            self.ended = True
            return True
        bs = v.token_bytes[t] if 0 <= t < len(v.token_bytes) else b""
        if not bs:
            return False
        st = self.advance_bytes(bs, self.state)
        if not st:
            return False
        self.state = st
        return True

    def advance_bytes(self, bs: bytes, state: Optional[frozenset] = None) -> frozenset:
        st = self.state if state is None else state
        step = self.cg.grammar.step
        for b in bs:
            st = step(st, b)
            if not st:
                return _EMPTY
        return st

    def is_complete(self) -> bool:
        return self.ended or () in self.state

    def fill_mask(self) -> np.ndarray:
        """uint32 [ceil(V/32)]: bit t & 31 of word t >> 5 set: token t is allowed next (read-only, shared)."""
        if self.ended:
            return self.cg.mask_of(frozenset([()]))
        return self.cg.mask_of(self.state)

    def state_key(self) -> bytes:
        return (b"E" if self.ended else b"") + repr(sorted(self.state)).encode()


class NativeMatcher:
    """Matcher on csrc/tokcore/grammar.cpp: same interface, same masks; the masks are cached under its state key."""

    def __init__(self, cg: CompiledGrammar):
        if _tokcore is None:
            raise RuntimeError("the native grammar matcher is not built (nats_llm_studio_amd.build.build_tokcore)")
        self.cg = cg
        self.m = _tokcore.GrammarMatcher(cg.grammar.native(), cg.vocab.native())

    def advance(self, token_id: int) -> bool:
        return self.m.advance(int(token_id))

    def is_complete(self) -> bool:
        return self.m.is_complete()

    def _fill(self) -> np.ndarray:
        return np.frombuffer(self.m.fill_mask(), dtype="<u4").astype(np.uint32)

    def fill_mask(self) -> np.ndarray:
        return self.cg.mask_of(self.m.state_key(), self._fill)

    def state_key(self) -> bytes:
        return self.m.state_key()


def native_available() -> bool:
    return _tokcore is not None


# ---- the request field -------------------------------------------------------------------------------------------
def parse_response_format(rf, vocab: Optional[GrammarVocab]) -> Optional[CompiledGrammar]:
    """The `response_format` field of a chat request -> SamplingParams.response_format (None: free text)."""
    if rf is None:
        return None
    if not isinstance(rf, dict):
        _bad("must be an object such as {\"type\": \"json_schema\", \"json_schema\": {\"schema\": {...}}}")
    t = rf.get("type")
    if t == "text":
        return None
    if t == "json_object":
        schema = {"type": "object"}
    elif t == "json_schema":
        js = rf.get("json_schema")
        if not isinstance(js, dict) or not isinstance(js.get("schema"), dict):
            _bad("'json_schema' must be an object that holds a 'schema' object")
        schema = js["schema"]
    else:
        _bad(f"unknown 'type' {t!r} (one of 'text', 'json_object', 'json_schema')")
    try:
        key = json.dumps(schema, sort_keys=True, ensure_ascii=False, separators=(",", ":"), allow_nan=False)
    except (TypeError, ValueError, RecursionError) as e:
        _bad(f"the schema is not JSON ({e})")
    if vocab is None:
        _bad("needs the model's tokenizer, which this engine was loaded without")
    with _LOCK:
        cg = vocab._grammars.get(key)
        if cg is not None:
            vocab._grammars.move_to_end(key)
            return cg
    try:
        g = compile_schema(schema)
    except RecursionError:
        _bad("the schema nests too deeply")
    cg = CompiledGrammar(g, vocab, key)
    with _LOCK:                     # (two requests may have compiled the same schema: the first one's is kept)
        cg = vocab._grammars.setdefault(key, cg)
        vocab._grammars.move_to_end(key)
        if len(vocab._grammars) > GRAMMAR_CACHE:
            vocab._grammars.popitem(last=False)
    return cg
