"""Reference for the response_format language L(schema): a plain recursive-descent prefix parser, one byte at a time,
written against the README's definitions and sharing no code with nats_llm_studio_amd.engine.grammar (no node table,
no stacks, no trie: it reads the JSON schema itself and backtracks over sets of end positions).

  is_prefix(schema, data)            data is a prefix of some sentence of L(schema) (a sentence is its own prefix)
  is_sentence(schema, data)
  longest_sentence_bytes(schema)     for schemas whose language is finite
  validate(schema, value)            a parsed JSON value is a value of the schema

Every parse function takes a position and returns the SET of positions where its construct may end. When the data
runs out inside a construct that was viable so far, the parser sets `hit`: since every construct that is begun can
be completed (bounds are consistent, the depth rule below never begins what cannot end), that is exactly "a proper
prefix of a sentence".
"""
import json

MAXD = 64
ESC = b'"\\/bfnrt'
HEX = b"0123456789abcdefABCDEF"


def spell(v):
    return json.dumps(v, ensure_ascii=False, separators=(",", ":")).encode("utf-8")


def _json_type(v, t):
    num = isinstance(v, (int, float)) and not isinstance(v, bool)
    return {"null": v is None, "boolean": isinstance(v, bool), "string": isinstance(v, str),
            "array": isinstance(v, list), "object": isinstance(v, dict), "number": num,
            "integer": num and float(v) == int(v)}[t]


class _P:
    def __init__(self, root, data):
        self.root, self.d, self.n, self.hit = root, bytes(data), len(data), False
        self._fit = {}

    # ---- schema helpers
    def deref(self, s):
        seen = 0
        while isinstance(s, dict) and "$ref" in s:
            cur = self.root
            for part in s["$ref"][2:].split("/"):
                cur = cur[part]
            s = cur
            seen += 1
            assert seen < 100
        return s

    def kinds(self, s):
        """The schema as a list of (kind, schema) alternatives: lit / string / number / integer / object / array / any
        / sub (another schema)."""
        s = self.deref(s)
        if s is True or s == {}:
            return [("any", None)]
        if "const" in s or "enum" in s:          # `type` next to them keeps the values of that type
            vals = [v for v in s.get("enum", [s.get("const")]) if "const" not in s or spell(v) == spell(s["const"])]
            if "type" in s:
                ts = s["type"] if isinstance(s["type"], list) else [s["type"]]
                vals = [v for v in vals if any(_json_type(v, t) for t in ts)]
            return [("lit", spell(v)) for v in vals]
        for kw in ("anyOf", "oneOf"):
            if kw in s:
                return [("sub", x) for x in s[kw]]
        t = s.get("type")
        if t is None:
            if "properties" in s or "required" in s or "additionalProperties" in s:
                t = "object"
            elif "items" in s or "minItems" in s or "maxItems" in s:
                t = "array"
            elif "minLength" in s or "maxLength" in s:
                t = "string"
            else:
                return [("any", None)]
        out = []
        for x in (t if isinstance(t, list) else [t]):
            if x == "null":
                out.append(("lit", b"null"))
            elif x == "boolean":
                out += [("lit", b"true"), ("lit", b"false")]
            else:
                out.append((x, s))
        return out

    def fits(self, s, k):
        """Can a value of s be completed with at most k containers nested inside one another?"""
        key = (id(s) if isinstance(s, dict) else None, k)
        if key in self._fit:
            return self._fit[key]
        self._fit[key] = False                       # a loop that opens no container fits nothing
        ok = False
        for kind, x in self.kinds(s):
            if kind in ("lit", "string", "number", "integer", "any"):
                ok = True
            elif kind == "sub":
                ok = self.fits(x, k)
            elif k >= 1 and kind == "object":
                props = x.get("properties") or {}
                ok = all(self.fits(props[r], k - 1) for r in x.get("required", []))
            elif k >= 1 and kind == "array":
                ok = x.get("minItems", 0) == 0 or "items" not in x or self.fits(x["items"], k - 1)
            if ok:
                break
        self._fit[key] = ok
        return ok

    # ---- bytes
    def lit(self, pos, bs):
        for i, b in enumerate(bs):
            if pos + i == self.n:
                self.hit = True
                return set()
            if self.d[pos + i] != b:
                return set()
        return {pos + len(bs)}

    def ws(self, pos):
        ends = {pos}
        if pos == self.n:
            self.hit = True
        elif self.d[pos] == 0x20:
            ends.add(pos + 1)
        elif self.d[pos] == 0x0A:
            p = pos + 1
            ends.add(p)
            for _ in range(16):
                if p == self.n:
                    self.hit = True
                    break
                if self.d[p] != 0x20:
                    break
                p += 1
                ends.add(p)
        return ends

    def seq_ws(self, starts):
        return set().union(*[self.ws(p) for p in starts]) if starts else set()

    def string(self, pos, mn=0, mx=None):
        ends = self.lit(pos, b'"')
        if not ends:
            return set()
        d, n, p, cnt = self.d, self.n, pos + 1, 0
        while True:
            if p == n:
                self.hit = True
                return set()
            b = d[p]
            if b == 0x22:
                return {p + 1} if cnt >= mn else set()
            if b < 0x20 or (mx is not None and cnt >= mx):
                return set()
            cnt += 1
            if b == 0x5C:
                if p + 1 == n:
                    self.hit = True
                    return set()
                e = d[p + 1]
                if e in ESC:
                    p += 2
                elif e == 0x75:
                    for i in range(4):
                        if p + 2 + i == n:
                            self.hit = True
                            return set()
                        if d[p + 2 + i] not in HEX:
                            return set()
                    p += 6
                else:
                    return set()
                continue
            if b < 0x80:
                p += 1
                continue
            if 0xC2 <= b <= 0xDF:
                need, lo, hi = 1, 0x80, 0xBF
            elif 0xE0 <= b <= 0xEF:
                need, lo, hi = 2, (0xA0 if b == 0xE0 else 0x80), (0x9F if b == 0xED else 0xBF)
            elif 0xF0 <= b <= 0xF4:
                need, lo, hi = 3, (0x90 if b == 0xF0 else 0x80), (0x8F if b == 0xF4 else 0xBF)
            else:
                return set()
            for i in range(need):
                if p + 1 + i == n:
                    self.hit = True
                    return set()
                c = d[p + 1 + i]
                if not (lo if i == 0 else 0x80) <= c <= (hi if i == 0 else 0xBF):
                    return set()
            p += 1 + need

    def digits(self, p, most):
        """Positions behind 1 .. most digits at p (hit when the data ends before `most` are read)."""
        out = set()
        for _ in range(most):
            if p == self.n:
                self.hit = True
                break
            if not 0x30 <= self.d[p] <= 0x39:
                break
            p += 1
            out.add(p)
        return out

    def number(self, pos, integer):
        d, n, p = self.d, self.n, pos
        if p < n and d[p] == 0x2D:
            p += 1
        if p == n:
            self.hit = True
            return set()
        if d[p] == 0x30:
            ints = {p + 1}
        elif 0x31 <= d[p] <= 0x39:
            ints = self.digits(p, 16)
        else:
            return set()
        if integer:
            return ints
        ends = set(ints)
        fr = set()
        for q in ints:
            if q == n:
                self.hit = True
            elif d[q] == 0x2E:
                fr |= self.digits(q + 1, 16)
        ends |= fr
        for q in ints | fr:
            if q == n:
                self.hit = True
            elif d[q] in b"eE":
                r = q + 1
                if r == n:
                    self.hit = True
                    continue
                if d[r] in b"+-":
                    r += 1
                ends |= self.digits(r, 3)
        return ends

    # ---- values
    def value(self, s, pos, depth):
        if not self.fits(s, MAXD - depth):
            return set()
        if pos == self.n:
            self.hit = True
            return set()
        ends = set()
        for kind, x in self.kinds(s):
            if kind == "lit":
                ends |= self.lit(pos, x)
            elif kind == "sub":
                ends |= self.value(x, pos, depth)
            elif kind == "string":
                ends |= self.string(pos, x.get("minLength", 0), x.get("maxLength"))
            elif kind in ("number", "integer"):
                ends |= self.number(pos, kind == "integer")
            elif kind == "any":
                ends |= self.string(pos) | self.number(pos, False)
                for w in (b"true", b"false", b"null"):
                    ends |= self.lit(pos, w)
                if depth < MAXD:
                    ends |= self.obj(None, pos, depth) | self.arr({}, pos, depth)
            elif depth < MAXD and kind == "object":
                ends |= self.obj(x if "properties" in x else None, pos, depth)
            elif depth < MAXD and kind == "array":
                ends |= self.arr(x, pos, depth)
        return ends

    def close(self, starts, ch):
        out = set()
        for p in self.seq_ws(starts):
            out |= self.lit(p, ch)
        return out

    def member(self, pos, first, key, vs, depth):
        """[, ws] key : ws value from pos; key None: any string."""
        starts = {pos}
        if not first:
            starts = self.seq_ws(self.lit(pos, b","))
        out = set()
        for p in starts:
            ke = self.string(p) if key is None else self.lit(p, spell(key))
            for q in ke:
                for r in self.seq_ws(self.lit(q, b":")):
                    out |= self.value(vs, r, depth + 1)
        return out

    def obj(self, s, pos, depth):
        starts = self.seq_ws(self.lit(pos, b"{"))
        if s is None:                                   # free-form: any members
            ends, first = set(), True
            while starts:                               # (every member reads bytes: the positions only grow)
                ends |= self.close(starts, b"}")
                nxt = set()
                for p in starts:
                    nxt |= self.member(p, first, None, True, depth)
                starts, first = nxt, False
            return ends
        props = list(s["properties"].items())
        req = set(s.get("required", []))

        def members(i, starts, first):
            if not starts:
                return set()
            ends = set()
            j = i
            while j < len(props):
                k, vs = props[j]
                if self.fits(vs, MAXD - depth - 1):
                    nxt = set()
                    for p in starts:
                        nxt |= self.member(p, first, k, vs, depth)
                    ends |= members(j + 1, nxt, False)
                if k in req:
                    return ends
                j += 1
            return ends | self.close(starts, b"}")
        return members(0, starts, True)

    def arr(self, s, pos, depth):
        starts = self.seq_ws(self.lit(pos, b"["))
        item = s.get("items", True)
        mn, mx = s.get("minItems", 0), s.get("maxItems")
        ends, k = set(), 0
        while starts:
            if k >= mn:
                ends |= self.close(starts, b"]")
            if (mx is not None and k >= mx) or not self.fits(item, MAXD - depth - 1):
                break
            nxt = set()
            for p in starts:
                for q in ({p} if k == 0 else self.seq_ws(self.lit(p, b","))):
                    nxt |= self.value(item, q, depth + 1)
            starts, k = nxt, k + 1
        return ends


def _run(schema, data):
    p = _P(schema, data)
    ends = p.value(schema, 0, 0)
    return p, ends


def is_sentence(schema, data) -> bool:
    p, ends = _run(schema, data)
    return len(data) in ends


def is_prefix(schema, data) -> bool:
    p, ends = _run(schema, data)
    return p.hit or len(data) in ends


WS = 17                 # a newline and 16 spaces
NUM = 1 + 16 + 1 + 16 + 2 + 3
INT = 1 + 16


def longest_sentence_bytes(schema) -> int:
    """The longest sentence of a schema without unbounded strings, unbounded arrays, free-form containers or
    recursion (anything else raises)."""
    p = _P(schema, b"")

    def longest(s, guard=0):
        if guard > 200:
            raise ValueError("recursive schema")
        best = 0
        for kind, x in p.kinds(s):
            if kind == "lit":
                v = len(x)
            elif kind == "sub":
                v = longest(x, guard + 1)
            elif kind == "number":
                v = NUM
            elif kind == "integer":
                v = INT
            elif kind == "string":
                v = 2 + 6 * x["maxLength"]
            elif kind == "array":
                m = x["maxItems"]
                v = 1 + WS + WS + 1 + (m * longest(x["items"], guard + 1) + (m - 1) * (1 + WS) if m else 0)
            elif kind == "object":
                pr = x["properties"]
                v = 1 + WS + WS + 1 + sum(len(spell(k)) + 1 + WS + longest(vs, guard + 1) for k, vs in pr.items())
                v += max(0, len(pr) - 1) * (1 + WS)
            else:
                raise ValueError("unbounded schema")
            best = max(best, v)
        return best
    return longest(schema)


def validate(schema, value) -> bool:
    p = _P(schema, b"")

    def ok(s, v):
        for kind, x in p.kinds(s):
            if kind == "any":
                return True
            if kind == "lit":
                if spell(v) == x:
                    return True
            elif kind == "sub":
                if ok(x, v):
                    return True
            elif kind == "string":
                if isinstance(v, str) and x.get("minLength", 0) <= len(v) and len(v) <= x.get("maxLength", len(v)):
                    return True
            elif kind == "integer":
                if isinstance(v, int) and not isinstance(v, bool):
                    return True
            elif kind == "number":
                if isinstance(v, (int, float)) and not isinstance(v, bool):
                    return True
            elif kind == "array":
                if (isinstance(v, list) and x.get("minItems", 0) <= len(v) <= x.get("maxItems", len(v))
                        and all(ok(x.get("items", True), e) for e in v)):
                    return True
            elif kind == "object" and isinstance(v, dict):
                if "properties" not in x:
                    return True
                pr = x["properties"]
                if (all(r in v for r in x.get("required", [])) and all(k in pr and ok(pr[k], e) for k, e in v.items())
                        and [k for k in pr if k in v] == list(v)):
                    return True
        return False
    return ok(schema, value)
