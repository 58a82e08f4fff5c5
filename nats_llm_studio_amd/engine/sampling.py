"""Sampling parameters (OpenAI / LM Studio chat fields) and the batched sampler.

Greedy rows never leave the device: the lm-head GEMV fuses the arg-max. Only
rows that ask for temperature / top-k / top-p / min-p / penalties go through
a sampler on their logits rows.

Every sampling path draws the SAME way: the kept tokens (logit_bias -> penalties -> temperature -> top-k ->
min-p -> top-p) are walked in index order and the token where the cumulative mass passes u * Z
is taken, with u = uniform01(seed, position) -- the counter-based splitmix64 variate of
csrc/kernels/sample.hip. A seeded request therefore yields the same tokens whether it is sampled
in the decode hipGraph, by the batched GPU sampler on the host-driven path (tensor parallel,
logits requested) or by this module's CPU reference.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch


MAX_TOP_LOGPROBS = 20      # ops.LP_TOP: entries of a device logprob record
LOGIT_BIAS_MAX = 300       # entries of a request's logit_bias (OpenAI's limit): the width of the device tables


class RequestError(ValueError):
    """A chat request field with an illegal value (the service answers 400 with this message)."""


@dataclass
class SamplingParams:
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    repeat_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    seed: Optional[int] = None
    max_tokens: int = 256
    stop: List[str] = field(default_factory=list)
    stop_token_ids: List[int] = field(default_factory=list)
    ignore_eos: bool = False
    # per-token log-probabilities of the model's own distribution (raw logits, temperature 1, before penalties
    # and truncation): the chosen token's, plus the `top_logprobs` (<= MAX_TOP_LOGPROBS) most likely tokens'.
    # They never change how a token is drawn: `greedy` does not look at them.
    logprobs: bool = False
    top_logprobs: int = 0
    # (token id, value) pairs sorted by id, ids distinct, values non-zero (<= LOGIT_BIAS_MAX of them): the value is
    # added to the token's raw fp32 logit in front of the penalties. A biased row is never `greedy`: at temperature 0
    # it takes the sampler's arg-max (lowest index on ties) instead of the arg-max fused into the LM head.
    logit_bias: Tuple[Tuple[int, float], ...] = ()
    # the compiled grammar of the request's `response_format` (engine/grammar.py CompiledGrammar), or None: free
    # text. A constrained row is never `greedy`: every token is drawn by the host-driven sampler behind the row's
    # allowed-token mask (stage -1: a disallowed token's logit counts as -inf in front of every other stage); at
    # temperature 0 that is the arg-max over the allowed tokens, lowest index on ties. Logprobs stay those of the raw
    # logits.
    response_format: Optional[object] = None

    @property
    def greedy(self) -> bool:
        return (self.temperature <= 0.0 and self.repeat_penalty == 1.0 and self.presence_penalty == 0.0
                and self.frequency_penalty == 0.0 and not self.logit_bias and self.response_format is None)

    @classmethod
    def from_request(cls, req: dict, default_max: int = 256, profile: Optional[str] = None,
                     vocab: Optional[int] = None, grammar_vocab=None) -> "SamplingParams":
        """OpenAI / LM Studio chat fields -> params. Fields the request omits come from `profile`
        (default: env NLS_SAMPLING_DEFAULTS, else "lmstudio"); see DEFAULT_PROFILES. `vocab`: the model's
        vocabulary size, the bound of logit_bias token ids (None: the range is not checked). `grammar_vocab`: the
        tokenizer's grammar vocabulary (Engine.grammar_vocab), which a `response_format` other than text needs."""
        stop = req.get("stop") or []
        if isinstance(stop, str):
            stop = [stop]
        mt = req.get("max_tokens", req.get("max_completion_tokens"))
        if mt is None or int(mt) < 0:
            mt = default_max
        d = defaults_for(req, profile)

        def get(key, conv):
            v = req.get(key)
            return conv(d[key]) if v is None else conv(v)
        rp = get("repeat_penalty", float)
        if not rp > 0.0:        # 0 / negative / NaN: clients send 0 for "off"; v / 0 would make the logits inf
            rp = 1.0
        lp = req.get("logprobs")
        if lp is None:
            lp = False
        if not isinstance(lp, bool):
            raise RequestError("'logprobs' must be a boolean")
        ntop = req.get("top_logprobs")
        if ntop is None:
            ntop = 0
        if isinstance(ntop, bool) or not isinstance(ntop, int) or not 0 <= ntop <= MAX_TOP_LOGPROBS:
            raise RequestError(f"'top_logprobs' must be an integer from 0 to {MAX_TOP_LOGPROBS}")
        if ntop > 0 and not lp:
            raise RequestError("'top_logprobs' requires 'logprobs': true")
        rf = None
        if req.get("response_format") is not None:
            from .grammar import parse_response_format
            rf = parse_response_format(req["response_format"], grammar_vocab)
            if rf is not None and bool(req.get("ignore_eos", False)):
                raise RequestError("'ignore_eos' cannot be combined with a 'response_format': a constrained "
                                   "request ends with its JSON value")
        return cls(
            response_format=rf,
            logprobs=lp,
            top_logprobs=ntop,
            logit_bias=parse_logit_bias(req.get("logit_bias"), vocab),
            temperature=get("temperature", float),
            top_k=get("top_k", int),
            top_p=get("top_p", float),
            min_p=get("min_p", float),
            repeat_penalty=rp,
            presence_penalty=float(req.get("presence_penalty", 0.0) or 0.0),
            frequency_penalty=float(req.get("frequency_penalty", 0.0) or 0.0),
            seed=req.get("seed"),
            max_tokens=int(mt),
            stop=list(stop),
            ignore_eos=bool(req.get("ignore_eos", False)),
        )


def parse_logit_bias(lb, vocab: Optional[int] = None) -> Tuple[Tuple[int, float], ...]:
    """The `logit_bias` field of a chat request -> SamplingParams.logit_bias. A JSON object of canonical decimal
    token ids (no sign, no leading zeros, no spaces) -> numbers in [-100, 100]; null / {} -> (); zero values are
    dropped. Anything else is a RequestError that names the field."""
    if lb is None:
        return ()
    if not isinstance(lb, dict):
        raise RequestError("'logit_bias' must be an object that maps token ids to numbers")
    if len(lb) > LOGIT_BIAS_MAX:
        raise RequestError(f"'logit_bias' holds {len(lb)} entries, more than {LOGIT_BIAS_MAX}")
    out = []
    for key, v in lb.items():
        if (not isinstance(key, str) or not key or not key.isascii() or not key.isdigit()
                or (len(key) > 1 and key[0] == "0")):
            raise RequestError(f"'logit_bias' key {key!r} is not a token id (a decimal string such as \"42\")")
        tid = int(key)
        if tid > 0x7FFFFFFF or (vocab is not None and tid >= vocab):
            raise RequestError(f"'logit_bias' token id {key} is outside the model's vocabulary"
                               + (f" (0 to {vocab - 1})" if vocab is not None else ""))
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not -100 <= v <= 100:      # (NaN, inf: not within)
            raise RequestError(f"'logit_bias' value of token {key} must be a number from -100 to 100")
        if float(v) != 0.0:
            out.append((tid, float(v)))
    return tuple(sorted(out))


def bias_tables(params: Sequence["SamplingParams"], width: Optional[int] = None):
    """The rows' logit_bias as the sampler's tables: (ids int32 [n, width], values fp32 [n, width]) numpy arrays,
    unused entries (-1, 0); None when no row has entries. width defaults to the longest row's count."""
    import numpy as np
    most = max((len(p.logit_bias) for p in params), default=0)
    if most == 0:
        return None
    width = most if width is None else width
    ids = np.full((len(params), width), -1, dtype=np.int32)
    val = np.zeros((len(params), width), dtype=np.float32)
    for i, p in enumerate(params):
        if p.logit_bias:
            ids[i, :len(p.logit_bias)] = [t for t, _ in p.logit_bias]
            val[i, :len(p.logit_bias)] = [v for _, v in p.logit_bias]
    return ids, val


# Values of the sampling fields a chat request omits. The reference forwards the request verbatim to LM Studio
# (`/root/reference/nats_llm_studio.go:348`), whose server fills omitted fields from its preset: temperature 0.8,
# top-k 40, top-p 0.95, min-p 0.05, repeat penalty 1.1 [ext: LM Studio defaults; no fixture in the reference pins
# them -- parity unpinned]. Decision (round 5):
#   "lmstudio" (default): a request that SAMPLES (temperature > 0) gets LM Studio's top-k / top-p / min-p /
#       repeat-penalty preset for the fields it omits -- the reference README's own payload `{"temperature":
#       0.7}` (README.md:196-204) samples as LM Studio would sample it. A request that omits temperature, or sends
#       0, decodes greedily with neutral penalties: deterministic output is this API's documented default (LM
#       Studio would sample at 0.8 there -- the one deliberate deviation).
#   "lmstudio-full": every omitted field from the preset, temperature 0.8 included (LM Studio's behaviour).
#   "neutral": the round-4 behaviour: omitted fields are neutral (top-k 0, top-p 1, min-p 0, penalty 1).
LMSTUDIO_PRESET = dict(temperature=0.8, top_k=40, top_p=0.95, min_p=0.05, repeat_penalty=1.1)
NEUTRAL = dict(temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, repeat_penalty=1.0)
DEFAULT_PROFILES = ("lmstudio", "lmstudio-full", "neutral")


def defaults_for(req: dict, profile: Optional[str] = None) -> dict:
    import os
    profile = profile or os.environ.get("NLS_SAMPLING_DEFAULTS", "lmstudio")
    if profile == "lmstudio-full":
        return LMSTUDIO_PRESET
    if profile == "lmstudio":
        t = req.get("temperature")
        if t is not None and float(t) > 0.0:
            return dict(LMSTUDIO_PRESET, temperature=0.0)
        return NEUTRAL
    if profile == "neutral":
        return NEUTRAL
    raise ValueError(f"NLS_SAMPLING_DEFAULTS: unknown profile {profile!r} (one of {DEFAULT_PROFILES})")


_M64 = (1 << 64) - 1


def uniform01(seed: int, pos: int) -> float:
    """Counter-based uniform in [0, 1) of (seed, position): bit-exact twin of sample.hip uniform01."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(pos) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 40) * (1.0 / 16777216.0)


def _mask_words(mask, nw: int):
    import numpy as np
    w = np.ascontiguousarray(mask, dtype=np.uint32)
    if w.ndim != 1:
        raise ValueError(f"a mask of shape {w.shape}: one row of uint32 words is expected")
    return w[:nw] if w.shape[0] >= nw else np.concatenate([w, np.zeros(nw - w.shape[0], dtype=np.uint32)])


def mask_allowed(mask, V: int):
    """A row's allowed-token mask (uint32 words, bit t & 31 of word t >> 5: token t is allowed) as a numpy bool [V].
    Bits at t >= V are ignored; words a short mask lacks count as zero (logit columns past the vocabulary)."""
    import numpy as np
    nw = (V + 31) // 32
    w = _mask_words(mask, nw)
    return np.unpackbits(w[:nw].astype("<u4").view(np.uint8), bitorder="little")[:V].astype(bool)


def sample_rows(logits: torch.Tensor, params: Sequence[SamplingParams], histories: Sequence[Sequence[int]],
                uniforms: Sequence, masks: Optional[Sequence] = None) -> List[int]:
    """logits [n, V] -> one token per row (CPU reference of the GPU sampler; `uniforms`: one variate per
    row -- a float in [0, 1), a torch.Generator, or None for a fresh random one). `masks`: per row an allowed-token
    mask (mask_allowed) or None; a disallowed token's logit counts as -inf in front of every other stage."""
    out = []
    for i, p in enumerate(params):
        l = logits[i].float()
        hist = histories[i]
        if masks is not None and masks[i] is not None:      # stage -1: -inf survives bias and penalties
            ok = torch.from_numpy(mask_allowed(masks[i], l.numel())).to(l.device)
            l = torch.where(ok, l, torch.full_like(l, float("-inf")))
        if p.logit_bias:                                    # first of all: raw fp32 logit + value
            ids = torch.tensor([t for t, _ in p.logit_bias if t < l.numel()], device=l.device, dtype=torch.long)
            add = torch.tensor([v for t, v in p.logit_bias if t < l.numel()], device=l.device, dtype=torch.float32)
            l = l.clone()
            l[ids] = l[ids] + add
        if hist and (p.repeat_penalty != 1.0 or p.presence_penalty or p.frequency_penalty):
            window = [int(t) for t in list(hist)[-64:] if 0 <= int(t) < l.numel()]    # -1 / out-of-range ids: ignored
            ids = torch.tensor(window, device=l.device, dtype=torch.long)
            uniq, cnt = torch.unique(ids, return_counts=True)
            vals = l[uniq]
            if p.repeat_penalty != 1.0:
                vals = torch.where(vals > 0, vals / p.repeat_penalty, vals * p.repeat_penalty)
            vals = vals - p.presence_penalty - p.frequency_penalty * cnt.float()
            l = l.clone()
            l[uniq] = vals
        l = torch.where(torch.isnan(l), torch.full_like(l, float("-inf")), l)     # NaN is never kept, as -inf
        if p.temperature <= 0.0:
            out.append(int(l.argmax()))
            continue
        l = l.double()
        mx = l.max()
        if not bool(mx > float("-inf")):                    # nothing finite: a valid id anyway, as the kernel
            out.append(0)
            continue
        lo = torch.tensor(float("-inf"), dtype=l.dtype)
        if p.top_k and 0 < p.top_k < l.numel():
            lo = torch.topk(l, p.top_k).values[-1]          # k-th largest logit (ties kept)
        if p.min_p > 0.0:
            lo = torch.maximum(lo, mx + p.temperature * math.log(p.min_p))
        w = torch.where(l >= lo, torch.exp((l - mx) / p.temperature), torch.zeros_like(l))
        if p.top_p < 1.0:                                   # smallest top set whose mass reaches top_p
            sw, si = torch.sort(w, descending=True)
            cum = torch.cumsum(sw, 0)
            n_keep = int(torch.searchsorted(cum, p.top_p * cum[-1]).item()) + 1
            thr = sw[min(n_keep, sw.numel()) - 1]
            w = torch.where(w >= thr, w, torch.zeros_like(w))
        cdf = torch.cumsum(w, 0)
        target = uniform(uniforms[i]) * float(cdf[-1])
        tok = int(torch.searchsorted(cdf, torch.tensor(target, dtype=cdf.dtype), right=True).item())
        kept = torch.nonzero(w > 0).flatten()
        if tok >= l.numel() or w[tok] <= 0:                  # rounding at the very end: last kept token
            tok = int(kept[-1]) if kept.numel() else 0
        out.append(tok)
    return out


HIST = 64      # penalty window (last tokens)


def uniform(u) -> float:
    """A row's variate: a float as given, a draw from a torch.Generator, or a fresh random one (None)."""
    if isinstance(u, float):
        return u
    if u is not None:
        return float(torch.rand(1, generator=u).item())
    import random
    return random.random()


def cand_positions(history: Sequence[int], cand_ids: Sequence[int]) -> List[int]:
    """Tensor-parallel candidate sampling: the history tokens as positions in a row of candidate ids (negative:
    an empty slot). History tokens outside the candidates cannot reach the kept set and are dropped."""
    at = {t: j for j, t in enumerate(cand_ids) if t >= 0}
    return [at[t] for t in history if t in at]


def cand_token(cand_ids: Sequence[int], j: int) -> int:
    """The token id of drawn candidate position j; an empty slot or a position outside the row gives 0."""
    return int(cand_ids[j]) if 0 <= j < len(cand_ids) and cand_ids[j] >= 0 else 0


def sample_rows_gpu(logits: torch.Tensor, params: Sequence[SamplingParams], histories: Sequence[Sequence[int]],
                    uniforms: Sequence, masks: Optional[Sequence] = None) -> List[int]:
    """All sampled rows of a step in ONE kernel launch (csrc/kernels/sample.hip).
    `logits` [n, V] fp32 on the GPU is used as scratch (penalties are applied in place; the entries a row's mask
    disallows are left -inf)."""
    return sample_rows_dev(logits, params, histories, uniforms, masks).cpu().tolist()


def mask_tables(masks: Optional[Sequence], n: int, V: int):
    """The rows' allowed-token masks as the sampler's tables: (words uint32 [n_masks, ceil(V/32)], rows int32 [n]:
    the table row of each logits row, -1: none) numpy arrays; None when no row has a mask. Only masked rows take a
    table row."""
    import numpy as np
    if masks is None or all(m is None for m in masks):
        return None
    nw = (V + 31) // 32
    rows = np.full(n, -1, dtype=np.int32)
    tab = []
    for i, m in enumerate(masks[:n]):
        if m is None:
            continue
        rows[i] = len(tab)
        tab.append(_mask_words(m, nw))
    # (the kernel samples a row whose table row is out of range unmasked: never hand it one)
    assert -1 <= int(rows.min()) and int(rows.max()) == len(tab) - 1, (rows, len(tab))
    return np.stack(tab), rows


def sample_rows_dev(logits: torch.Tensor, params: Sequence[SamplingParams], histories: Sequence[Sequence[int]],
                    uniforms: Sequence, masks: Optional[Sequence] = None) -> torch.Tensor:
    """sample_rows_gpu without the read-back: the drawn ids as an int32 device tensor, stream-ordered."""
    import ctypes
    import numpy as np
    from ..ops import _lib
    n, V = len(params), logits.shape[1]
    if logits.shape[0] < n:
        raise ValueError(f"{logits.shape[0]} logit rows for {n} sampling requests")
    logits = logits[:n]
    lg = logits if logits.is_contiguous() and logits.dtype == torch.float32 else logits.float().contiguous()
    P = (_lib.SampleParams * n)()
    hist = np.full((n, HIST), -1, dtype=np.int32)
    for i, p in enumerate(params):
        h = list(histories[i])[-HIST:]
        hist[i, :len(h)] = h
        P[i] = _lib.SampleParams(p.temperature, p.top_p, p.min_p, p.repeat_penalty, p.presence_penalty,
                                 p.frequency_penalty, uniform(uniforms[i]), int(p.top_k or 0), len(h),
                                 len(p.logit_bias))
    dev = lg.device
    # pinned, non_blocking uploads: a pageable upload would wait for the whole stream (the prefill chunk)
    pbytes = torch.frombuffer(bytearray(bytes(P)), dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)
    hd = torch.from_numpy(hist).pin_memory().to(dev, non_blocking=True)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tabs = bias_tables(params)
    mt = mask_tables(masks, n, V)
    if mt is not None:                  # (masked-out entries of the rows stay -inf)
        bi = bv = None
        if tabs is not None:
            bi = torch.from_numpy(tabs[0]).pin_memory().to(dev, non_blocking=True)
            bv = torch.from_numpy(tabs[1]).pin_memory().to(dev, non_blocking=True)
        mw = torch.from_numpy(mt[0].view(np.int32)).pin_memory().to(dev, non_blocking=True)
        mr = torch.from_numpy(mt[1]).pin_memory().to(dev, non_blocking=True)
        _lib.check(_lib.lib().nls_sample_mask(lg.data_ptr(), lg.stride(0), n, V, pbytes.data_ptr(), hd.data_ptr(), HIST,
                                              bi.data_ptr() if bi is not None else None,
                                              bv.data_ptr() if bv is not None else None,
                                              bi.shape[1] if bi is not None else 0, mw.data_ptr(), mw.shape[1],
                                              mr.data_ptr(), mw.shape[0], out.data_ptr(), stream),
                   "nls_sample_mask")
        return out
    if tabs is not None:                # (the kernel takes the biases off again: the rows are left raw)
        bi = torch.from_numpy(tabs[0]).pin_memory().to(dev, non_blocking=True)
        bv = torch.from_numpy(tabs[1]).pin_memory().to(dev, non_blocking=True)
        _lib.check(_lib.lib().nls_sample_bias(lg.data_ptr(), lg.stride(0), n, V, pbytes.data_ptr(), hd.data_ptr(), HIST,
                                              bi.data_ptr(), bv.data_ptr(), bi.shape[1], out.data_ptr(), stream),
                   "nls_sample_bias")
        return out
    _lib.check(_lib.lib().nls_sample(lg.data_ptr(), lg.stride(0), n, V, pbytes.data_ptr(), hd.data_ptr(), HIST,
                                     out.data_ptr(), stream), "nls_sample")
    return out
