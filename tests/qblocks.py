"""Block generators and a field-level view of the GGUF block formats, for kernel tests (a plain helper module).

`gguf.quants.random_blocks` fills multi-GB checkpoints quickly and leaves most of each format untouched (one `d` per
tensor, scales in a narrow positive band). `structured_blocks` writes block bytes that use every field:

  full     every field over its whole legal range, different in every block: |d|, |dmin|, |m| log-uniform over the
           normal f16 values 2^-14 .. 2^-5; d of both signs where ggml writes both (SIGNED_D); Q4_1 / Q5_1 with an m
           independent of d; every scale / min / quant byte uniformly random (6-bit fields 0..63, Q6_K int8 scales
           -128..127, Q3_K -32..31, Q2_K nibbles 0..15, IQ4_XS ls 0..63).
           F16 / BF16 / F32 have no fields: Gaussian values under a log-uniform scale per 8 values.
  tiny_d   (TINY_TYPES: the K-quants and Q8_0) d / dmin below the f16 normal range, 2^-20 .. 2^-15; the rest as full.
  integer  every dequantised value is exactly representable in f16 (a multiple of the cell's unit with fewer than
           2048 units), so a single-rounding FMA reproduces it whatever the order: d, dmin powers of two (the formats
           with sub-block scales: 0.5 / 1 / 2, the neighbour in the 16-row tile and the neighbour along K always
           another one; the 32-value block formats: the eight 2^-3 .. 2^4 in another order per super-block), scales
           distinct within a block and cut where the value would outgrow 11 bits (Q6_K |sc| <= 63, IQ4_XS
           |ls - 32| <= 16, Q4_K / Q5_K only in the cells whose dmin is finer than their d).

`fields` reads block bytes back into one common form, value[k] = a[s] * q[k] + c[s] per sub-block s with
a = d * sc and c = csign * dmin * m -- the DEVICE form of the re-encoded formats (Q4_0: d*q - 8d, Q3_K: Q6_K's
d*sc*(q6 - 32), IQ4: d*(ls - 32) * kv[q]). The quant values q come from the numpy reference codec itself (the block
decoded with a unit header), so `decode(fields(...))` equals `Q.dequantize` -- which stays the reference of every
test -- and the fault models of test_weight_sensitivity.py edit fields, not bytes.
"""
import numpy as np

from nats_llm_studio_amd.gguf import quants as Q
from nats_llm_studio_amd.gguf.constants import GGMLType as T, GGML_BLOCK

FAMILIES = ("full", "tiny_d", "integer")
K4 = (T.Q4_K, T.Q5_K)
B32 = (T.Q8_0, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.IQ4_NL)          # one f16 d (and m) per 32 values
ALL_TYPES = (T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0, T.F16, T.BF16, T.F32, T.Q4_0, T.Q4_1, T.Q5_0, T.Q5_1, T.Q3_K, T.Q2_K,
             T.IQ4_NL, T.IQ4_XS)
FLOATS = (T.F16, T.BF16, T.F32)      # no block fields: one "scale" of 1, the value itself as q (loader indexing only)
TINY_TYPES = (T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0, T.Q3_K, T.Q2_K)
SIGNED_D = (T.Q4_0, T.Q5_0, T.Q8_0, T.IQ4_NL, T.IQ4_XS, T.Q3_K, T.Q6_K)
# byte offsets inside a block: d, dmin-or-m (None: the format has none)
_D_AT = {T.Q4_K: 0, T.Q5_K: 0, T.Q6_K: 208, T.Q8_0: 0, T.Q4_0: 0, T.Q4_1: 0, T.Q5_0: 0, T.Q5_1: 0, T.Q3_K: 108,
         T.Q2_K: 80, T.IQ4_NL: 0, T.IQ4_XS: 0}
_M_AT = {T.Q4_K: 2, T.Q5_K: 2, T.Q4_1: 2, T.Q5_1: 2, T.Q2_K: 82}
_QABS = {T.Q4_K: 15, T.Q5_K: 31}
P3 = np.array([0.5, 1.0, 2.0])


def families_of(t):
    return tuple(f for f in FAMILIES if f != "tiny_d" or t in TINY_TYPES)


def _f16b(x):
    return np.asarray(x, np.float64).astype(np.float16).reshape(-1).view(np.uint8).reshape(-1, 2)


def _log_uniform(rng, n, lo, hi, signed):
    v = np.exp2(rng.uniform(lo, hi, n))
    return v * rng.choice(np.array([-1.0, 1.0]), n) if signed else v


def _distinct(rng, lo, hi, n):
    """n distinct integers of lo..hi in random order (with repeats only when the range is shorter than n)."""
    pool = np.arange(lo, hi + 1)
    return rng.permutation(pool)[:n] if len(pool) >= n else rng.choice(pool, n)


def _write_scales(t, b, sc, m=None):
    """sc (, m) int [nblk, S] -> the scale bytes of blocks b (uint8 [nblk, nbytes], in place)."""
    if t in K4:
        b[:, 4:16] = Q._pack_k4_scales(sc.astype(np.uint8), m.astype(np.uint8))
    elif t == T.Q6_K:
        b[:, 192:208] = sc.astype(np.int8).view(np.uint8)
    elif t == T.Q3_K:
        b[:, 96:108] = Q._pack_q3_scales(sc + 32)
    elif t == T.Q2_K:
        b[:, 0:16] = (sc | (m << 4)).astype(np.uint8)
    elif t == T.IQ4_XS:
        b[:, 2:8] = Q._pack_iq4xs_scales(sc + 32)


def structured_blocks(t, rows, K, family, rng):
    """Raw block bytes (uint8, flat) of a [rows, K] tensor of ggml type t in the given family (module docstring)."""
    t = T(t)
    if family not in families_of(t):
        raise ValueError(f"{t.name} has no {family} family")
    if t in FLOATS:      # full: Gaussian values under a log-uniform scale per 8 values; integer: -127 .. 127
        n = rows * K
        v = (rng.integers(-127, 128, n).astype(np.float32) if family == "integer" else
             rng.standard_normal(n, dtype=np.float32) * np.repeat(_log_uniform(rng, n // 8, -12, 2, False), 8))
        return Q.quantize(v, t)
    blk, nbytes = GGML_BLOCK[t]
    nblk = rows * K // blk
    per_row = K // blk
    b = rng.integers(0, 256, size=(nblk, nbytes), dtype=np.uint8)
    if family in ("full", "tiny_d"):
        lo, hi = (-14, -5) if family == "full" else (-20, -15)
        b[:, _D_AT[t]:_D_AT[t] + 2] = _f16b(_log_uniform(rng, nblk, lo, hi, t in SIGNED_D))
        if t in _M_AT:
            b[:, _M_AT[t]:_M_AT[t] + 2] = _f16b(_log_uniform(rng, nblk, lo, hi, t in (T.Q4_1, T.Q5_1)))
        return b.reshape(-1)
    r = np.repeat(np.arange(rows), per_row)
    s = np.tile(np.arange(per_row), rows)
    sign = rng.choice(np.array([-1.0, 1.0]), nblk) if t in SIGNED_D else np.ones(nblk)
    if t in B32:
        # the eight powers of two 2^-3 .. 2^4, in another order in every (row, super-block) header
        e = np.stack([rng.permutation(8) for _ in range(nblk // 8)]).reshape(-1) - 3
        b[:, 0:2] = _f16b(sign * np.exp2(e))
        if t in _M_AT:
            b[:, 2:4] = _f16b(0.5 * rng.integers(-64, 65, nblk))
        return b.reshape(-1)
    d = P3[(r + s) % 3]
    dmin = P3[(r + 2 * s + 1) % 3]
    b[:, _D_AT[t]:_D_AT[t] + 2] = _f16b(sign * d)
    if t in _M_AT:
        b[:, _M_AT[t]:_M_AT[t] + 2] = _f16b(dmin)
    if t in K4:
        # |d*sc*q| + |dmin*m| < 2048 units of min(d, dmin): only d = 2 (or 1) over dmin = 0.5 cuts the 6-bit range
        m = rng.integers(0, 64, size=(nblk, 8))
        cap = np.floor((2047 * np.minimum(d, dmin) - dmin * 63) / (d * _QABS[t])).astype(int).clip(0, 63)
        sc = np.stack([_distinct(rng, 0, c, 8) for c in cap])
        _write_scales(t, b, sc, m)
    elif t == T.Q6_K:
        _write_scales(t, b, np.stack([_distinct(rng, -63, 63, 16) for _ in range(nblk)]))
    elif t == T.Q3_K:
        _write_scales(t, b, np.stack([_distinct(rng, -32, 31, 16) for _ in range(nblk)]))
    elif t == T.Q2_K:
        _write_scales(t, b, np.stack([rng.permutation(16) for _ in range(nblk)]), rng.integers(0, 16, size=(nblk, 16)))
    elif t == T.IQ4_XS:
        _write_scales(t, b, np.stack([_distinct(rng, -16, 16, 8) for _ in range(nblk)]))
    return b.reshape(-1)


def _unit_header(t, b):
    """A copy of blocks b whose header makes the reference codec return the quant values themselves."""
    u = b.copy()
    one = _f16b(np.ones(len(u)))
    u[:, _D_AT[t]:_D_AT[t] + 2] = one
    if t in _M_AT:
        u[:, _M_AT[t]:_M_AT[t] + 2] = 0
    n = len(u)
    if t in K4:
        _write_scales(t, u, np.ones((n, 8), int), np.zeros((n, 8), int))
    elif t in (T.Q6_K, T.Q3_K):
        _write_scales(t, u, np.ones((n, 16), int))
    elif t == T.Q2_K:
        _write_scales(t, u, np.ones((n, 16), int), np.zeros((n, 16), int))
    elif t == T.IQ4_XS:
        _write_scales(t, u, np.ones((n, 8), int))
    return u


def fields(t, raw, rows, K):
    """Block bytes -> dict(t, d [R, nb, Sd], dmin [R, nb, Sd] | None, sc [R, nb, S], m [R, nb, S] | None, csign,
    q [R, nb, 256]) in float64 / int64; Sd = 1 (one d per super-block) or 8 = S (one per 32 values). See decode()."""
    t = T(t)
    blk, nbytes = GGML_BLOCK[t]
    nb = K // 256
    if t in FLOATS:
        return dict(t=t, d=np.ones((rows, nb, 1)), dmin=None, sc=np.ones((rows, nb, 8), np.int64), m=None, csign=-1.0,
                    q=Q.dequantize(raw, t, (rows, nb, 256)).astype(np.float64))
    b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, nbytes)
    q = Q.dequantize(_unit_header(t, b).reshape(-1), t, (rows, nb, 256)).astype(np.float64)
    f16 = lambda at: b[:, at:at + 2].copy().view(np.float16)[:, 0].astype(np.float64)
    d = f16(_D_AT[t])
    f = dict(t=t, dmin=None, m=None, csign=-1.0)
    if t in B32:
        f["d"] = d.reshape(rows, nb, 8)
        f["sc"] = np.ones((rows, nb, 8), np.int64)
        if t in (T.Q4_0, T.Q5_0):          # device form d*q + m with q unsigned and m = -8d / -16d
            off = 8 if t == T.Q4_0 else 16
            q = q + off
            f["dmin"], f["m"] = f["d"].copy(), np.full((rows, nb, 8), off, np.int64)
        elif t in (T.Q4_1, T.Q5_1):
            f["dmin"], f["m"], f["csign"] = f16(2).reshape(rows, nb, 8), np.ones((rows, nb, 8), np.int64), 1.0
    else:
        f["d"] = d.reshape(rows, nb, 1)
        if t in _M_AT:
            f["dmin"] = f16(_M_AT[t]).reshape(rows, nb, 1)
        if t in K4:
            sc, m = Q._unpack_k4_scales(b[:, 4:16])
            f["sc"], f["m"] = sc.astype(np.int64).reshape(rows, nb, 8), m.astype(np.int64).reshape(rows, nb, 8)
        elif t == T.Q6_K:
            f["sc"] = b[:, 192:208].copy().view(np.int8).astype(np.int64).reshape(rows, nb, 16)
        elif t == T.Q3_K:
            f["sc"] = (Q._unpack_q3_scales(b[:, 96:108]) - 32).astype(np.int64).reshape(rows, nb, 16)
        elif t == T.Q2_K:
            f["sc"] = (b[:, 0:16] & 15).astype(np.int64).reshape(rows, nb, 16)
            f["m"] = (b[:, 0:16] >> 4).astype(np.int64).reshape(rows, nb, 16)
        elif t == T.IQ4_XS:
            f["sc"] = (Q._unpack_iq4xs_scales(b) - 32).astype(np.int64).reshape(rows, nb, 8)
    f["q"] = q
    return f


def scale_terms(f):
    """(a, c) float64 [R, nb, S]: value = a[s] * q + c[s]."""
    a = f["d"] * f["sc"]
    c = f["csign"] * f["dmin"] * f["m"] if f["m"] is not None else np.zeros_like(a)
    return a, c


def _expand(v):
    return np.repeat(v, 256 // v.shape[2], axis=2)


def decode(f):
    """fields -> (W, mag) float64 [R, K]: the dequantised matrix and |a*q| + |c|, the size of the two terms a
    kernel adds per element (no cancellation between the scale and the min term)."""
    a, c = scale_terms(f)
    a, c = _expand(a), _expand(c)
    R = a.shape[0]
    return (a * f["q"] + c).reshape(R, -1), (np.abs(a * f["q"]) + np.abs(c)).reshape(R, -1)


def emulate(f):
    """The kernels' dequantisation arithmetic (csrc/kernels/common.h): a = d*sc and c = -dmin*m each rounded to
    f16, then ONE f16 rounding of a*q + c. Q2_K runs as F16 weights, rounded once from the fp32 value at load
    (ops/transcode.py); IQ4_XS's load-time f16(d*(ls - 32)) is the rounding of a. -> float64 [R, K] of f16 values."""
    a, c = scale_terms(f)
    with np.errstate(over="ignore"):
        if f["t"] != T.Q2_K:
            a, c = a.astype(np.float16).astype(np.float64), c.astype(np.float16).astype(np.float64)
        v = (_expand(a) * f["q"] + _expand(c))
        if f["t"] == T.Q2_K:
            v = v.astype(np.float32)
        return v.astype(np.float16).astype(np.float64).reshape(a.shape[0], -1)
