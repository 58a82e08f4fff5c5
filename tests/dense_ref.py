"""Reference side of tests/test_dense_gemm_sensitivity.py (and of the dense cases of test_rowops_sensitivity.py /
test_weight_sensitivity.py): numpy only, no import of ops. The dense f16 GEMMs compute

    y[m, ycol + n] (epilogue) alpha * sum_k x[m, k] * W[n, k]        x f16 [M, K], W f16 [rows, K] row-major

per launch segment (W, ycol). Here: the instances and what their plan admits, the input families (integer, one-hot,
full), fp64 / int64 references of every epilogue as the WHOLE output buffer a launch must leave (sentinel outside the
targets), the fault models, and an fp32 emulation of the kernels' arithmetic: f16 products (exact in fp32), an fp32 sum
in ascending 32-deep slices from a zero accumulator, split-K slabs over 64-column steps [K/64 * s / ks, K/64 * (s + 1)
/ ks) summed in slice order, alpha after the sum, silu as g * (1 / (1 + exp2(g * -log2e))) in fp32."""
import functools

import numpy as np

SENT = -7.0                     # exact in f16 and f32: what y holds outside a launch's targets
LOG2E = 1.4426950408889634
# every dense instance of tests/gemm_digest_cases.py: (mode, waves, rt)
INSTANCES = [(m, w, r) for m in (4, 5) for w in (8, 16) for r in (4, 2)] + [(6, 8, 2), (10, 8, 1), (10, 8, 2),
                                                                              (14, 8, 2)]
# largest relative error of the emulated fp32 silu(g) u against fp64 for |g| <= 16, pinned on the CPU by
# test_dense_gemm_sensitivity.test_emulated_noise_bounds_tol and test_weight_sensitivity.test_swiglu_integer_inputs
SILU_EMU = 1.0e-6
SILU_TOL = 4 * SILU_EMU
F_T, F_C = 10, 5                # the localised faults: 64-column K-step 10, 16-byte chunk 5 of it
F_K0 = 64 * F_T + 8 * F_C


def tile_rows(cfg):
    mode, _, rt = cfg
    return 96 if mode == 14 else 256 // rt if mode == 10 else 256 if mode == 5 else 128


def block_rows(cfg):
    mode, _, rt = cfg
    return 128 if mode == 14 else 256 if mode == 10 else 64 * rt


def ring_depth(cfg):
    """K-steps between two uses of one LDS stage: modes 4 / 5 rings of 3, mode 6 of 2, mode 10 two K-tile buffers,
    mode 14 four slots."""
    return {14: 4, 10: 2, 6: 2}.get(cfg[0], 3)


def admits(cfg, epi, ks, K, rows=()):
    """What the dispatcher's plan takes (csrc/kernels/qgemv.hip) of the launches this suite makes. rows: the weight
    rows of every launch segment."""
    if epi == "slabs" and ks < 2:
        return False
    if cfg[0] == 10 and any(r % 4 for r in rows):      # epi_cols4 stores four columns / slab floats at a time
        return False
    if cfg[0] == 14:
        if epi in ("swiglu", "argmax", "f32_argmax"):
            return False
        return all((K // 64 * s // ks) % 2 == 0 for s in range(1, ks))      # slices of whole 128-column K-tiles
    return True


def partial_rows(cfg, epi="f32"):
    """Rows of the partial last weight tile: no multiple of 16 where the plan allows (SwiGLU wants whole 16-row
    groups; mode 10 stores four columns at a time and its plan refuses a row count that is no multiple of 4:
    test_dense_gemm_sensitivity.test_mode10_refuses_rows_no_multiple_of_4)."""
    return 48 if epi == "swiglu" else 44 if cfg[0] == 10 else 37


def kslices(K, ks):
    nk = K // 64
    return [(64 * (nk * s // ks), 64 * (nk * (s + 1) // ks)) for s in range(ks)]


def pad64(M):
    return (M + 63) // 64 * 64


def al4(c):
    return (c + 3) // 4 * 4


def ld_of(segs, epi="f32"):
    """Row stride of the y buffer of a launch: 8 columns wider than the last target, a multiple of 4."""
    return al4(max(c + w.shape[0] // (2 if epi == "swiglu" else 1) for w, c in segs)) + 8


# ------------------------------------------------------------------------------------------------------ families

@functools.lru_cache(maxsize=None)
def int_weights(rows, K, seed=0, lo=-8):
    """Integers lo .. 8 times a power of two per row, 2^-3 .. 2^4, another in neighbouring rows: exact in f16. Every
    fourth row is non-negative under 2^1 / 2^-2: against the non-negative activation rows its sums pass 2048 units,
    where not every integer is an f16 value, and stay inside f16 at K <= 1536."""
    q = np.random.default_rng(1000 + 7 * rows + K + seed).integers(lo, 9, (rows, K)).astype(np.float64)
    e = (np.arange(rows) * 3 + seed) % 8 - 3
    q[3::4] = np.abs(q[3::4])
    e[3::8], e[7::8] = 1, -2
    return q * 2.0 ** e[:, None]


@functools.lru_cache(maxsize=None)
def int_acts(M, K, seed=0, lo=-2, hi=2):
    """Integers lo .. hi; every fourth row non-negative (int_weights)."""
    x = np.random.default_rng(2000 + K + seed).integers(lo, hi + 1, (M, K)).astype(np.float64)
    x[3::4] = np.abs(x[3::4])
    return x


@functools.lru_cache(maxsize=None)
def int_base(nrows, ld, seed=0):
    return np.random.default_rng(3000 + ld + seed).integers(-1000, 1001, (nrows, ld)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def hot_acts(K, stride=37, off=5):
    """[K, K]: row m is 1 at column k_m = (stride m + off) % K, the k_m walking every K position."""
    x = np.zeros((K, K))
    x[np.arange(K), hot_cols(K, K, stride, off)] = 1.0
    return x


def hot_cols(n, K, stride=37, off=5):
    return (np.arange(n) * stride + off) % K


@functools.lru_cache(maxsize=None)
def hot_weights(rows, K):
    w = np.zeros((rows, K))
    w[np.arange(rows), hot_cols(rows, K)] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def full_range(n, K, seed=0):
    """Finite f16 of the whole range and both signs, subnormals included (as float64)."""
    b = np.random.default_rng(4000 + n + K + seed).integers(0, 65536, (n, K)).astype(np.uint16)
    b = np.where((b >> 10) & 31 == 31, b & ~np.uint16(1 << 14), b).astype(np.uint16)
    return b.view(np.float16).astype(np.float64)


@functools.lru_cache(maxsize=None)
def full_rows(n, K, seed=0):
    """Gaussian rows under a per-row log-uniform scale 2^-6 .. 2^6, rounded to f16 (as float64)."""
    rng = np.random.default_rng(5000 + n + K + seed)
    v = rng.standard_normal((n, K)) * 2.0 ** rng.uniform(-6, 6, (n, 1))
    return v.astype(np.float16).astype(np.float64)


def interleaved(n):
    """Gate rows of n interleaved [g0..g7, u0..u7] rows (the up row of gate row i is i + 8), in output order."""
    j = np.arange(n // 2)
    return (j // 8) * 16 + j % 8


# --------------------------------------------------------------------------------------------- rounding and silu

def rne_f16(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def trunc_f16(v):
    r = rne_f16(v)
    over = np.abs(r) > np.abs(v)
    with np.errstate(over="ignore"):
        return np.where(over, np.nextafter(r.astype(np.float16), np.float16(0)).astype(np.float64), r)


def half_ulp_f16(a):
    """Half an f16 ulp at magnitude a (subnormal floor 2^-25)."""
    e = np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -14)))
    return 2.0 ** (e - 11)


def silu64(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def silu32(g):
    g = np.asarray(g, np.float32)
    one = np.float32(1.0)
    return g * (one / (one + np.exp2(g * np.float32(-LOG2E))))


# ------------------------------------------------------------------------------------------------------ products

def _faulty_operands(x, w, fault):
    k0, R = F_K0, w.shape[0]
    if fault == "W chunk from the neighbouring chunk":
        w = w.copy()
        w[:, k0:k0 + 8] = w[:, (k0 ^ 8):(k0 ^ 8) + 8]
    elif fault == "W chunk from the neighbouring row":
        w2 = w.copy()
        w2[:, k0:k0 + 8] = w[np.minimum(np.arange(R) ^ 1, R - 1), k0:k0 + 8]
        w = w2
    elif fault == "x chunk from the neighbouring row":
        x2 = x.copy()
        x2[:, k0:k0 + 8] = x[np.minimum(np.arange(len(x)) ^ 1, len(x) - 1), k0:k0 + 8]
        x = x2
    return x, w


def _mm(a, b, emu):
    """a @ b^T: fp64, or the emulation's fp32 sum in ascending 32-deep slices."""
    if not emu:
        return a @ b.T
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k in range(0, a.shape[1], 32):
        acc = acc + a32[:, k:k + 32] @ b32[:, k:k + 32].T
    return acc


_PRODUCTS = {}


def slab_products(x, w, ks, fault=None, depth=3, emu=False, mag=False):
    """[ks, M, rows]: slab s = the partial sum of K-slice s (mag: of |x| |w|). The fault-free fp64 products are
    computed once per (x, w, ks) -- the operands are the cached, read-only arrays of the families -- and shared."""
    if fault is None and not emu:
        key = (id(x), id(w), ks, mag)
        if key not in _PRODUCTS:
            if len(_PRODUCTS) >= 48:
                _PRODUCTS.clear()
            a, b = (np.abs(x), np.abs(w)) if mag else (x, w)
            _PRODUCTS[key] = (x, w, np.stack([a[:, k0:k1] @ b[:, k0:k1].T for k0, k1 in kslices(x.shape[1], ks)]))
        return _PRODUCTS[key][2]
    x, w = _faulty_operands(x, w, fault)
    bounds = kslices(x.shape[1], ks)
    if ks > 1 and fault == "slice boundary one step off":          # both sides: the sum keeps every step
        (a, b), (_, c) = bounds[-2], bounds[-1]
        bounds[-2:] = [(a, b + 64), (b + 64, c)]
    if ks > 1 and fault == "one K-step in two slices":
        a, b = bounds[-2]
        bounds[-2] = (a, b + 64)
    out = []
    for k0, k1 in bounds:
        p = _mm(x[:, k0:k1], w[:, k0:k1], emu)
        t = 64 * F_T
        if k0 <= t < k1 and fault in ("K-step dropped", "K-step doubled", "K-step of the stage one ring depth earlier"):
            cur = x[:, t:t + 64] @ w[:, t:t + 64].T
            if fault == "K-step dropped":
                p = p - cur
            elif fault == "K-step doubled":
                p = p + cur
            elif t - 64 * depth >= k0:
                t0 = t - 64 * depth
                p = p - cur + x[:, t0:t0 + 64] @ w[:, t0:t0 + 64].T
        out.append(p)
    return np.stack(out)


OPERAND_FAULTS = ["W chunk from the neighbouring chunk", "W chunk from the neighbouring row",
                  "x chunk from the neighbouring row", "K-step dropped", "K-step doubled",
                  "K-step of the stage one ring depth earlier"]
SLICE_FAULTS = ["slice boundary one step off", "one K-step in two slices", "slab dropped",
                "slab written to the neighbouring slice"]
PLACE_FAULTS = ["clamped row stored past M", "clamped row stored past rows",
                "boundary tile at the neighbouring segment's column offset"]
SCALE_FAULTS = ["alpha omitted", "alpha applied to the base too", "add overwrites"]
STORE_FAULTS = ["f16 store truncates"]
SWIGLU_FAULTS = ["gate paired with the neighbouring group's up row", "gate and up exchanged"]
ARGMAX_FAULTS = ["ties taken at the highest index", "partial tile left out", "key taken before alpha"]


def run(x, segs, M, epi, alpha=1.0, ks=1, base=None, nrows=None, ld=None, tile=128, fault=None, depth=3, emu=False,
        tol=0.0, silu_tol=0.0):
    """What one launch must leave. segs: [(W [rows, K], ycol)]; x [>= M, K]; y is [nrows, ld] and holds SENT (add:
    `base`, a whole buffer) before the launch. Returns y = the reference buffer, lim = the per-element bound (0:
    EQUAL -- everything outside the targets, and every target when tol is 0; f16 outputs with a bound 0 are the
    round-to-nearest f16 of the reference), slabs / slab_lim [ks, M, sum of rows] for ks > 1, ids / vals [M] for the
    arg-max epilogues. tol: the relative bound of one dot product on its own size B = sum |x| |w|. emu: the fp32
    emulation in place of fp64. fault: one of the fault models, applied to this reference."""
    dt = np.float32 if emu else np.float64
    rows = [w.shape[0] for w, _ in segs]
    col0 = np.concatenate([[0], np.cumsum(rows)]).astype(int)
    xm = x if fault is None and not emu else x[:M]          # (the shared products cover every row of x)
    sl = np.concatenate([slab_products(xm, w, ks, fault, depth, emu)[:, :M] for w, _ in segs], axis=2).astype(dt)
    Bs = (np.concatenate([slab_products(x, w, ks, mag=True)[:, :M] for w, _ in segs], axis=2) if tol
          else np.zeros(sl.shape))
    out = {}
    if ks > 1:
        if fault == "slab dropped":
            sl[ks // 2] = 0
        if fault == "slab written to the neighbouring slice":
            sl[ks // 2 - 1], sl[ks // 2] = sl[ks // 2], np.nan
        out["slabs"], out["slab_lim"] = sl.astype(np.float64), tol * Bs
    tot = sl[0].copy()
    for s in range(1, ks):
        tot = tot + sl[s]
    B = np.abs(alpha) * Bs.sum(0)
    al = dt(1.0 if fault == "alpha omitted" else alpha)
    v = tot * al
    nrows = M if nrows is None else nrows
    half = epi == "swiglu"
    ld = ld_of(segs, epi) if ld is None else ld
    y = np.full((nrows, ld), SENT, np.float64) if base is None else np.asarray(base, np.float64).copy()
    lim = np.zeros((nrows, ld))
    for i, (w, ycol) in enumerate(segs):
        c0, n = col0[i], rows[i]
        vi, Bi = v[:, c0:c0 + n], B[:, c0:c0 + n]
        if epi in ("f32", "f32_argmax"):
            y[:M, ycol:ycol + n], lim[:M, ycol:ycol + n] = vi, tol * Bi
        elif epi == "add":
            b = y[:M, ycol:ycol + n].astype(dt)
            if fault == "alpha applied to the base too":
                r = (b + tot[:, c0:c0 + n]) * al
            elif fault == "add overwrites":
                r = vi
            else:
                r = b + vi
            y[:M, ycol:ycol + n], lim[:M, ycol:ycol + n] = r, tol * (np.abs(b) + Bi)
        elif epi == "act":
            _f16(y, lim, slice(0, M), slice(ycol, ycol + n), vi, tol * Bi, fault)
        elif epi == "swiglu":
            gi = interleaved(n)
            ui = gi + (24 if fault == "gate paired with the neighbouring group's up row" else 8)
            ui = np.where(ui < n, ui, gi + 8)
            if fault == "gate and up exchanged":
                gi, ui = ui, gi
            g, u, Bg, Bu = vi[:, gi], vi[:, ui], Bi[:, gi], Bi[:, ui]
            if emu:
                r = silu32(g) * u
                sg = 0.0
            else:
                with np.errstate(over="ignore"):
                    sg = 1.0 / (1.0 + np.exp(-g))
                r = g * sg * u
            b = tol * (np.abs(sg * (1 + g * (1 - sg)) * u) * Bg + np.abs(g * sg) * Bu) + tol * tol * Bg * Bu / 2 \
                + silu_tol * np.abs(r)
            _f16(y, lim, slice(0, M), slice(ycol, ycol + n // 2), r, b, fault)
    if fault == "clamped row stored past M" and nrows > M:
        y[M] = y[M - 1]
    if fault == "clamped row stored past rows":
        w, ycol = segs[-1]
        y[:M, ycol + rows[-1]] = y[:M, ycol + rows[-1] - 1]
    if fault == "boundary tile at the neighbouring segment's column offset" and len(segs) > 1:
        (_, y0), (_, y1) = segs[0], segs[1]          # the second segment's first tile lands on the first segment's
        n1 = min(tile, rows[1])
        moved = y[:M, y1:y1 + n1].copy()
        y[:M, y1:y1 + n1] = SENT if base is None else base[:M, y1:y1 + n1]
        y[:M, y0:y0 + n1] = moved
    if "argmax" in epi:
        key = (tot if fault == "key taken before alpha" else v).astype(np.float64)
        idx = np.concatenate([c + np.arange(r) for (_, c), r in zip(segs, rows)])
        if fault == "partial tile left out":
            r0 = (rows[-1] - 1) // tile * tile
            key = key[:, :col0[-2] + r0]
        if fault == "ties taken at the highest index":
            j = key.shape[1] - 1 - np.argmax(key[:, ::-1], axis=1)
        else:
            j = np.argmax(key, axis=1)          # the first maximum
        out["ids"], out["vals"] = idx[j], v.astype(np.float64)[np.arange(M), j]
    out["y"], out["lim"] = y, lim
    return out


def _f16(y, lim, rs, cs, r, b, fault):
    """An f16 target: EQUAL to the round-to-nearest f16 where the value is exact (bound 0), else within the bound plus
    half an ulp at the largest value the bound admits."""
    r = np.asarray(r, np.float64)
    st = trunc_f16(r) if fault == "f16 store truncates" else rne_f16(r)
    exact = np.asarray(b) == 0
    y[rs, cs] = st if fault is not None else np.where(exact, st, r)
    lim[rs, cs] = np.where(exact, 0.0, b + half_ulp_f16(np.abs(r) + b))


def judge(got, ref):
    """(largest |got - ref| / bound, its index, number of elements outside their bound). An element with bound 0 must
    be EQUAL: one that differs, or a NaN, counts as inf."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref["y"])
    lim = ref["lim"]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(r) | (r == np.inf), r, np.inf)
    r = np.where(np.isnan(got), np.inf, r)
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(v) for v in i), int((r > 1).sum())


def judge_slabs(got, ref):
    return judge(got, dict(y=ref["slabs"], lim=ref["slab_lim"]))


def where(i, K=None):
    """A readable place for a failure at output (m, n) -- and, for the one-hot families, at K position k."""
    s = f"activation row {i[0]}, output column {i[1]}"
    if K is not None:
        s += f" -> K-step {K // 64}, 16-byte chunk {K % 64 // 8}, element {K % 8}"
    return s


def unpack_keys(keys):
    """(value, id) of the device's 64-bit arg-max keys (uint64 [M]); a zero key (never written) gives id -1."""
    k = np.asarray(keys).view(np.uint64)
    u = (k >> np.uint64(32)).astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u).astype(np.uint32)
    ids = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return bits.view(np.float32).astype(np.float64), np.where(k == 0, -1, ids)
