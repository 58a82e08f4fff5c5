"""fp64 references, input families, the metric and the fault models of tests/test_rowops_sensitivity.py: the RoPE
rotation with the paged K/V append, the RMSNorms and the residual adds fused into them. Nothing here calls ops:
the references are numpy, generic over the dtype so that the same code in float32 IS the emulation of the kernels'
arithmetic (fp32 products and sums, the slab order, 1 / sqrt of the fp32 mean)."""
import numpy as np
import torch

SENT = -7.0          # exact in bf16, f16, f32 and fp8 e4m3: what every output buffer holds before the launch
BF16, FP8, F16, F32 = torch.bfloat16, torch.float8_e4m3fn, torch.float16, torch.float32
F8MAX = 448.0


# ------------------------------------------------------------------------------------------------------- metric

def round_term(ref, dt):
    """Half an ulp of a round-to-nearest store of `ref` in the output format (below the normal range: half the
    subnormal spacing). bf16 shares fp32's exponent range, so it has no floor here."""
    a = np.abs(ref)
    if dt == BF16:
        return 2.0 ** -8 * a
    if dt == F16:
        return np.maximum(2.0 ** -11 * a, 2.0 ** -25)
    if dt == FP8:
        return np.maximum(2.0 ** -4 * a, 2.0 ** -10)
    return 2.0 ** -24 * a


def ratio(out, ref, scale, dt, arith, written=None):
    """|out - ref| over the element's tolerance round_term(ref) + arith * scale; elements that are no target
    (written False) must equal ref, the sentinel. The e4m3 reference is clamped to +-448. NaN counts as inf."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    if dt == FP8:
        ref = np.clip(ref, -F8MAX, F8MAX)
    tol = round_term(ref, dt) + arith * np.asarray(scale, np.float64)
    if written is not None:
        tol = np.where(written, tol, 0.0)
    err = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return np.where(np.isfinite(r), r, np.inf)


def store(a, dt, clamp=True, trunc=False):
    """float64 array -> what a store of it in `dt` reads back (float64). e4m3 saturates like kv_st4 unless clamp is
    off (torch's cast then gives NaN above 464); trunc: a truncating (round-toward-zero) bf16 / f16 store."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if trunc and dt == BF16:
        return (a.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    if trunc:
        h = a.astype(np.float16)
        h = np.where(np.abs(h.astype(np.float64)) > np.abs(a), np.nextafter(h, np.float16(0)), h)
        return h.astype(np.float64)
    t = torch.from_numpy(a)
    if dt == FP8 and clamp:
        t = t.clamp(-F8MAX, F8MAX)
    return t.float().to(dt).float().double().numpy()


# ------------------------------------------------------------------------------------------ RoPE + append: inputs

def tag_table(kv, D):
    """A synthetic (cos, sin) table whose entries are exact in the K cache's format and name their own coordinates:
    bf16 cos[p, i] = (64 + i) 2^(p % 16 - 8), sin[p, i] = -(64 + i) 2^(p // 16 - 8) over 256 rows; e4m3 (4
    significant bits) cos = (8 + i % 8) 2^(p % 8 - 4), sin = -(8 + i // 8 % 8) 2^(p // 8 - 4) over 64 rows."""
    m, pe = (64, 16) if kv == BF16 else (8, 8)
    p = np.arange(pe * pe)[:, None]
    i = np.arange(D // 2)[None, :]
    cm, sm = (m + i % m), (m + (i % m if m == 64 else i // m % m))
    cs = np.stack([cm * 2.0 ** (p % pe - pe // 2), -sm * 2.0 ** (p // pe - pe // 2)], -1)
    return torch.from_numpy(cs.astype(np.float32))


def real_table(P, D, base, freq_factors=None):
    """ops.rope_table's formula in numpy (float64 angles, float32 entries)."""
    inv = 1.0 / (base ** (np.arange(0, D, 2, dtype=np.float64) / D))
    if freq_factors is not None:
        inv = inv / np.asarray(freq_factors, np.float64)
    ang = np.arange(P, dtype=np.float64)[:, None] * inv[None, :]
    return torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32))


def _positions(g, T, P):
    """Unsorted, repeated, with 0 (the identity rotation, on row 0: never a padding row), the table's last row and 1;
    from T = 5 the last table row also sits on a row that writes K / V, and one position repeats."""
    pos = torch.randint(0, P, (T,), generator=g)
    for j, v in enumerate((0, P - 1, 1, P - 1, 1)):
        if j < T:
            pos[j] = v
    return pos.to(torch.int32)


def _slots(g, T):
    """A random permutation into T + 5 slots; rows 1 and T - 1 are padding rows (slot -1) from T = 3."""
    slot = torch.randperm(T + 5, generator=g)[:T].to(torch.int32)
    if T >= 3:
        slot[1] = -1
        slot[T - 1] = -1
    return slot


def _split(x, ks, g, big=0.0):
    """ks slabs whose fp32 sum in the order 0..ks-1 is exactly x when x and the parts share a grid (tag), and
    large slabs that cancel to x otherwise (big: their size relative to 1)."""
    if ks == 1:
        return x[None].clone()
    if big:
        parts = torch.randn(ks - 1, *x.shape, generator=g) * big
    else:
        parts = torch.randint(-256, 257, (ks - 1, *x.shape), generator=g).float() * 2.0 ** -6
    first = x.double() - parts.double().sum(0)
    return torch.cat([first.float()[None], parts])


def rope_case(fam, kv, T, Hq, Hkv, D, ks=1, neox=False, bias=False, qk=None, seed=0, base=1e4, ff=False, P=256,
              var=0, pad=8):
    """One RoPE + append problem. fam: tag | real | saturate | slabs | eps. qk = eps of the per-head Q/K norm
    (weights of both signs, log-uniform) or None. Rows of the slabs and of q_out are `pad` columns wider than
    their payload. var: the pass of the tag family (what the head exponent names)."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * T + ks + D)
    ncol = (Hq + 2 * Hkv) * D
    half = D // 2
    if fam == "tag":
        cs = tag_table(kv, D)
    else:
        cs = real_table(P, D, base, (1.0 + 7.0 * torch.rand(half, generator=g)).numpy() if ff else None)
    P = cs.shape[0]
    pos, slot = _positions(g, T, P), _slots(g, T)
    t_, h_ = torch.arange(T)[:, None, None], torch.arange(Hq + 2 * Hkv)[None, :, None]
    bv = None
    if fam == "tag":
        # pairs (2^e, 0) or (0, 2^e), e naming row and head; V: integer tags of (row, head, column)
        e = ((3 * t_ + 5 * h_ + var) % 13 - 6) if kv == BF16 else ((t_ + 2 * h_ if var == 0 else h_ + 3 * t_) % 4 - 2)
        i_ = torch.arange(half)[None, None, :]
        first = ((t_ + h_ + i_ + var) % 2 == 0)
        x = torch.zeros(T, Hq + 2 * Hkv, D)
        a, b = (slice(0, half), slice(half, D)) if neox else (slice(0, D, 2), slice(1, D, 2))
        x[:, :, a] = torch.where(first, 2.0 ** e, 0.0)
        x[:, :, b] = torch.where(first, 0.0, 2.0 ** e)
        c_ = torch.arange(D)[None, None, :]
        hv = h_[:, Hq + Hkv:] - Hq - Hkv
        if kv == BF16:
            vt = ((t_ * Hkv + hv) * D + c_ + var) % 251 + 1
        else:
            vt = (1 + (c_ + 3 * hv + var) % 15) * 2.0 ** ((t_ + hv + c_ // 15) % 4)
        x[:, Hq + Hkv:] = vt.float()
        x = x.reshape(T, ncol)
        if bias:
            bv = torch.randint(-64, 65, (ncol,), generator=g).float() * 2.0 ** -6
            x = x - bv
        slabs = _split(x, ks, g)
    else:
        scale = 2.0 ** (torch.rand(T, Hq + 2 * Hkv, 1, generator=g) * 12 - 6)     # per head, log-uniform
        x = torch.randn(T, Hq + 2 * Hkv, D, generator=g) * scale
        if fam == "saturate":       # K and V values around and far above the e4m3 limit, next to small ones
            big = torch.tensor([447.0, 448.0, 449.0, 464.0, 480.0, 1e4])
            x = torch.randn(T, Hq + 2 * Hkv, D, generator=g) * 0.5
            kvp = x[:, Hq:].clone()
            idx = torch.randperm(kvp.numel(), generator=g)[:kvp.numel() // 4]
            sg = torch.where(torch.rand(idx.numel(), generator=g) < 0.5, -1.0, 1.0)
            kvp.view(-1)[idx] = big[torch.randint(0, 6, (idx.numel(),), generator=g)] * sg
            x[:, Hq:] = kvp
        if fam == "eps":            # heads with a mean square of eps / 100, eps and 100 eps
            x = torch.randn(T, Hq + 2 * Hkv, D, generator=g)
            x = x / x.pow(2).mean(-1, keepdim=True).sqrt()
            x = x * (qk * 10.0 ** (2.0 * ((t_ + h_) % 3 - 1))) ** 0.5
        x = x.reshape(T, ncol)
        if bias:
            bv = torch.randn(ncol, generator=g)
        slabs = _split(x, ks, g, big=64.0 * float(x.abs().max()) if fam == "slabs" else 1.0)
    ld, ldq = ncol + pad, Hq * D + pad
    full = torch.randn(slabs.shape[0], T, ld, generator=g)       # the padding columns hold noise nobody may read
    full[:, :, :ncol] = slabs
    c = dict(fam=fam, kv=kv, T=T, Hq=Hq, Hkv=Hkv, D=D, ks=ks, neox=neox, slabs=full, pos=pos, slot=slot, cs=cs, bias=bv,
             qk=qk, nslot=T + 5, ldq=ldq, qw=None, kw=None)
    if qk is not None:
        for n in ("qw", "kw"):
            sg = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
            c[n] = sg * 2.0 ** (torch.rand(D, generator=g) * 4 - 2)
    return c


# --------------------------------------------------------------------------------------- RoPE + append: reference

def sumsq(h, dt):
    """Sum of squares over the last axis. float32: as every kernel here forms it -- a lane adds the squares of its 4
    consecutive values in order, the lanes' partial sums meet in a binary tree (xor shuffles); all in fp32."""
    sq = (h * h).astype(dt)
    if dt == np.float64:
        return sq.sum(-1, keepdims=True)
    g = sq.reshape(*sq.shape[:-1], -1, 4)
    p = ((g[..., 0] + g[..., 1]) + g[..., 2]) + g[..., 3]
    n = 1 << max(0, int(p.shape[-1] - 1).bit_length())
    p = np.concatenate([p, np.zeros((*p.shape[:-1], n - p.shape[-1]), dt)], -1)
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p


def rope_ref(c, dt=np.float64, bias_after=False, k_unrot=False, v_rot=False, k_swap=False, flat_q=False):
    """The whole operation on one case: the slab sum in fp32 in the order 0..ks-1 and the bias add in fp32 (both
    exactly defined), then in `dt` the optional per-head RMSNorm and the rotation with cs[pos[t]]; Q into a q_out of
    row stride ldq, K and V into slot[t] unless it is negative. Returns the three full buffers (sentinel where nothing
    is written), the scale |x0 cos| + |x1 sin| of every rotated element (0 for V: a plain store) and the written
    masks. dt = float32 is the emulation of the kernels' arithmetic. The keyword faults are those that no change of the
    inputs expresses (module docstring of the tests)."""
    T, Hq, Hkv, D, neox = c["T"], c["Hq"], c["Hkv"], c["D"], c["neox"]
    ncol, half = (Hq + 2 * Hkv) * D, D // 2
    s = c["slabs"].numpy()
    x = s[0, :, :ncol].astype(np.float32)
    for k in range(1, s.shape[0]):
        x = (x + s[k, :, :ncol]).astype(np.float32)
    b = None if c["bias"] is None else c["bias"].numpy().astype(np.float32)
    if b is not None and not bias_after:
        x = (x + b[None, :]).astype(np.float32)
    x = x.astype(dt).reshape(T, Hq + 2 * Hkv, D)
    tb = c["cs"].numpy().astype(dt)[c["pos"].numpy().astype(np.int64)]
    cc, sn = tb[:, None, :, 0], tb[:, None, :, 1]

    def norm(h, w):
        if c["qk"] is None:
            return h
        ms = sumsq(h, dt) / dt(D) + dt(c["qk"])
        return h * (dt(1) / np.sqrt(ms)) * w.numpy().astype(dt)

    def rot(h):
        if neox:
            x0, x1 = h[..., :half], h[..., half:]
        else:
            x0, x1 = h[..., 0::2], h[..., 1::2]
        y0, y1 = x0 * cc - x1 * sn, x0 * sn + x1 * cc
        sc = np.abs(x0 * cc) + np.abs(x1 * sn), np.abs(x0 * sn) + np.abs(x1 * cc)
        if neox:
            return np.concatenate([y0, y1], -1), np.concatenate(sc, -1)
        return np.stack([y0, y1], -1).reshape(h.shape), np.stack(sc, -1).reshape(h.shape)

    qn, kn = norm(x[:, :Hq], c["qw"]), norm(x[:, Hq:Hq + Hkv], c["kw"])
    (q, qs), (k, ks_) = rot(qn), rot(kn)
    v = x[:, Hq + Hkv:].copy()
    if k_unrot:
        k[:, -1] = kn[:, -1]
    if v_rot:
        v[:, :1] = rot(v[:, :1])[0]
    if k_swap and Hkv > 1:
        k = k[:, np.arange(Hkv) ^ 1]
    if b is not None and bias_after:
        bb = b.astype(dt).reshape(Hq + 2 * Hkv, D)
        q, k, v = q + bb[None, :Hq], k + bb[None, Hq:Hq + Hkv], v + bb[None, Hq + Hkv:]
    ldq, ns = c["ldq"], c["nslot"]
    Q, Qs = np.full((T, ldq), SENT, np.float64), np.zeros((T, ldq))
    if flat_q:
        Q.reshape(-1)[:T * Hq * D] = q.reshape(-1)
        Qs.reshape(-1)[:T * Hq * D] = qs.reshape(-1)
        Qw = (np.arange(T * ldq) < T * Hq * D).reshape(T, ldq)
    else:
        Q[:, :Hq * D], Qs[:, :Hq * D] = q.reshape(T, -1), qs.reshape(T, -1)
        Qw = np.broadcast_to(np.arange(ldq) < Hq * D, (T, ldq))
    K, V = np.full((ns, Hkv, D), SENT, np.float64), np.full((ns, Hkv, D), SENT, np.float64)
    Ks, Kw = np.zeros((ns, Hkv, D)), np.zeros((ns, Hkv, D), bool)
    for t, sl in enumerate(c["slot"].tolist()):
        if sl >= 0:
            K[sl], Ks[sl], V[sl], Kw[sl] = k[t], ks_[t], v[t], True
    return dict(q=Q, k=K, v=V, qs=Qs, ks=Ks, vs=np.zeros_like(Ks), qw=Qw, kw=Kw, vw=Kw)


def rope_stored(r, kv, clamp=True, trunc=False):
    """What a correct round-to-nearest store of the reference buffers reads back."""
    return dict(q=store(r["q"], BF16, trunc=trunc), k=store(r["k"], kv, clamp, trunc and kv == BF16),
                v=store(r["v"], kv, clamp))


def rope_ratio(out, ref, kv, arith):
    """Largest ratio over q_out, the K cache and the V cache (dict q / k / v of float arrays) with where it is."""
    worst = (0.0, "")
    for n, dt in (("q", BF16), ("k", kv), ("v", kv)):
        r = ratio(out[n], ref[n], ref[n + "s"], dt, arith, ref[n + "w"])
        i = np.unravel_index(np.argmax(r), r.shape)
        if r[i] >= worst[0]:
            worst = (float(r[i]), f"{n}{tuple(int(j) for j in i)} out {np.asarray(out[n])[i]} ref {ref[n][i]}")
    return worst


def rope_noise(c):
    """The emulated fp32 arithmetic against fp64, |emu - ref| over the element's scale, at its largest."""
    r, e = rope_ref(c), rope_ref(c, np.float32)
    worst = 0.0
    for n in "qk":
        m = r[n + "w"] & (r[n + "s"] > 0)
        if m.any():
            worst = max(worst, float((np.abs(e[n] - r[n])[m] / r[n + "s"][m]).max()))
    return worst


def rope_faults(c):
    """(name, faulty case, keyword faults of rope_ref, store without the clamp) for every fault model that applies
    to this case."""
    T, half, cs, pos, slot = c["T"], c["D"] // 2, c["cs"], c["pos"], c["slot"]
    P = cs.shape[0]
    i = torch.arange(half)

    def w(**kw):
        return {**c, **kw}

    cs1 = cs.clone()
    cs1[:, 2:4] = cs[:, 3:5]
    yield "A1 4-column group 1 takes the next pair's angle", w(cs=cs1), {}, False
    cs2 = cs.clone()
    cs2[:, half - 8:] = cs[:, torch.clamp(i[half - 8:] + 1, max=half - 1)]
    yield "A1 last 8 pairs of a head take the next pair's angle", w(cs=cs2), {}, False
    yield "A2 table row p + 1", w(pos=torch.clamp(pos + 1, max=P - 1)), {}, False
    yield "A2 table row p - 1", w(pos=torch.clamp(pos - 1, min=0)), {}, False
    if T > 1:
        yield "A2 the neighbouring token's position", w(pos=torch.roll(pos, 1)), {}, False
    yield "A3 sin sign flipped", w(cs=cs * torch.tensor([1.0, -1.0])), {}, False
    yield "A3 cos and sin exchanged", w(cs=cs.flip(-1)), {}, False
    yield "A4 the other pairing", w(neox=not c["neox"]), {}, False
    yield "A5 last K head not rotated", c, dict(k_unrot=True), False
    yield "A5 first V head rotated", c, dict(v_rot=True), False
    if c["Hkv"] > 1:
        yield "A5 K head written to head h ^ 1", c, dict(k_swap=True), False
    rows = torch.arange(T, dtype=torch.int32)
    yield "A6 row index in place of slot[t]", w(slot=torch.where(slot >= 0, rows, slot)), {}, False
    if T > 1:
        yield "A6 the neighbouring row's slot", w(slot=torch.roll(slot, 1)), {}, False
    if bool((slot < 0).any()):
        for name, to in (("slot 0", torch.zeros_like(slot)), ("the last slot", torch.full_like(slot, c["nslot"] - 1)),
                         ("its row index", rows)):
            yield f"A6 a slot -1 row written to {name}", w(slot=torch.where(slot < 0, to, slot)), {}, False
    if c["bias"] is not None:
        yield "A7 bias added after the rotation", c, dict(bias_after=True), False
        yield "A7 bias of the neighbouring pair", w(bias=torch.roll(c["bias"], -2)), {}, False
        bz = c["bias"].clone()
        bz[(c["Hq"] + c["Hkv"]) * c["D"]:] = 0
        yield "A7 bias omitted on V", w(bias=bz), {}, False
    s = c["slabs"]
    if s.shape[0] > 1:
        yield "A8 one slab dropped", w(slabs=s[:-1]), {}, False
        yield "A8 later slabs read one row off", w(slabs=torch.cat([s[:1], torch.roll(s[1:], 1, 1)])), {}, False
    yield "A8 one slab doubled", w(slabs=torch.cat([s, s[-1:]])), {}, False
    if c["kv"] == FP8:
        yield "A9 fp8 without the clamp", c, {}, True
    if c["ldq"] > c["Hq"] * c["D"] and T > 1:
        yield "A10 Q written with stride Hq*D into a wider q_out", c, dict(flat_q=True), False


# -------------------------------------------------------------------------------------------------------- norms

def norm_weights(D, g):
    """Both signs, log-uniform over 2^-3 .. 2^3, another value in every column."""
    sg = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
    return sg * 2.0 ** (torch.rand(D, generator=g) * 6 - 3)


def norm_rows(fam, D, g, eps=1e-5, M=5):
    """Rows [M, D] f32 of one family: scaled (M Gaussian rows under 2^-12 .. 2^12), eps (3 rows with a mean square of
    eps / 100, eps, 100 eps), spike (2 rows: one element 2^12 times the rest, at column 0 and at column D - 1),
    integer (M rows of integers)."""
    if fam == "scaled":
        return torch.randn(M, D, generator=g) * 2.0 ** (torch.rand(M, 1, generator=g) * 24 - 12)
    if fam == "eps":
        x = torch.randn(3, D, generator=g)
        x = x / x.pow(2).mean(1, keepdim=True).sqrt()
        return x * (eps * torch.tensor([[0.01], [1.0], [100.0]])).sqrt()
    if fam == "spike":
        x = torch.randn(2, D, generator=g)
        x[0, 0], x[1, D - 1] = 4096.0, -4096.0
        return x
    return torch.randint(-1000, 1001, (M, D), generator=g).float()


def rms_ref(x, w, eps, dt=np.float64, fault=None):
    """rmsnorm(x) * w over the rows of x [M, D] in `dt` (float32: sumsq's fp32 sum of fp32 squares, 1 / sqrt of the
    fp32 mean, fp32 products). fault: one of RMS_FAULTS."""
    x, w = np.asarray(x).astype(dt), np.asarray(w).astype(dt)
    D = x.shape[1]
    xs = x
    if fault == "B3 last float4 group left out of the sum":
        xs = x[:, :-4]
    if fault == "B3 first float4 group counted twice":
        xs = np.concatenate([x[:, :4], x], 1)
    ss = sumsq(xs, dt)
    n = D
    if fault and fault.startswith("B2"):
        n = -(-D // int(fault.split()[-1])) * int(fault.split()[-1])
    ms = ss / dt(n)
    e = dt(eps)
    if fault == "B1 eps dropped":
        e = dt(0)
    if fault == "B1 eps times D":
        e = dt(eps * D)
    inv = dt(1) / (np.sqrt(ms) + e) if fault == "B1 eps added after the root" else dt(1) / np.sqrt(ms + e)
    if fault == "B5 statistic of the neighbouring row":
        inv = np.roll(inv, 1, 0)
    if fault == "B4 weight of the neighbouring group (i + 4)":
        w = np.roll(w, -4)
    if fault == "B4 weight of the neighbouring group (i - 4)":
        w = np.roll(w, 4)
    if fault == "B4 no weight":
        w = np.ones_like(w)
    return x * inv * w[None, :]


RMS_FAULTS = ["B1 eps dropped", "B1 eps added after the root", "B1 eps times D",
              "B2 mean over the width rounded up to 1024", "B2 mean over the width rounded up to 2048",
              "B3 last float4 group left out of the sum", "B3 first float4 group counted twice",
              "B4 weight of the neighbouring group (i + 4)", "B4 weight of the neighbouring group (i - 4)",
              "B4 no weight", "B5 statistic of the neighbouring row"]
ADD_FAULTS = ["B6 slab dropped", "B6 slab doubled", "B6 alpha also on the base", "B6 alpha omitted",
              "B6 h computed from the row before the add", "B6 x not written back"]
MOE_FAULTS = ["B7 combine weight of the neighbouring slot", "B7 expert row of the neighbouring token",
              "B7 last slot dropped"]


def add_ref(x, slabs, alpha, fault=None):
    """x + alpha * sum_k slab_k: the slab sum in fp32 from 0 in the order 0..ks-1 (exactly defined), the rest in
    float64. Returns (new x, its size |x| + |alpha acc|: what the two fp32 roundings of the update scale with)."""
    s = np.asarray(slabs, np.float32)
    if fault == "B6 slab dropped":
        s = s[:-1]
    if fault == "B6 slab doubled":
        s = np.concatenate([s, s[-1:]])
    acc = np.zeros(s.shape[1:], np.float32)
    for k in range(s.shape[0]):
        acc = (acc + s[k]).astype(np.float32)
    x, acc = np.asarray(x, np.float64), acc.astype(np.float64)
    a = 1.0 if fault == "B6 alpha omitted" else float(alpha)
    if fault == "B6 alpha also on the base":
        x = a * x
    return x + a * acc, np.abs(x) + np.abs(a * acc)


def moe_ref(x, y, wt, alpha, fault=None):
    """x[t] + alpha * sum_j wt[t, j] y[t k + j] in float64, with its size |x| + |alpha| sum |w y|."""
    x, wt = np.asarray(x, np.float64), np.asarray(wt, np.float64)
    T, k = wt.shape
    y = np.asarray(y, np.float64).reshape(T, k, -1)
    if fault == "B7 combine weight of the neighbouring slot":
        wt = np.roll(wt, 1, 1)
    if fault == "B7 expert row of the neighbouring token":
        y = np.roll(y, 1, 0)
    if fault == "B7 last slot dropped":
        wt = np.concatenate([wt[:, :-1], 0 * wt[:, -1:]], 1)
    t = alpha * wt[:, :, None] * y
    return x + t.sum(1), np.abs(x) + np.abs(t).sum(1)


def rms_ratio(out, ref, dt, arith):
    """Rows of a norm output (possibly wider than D and longer than M: everything else keeps the sentinel) against
    ref [M, D], every element on the scale |ref|."""
    out = np.asarray(out, np.float64)
    M, D = ref.shape
    full = np.full(out.shape, SENT)
    full[:M, :D] = ref
    wr = np.zeros(out.shape, bool)
    wr[:M, :D] = True
    r = ratio(out, full, np.abs(full), dt, arith, wr)
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), f"row {i[0]} column {i[1]}: out {out[i]} ref {full[i]}"


def x_ratio(x_out, x_ref, size, nround):
    """The written-back residual against its reference: within nround fp32 roundings (2^-24 each) of its size
    |x| + |update|; nround = 0: equality (the integer family)."""
    err = np.abs(np.asarray(x_out, np.float64) - x_ref)
    tol = nround * 2.0 ** -24 * size
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return float(np.where(np.isfinite(r), r, np.inf).max())
