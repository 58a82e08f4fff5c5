"""A routed MoE FFN block (E experts, top-k) for the expert-table tests: random quantised experts, the block run
through ops (route -> gate|up -> down -> combine) and its fp32 reference over the dequantised weights.

The reference takes the routing (`sel`, `topw`) as an input, the device's own when the block ran there: two router
logits a few 1e-4 apart may legitimately swap under another summation order, and a test of the expert launches
must not fail for that."""
import numpy as np
import torch

from nats_llm_studio_amd import ops
from nats_llm_studio_amd.gguf import quants as Q

SENT = -7.0

# Bound of the block output against the fp32 reference, relative to the largest |reference| value -- the bound of
# the GEMV tests (test_kernels_gpu._close). What separates the two: activations and the SwiGLU output are rounded to
# f16 (2^-11 relative each), the dequantised weights are exact in both, sums are fp32 over K = 256: a few 1e-3 of
# the largest value at most, so 2e-2 holds with room and a wrong expert (an independent random matrix: error of the
# order of the output itself) misses it by far more than 10x.
BLOCK_TOL = 2e-2


class Experts:
    """E experts: gate|up [2F, K] (rows interleaved in eights, ops.interleave_gate_up) and down [D, F]."""

    def __init__(self, E, K, F, D, gu_type, dn_type, device, seed=0):
        rng = np.random.default_rng(seed)
        self.E, self.K, self.F, self.D = E, K, F, D
        self.gu, self.dn, gud, dnd = [], [], [], []
        for _ in range(E):
            g = Q.random_blocks(gu_type, F * K, 0.05, rng)
            u = Q.random_blocks(gu_type, F * K, 0.05, rng)
            raw = ops.interleave_gate_up(g, u, gu_type, F, K)
            self.gu.append(ops.QWeight(raw, gu_type, 2 * F, K, device))
            gud.append(ops.QWeight(raw, gu_type, 2 * F, K, "cpu").dense())
            raw = Q.random_blocks(dn_type, D * F, 0.05, rng)
            self.dn.append(ops.QWeight(raw, dn_type, D, F, device))
            dnd.append(ops.QWeight(raw, dn_type, D, F, "cpu").dense())
        self.gu_rows = torch.cat(gud)              # fp32 [E * 2F, K]: expert e's rows start at e * 2F
        self.dn_dense = torch.stack(dnd)           # fp32 [E, D, F]
        self.tab_gu, self.tab_dn = ops.ExpertTable(self.gu), ops.ExpertTable(self.dn)


def buffers(E, T, k, F, D, device, cap=None, guard=64):
    """Route and expert buffers with sentinel fills; row maps carry a guard tail past E * cap."""
    cap = cap or (T + 63) // 64 * 64
    i32 = dict(dtype=torch.int32, device=device)
    return dict(
        cap=cap,
        topw=torch.zeros(T * k, device=device),
        counts=torch.zeros(E, **i32),
        xrows=torch.full((E * cap + guard,), int(SENT), **i32),
        yrows=torch.full((E * cap + guard,), int(SENT), **i32),
        sel=torch.full((T * k,), -1, **i32),
        act=torch.full((cap * k + 64, F), SENT, dtype=ops.ACT_DTYPE, device=device),
        yexp=torch.full((cap * k + 64, D), SENT, dtype=torch.float32, device=device),
    )


def run_block(ex: Experts, x, logits, T, k, b, table=True, selected=False, gu_cfg=None, dn_cfg=None):
    """Route `logits` and run the experts over x[:T] into b["yexp"]: through the expert tables (one launch per
    projection) or, table=False, through launches of 8 by-value segments each. Returns the combined [T, D]."""
    E, cap = ex.E, b["cap"]
    ops.moe_route(logits, T, k, b["topw"], b["counts"], b["xrows"], b["yrows"], cap, sel=b["sel"])
    gu_cfg, dn_cfg = gu_cfg or {}, dn_cfg or {}

    def sel(s0):
        return (b["sel"], T * k, s0) if selected else None
    xr, yr, cn = b["xrows"], b["yrows"], b["counts"]
    if table:
        ops.qgemv([ops.Seg(ex.gu[0], 0, xr, yr, cn)], x, b["act"], T, epi="swiglu", sel=sel(0),
                  table=(ex.tab_gu, cap), **gu_cfg)
        ops.qgemv([ops.Seg(ex.dn[0], 0, yr, yr, cn)], b["act"], b["yexp"], T, epi="f32", sel=sel(0),
                  table=(ex.tab_dn, cap), **dn_cfg)
    else:
        for s0 in range(0, E, 8):
            segs = [ops.Seg(ex.gu[e], 0, xr[e * cap:], yr[e * cap:], cn[e:e + 1]) for e in range(s0, min(E, s0 + 8))]
            ops.qgemv(segs, x, b["act"], T, epi="swiglu", sel=sel(s0), **gu_cfg)
        for s0 in range(0, E, 8):
            segs = [ops.Seg(ex.dn[e], 0, yr[e * cap:], yr[e * cap:], cn[e:e + 1]) for e in range(s0, min(E, s0 + 8))]
            ops.qgemv(segs, b["act"], b["yexp"], T, epi="f32", sel=sel(s0), **dn_cfg)
    out = torch.zeros(T, ex.D, device=x.device)
    ops.moe_combine(b["yexp"], b["topw"], T, k, out)
    return out


def block_reference(ex: Experts, x, sel, topw, T, k, width=None, swap=None):
    """fp32: out[t] = sum_j topw[t, j] * down_e(silu(gate_e x_t) * up_e x_t), e = sel[t, j], and the [T * k, D]
    expert rows. `width`: the expert width the reference believes in (expert e's gate|up rows start at
    e * 2 * width, wrapping: what taking the dense FFN key for the expert key does to the strides);
    `swap` = (a, b): experts a and b exchanged."""
    F, D = ex.F, ex.D
    w = width or F
    x = x[:T].float().cpu()
    sel = sel[:T * k].cpu().view(T, k).tolist()
    topw = topw[:T * k].float().cpu().view(T, k)
    n = ex.gu_rows.shape[0]
    rows = torch.zeros(T * k, D)
    for t in range(T):
        for j in range(k):
            e = sel[t][j]
            if swap and e in swap:
                e = swap[1] if e == swap[0] else swap[0]
            idx = (torch.arange(2 * F) + e * 2 * w) % n
            a4 = (x[t] @ ex.gu_rows[idx].t()).view(F // 8, 2, 8)
            act = (torch.nn.functional.silu(a4[:, 0]) * a4[:, 1]).reshape(F)
            rows[t * k + j] = act @ ex.dn_dense[e].t()
    out = (topw[:, :, None] * rows.view(T, k, D)).sum(1)
    return out, rows


def rel_err(out, ref):
    return ((out.float().cpu() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()
