"""Device ops. CUDA(HIP) tensors -> hand-written gfx950 kernels in `_kernels.so`;
CPU tensors -> the pure-torch fp32 reference of the same op (tests, CPU stub runs).

The CPU branch is never taken for GPU tensors: a missing kernel library on a GPU
box raises instead of silently running eager PyTorch.
"""
from __future__ import annotations

import ctypes
import math
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..gguf.constants import GGMLType, GGML_BLOCK
from ..gguf.quants import dequantize
from . import _lib
from . import transcode

EPI = {"f32": 0, "act": 1, "add": 2, "swiglu": 3, "slabs": 4, "argmax": 5, "rope": 6}
import os as _os
# Path-A row-parallel GEMVs of up to this many rows run the next RMSNorm in their last workgroup.
# Off by default: measured on MI355X at batch 1 it LENGTHENS the step (2.43 vs 2.25 ms/token) -- the
# last workgroup's ticket + acquire + row reload sit on the critical path and cost more than the
# separate norm launch inside a hipGraph (profiles/rocprof_b1_r02_addnorm.txt). NLS_ADDNORM=8 enables.
ADDNORM_MAX_M = int(_os.environ.get("NLS_ADDNORM", "0"))
# Large-M GEMMs switch to the dense f16 kernel (mode 4, csrc/kernels/hgemm.hip) from this many rows
# on, for weights that carry an f16 copy (QWeight.expand_dense)
DENSE_MIN_M = int(_os.environ.get("NLS_DENSE_GEMM_M", "128"))
# launch config of the mapped-row (MoE expert) path-A GEMV: mode, waves, row tiles, split
# (Mixtral-8x7B batch 1 / 16, profiles/moe_selected_experts.txt: 0,4,2,1 3.90 / 10.0 ms per step vs 0,8,1,1
# 4.94 / 15.1)
MOE_GEMV = tuple(int(v) for v in _os.environ.get("NLS_MOE_GEMV", "0,4,2,1").split(","))
# Every large-M projection runs on the hand-written dense GEMMs (modes 4/5/10, tuning "d:" entries). The
# library GEMM that r02-r03 dispatched for some shapes ("mode 7": hipBLASLt via torch.mm + a separate epilogue)
# is gone from the engine; tools/dense_tune.py keeps measuring against it as the reference
# (profiles/dense_tune_r04.jsonl).
ACT_DTYPE = torch.float16   # activation dtype of every GEMM/GEMV input and SwiGLU/RMSNorm/attention output


def _stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------
# Quantised weights
# ---------------------------------------------------------------------------

def to_device_layout(raw: np.ndarray, ggml_type: int, rows: int, K: int) -> np.ndarray:
    """ggml block bytes -> the "rows" layout (embedding tables; see csrc/kernels/common.h)."""
    t = GGMLType(ggml_type)
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    if t == GGMLType.Q6_K:
        b = raw.reshape(-1, 210)
        return np.concatenate([b[:, 0:128].reshape(-1), b[:, 128:192].reshape(-1), b[:, 192:208].reshape(-1),
                               b[:, 208:210].reshape(-1)])
    if t == GGMLType.Q8_0:
        b = raw.reshape(-1, 34)
        return np.concatenate([b[:, 2:34].reshape(-1), b[:, 0:2].reshape(-1)])
    return raw


TILE_BYTES = {GGMLType.Q4_K: 2304, GGMLType.Q5_K: 2816, GGMLType.Q6_K: 3360, GGMLType.Q8_0: 4352,
              GGMLType.F16: 8192, GGMLType.BF16: 8192, GGMLType.F32: 16384}


def tile_layout(raw: torch.Tensor, ggml_type: int, rows: int, K: int) -> torch.Tensor:
    """ggml block bytes (uint8 tensor, any device) -> the GEMV "tiled" layout: rows padded to
    16, one contiguous tile-block per (16-row tile, 256-value super-block), arranged so every
    wave-wide 16-B load reads 1 KiB contiguous (csrc/kernels/common.h)."""
    t = GGMLType(ggml_type)
    nb = K // 256
    rp = (rows + 15) // 16 * 16
    T = rp // 16
    rb = row_bytes(t, K)
    b = raw.reshape(rows, rb)
    if rp != rows:
        b = torch.cat([b, torch.zeros(rp - rows, rb, dtype=torch.uint8, device=b.device)])
    if t in (GGMLType.Q4_K, GGMLType.Q5_K):
        bs = 144 if t == GGMLType.Q4_K else 176
        q0 = 16 if t == GGMLType.Q4_K else 48
        B = b.reshape(T, 16, nb, bs)
        parts = [B[..., 0:16].permute(0, 2, 1, 3).reshape(T, nb, 256)]
        if t == GGMLType.Q5_K:        # QH[g][r][8]: qh bytes 8g..8g+7
            parts.append(B[..., 16:48].reshape(T, 16, nb, 4, 8).permute(0, 2, 3, 1, 4).reshape(T, nb, 512))
        # P_h[g][r] = chunk 2h bytes 8g..+8 | chunk 2h+1 bytes 8g..+8   (qs byte = 32c + 8g + i)
        qs = B[..., q0:q0 + 128].reshape(T, 16, nb, 2, 2, 4, 8)
        parts.append(qs.permute(0, 2, 3, 5, 1, 4, 6).reshape(T, nb, 2048))
    elif t == GGMLType.Q6_K:
        B = b.reshape(T, 16, nb, 210)
        ql = B[..., 0:128].reshape(T, 16, nb, 2, 2, 4, 8)          # ql byte = 64n + 32run + 8g + i
        qh = B[..., 128:192].reshape(T, 16, nb, 2, 4, 8)           # qh byte = 32n + 8g + i
        parts = [ql.permute(0, 2, 3, 5, 1, 4, 6).reshape(T, nb, 2048),     # QL_n[g][r][run][8]
                 qh.permute(0, 2, 4, 1, 3, 5).reshape(T, nb, 1024),        # QH[g][r][n][8]
                 B[..., 192:208].permute(0, 2, 1, 3).reshape(T, nb, 256),
                 B[..., 208:210].permute(0, 2, 1, 3).reshape(T, nb, 32)]
    elif t == GGMLType.Q8_0:
        B = b.reshape(T, 16, nb, 8, 34)
        d = B[..., 0:2].permute(0, 2, 1, 3, 4).reshape(T, nb, 256)
        qs = B[..., 2:34].reshape(T, 16, nb, 4, 2, 4, 8)           # block 2p + bb, byte 8g + i
        parts = [qs.permute(0, 2, 3, 5, 1, 4, 6).reshape(T, nb, 4096), d]
    elif t in (GGMLType.F16, GGMLType.BF16):
        parts = [b.reshape(T, 16, nb, 8, 4, 16).permute(0, 2, 3, 4, 1, 5).reshape(T, nb, 8192)]
    elif t == GGMLType.F32:
        parts = [b.reshape(T, 16, nb, 8, 4, 2, 16).permute(0, 2, 3, 5, 4, 1, 6).reshape(T, nb, 16384)]
    else:
        raise NotImplementedError(f"tiled layout for {t.name}")
    out = torch.cat(parts, dim=2) if len(parts) > 1 else parts[0]
    assert out.shape[2] == TILE_BYTES[t]
    return out.reshape(-1).contiguous()


def row_bytes(ggml_type: int, K: int) -> int:
    blk, nb = GGML_BLOCK[GGMLType(ggml_type)]
    return K // blk * nb


class QWeight:
    """A [rows, K] weight matrix resident on `device` in its quantised form.

    layout="tiled" (GEMV/GEMM operands) or "rows" (embedding tables, row gathers). `gtype` is the GGUF
    block type of the file; `type` the format the kernels execute (the same, except for the formats
    ops/transcode.py re-encodes at load: Q4_0/Q4_1/Q5_0/Q5_1 -> Q51, Q3_K -> Q6_K, Q2_K -> F16, and
    IQ4_NL/IQ4_XS -> IQ4: per (16-row tile, 256 values) 2304 bytes = [16 rows x 8 f16 scales] | the 4-bit codebook
    indices in Q4_K's nibble arrangement; the scale of 32 values is d (IQ4_NL, exact) or f16(d*(ls-32)) (IQ4_XS: the
    fp32 product rounded once, <= 2^-11 relative). As embedding tables ("rows") both become Q8_0 rows, qs = kv[q]."""

    def __init__(self, raw: np.ndarray, ggml_type: int, rows: int, K: int, device, name: str = "",
                 layout: str = "tiled"):
        self.gtype = int(ggml_type)
        self.type = int(ggml_type)
        self.rows = int(rows)
        self.K = int(K)
        self.name = name
        self.layout = layout
        self.device = torch.device(device)
        if K % 256:
            raise ValueError(f"{name}: K={K} is not a multiple of 256")
        with warnings.catch_warnings():     # read-only mmap views: copied below
            warnings.simplefilter("ignore", UserWarning)
            if GGMLType(ggml_type) in transcode.TRANSCODED:
                t = torch.from_numpy(np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(-1)))
                t = t.to(self.device) if self.device.type != "cpu" else t
                t, self.type = transcode.device_form(t, ggml_type, rows, K, layout)
                if layout == "rows":
                    t = torch.from_numpy(np.ascontiguousarray(to_device_layout(t.cpu().numpy(), self.type, rows, K)))
                    self.data = t.to(self.device) if self.device.type != "cpu" else t.clone()
                elif self.type in (transcode.QT_Q51, transcode.QT_IQ4):
                    self.data = t
                else:
                    self.data = tile_layout(t, self.type, rows, K)
            elif layout == "rows":
                t = torch.from_numpy(np.ascontiguousarray(to_device_layout(raw, ggml_type, rows, K)))
                self.data = t.to(self.device) if self.device.type != "cpu" else t.clone()
            else:
                t = torch.from_numpy(np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(-1)))
                t = t.to(self.device) if self.device.type != "cpu" else t
                self.data = tile_layout(t, ggml_type, rows, K)
        self._raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1) if self.device.type == "cpu" else None
        self._dense = None
        self.d16: Optional[torch.Tensor] = None    # row-major f16 copy for the large-M GEMM (mode 4)

    def to_f16(self) -> "QWeight":
        """This matrix re-encoded as tiled F16 (its dequantised values): for a fused launch whose segments
        would otherwise need two kernel type-sets (e.g. a Q2_K model's Q|K|V with a Q3_K V)."""
        if self.device.type == "cpu" or self.type == int(GGMLType.F16):
            return self
        w = QWeight.__new__(QWeight)
        w.__dict__.update(self.__dict__)
        w.type = int(GGMLType.F16)
        w.data = tile_layout(self.dense(torch.float16).contiguous().view(torch.uint8).reshape(-1), GGMLType.F16,
                             self.rows, self.K)
        w.d16 = None
        return w

    def expand_dense(self) -> int:
        """Keep a dequantised row-major f16 copy next to the quantised tiles (GPU; idempotent).
        Returns the bytes it added. Large-M GEMMs then run on MFMA without in-kernel dequantisation;
        the copy is the HIP dequant kernel's output, i.e. the very f16 values modes 2/3 feed their MFMAs."""
        if self.device.type != "cuda" or self.layout != "tiled" or self.d16 is not None:
            return 0
        self.d16 = self.dense(torch.float16).contiguous()
        return self.d16.numel() * 2

    @staticmethod
    def expand_dense_group(ws: Sequence["QWeight"]) -> int:
        """expand_dense for matrices launched together as adjacent output columns (a layer's Q|K|V): their f16
        copies become consecutive row ranges of ONE buffer, so a dense launch sees a single segment (_seg_arr
        merges them) -- no partial weight tile at each segment end, e.g. 64 whole 96-row tiles for Llama-3-8B's
        6144 Q|K|V rows instead of 43 + 11 + 11. Falls back to per-matrix copies when shapes or devices differ."""
        ws = list(ws)
        if (len(ws) < 2 or any(w.device.type != "cuda" or w.layout != "tiled" or w.d16 is not None for w in ws)
                or len({w.K for w in ws}) != 1 or len({str(w.device) for w in ws}) != 1):
            return sum(w.expand_dense() for w in ws)
        buf = torch.empty(sum(w.rows for w in ws), ws[0].K, dtype=torch.float16, device=ws[0].device)
        r0 = 0
        for w in ws:
            buf[r0:r0 + w.rows].copy_(w.dense(torch.float16))
            w.d16 = buf[r0:r0 + w.rows]
            r0 += w.rows
        return buf.numel() * 2

    @property
    def dense_bytes(self) -> int:
        return self.rows * self.K * 2

    @property
    def nbytes(self) -> int:
        return self.data.numel()

    def dense(self, dtype=torch.float32) -> torch.Tensor:
        """Dequantised [rows, K] (CPU: numpy ggml codec; GPU: HIP dequant kernel, f16)."""
        if self.device.type == "cpu":
            if self._dense is None:
                self._dense = torch.from_numpy(dequantize(self._raw, self.gtype, (self.rows, self.K)).copy())
            return self._dense.to(dtype)
        out = torch.empty(self.rows, self.K, dtype=ACT_DTYPE, device=self.device)
        _lib.check(_lib.lib().nls_dequant(self.data.data_ptr(), self.type, self.rows, self.K, out.data_ptr(),
                                          self.K, _stream_ptr(out)), "nls_dequant")
        return out.to(dtype)


# the device types each kernel type-set holds, in the sets' order (KSETS in csrc/kernels/gemv_args.h)
_KERNEL_SETS = ({12, 14}, {13, 14, 8}, {1, 30, 0}, {transcode.QT_Q51, 14, 8}, {transcode.QT_IQ4, 13, 14, 8})


def kernel_set(types) -> Optional[int]:
    """The HIP kernel type-set that runs one launch over segments of these device types: the lowest-numbered set
    that holds them all (type_set in csrc/kernels/qgemv.hip), None if no single set does."""
    ts = set(int(t) for t in types)
    return next((k for k, held in enumerate(_KERNEL_SETS) if ts <= held), None)


def interleave_gate_up(gate_raw: np.ndarray, up_raw: np.ndarray, ggml_type: int, rows: int, K: int,
                       group: int = 8) -> np.ndarray:
    """Rows [g0..g7, u0..u7, g8..g15, u8..u15, ...] so one 16-row MFMA tile yields 8 SwiGLU outputs."""
    rb = row_bytes(ggml_type, K)
    g = np.asarray(gate_raw).view(np.uint8).reshape(rows // group, group, rb)
    u = np.asarray(up_raw).view(np.uint8).reshape(rows // group, group, rb)
    return np.ascontiguousarray(np.concatenate([g, u], axis=1)).reshape(-1)


@dataclass
class Seg:
    w: QWeight
    ycol: int = 0
    xmap: Optional[torch.Tensor] = None     # int32 [max rows]
    ymap: Optional[torch.Tensor] = None     # int32 [max rows]
    mcount: Optional[torch.Tensor] = None   # int32 [1]


class ExpertTable:
    """The local experts of one MoE projection (same type, rows and K) as a device array of their weight pointers:
    a launch over the table (qgemv(table=...)) serves any number of experts, where the by-value segment list of a
    launch holds 8. Built once per layer and projection at load; it keeps the weights alive."""

    def __init__(self, ws: Sequence[QWeight]):
        self.ws = list(ws)
        w0 = self.ws[0]
        if any((w.type, w.rows, w.K, w.layout, w.device) != (w0.type, w0.rows, w0.K, w0.layout, w0.device)
               for w in self.ws):
            raise ValueError("ExpertTable: the experts of a projection must share type, shape and device")
        self.ptrs = None
        if w0.device.type == "cuda":
            self.ptrs = torch.tensor([w.data.data_ptr() for w in self.ws], dtype=torch.int64, device=w0.device)

    def __len__(self) -> int:
        return len(self.ws)


_WS = {}
_WS_OLD = []   # superseded workspaces stay alive: captured hipGraphs may still point at them


def _workspace(dev, n: int) -> torch.Tensor:
    """Split-K partial-slab workspace (64 MiB minimum; only grows, never freed)."""
    w = _WS.get(dev)
    if w is None or w.numel() < n:
        if w is not None:
            _WS_OLD.append(w)
        w = torch.empty(max(n, 16 << 20), dtype=torch.float32, device=dev)
        _WS[dev] = w
    return w


def dense_ok(segs: Sequence[Seg], M: int) -> bool:
    """May this launch run on the dense f16 GEMM (modes 4-6; the tuning table can still prefer the
    quantised kernel for the shape)?"""
    return M >= DENSE_MIN_M and all(s.w.d16 is not None and s.xmap is None and s.ymap is None for s in segs)


def gemv_config(segs: Sequence[Seg], M: int):
    """(mode, waves, rt, ks) for a launch. mode 0 = waves split K (small batch, mapped rows);
    mode 1 = waves split rows over an LDS-staged activation tile (+ split-K across workgroups);
    mode 2 = large-M LDS-dequant GEMM (K-quants; rt = waves along M: 256- or 128-row blocks);
    mode 4/5 = large-M dense f16 GEMM on the weights' f16 copies, 128/256 weight rows per workgroup
    (rt as mode 2)."""
    from . import tuning
    if dense_ok(segs, M):
        cfg = tuning.select_dense(segs, M)
        if cfg is not None and cfg[0] == 14 and len(_merge_dense(segs)) > 1:
            # mode 14's entries were measured on ONE merged f16 buffer (expand_dense_group: 64 whole 96-row tiles for
            # Llama-3-8B's Q|K|V); per-matrix copies make 65 tiles, 288 workgroups, and it loses to mode 4 (73 vs 45 us).
            # Same ks, so the same sums: mode 4's 16-wave instance at 128-row blocks.
            cfg = (4, 16, 2, cfg[3])
        if cfg is not None:
            return cfg
    return tuning.select(segs, M)


DENSE_MODES = (4, 5, 6, 10, 14)


def _merge_dense(segs: Sequence[Seg]):
    """[d16 pointer, rows, K, ycol, seg] per launch segment: adjacent unmapped segments whose f16 copies are consecutive
    rows of one buffer (QWeight.expand_dense_group) and whose output columns are adjacent merge into one."""
    out = []
    for s in segs:
        if s.w.d16 is None:
            raise ValueError(f"{s.w.name}: dense modes {DENSE_MODES} need QWeight.expand_dense()")
        p = s.w.d16.data_ptr()
        plain = s.xmap is None and s.ymap is None and s.mcount is None
        if out and plain and out[-1][4].xmap is None and out[-1][4].ymap is None and out[-1][4].mcount is None:
            q, rows, K, ycol, s0 = out[-1]
            if K == s.w.K and q + rows * K * 2 == p and ycol + rows == s.ycol:
                out[-1] = [q, rows + s.w.rows, K, ycol, s0]
                continue
        out.append([p, s.w.rows, s.w.K, s.ycol, s])
    return out


def _seg_arr(segs: Sequence[Seg], mode: int):
    """ctypes segment list of a launch (pass len(arr) as the segment count): the dense modes point at the row-major
    f16 copies, adjacent copies of one buffer merged into one segment (_merge_dense); MoE row maps included (the
    dense GEMM gathers/scatters mapped rows like mode 2)."""
    if mode in DENSE_MODES:
        merged = _merge_dense(segs)
        arr = (_lib.NlsSeg * len(merged))()
        for i, (p, rows, K, ycol, s) in enumerate(merged):
            arr[i] = _lib.NlsSeg(p, _p(s.xmap), _p(s.ymap), _p(s.mcount), 1, rows, K, ycol)
        return arr
    arr = (_lib.NlsSeg * len(segs))()
    for i, s in enumerate(segs):
        arr[i] = _lib.NlsSeg(s.w.data.data_ptr(), _p(s.xmap), _p(s.ymap), _p(s.mcount), s.w.type, s.w.rows, s.w.K,
                             s.ycol)
    return arr


NORM_FUSE_LDS = 54 * 1024      # staged-row budget of the fused-norm GEMV (64 KiB LDS minus the reduce area)


def norm_fusable(M: int, K: int) -> bool:
    """Can a path-A GEMV fold the RMSNorm of its M input rows (K wide) into its activation staging?"""
    return M <= 16 and M * K * 2 <= NORM_FUSE_LDS


def _ws_floats(segs: Sequence[Seg], M: int, mode: int, ks: int) -> int:
    """Floats a launch writes into the split-K workspace (the dispatcher's NlsPlan.ws_floats): ks slabs of M rows as
    wide as all the segments' rows -- mapped split-K: as one segment's, the experts share the output columns."""
    if mode == 0 or ks <= 1:
        return 0
    return ks * M * (segs[0].w.rows if all(s.ymap is not None for s in segs) else sum(s.w.rows for s in segs))


def _launch(segs: Sequence[Seg], x: torch.Tensor, y: torch.Tensor, M: int, alpha: float, epi: str, cfg, *, fz=None,
            argmax: Optional[torch.Tensor] = None, label: str = "nls_qgemv", soft: bool = False) -> bool:
    """Every call of the kernel library's one launch entry: segment array, split-K workspace and its size, the call,
    the result check under `label`. soft: False where the dispatcher refuses these arguments (code -1: nothing was
    launched, the caller tries its next config); any other failure raises either way."""
    mode, waves, rt, ks = cfg
    arr = _seg_arr(segs, mode)
    n = _ws_floats(segs, M, mode, ks)
    ws = _workspace(x.device, n).data_ptr() if n else None
    rc = _lib.lib().nls_qgemv(arr, len(arr), x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), M, float(alpha),
                              EPI[epi], _p(argmax), waves, rt, mode, ks, ws, n, _stream_ptr(x),
                              None if fz is None else ctypes.byref(fz))
    if soft and rc == -1:
        return False
    _lib.check(rc, label)
    return True


def _launch_slabs(segs: Sequence[Seg], x: torch.Tensor, y: torch.Tensor, M: int, alpha: float, cfg) -> torch.Tensor:
    """A split-K launch that leaves its ks partial slabs ([ks][M][sum of rows] f32) to the next kernel instead of
    reducing them. Returns the workspace that holds them."""
    _launch(segs, x, y, M, alpha, "slabs", cfg)
    return _WS[x.device]


def _fuse_norm(norm) -> "_lib.NlsFuse":
    """norm = (xf, w, eps[, ssq, ldss, nparts]) as the fused input RMSNorm of a launch."""
    xf, nw, eps = norm[:3]
    fz = _lib.NlsFuse(xf=xf.data_ptr(), ldxf=xf.stride(0), nw=nw.data_ptr(), eps=float(eps))
    if len(norm) == 6 and norm[3] is not None:
        fz.ssq_in, fz.ldss, fz.nss_in = norm[3].data_ptr(), int(norm[4]), int(norm[5])
    return fz


def _fuse_rope(fz, pos, slot, cs, bias, q_out, kc, vc, Hq: int, Hkv: int, D: int):
    """The RoPE + KV-append epilogue operands, added to `fz`."""
    fz.pos, fz.slot, fz.cs, fz.bias = pos.data_ptr(), slot.data_ptr(), cs.data_ptr(), _p(bias)
    fz.q_out, fz.ldq, fz.kc, fz.vc = q_out.data_ptr(), q_out.stride(0), kc.data_ptr(), vc.data_ptr()
    fz.Hq, fz.Hkv, fz.D = Hq, Hkv, D
    return fz


def _check_table(segs: Sequence[Seg], table, norm, argmax):
    tab, cap = table
    s0 = segs[0]
    if len(segs) != 1 or s0.mcount is None or s0.w is not tab.ws[0] or norm is not None or argmax is not None:
        raise ValueError("qgemv(table=): one mapped segment over the table's first expert")
    if s0.mcount.numel() < len(tab) or any(t is not None and t.numel() < len(tab) * cap for t in (s0.xmap, s0.ymap)):
        # the kernels index expert e's maps and count unchecked: fail here, not with a device fault
        raise ValueError("qgemv(table=): row maps / counts shorter than the table's experts x cap")


def qgemv(segs: Sequence[Seg], x: torch.Tensor, y: torch.Tensor, M: int, alpha: float = 1.0, epi: str = "f32",
          argmax: Optional[torch.Tensor] = None, waves: int = 0, rt: int = 1, mode: int = -1, ks: int = 1,
          norm=None, sel=None, table=None):
    """y (epilogue) alpha * x[:M] @ W^T for each segment. x: f16 [>=pad16(M), K].
    table = (ExpertTable, cap): `segs` is ONE segment with expert 0's row maps and count; expert e's weights come
    from the table, its maps lie e * cap entries on, its count e entries on (the MoE buffers' layout). Modes 0-2.
    sel = (int32 slots tensor, n_slots, base): MoE decode with few tokens -- launch only the routed experts' tiles
    (path A, mapped rows); slot i serves segment sel[i] - base.
    norm = (xf f32 [M, K], w f32 [K], eps[, ssq, ldss, nparts]): the GEMV input is f16(rmsnorm(xf) * w),
    computed inside the kernel (batch <= a few rows; `x` is then ignored on the GPU). With the partial
    sums of squares a qgemv_add_ssq producer left in `ssq`, the kernel skips the reduction pass and the
    tuned path-B (XL) config stays usable."""
    if not x.is_cuda:
        return _qgemv_cpu(segs, x, y, M, alpha, epi, argmax, norm, table)
    mapped = any(s.xmap is not None for s in segs)
    if norm is not None:
        return _qgemv_norm(segs, y, M, alpha, epi, argmax, norm, mapped)
    # 1. dtype and rows
    if table is not None:
        _check_table(segs, table, norm, argmax)
    if x.dtype != ACT_DTYPE:
        raise TypeError(f"qgemv: activations must be {ACT_DTYPE}, got {x.dtype}")
    routed = sel is not None or table is not None
    if not mapped and not routed and (x.shape[0] < M or (epi != "argmax" and y.shape[0] < M)):
        # the kernels index rows 0..M-1 unchecked: fail here, not with a device fault
        raise ValueError(f"qgemv: M={M} rows but x has {x.shape[0]}, y {y.shape[0]}")
    # 2. launch config
    if mode < 0 or waves == 0:
        mode, waves, rt, ks = MOE_GEMV if mapped or routed else gemv_config(segs, M)
    if sel is not None:
        mode, ks = 0, (1 if table is None else ks)
    if M > 64 and mode == 0 and not routed:
        # mapped (MoE) rows / path A: chunks of 64 rows
        for m0 in range(0, M, 64):
            mm = min(64, M - m0)
            qgemv(segs, x[m0:], y[m0:], mm, alpha, epi, None if argmax is None else argmax[m0:], waves, rt,
                  mode, ks)
        return y
    # 3. fused operands
    fz, label = None, "nls_qgemv"
    if routed:
        fz, label = _lib.NlsFuse(), "nls_qgemv(sel)"
        if sel is not None:
            fz.sel, fz.sel_slots, fz.sel_base = sel[0].data_ptr(), int(sel[1]), int(sel[2])
        if table is not None:
            fz.tab, fz.tab_n, fz.tab_cap = table[0].ptrs.data_ptr(), len(table[0]), int(table[1])
            label = "nls_qgemv(table)"
    # 4. launch
    _launch(segs, x, y, M, alpha, epi, (mode, waves, rt, ks), fz=fz, argmax=argmax, label=label)
    return y


def _qgemv_norm(segs, y, M, alpha, epi, argmax, norm, mapped):
    """qgemv(norm=) on the GPU: path A at the tuned instance (4 waves x 2 tiles where the tuned config is another
    path); with the partial sums the tuned path-A / path-B config first, where the dispatcher takes it."""
    split = len(norm) == 6 and norm[3] is not None
    if split and (mapped or M > 16):
        raise ValueError("fused-norm GEMV needs unmapped rows and M <= 16")
    if not split and (mapped or not norm_fusable(M, segs[0].w.K)):
        raise ValueError("fused-norm GEMV needs unmapped rows and M*K*2 <= NORM_FUSE_LDS")
    cfg = gemv_config(segs, M)
    if split:
        cands, label = ([cfg] if cfg[0] in (0, 1) else []) + [(0, 4, 2, 1)], "nls_qgemv(norm+ssq)"
    else:
        cands, label = [(0, cfg[1], cfg[2], 1) if cfg[0] == 0 else (0, 4, 2, 1)], "nls_qgemv(norm)"
    fz = _fuse_norm(norm)
    for c in cands:
        if _launch(segs, norm[0], y, M, alpha, epi, c, fz=fz, argmax=argmax, label=label, soft=split):
            return y
    raise ValueError("no launch config takes the split-RMSNorm operands")


def _qgemv_cpu(segs, x, y, M, alpha, epi, argmax, norm, table):
    """The fp32 reference of qgemv (CPU tensors)."""
    if norm is not None:
        xf, nw, eps = norm[:3]
        xs = xf[:M].float()
        x = (xs * torch.rsqrt(xs.pow(2).mean(dim=1, keepdim=True) + eps) * nw.float()).to(ACT_DTYPE)
    if table is not None:      # the same segments, one by one
        _check_table(segs, table, norm, argmax)
        (tab, cap), s0 = table, segs[0]
        segs = [Seg(w, s0.ycol, None if s0.xmap is None else s0.xmap[e * cap:],
                    None if s0.ymap is None else s0.ymap[e * cap:], s0.mcount[e:e + 1])
                for e, w in enumerate(tab.ws)]
    for s in segs:
        W = s.w.dense()
        if s.xmap is not None:
            cnt = int(s.mcount.item()) if s.mcount is not None else M
            cnt = min(cnt, M)
            xi = s.xmap[:cnt].long()
            yi = s.ymap[:cnt].long() if s.ymap is not None else torch.arange(cnt)
            xs = x.index_select(0, xi).float()
        else:
            cnt = M
            xs = x[:M].float()
            yi = torch.arange(M)
        if cnt == 0:
            continue
        acc = alpha * (xs @ W.t())
        n = W.shape[0]
        if epi == "swiglu":
            a4 = acc.view(cnt, n // 16, 2, 8)
            g, u = a4[:, :, 0, :], a4[:, :, 1, :]
            out = (torch.nn.functional.silu(g) * u).reshape(cnt, n // 2)
            y[yi, s.ycol:s.ycol + n // 2] = out.to(y.dtype)
        elif epi == "add":
            y[yi, s.ycol:s.ycol + n] += acc.to(y.dtype)
        elif epi != "argmax":
            y[yi, s.ycol:s.ycol + n] = acc.to(y.dtype)
        if argmax is not None:
            v, idx = acc.max(dim=1)
            key = _argmax_keys(v, idx + s.ycol)
            argmax[yi] = torch.maximum(argmax[yi], key)
    return y


def qgemv_add_ssq(seg: Seg, xin: torch.Tensor, x: torch.Tensor, M: int, alpha: float, ssq: torch.Tensor,
                  ldss: int, cfg=None) -> Optional[int]:
    """x[:M] += alpha * xin @ W^T, and when the launch runs on path A, each workgroup also leaves its
    share of sum(x_new^2) per token in ssq[m * ldss + wg] for the next fused-norm GEMV (split RMSNorm:
    no norm launch, no reduction pass in the consumer). Returns the number of shares (the launch's tile count,
    NlsPlan.tiles), or None when this launch cannot produce them (the consumer then normalises from the full
    rows)."""
    if x.is_cuda and seg.xmap is None and M <= 32:
        mode, waves, rt, ks = cfg or gemv_config([seg], M)
        ntile = -(-seg.w.rows // (16 * rt))
        if mode == 0 and ntile <= ldss:
            fz = _lib.NlsFuse(ssq_out=ssq.data_ptr(), ldss=int(ldss))
            if _launch([seg], xin, x, M, alpha, "add", (0, waves, rt, 1), fz=fz, label="nls_qgemv(ssq)", soft=True):
                return ntile
    qgemv([seg], xin, x, M, alpha=alpha, epi="add")
    return None


def qgemv_add_rmsnorm(seg: Seg, xin: torch.Tensor, x: torch.Tensor, norm_w: torch.Tensor, h: torch.Tensor, M: int,
                      alpha: float, eps: float, cfg=None, counter: Optional[torch.Tensor] = None):
    """x[:M] += alpha * xin @ W^T, then h[:M] = rmsnorm(x[:M]) * norm_w (f16). With a split-K
    launch config the partial slabs are reduced by the fused reduce+residual+RMSNorm kernel; a few-row
    path-A launch (M <= ADDNORM_MAX_M, `counter`: a zeroed int32 device word) normalises in its last
    workgroup, so the norm costs no launch at all."""
    if x.is_cuda and seg.xmap is None and seg.ycol == 0 and seg.w.rows == x.shape[1]:
        mode, waves, rt, ks = cfg or gemv_config([seg], M)
        if mode == 0 and counter is not None and M <= ADDNORM_MAX_M:
            fz = _lib.NlsFuse(hout=h.data_ptr(), ldh=h.stride(0), onw=norm_w.data_ptr(), cnt=counter.data_ptr(),
                              eps=float(eps))
            _launch([seg], xin, x, M, alpha, "add", (0, waves, rt, 1), fz=fz, label="nls_qgemv(addnorm)")
            return h
        if mode != 0 and ks > 1:
            ws = _launch_slabs([seg], xin, x, M, alpha, (mode, waves, rt, ks))
            _lib.check(_lib.lib().nls_splitk_add_rmsnorm(ws.data_ptr(), ks, M, float(alpha), x.data_ptr(), x.stride(0),
                                                         norm_w.data_ptr(), h.data_ptr(), h.stride(0), x.shape[1],
                                                         float(eps), _stream_ptr(x)), "nls_splitk_add_rmsnorm")
            return h
    if cfg is not None and x.is_cuda:
        mode, waves, rt, ks = cfg
        qgemv([seg], xin, x, M, alpha=alpha, epi="add", mode=mode, waves=waves, rt=rt, ks=ks)
    else:
        qgemv([seg], xin, x, M, alpha=alpha, epi="add")
    return rmsnorm(x, norm_w, h, M, eps)


def qgemv_add_norm_route(seg: Seg, xin: torch.Tensor, x: torch.Tensor, nw: torch.Tensor, h: torch.Tensor, M: int,
                         alpha: float, eps: float, counter: torch.Tensor, wr: torch.Tensor, logits: torch.Tensor, k: int,
                         topw: torch.Tensor, counts: torch.Tensor, xrows: torch.Tensor, yrows: torch.Tensor, cap: int,
                         renorm: bool = True, sel: Optional[torch.Tensor] = None) -> bool:
    """MoE decode (M <= 4 tokens): the o projection x[:M] += alpha * xin @ W^T, then -- in its last workgroup --
    the FFN RMSNorm h = f16(rmsnorm(x) * nw), the router logits h @ wr^T and the top-k route (moe_route): the
    separate norm + router + route launch (moe_norm_route) folded into the projection. False (nothing done)
    where the fused launch does not apply; the caller then runs the two launches."""
    if not x.is_cuda or seg.xmap is not None or seg.ycol or seg.w.rows != x.shape[1] or M > 4:
        return False
    mode, waves, rt, ks = gemv_config([seg], M)
    if mode != 0:
        waves, rt = 4, 1
    fz = _lib.NlsFuse(hout=h.data_ptr(), ldh=h.stride(0), onw=nw.data_ptr(), cnt=counter.data_ptr(), eps=float(eps),
                      wr=wr.data_ptr(), E=int(wr.shape[0]), topk=int(k), renorm=int(renorm), rcap=int(cap),
                      rlogits=logits.data_ptr(), topw=topw.data_ptr(), counts=counts.data_ptr(),
                      xrows=xrows.data_ptr(), yrows=yrows.data_ptr(), rsel=_p(sel))
    return _launch([seg], xin, x, M, alpha, "add", (0, waves, rt, 1), fz=fz, label="nls_qgemv(add+norm+route)",
                   soft=True)


def _argmax_keys(v: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    u = v.float().view(torch.int32).long() & 0xFFFFFFFF
    neg = (u & 0x80000000) != 0
    u = torch.where(neg, (~u) & 0xFFFFFFFF, u | 0x80000000)
    # GPU keys are unsigned u64; on CPU flip the top bit so signed int64 order == unsigned order
    return ((u ^ 0x80000000) << 32) | (0xFFFFFFFF - idx.long())


def argmax_reset(keys: torch.Tensor):
    """Initial value of a fused-argmax key buffer (smaller than every key). Decode on one GPU re-arms the
    keys inside argmax_unpack(rearm=True) instead of a separate launch (LlamaModel._keys_clean)."""
    if keys.is_cuda:
        keys.zero_()
    else:
        keys.fill_(torch.iinfo(torch.int64).min)


# ---------------------------------------------------------------------------
# Normalisation, RoPE + KV append, embedding, attention, sampling, MoE routing
# ---------------------------------------------------------------------------

def rmsnorm(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, M: int, eps: float):
    D = x.shape[1]
    if x.is_cuda:
        _lib.check(_lib.lib().nls_rmsnorm(x.data_ptr(), x.stride(0), w.data_ptr(), out.data_ptr(), out.stride(0), M,
                                          D, float(eps), int(out.dtype == torch.float32), _stream_ptr(x)),
                   "nls_rmsnorm")
        return out
    xs = x[:M].float()
    r = xs * torch.rsqrt(xs.pow(2).mean(dim=1, keepdim=True) + eps) * w.float()
    out[:M] = r.to(out.dtype)
    return out


def rope_inv_freq(head_dim: int, base: float, freq_factors=None) -> np.ndarray:
    """theta_i = base^(-2i/D), divided by GGUF `rope_freqs.weight` when present (Llama-3.1+ long-context
    frequency scaling, llama.cpp `rope_freq_factors`)."""
    inv = 1.0 / (base ** (np.arange(0, head_dim, 2, dtype=np.float64) / head_dim))
    if freq_factors is not None:
        inv = inv / np.asarray(freq_factors, dtype=np.float64).reshape(-1)[:head_dim // 2]
    return inv


def rope_table(max_pos: int, head_dim: int, base: float, device, freq_factors=None,
               pos_scale: float = 1.0) -> torch.Tensor:
    """[max_pos, D/2, 2] (cos, sin). `pos_scale` < 1: linear RoPE scaling (`rope.scaling.type=linear`)."""
    inv = rope_inv_freq(head_dim, base, freq_factors)
    ang = (np.arange(max_pos, dtype=np.float64) * pos_scale)[:, None] * inv[None, :]
    cs = np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)   # [P, D/2, 2]
    return torch.from_numpy(cs).to(device)


# K/V cache element types: bf16, or OCP fp8 e4m3 (half the attention bytes per decode step; opt-in,
# NLS_KV_DTYPE=fp8 -- the kernels saturate to +-448 and convert exactly to bf16 on load)
KV_DTYPES = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}


def _kv_fn(name: str, kc: torch.Tensor):
    """The kernel entry point for this cache's element type (`<name>8`: fp8)."""
    if kc.dtype == torch.float8_e4m3fn:
        return getattr(_lib.lib(), name + "8")
    if kc.dtype != torch.bfloat16:
        raise TypeError(f"{name}: KV cache dtype {kc.dtype} (bf16 or float8_e4m3fn)")
    return getattr(_lib.lib(), name)


def _kv_cast(v: torch.Tensor, dtype) -> torch.Tensor:
    """The CPU paths' cache store: fp8 e4m3 saturates to +-448 as the kernels' kv_st4 does (torch's cast alone gives
    NaN above 464)."""
    if dtype == torch.float8_e4m3fn:
        v = v.clamp(-448.0, 448.0)
    return v.to(dtype)


def rope_kv(qkv: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, cs: torch.Tensor, q_out: torch.Tensor,
            kc: torch.Tensor, vc: torch.Tensor, T: int, Hq: int, Hkv: int, D: int, neox: bool = False,
            bias: Optional[torch.Tensor] = None):
    """kc/vc: [slots, Hkv, D] bf16 for one layer. slot (int32) < 0 skips the cache write.
    `bias` (f32 [(Hq+2*Hkv)*D], Qwen2 QKV bias) is added before the rotation."""
    if qkv.is_cuda:
        _lib.check(_kv_fn("nls_rope_kv", kc)(qkv.data_ptr(), qkv.stride(0), 1, 0, _p(bias), pos.data_ptr(),
                                          slot.data_ptr(), cs.data_ptr(), q_out.data_ptr(), q_out.stride(0),
                                          kc.data_ptr(), vc.data_ptr(), T, Hq, Hkv, D, int(neox), _stream_ptr(qkv)),
                   "nls_rope_kv")
        return
    x = qkv[:T, :(Hq + 2 * Hkv) * D].float()             # rows may be wider than their Q|K|V payload
    if bias is not None:
        x = x + bias.float()[None, :x.shape[1]]
    p = pos[:T].long()
    c, s = cs[p, :, 0], cs[p, :, 1]                      # [T, D/2]

    def rot(h):                                          # h: [T, H, D]
        if neox:
            x0, x1 = h[..., :D // 2], h[..., D // 2:]
        else:
            x0, x1 = h[..., 0::2], h[..., 1::2]
        cc, ss = c[:, None, :], s[:, None, :]
        y0, y1 = x0 * cc - x1 * ss, x0 * ss + x1 * cc
        if neox:
            return torch.cat([y0, y1], dim=-1)
        return torch.stack([y0, y1], dim=-1).flatten(-2)

    q = rot(x[:, :Hq * D].view(T, Hq, D))
    k = rot(x[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D))
    v = x[:, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].view(T, Hkv, D)
    q_out[:T, :Hq * D] = q.reshape(T, Hq * D).to(q_out.dtype)
    sl = slot[:T].long()
    ok = sl >= 0
    kc[sl[ok]] = _kv_cast(k[ok], kc.dtype)
    vc[sl[ok]] = _kv_cast(v[ok], vc.dtype)


def qk_norm_rope_kv(qkv: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, cs: torch.Tensor, q_out: torch.Tensor,
                    kc: torch.Tensor, vc: torch.Tensor, T: int, Hq: int, Hkv: int, D: int, qw: torch.Tensor,
                    kw: torch.Tensor, eps: float, neox: bool = False, ks: int = 1, slab: int = 0):
    """rope_kv for the families with a per-head Q/K RMSNorm (Qwen3): every Q and K head is normalised over its D
    values with the weights qw / kw (f32 [D], shared by the heads) before the rotation; V is appended as it is.
    ks > 1: `qkv` holds ks split-K partial slabs (stride `slab` floats), summed in the order 0..ks-1 first."""
    if qkv.is_cuda:
        if qw.dtype != torch.float32 or kw.dtype != torch.float32 or qw.numel() != D or kw.numel() != D:
            raise ValueError(f"qk_norm_rope_kv: norm weights must be f32 [{D}]")
        _lib.check(_kv_fn("nls_qknorm_rope_kv", kc)(qkv.data_ptr(), qkv.stride(0), int(ks), int(slab), qw.data_ptr(),
                                                    kw.data_ptr(), float(eps), pos.data_ptr(), slot.data_ptr(),
                                                    cs.data_ptr(), q_out.data_ptr(), q_out.stride(0), kc.data_ptr(),
                                                    vc.data_ptr(), T, Hq, Hkv, D, int(neox), _stream_ptr(qkv)),
                   "nls_qknorm_rope_kv")
        return
    ncol = (Hq + 2 * Hkv) * D
    ld = qkv.stride(0)
    flat = qkv.reshape(-1).float()
    x = torch.zeros(T, ncol)
    for k in range(ks):                                  # slab k: rows of stride ld, starting k * slab floats in
        x = x + torch.as_strided(flat, (T, ncol), (ld, 1), k * slab)
    p = pos[:T].long()
    c, s = cs[p, :, 0], cs[p, :, 1]                      # [T, D/2]

    def rms(h, w):                                       # h: [T, H, D]
        return h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * w.float()

    def rot(h):
        if neox:
            x0, x1 = h[..., :D // 2], h[..., D // 2:]
        else:
            x0, x1 = h[..., 0::2], h[..., 1::2]
        cc, ss = c[:, None, :], s[:, None, :]
        y0, y1 = x0 * cc - x1 * ss, x0 * ss + x1 * cc
        if neox:
            return torch.cat([y0, y1], dim=-1)
        return torch.stack([y0, y1], dim=-1).flatten(-2)

    q = rot(rms(x[:, :Hq * D].view(T, Hq, D), qw))
    k = rot(rms(x[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D), kw))
    v = x[:, (Hq + Hkv) * D:].view(T, Hkv, D)
    q_out[:T, :Hq * D] = q.reshape(T, Hq * D).to(q_out.dtype)
    sl = slot[:T].long()
    ok = sl >= 0
    kc[sl[ok]] = _kv_cast(k[ok], kc.dtype)
    vc[sl[ok]] = _kv_cast(v[ok], vc.dtype)


def qkv_rope_kv(segs: Sequence[Seg], h: torch.Tensor, qkv: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor,
                cs: torch.Tensor, q_out: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, T: int, Hq: int, Hkv: int,
                D: int, neox: bool = False, cfg=None, bias: Optional[torch.Tensor] = None, norm=None,
                fuse_rope: bool = True, qk_norm=None):
    """QKV projection + RoPE + paged KV append. A path-A (few-row) launch rotates in the GEMV epilogue
    and writes q / K / V directly (one launch); with a split-K launch config the partial slabs are
    summed inside the RoPE kernel (no separate reduce pass, no fp32 qkv round trip).
    qk_norm = (qw, kw, eps): per-head Q/K RMSNorm before the rotation (Qwen3) -- the projection is followed by
    the stand-alone norm + RoPE + append kernel (qk_norm_rope_kv; no epilogue of the projection kernels knows the
    norm, and such a family has no QKV bias); a split-K launch config leaves its slabs to that kernel."""
    if qk_norm is not None and bias is not None:
        raise ValueError("qkv_rope_kv: a Q/K norm with a QKV bias is not supported")

    def rope(src, ks=1, slab=0):
        if qk_norm is not None:
            return qk_norm_rope_kv(src, pos, slot, cs, q_out, kc, vc, T, Hq, Hkv, D, *qk_norm, neox, ks=ks, slab=slab)
        if ks == 1:
            return rope_kv(src, pos, slot, cs, q_out, kc, vc, T, Hq, Hkv, D, neox, bias)
        _lib.check(_kv_fn("nls_rope_kv", kc)(src.data_ptr(), src.stride(0), ks, slab, _p(bias), pos.data_ptr(),
                                             slot.data_ptr(), cs.data_ptr(), q_out.data_ptr(), q_out.stride(0),
                                             kc.data_ptr(), vc.data_ptr(), T, Hq, Hkv, D, int(neox), _stream_ptr(h)),
                   "nls_rope_kv")

    if h.is_cuda and all(s.xmap is None for s in segs):
        mode, waves, rt, ks = cfg or gemv_config(segs, T)
        ncol = sum(s.w.rows for s in segs)
        # plain rows: contiguous Q|K|V columns from 0, exactly the heads' values
        plain = (ncol == (Hq + 2 * Hkv) * D
                 and all(s.ycol == sum(x.w.rows for x in segs[:i]) for i, s in enumerate(segs)))
        epilogue = plain and qk_norm is None and not neox and fuse_rope and kc.dtype == torch.bfloat16
        if epilogue and ((mode == 0 and T <= 64) or (mode in (4, 5, 10, 14) and ks == 1 and norm is None)):
            # RoPE + KV append in the epilogue of path A or of the large-M GEMM on the dense f16 copies (no f32 qkv
            # round trip, no RoPE launch)
            if norm is not None and not norm_fusable(T, segs[0].w.K):
                raise ValueError("fused-norm GEMV needs M*K*2 <= NORM_FUSE_LDS")
            fz = _fuse_rope(_lib.NlsFuse() if norm is None else _fuse_norm(norm), pos, slot, cs, bias, q_out, kc, vc,
                            Hq, Hkv, D)
            _launch(segs, h, qkv, T, 1.0, "rope", (mode, waves, rt, 1), fz=fz,
                    label="nls_qgemv(rope)" if mode == 0 else "nls_qgemv(dense rope)")
            return
        if norm is None and mode != 0 and ks > 1 and plain:
            ws = _launch_slabs(segs, h, qkv, T, 1.0, (mode, waves, rt, ks))
            return rope(ws[:ks * T * ncol].view(ks * T, ncol), ks, T * ncol)
        if norm is None and cfg is not None and qk_norm is not None:
            qgemv(segs, h, qkv, T, waves=waves, rt=rt, mode=mode, ks=ks)
            return rope(qkv)
    qgemv(segs, h, qkv, T, norm=norm)
    rope(qkv)


def embed(ids: torch.Tensor, w: QWeight, out: torch.Tensor, T: int, scale: float = 1.0, prev=None):
    """out[:T] = scale * W[ids[:T]]. prev = (next_ids, use_prev) (chained decode): first
    ids[t] = next_ids[t] where use_prev[t] != 0 (in the same launch on the GPU)."""
    if ids.is_cuda:
        if prev is not None:
            nxt, use = prev
            _lib.check(_lib.lib().nls_embed_prev(ids.data_ptr(), nxt.data_ptr(), use.data_ptr(), T, w.data.data_ptr(),
                                                 w.type, w.rows, w.K, out.data_ptr(), out.stride(0), float(scale),
                                                 _stream_ptr(ids)), "nls_embed_prev")
            return out
        _lib.check(_lib.lib().nls_embed(ids.data_ptr(), T, w.data.data_ptr(), w.type, w.rows, w.K, out.data_ptr(),
                                        out.stride(0), float(scale), _stream_ptr(ids)), "nls_embed")
        return out
    if prev is not None:
        nxt, use = prev
        torch.where(use[:T] != 0, nxt[:T], ids[:T], out=ids[:T])
    out[:T] = scale * w.dense()[ids[:T].long()]
    return out


def attention(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, block_tables: torch.Tensor,
              tok_seq: torch.Tensor, ctx_len: torch.Tensor, out: torch.Tensor, T: int, Hq: int, Hkv: int, D: int,
              block_size: int, scale: float, chunk: int = 256, n_split: int = 1,
              workspace: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None):
    """Paged GQA attention; query t attends to the first ctx_len[t] positions of sequence tok_seq[t].
    n_split > 1 (flash-decoding): `counters` (zeroed int32 [>= T*Hkv]) lets the last split of each
    (token, kv head) merge the partials in-kernel; without it a combine kernel runs."""
    if q.is_cuda:
        po = pml = None
        if counters is not None and (counters.numel() < T * Hkv or counters.dtype != torch.int32):
            raise ValueError("attention counters must be int32 with >= T*Hkv entries")
        if n_split > 1:
            need = T * Hq * n_split * (D + 2)
            if workspace is None or workspace.numel() < need:
                workspace = torch.empty(need, dtype=torch.float32, device=q.device)
            po = workspace.data_ptr()
            pml = po + T * Hq * n_split * D * 4
        _lib.check(_kv_fn("nls_attn_decode", kc)(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(),
                                              block_tables.data_ptr(), block_tables.stride(0), tok_seq.data_ptr(),
                                              ctx_len.data_ptr(), T, Hq, Hkv, D, block_size, float(scale), chunk,
                                              n_split, out.data_ptr(), out.stride(0), po, pml,
                                              _p(counters) if n_split > 1 else None, _stream_ptr(q)),
                   "nls_attn_decode")
        return out
    G = Hq // Hkv
    for t in range(T):
        n = int(ctx_len[t])
        if n <= 0:
            out[t, :Hq * D] = 0
            continue
        bt = block_tables[int(tok_seq[t])].long()
        p = torch.arange(n)
        slots = bt[p // block_size] * block_size + p % block_size
        k = kc[slots].float()                                  # [n, Hkv, D]
        v = vc[slots].float()
        qq = q[t, :Hq * D].float().view(Hkv, G, D)
        s = torch.einsum("hgd,nhd->hgn", qq, k) * scale
        pr = torch.softmax(s, dim=-1)
        o = torch.einsum("hgn,nhd->hgd", pr, v)
        out[t, :Hq * D] = o.reshape(Hq * D).to(out.dtype)
    return out


# attn_prefill.hip: the 8-wave 32x32x16 kernel takes 64-token query blocks; NLS_PREFILL_V1=1 selects the first
# kernel (4 waves, 32-token blocks) for A/B
PREFILL_V1 = _os.environ.get("NLS_PREFILL_V1", "0") == "1"
PREFILL_QT = 32 if PREFILL_V1 else 64      # tokens per attention_prefill query block


def prefill_blocks(tok_seq, pos, T: int):
    """Query blocks for attention_prefill: (t0, ntok<=PREFILL_QT, seq, pos0) over runs of consecutive
    tokens of one sequence (numpy int arrays in, int32 [nqb, 4] out)."""
    ts = np.asarray(tok_seq[:T])
    ps = np.asarray(pos[:T])
    if T == 0:
        return np.zeros((0, 4), np.int32)
    cut = np.flatnonzero((ts[1:] != ts[:-1]) | (ps[1:] != ps[:-1] + 1)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [T]])
    out = []
    for a, b in zip(starts, ends):
        for t in range(a, b, PREFILL_QT):
            out.append((t, min(PREFILL_QT, b - t), ts[a], ps[t]))
    return np.asarray(out, dtype=np.int32).reshape(-1, 4)


def attention_prefill_ok(Hq: int, Hkv: int, D: int) -> bool:
    return Hq % Hkv == 0 and (Hq // Hkv) % 4 == 0 and D in (64, 128)


def attention_prefill(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, block_tables: torch.Tensor,
                      qblocks: torch.Tensor, nqb: int, tok_seq: torch.Tensor, ctx_len: torch.Tensor,
                      out: torch.Tensor, T: int, Hq: int, Hkv: int, D: int, block_size: int, scale: float):
    """Causal MFMA flash attention over the paged cache for prompt chunks (query blocks of PREFILL_QT tokens,
    ops.prefill_blocks)."""
    if q.is_cuda:
        _lib.check(_kv_fn("nls_attn_prefill_v1" if PREFILL_V1 else "nls_attn_prefill", kc)(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(),
                                               block_tables.data_ptr(), block_tables.stride(0), qblocks.data_ptr(),
                                               nqb, Hq, Hkv, D, block_size, float(scale), out.data_ptr(),
                                               out.stride(0), _stream_ptr(q)), "nls_attn_prefill")
        return out
    return attention(q, kc, vc, block_tables, tok_seq, ctx_len, out, T, Hq, Hkv, D, block_size, scale)


def argmax(logits: torch.Tensor, M: int, out: torch.Tensor):
    V = logits.shape[1]
    if logits.is_cuda:
        _lib.check(_lib.lib().nls_argmax(logits.data_ptr(), logits.stride(0), M, V, out.data_ptr(),
                                         _stream_ptr(logits)), "nls_argmax")
        return out
    out[:M] = logits[:M].float().argmax(dim=1).to(out.dtype)
    return out


def topc_candidates(logits: torch.Tensor, n: int, C: int, vocab_lo: int, valid: int):
    """Per row, the C largest logits of a vocab shard (columns [0, valid) of `logits`; the rest are padding)
    in increasing vocabulary order: (values f32 [n, C], global token ids int32 [n, C]), padded with
    (-inf, -1) where the shard holds fewer than C tokens. Tensor-parallel sampling gathers these instead of
    the [n, vocab] logits (engine: _gather / _sample_candidates).

    GPU: ONE launch of sample.hip topc_kernel (radix select + in-order compaction) writing both planes of a
    [2, n, C] int32 block -- the source buffer of the candidate all-gather, which comm.gather_candidates uses as it
    is (`_packed`): no topk / sort / gather / fill / stack kernels in the captured decode graph."""
    if logits.is_cuda:
        if logits.dtype != torch.float32 or logits.stride(1) != 1:
            raise TypeError("topc_candidates: fp32 row-major logits")
        src = torch.empty(2, n, C, dtype=torch.int32, device=logits.device)
        _lib.check(_lib.lib().nls_topc(logits.data_ptr(), logits.stride(0), n, int(valid), C, int(vocab_lo),
                                       src.data_ptr(), _stream_ptr(logits)), "nls_topc")
        v, i = src[0].view(torch.float32), src[1]
        v._packed = i._packed = src
        return v, i
    k = max(0, min(C, valid))
    v = torch.full((n, C), float("-inf"), dtype=torch.float32, device=logits.device)
    i = torch.full((n, C), -1, dtype=torch.int32, device=logits.device)
    if k and n:
        tv, ti = torch.topk(logits[:n, :valid].float(), k, dim=1)
        ti, order = torch.sort(ti, dim=1)                    # vocabulary order within the shard
        v[:, :k] = torch.gather(tv, 1, order)
        i[:, :k] = (ti + vocab_lo).to(torch.int32)
    return v, i


def argmax_unpack(keys: torch.Tensor, n: int, out: torch.Tensor, rearm: bool = False):
    """Token ids from the fused arg-max keys. rearm: reset keys[:n] in the same launch (see argmax_reset)."""
    if keys.is_cuda:
        fn = _lib.lib().nls_argmax_unpack_rearm if rearm else _lib.lib().nls_argmax_unpack
        _lib.check(fn(keys.data_ptr(), n, out.data_ptr(), _stream_ptr(keys)), "nls_argmax_unpack")
        return out
    out[:n] = (0xFFFFFFFF - (keys[:n] & 0xFFFFFFFF)).to(out.dtype)
    if rearm:
        argmax_reset(keys[:n])
    return out


SAMPLE_PARAMS_BYTES = 40      # csrc/kernels/sample.hip SampleParams


def sample_params_bytes(p=None, n_bias: Optional[int] = None) -> bytes:
    """Device SampleParams of one row; None: a greedy row (skipped by the in-graph sampler). n_bias: the entries
    of the row's logit_bias table the sampler applies (default: all of p.logit_bias; 0 where the launch gets no
    tables)."""
    if p is None:
        sp = _lib.SampleParams(0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0, 0, 0)
    else:
        nb = len(getattr(p, "logit_bias", ())) if n_bias is None else int(n_bias)
        sp = _lib.SampleParams(p.temperature, p.top_p, p.min_p, p.repeat_penalty, p.presence_penalty,
                               p.frequency_penalty, 0.0, int(p.top_k or 0), 0, nb)
    raw = bytes(sp)
    assert len(raw) == SAMPLE_PARAMS_BYTES
    return raw


def sample_decode(logits: torch.Tensor, n: int, params: torch.Tensor, seeds: torch.Tensor, pos: torch.Tensor,
                  ctx_len: torch.Tensor, hist: torch.Tensor, next_ids: torch.Tensor,
                  bias_ids: Optional[torch.Tensor] = None, bias_val: Optional[torch.Tensor] = None):
    """In-graph sampling of decode rows [0, n): rows whose device params ask for sampling overwrite
    next_ids with a draw (uniform from (seed, position)), appending it to their history ring. With the logit_bias
    tables (`bias_ids` int32 / `bias_val` fp32, [rows, stride], a row's first n_bias entries -- distinct ids --
    used), a row's biases are added to its raw logits for the draw and taken off again: the row is left raw."""
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise TypeError("sample_decode: fp32 row-major logits")
    if bias_ids is not None or bias_val is not None:
        if (bias_ids is None or bias_val is None or bias_ids.dtype != torch.int32 or bias_val.dtype != torch.float32
                or bias_ids.shape != bias_val.shape or bias_ids.dim() != 2 or bias_ids.shape[0] < n
                or not bias_ids.is_contiguous() or not bias_val.is_contiguous()):
            raise TypeError("sample_decode: int32 ids / fp32 values, contiguous [rows >= n, stride] tables")
        _lib.check(_lib.lib().nls_sample_decode_bias(
            logits.data_ptr(), logits.stride(0), n, logits.shape[1], params.data_ptr(), seeds.data_ptr(),
            pos.data_ptr(), ctx_len.data_ptr(), hist.data_ptr(), hist.shape[1], bias_ids.data_ptr(),
            bias_val.data_ptr(), bias_ids.shape[1], next_ids.data_ptr(), _stream_ptr(logits)), "nls_sample_decode_bias")
        return
    _lib.check(_lib.lib().nls_sample_decode(logits.data_ptr(), logits.stride(0), n, logits.shape[1], params.data_ptr(),
                                            seeds.data_ptr(), pos.data_ptr(), ctx_len.data_ptr(), hist.data_ptr(),
                                            hist.shape[1], next_ids.data_ptr(), _stream_ptr(logits)),
               "nls_sample_decode")


def sample_decode_cand(vals: torch.Tensor, ids: torch.Tensor, n: int, params: torch.Tensor, seeds: torch.Tensor,
                       pos: torch.Tensor, ctx_len: torch.Tensor, hist: torch.Tensor, next_ids: torch.Tensor):
    """In-graph sampling of tensor-parallel decode rows [0, n) from the gathered candidates (values `vals`
    [n, M] in vocabulary order -- scratch, penalties are applied in place -- and global ids `ids` [n, M]):
    sample_decode's semantics with the history ring mapped onto candidate positions."""
    M = vals.shape[1]
    if vals.is_cuda:
        if vals.dtype != torch.float32 or vals.stride(1) != 1 or ids.stride(1) != 1:
            raise TypeError("sample_decode_cand: fp32 / int32 row-major candidates")
        _lib.check(_lib.lib().nls_sample_decode_cand(vals.data_ptr(), vals.stride(0), n, M, ids.data_ptr(),
                                                     ids.stride(0), params.data_ptr(), seeds.data_ptr(), pos.data_ptr(),
                                                     ctx_len.data_ptr(), hist.data_ptr(), hist.shape[1],
                                                     next_ids.data_ptr(), _stream_ptr(vals)), "nls_sample_decode_cand")
        return
    # CPU twin of sample.hip sample_decode_cand_kernel (gloo rehearsals of the tensor-parallel path)
    from ..engine.sampling import SamplingParams, cand_positions, cand_token, sample_rows, uniform01
    raw = params.cpu().numpy()
    S = hist.shape[1]
    for r in range(n):
        if int(ctx_len[r]) <= 0:
            continue
        sp = _lib.SampleParams.from_buffer_copy(raw[r].tobytes())
        p = SamplingParams(temperature=sp.temperature, top_k=sp.top_k, top_p=sp.top_p, min_p=sp.min_p,
                           repeat_penalty=sp.repeat_penalty, presence_penalty=sp.presence_penalty,
                           frequency_penalty=sp.frequency_penalty)
        if p.greedy:
            continue
        ps = int(pos[r])
        nh = min(S, ps + 1)
        idl = ids[r].tolist()
        hp = cand_positions(hist[r, :nh].tolist(), idl)
        seed = int(seeds[r]) & 0xFFFFFFFFFFFFFFFF
        j = sample_rows(vals[r:r + 1].float(), [p], [hp], [uniform01(seed, ps)])[0]
        tok = cand_token(idl, j)
        next_ids[r] = tok
        hist[r, (ps + 1) % S] = tok


LP_TOP, LP_REC = _lib.LP_TOP, _lib.LP_REC     # logprob records (checked against the library when it loads)


def logprob_stash(n: int, hist_stride: int, device) -> torch.Tensor:
    """Scratch of token_logprobs for n rows: a penalised row's history window with its raw logits."""
    return torch.zeros(n, 1 + 2 * hist_stride, dtype=torch.int32, device=device)


def token_logprobs(logits: torch.Tensor, n: int, n_top: torch.Tensor, rec: torch.Tensor, V: Optional[int] = None,
                   ctx_len: Optional[torch.Tensor] = None, params: Optional[torch.Tensor] = None,
                   pos: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
                   stash: Optional[torch.Tensor] = None):
    """Per-token log-probabilities of rows [0, n), first half (BEFORE the sampler touches the rows): log_softmax of
    the raw fp32 logits over columns [0, V) at temperature 1, non-finite entries skipped. Row r with n_top[r] >= 0
    (and ctx_len[r] > 0, if given) gets the n_top[r] (<= LP_TOP) most likely tokens into its record rec[r] (LP_REC
    int32 words), by descending logit, ties by lower id, padded with (-1, -inf) when the row has fewer finite
    entries; other records are left untouched. With `stash` (logprob_stash) and the sampler's device tables
    (`params`, `pos`, `hist`), the raw logits of a penalised row's history window are kept for
    token_logprobs_pick, which completes the records once the tokens are drawn."""
    V = logits.shape[1] if V is None else int(V)
    if logits.is_cuda:
        if logits.dtype != torch.float32 or logits.stride(1) != 1 or rec.dtype != torch.int32 or not rec.is_contiguous():
            raise TypeError("token_logprobs: fp32 row-major logits, contiguous int32 records")
        if n_top.dtype != torch.int32 or rec.shape[1] != LP_REC or V > logits.shape[1]:
            raise TypeError("token_logprobs: int32 n_top, LP_REC-word records, V within the row")
        S = hist.shape[1] if hist is not None else (stash.shape[1] - 1) // 2 if stash is not None else 0
        if stash is not None and (stash.shape[0] < n or stash.shape[1] != 1 + 2 * S or not stash.is_contiguous()):
            raise TypeError("token_logprobs: stash does not match the history ring")
        _lib.check(_lib.lib().nls_logprobs(logits.data_ptr(), logits.stride(0), n, V, n_top.data_ptr(), _p(ctx_len),
                                           _p(params) if stash is not None else None, _p(pos), _p(hist), S,
                                           rec.data_ptr(), _p(stash), _stream_ptr(logits)), "nls_logprobs")
        return rec
    # CPU twin: fp64 log_softmax, stable sort on (-logit, id). Words 0..1 hold the fp64 log-sum-exp for the pick
    # (the CPU samplers never rewrite the logits row: no stash)
    for r in range(n):
        nt = min(int(n_top[r]), LP_TOP)
        if nt < 0 or (ctx_len is not None and int(ctx_len[r]) <= 0):
            continue
        row = logits[r, :V].float()
        fin = torch.nonzero(row > float("-inf")).flatten()          # drops -inf and NaN
        x = row[fin].double()
        lse = torch.logsumexp(x, 0) if fin.numel() else torch.zeros((), dtype=torch.float64)
        rec[r, 0:2] = lse.reshape(1).view(torch.int32)
        k = min(nt, fin.numel())
        order = torch.sort(-x, stable=True).indices[:k]
        lp = torch.full((LP_TOP,), float("-inf"), dtype=torch.float32)
        ids = torch.full((LP_TOP,), -1, dtype=torch.int32)
        lp[:k] = (x[order] - lse).float()
        ids[:k] = fin[order].to(torch.int32)
        rec[r, 2:2 + LP_TOP] = lp.view(torch.int32)
        rec[r, 2 + LP_TOP:2 + 2 * LP_TOP] = ids
    return rec


def token_logprobs_pick(logits: torch.Tensor, n: int, n_top: torch.Tensor, next_ids: torch.Tensor, rec: torch.Tensor,
                        V: Optional[int] = None, ctx_len: Optional[torch.Tensor] = None,
                        stash: Optional[torch.Tensor] = None):
    """Second half (AFTER the sampler): the chosen token next_ids[r] and its log-probability -- from the raw logit
    that token_logprobs stashed when the sampler has rewritten it -- into words 0 / 1 of the records."""
    V = logits.shape[1] if V is None else int(V)
    if logits.is_cuda:
        if next_ids.dtype != torch.int32 or next_ids.numel() < n:
            raise TypeError("token_logprobs_pick: int32 ids, one per row")
        S = (stash.shape[1] - 1) // 2 if stash is not None else 0
        _lib.check(_lib.lib().nls_logprobs_pick(logits.data_ptr(), logits.stride(0), n, V, n_top.data_ptr(),
                                                _p(ctx_len), next_ids.data_ptr(), _p(stash), S, rec.data_ptr(),
                                                _stream_ptr(logits)), "nls_logprobs_pick")
        return rec
    for r in range(n):
        if int(n_top[r]) < 0 or (ctx_len is not None and int(ctx_len[r]) <= 0):
            continue
        t = int(next_ids[r])
        lse = rec[r, 0:2].clone().view(torch.float64)[0]
        raw = logits[r, t].double() if 0 <= t < V else torch.tensor(float("-inf"), dtype=torch.float64)
        rec[r, 0] = t
        rec[r, 1:2] = (raw - lse).float().reshape(1).view(torch.int32)
    return rec


def shard_logprobs(logits: torch.Tensor, n: int, n_top: torch.Tensor, next_ids: torch.Tensor, vocab_lo: int,
                   valid: int, part: torch.Tensor, ctx_len: Optional[torch.Tensor] = None):
    """Tensor-parallel logprobs, per rank: rows [0, n) of this rank's vocab shard (columns [0, valid) of `logits`
    hold the ids [vocab_lo, vocab_lo + valid); valid may be 0) -> shard partials part[r] of LP_REC int32 words:
    max (f32 bits; -inf: no finite entry) | sum exp(l - max) (0: none) | the min(n_top[r], finite count) largest RAW
    logits, by (value descending, id ascending), then -inf | their GLOBAL ids, then -1 | the raw logit of next_ids[r]
    if the shard owns it | 1 if it does, else 0. Rows with n_top[r] < 0 (or ctx_len[r] <= 0) are left untouched.
    The partials of every rank, gathered (comm.gather_words), go to merge_logprobs."""
    valid = int(valid)
    if part.dtype != torch.int32 or part.shape[1] != LP_REC or not part.is_contiguous() or part.shape[0] < n:
        raise TypeError("shard_logprobs: contiguous int32 partials of LP_REC words, one per row")
    if valid < 0 or valid > logits.shape[1] or n_top.dtype != torch.int32 or next_ids.dtype != torch.int32:
        raise TypeError("shard_logprobs: int32 n_top / next_ids, valid within the row")
    if logits.is_cuda:
        if logits.dtype != torch.float32 or logits.stride(1) != 1 or next_ids.numel() < n or n_top.numel() < n:
            raise TypeError("shard_logprobs: fp32 row-major logits, one n_top and one id per row")
        _lib.check(_lib.lib().nls_logprobs_shard(logits.data_ptr(), logits.stride(0), n, valid, int(vocab_lo),
                                                 n_top.data_ptr(), _p(ctx_len), next_ids.data_ptr(), part.data_ptr(),
                                                 _stream_ptr(logits)), "nls_logprobs_shard")
        return part
    # CPU twin: fp64 sums, stable sort on (-logit, id); the words are the device's (f32 bits)
    for r in range(n):
        nt = min(int(n_top[r]), LP_TOP)
        if nt < 0 or (ctx_len is not None and int(ctx_len[r]) <= 0):
            continue
        row = logits[r, :valid].float()
        fin = torch.nonzero(row > float("-inf")).flatten()          # drops -inf and NaN
        x = row[fin].double()
        k = min(nt, fin.numel())
        f = torch.full((2 + LP_TOP,), float("-inf"), dtype=torch.float32)
        ids = torch.full((LP_TOP,), -1, dtype=torch.int32)
        f[1] = 0.0
        if fin.numel():
            f[0] = x.max().float()
            f[1] = torch.exp(x - x.max()).sum().float()
            order = torch.sort(-x, stable=True).indices[:k]
            f[2:2 + k] = row[fin[order]]
            ids[:k] = (fin[order] + vocab_lo).to(torch.int32)
        t = int(next_ids[r]) - int(vocab_lo)
        own = 0 <= t < valid
        part[r, :2 + LP_TOP] = f.view(torch.int32)
        part[r, 2 + LP_TOP:2 + 2 * LP_TOP] = ids
        part[r, 2 + 2 * LP_TOP] = int(row[t:t + 1].view(torch.int32)[0]) if own else 0
        part[r, 3 + 2 * LP_TOP] = int(own)
    return part


def merge_logprobs(parts: torch.Tensor, n: int, world: int, n_top: torch.Tensor, next_ids: torch.Tensor,
                   rec: torch.Tensor, ctx_len: Optional[torch.Tensor] = None):
    """The gathered shard partials parts [n, world * LP_REC] (rank p at columns [LP_REC p, LP_REC (p + 1)), world
    <= 8) -> the records rec[r] that token_logprobs + token_logprobs_pick write for the whole row (logprob_records
    reads them): M = max m_p over the shards with z_p > 0, Z = sum z_p exp(m_p - M), an entry is (v - M) - log Z.
    The top n_top[r] are ranked over the gathered candidates by (value descending, global id ascending) -- exact,
    ties at the cut included: the global top-n lies in the union of the shards' top-n under the same order. The
    chosen token next_ids[r] takes the raw logit of the shard that owns it, -inf when none does."""
    world = int(world)
    if (parts.dtype != torch.int32 or parts.dim() != 2 or parts.shape[1] != world * LP_REC or parts.stride(1) != 1
            or parts.stride(0) != world * LP_REC or parts.shape[0] < n or not 1 <= world <= 8):
        raise TypeError("merge_logprobs: contiguous int32 partials [n, world * LP_REC], world <= 8")
    if (rec.dtype != torch.int32 or rec.shape[1] != LP_REC or not rec.is_contiguous() or rec.shape[0] < n
            or n_top.dtype != torch.int32 or next_ids.dtype != torch.int32):
        raise TypeError("merge_logprobs: contiguous int32 records of LP_REC words, int32 n_top / next_ids")
    if parts.is_cuda:
        if next_ids.numel() < n or n_top.numel() < n:
            raise TypeError("merge_logprobs: one n_top and one id per row")
        _lib.check(_lib.lib().nls_logprobs_merge(parts.data_ptr(), n, world, n_top.data_ptr(), _p(ctx_len),
                                                 next_ids.data_ptr(), rec.data_ptr(), _stream_ptr(parts)),
                   "nls_logprobs_merge")
        return rec
    for r in range(n):                         # CPU twin, fp64
        nt = min(int(n_top[r]), LP_TOP)
        if nt < 0 or (ctx_len is not None and int(ctx_len[r]) <= 0):
            continue
        p = parts[r].reshape(world, LP_REC)
        f = p.view(torch.float32).double()
        live = f[:, 1] > 0
        if bool(live.any()):
            M = f[live, 0].max()
            logz = torch.log((f[live, 1] * torch.exp(f[live, 0] - M)).sum())
        else:                                  # no finite entry anywhere: the chosen entry is the raw logit
            M = logz = torch.zeros((), dtype=torch.float64)
        ids = p[:, 2 + LP_TOP:2 + 2 * LP_TOP].reshape(-1)
        vals = f[:, 2:2 + LP_TOP].reshape(-1)
        have = torch.nonzero(ids >= 0).flatten()
        have = have[torch.sort(ids[have], stable=True).indices]     # id ascending, then stable on -value
        order = have[torch.sort(-vals[have], stable=True).indices][:nt]
        k = order.numel()
        lp = torch.full((LP_TOP,), float("-inf"), dtype=torch.float32)
        ti = torch.full((LP_TOP,), -1, dtype=torch.int32)
        lp[:k] = ((vals[order] - M) - logz).float()
        ti[:k] = ids[order]
        own = torch.nonzero(p[:, 3 + 2 * LP_TOP] == 1).flatten()
        raw = f[int(own[0]), 2 + 2 * LP_TOP] if own.numel() else torch.tensor(float("-inf"), dtype=torch.float64)
        rec[r, 0] = int(next_ids[r])
        rec[r, 1:2] = ((raw - M) - logz).float().reshape(1).view(torch.int32)
        rec[r, 2:2 + LP_TOP] = lp.view(torch.int32)
        rec[r, 2 + LP_TOP:2 + 2 * LP_TOP] = ti
    return rec


def logprob_records(words: np.ndarray, rows: Sequence[int], n_tops: Sequence[int]) -> list:
    """Rows `rows` of a host record block [n, LP_REC] (int32, numpy) -> one (token id, logprob, [(id, logprob),
    ...]) each: at most n_tops[j] pairs, the (-1, -inf) padding of a row with fewer finite logits dropped. A decode
    step's rows are converted in one go (per-row numpy calls would cost more than the conversion)."""
    if not len(rows):
        return []
    w = np.ascontiguousarray(words[np.asarray(rows, dtype=np.int64)], dtype=np.int32)
    f = w.view(np.float32)
    cid, clp = w[:, 0].tolist(), f[:, 1].tolist()
    tv, ti = f[:, 2:2 + LP_TOP].tolist(), w[:, 2 + LP_TOP:2 + 2 * LP_TOP].tolist()
    out = []
    for j, n in enumerate(n_tops):
        k = max(0, min(int(n), LP_TOP))
        out.append((cid[j], clp[j], [(i, v) for i, v in zip(ti[j][:k], tv[j][:k]) if i >= 0]))
    return out


def logprob_record(words, n_top: int) -> tuple:
    """logprob_records of one record (LP_REC int32 words)."""
    return logprob_records(np.asarray(words).reshape(1, LP_REC), [0], [n_top])[0]


def moe_norm_route(x: torch.Tensor, nw: torch.Tensor, eps: float, wr: torch.Tensor, h: torch.Tensor,
                   logits: torch.Tensor, T: int, k: int, topw: torch.Tensor, counts: torch.Tensor, xrows: torch.Tensor,
                   yrows: torch.Tensor, cap: int, renorm: bool = True, sel: Optional[torch.Tensor] = None) -> bool:
    """h[:T] = rmsnorm(x[:T]) * nw (f16), router logits h @ wr^T (wr: the router's f16 copy [E, D]) and the
    top-k route, in one launch on the GPU (T <= 4, E in {2, 4, 8}). Returns False, having done nothing,
    when the fused kernel does not take the shape."""
    E = wr.shape[0]
    if x.is_cuda:
        rc = _lib.lib().nls_moe_norm_route(x.data_ptr(), x.stride(0), nw.data_ptr(), float(eps), x.shape[1],
                                           wr.data_ptr(), h.data_ptr(), h.stride(0), logits.data_ptr(), T, E, k,
                                           int(renorm), topw.data_ptr(), counts.data_ptr(), xrows.data_ptr(),
                                           yrows.data_ptr(), cap, _p(sel), _stream_ptr(x))
        if rc == -1:
            return False
        _lib.check(rc, "nls_moe_norm_route")
        return True
    rmsnorm(x, nw, h, T, eps)
    logits[:T] = h[:T].float() @ wr.float().t()
    moe_route(logits, T, k, topw, counts, xrows, yrows, cap, renorm, sel)
    return True


def router_logits(h: torch.Tensor, wr: torch.Tensor, logits: torch.Tensor, T: int,
                  zero: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits[:T] = h[:T] @ wr^T for a MoE router (wr: its f16 copy [E, D], E in {2, 4, 8}): one launch of
    T / 4 workgroups (ops.hip router_logits_kernel) instead of a GEMM tiled for 128-row weight blocks.
    `zero` (int32, optional): zeroed in the same launch (the next moe_route's expert counts)."""
    E, D = wr.shape
    if h.is_cuda:
        if h.dtype != ACT_DTYPE or wr.dtype != ACT_DTYPE or logits.dtype != torch.float32 or logits.shape[1] != E \
                or not wr.is_contiguous() or logits.stride(0) != E or h.stride(1) != 1 or h.shape[1] < D:
            raise ValueError("router_logits: f16 h / wr, f32 contiguous logits [>= T, E]")
        if zero is not None and (zero.dtype != torch.int32 or not zero.is_contiguous()):
            raise ValueError("router_logits: zero must be contiguous int32")
        _lib.check(_lib.lib().nls_router_logits(h.data_ptr(), h.stride(0), wr.data_ptr(), D, E, logits.data_ptr(), T,
                                                _p(zero), 0 if zero is None else zero.numel(), _stream_ptr(h)),
                   "nls_router_logits")
        return logits
    logits[:T] = h[:T, :D].float() @ wr.float().t()
    if zero is not None:
        zero.zero_()
    return logits


def moe_route(logits: torch.Tensor, T: int, k: int, topw: torch.Tensor, counts: torch.Tensor, xrows: torch.Tensor,
              yrows: torch.Tensor, cap: int, renorm: bool = True, sel: Optional[torch.Tensor] = None,
              counts_zeroed: bool = False):
    """Top-k routing: per-expert row lists (counts / xrows / yrows) and weights topw; `sel` (optional,
    int32 [>= T*k]) receives each (token, slot)'s expert id for device-selected expert launches.
    counts_zeroed: an earlier launch on the stream already zeroed `counts` (router_logits(zero=counts))."""
    E = logits.shape[1]
    if logits.is_cuda:
        if E > 128 or k > 8:     # (before the memset below: a refused route touches no buffer)
            raise RuntimeError(f"nls_moe_route failed with code -1 (E={E} > 128 or k={k} > 8)")
        if T > 4 and not counts_zeroed:   # one-workgroup launches (T <= 4) zero the counts in-kernel
            counts.zero_()
        _lib.check(_lib.lib().nls_moe_route(logits.data_ptr(), T, E, k, int(renorm), topw.data_ptr(),
                                            counts.data_ptr(), xrows.data_ptr(), yrows.data_ptr(), cap, _p(sel),
                                            _stream_ptr(logits)), "nls_moe_route")
        return
    # the kernels' contract (moe_route.h): the maximum ignores NaNs, a NaN probability never wins, ties and NaNs
    # go to the lowest unused expert -- a stable sort on (-p, index) with NaNs last (torch.topk promises no tie order)
    l = logits[:T].float()
    mx = torch.where(torch.isnan(l), torch.full_like(l, float("-inf")), l).max(dim=-1, keepdim=True).values
    p = torch.exp(l - mx)
    key = torch.where(torch.isnan(p), torch.full_like(p, float("inf")), -p)
    e = torch.sort(key, dim=-1, stable=True).indices[:, :k]
    w = torch.gather(p, 1, e) / p.sum(dim=-1, keepdim=True)
    if renorm:
        w = w / w.sum(dim=-1, keepdim=True)
    topw[:T * k] = w.reshape(-1)
    counts.zero_()
    lists = {}
    for t, row in enumerate(e.tolist()):
        for j, ex in enumerate(row):
            lists.setdefault(ex, []).append((t, t * k + j))
    for ex, pr in lists.items():
        xrows[ex * cap:ex * cap + len(pr)] = torch.tensor([a for a, _ in pr], dtype=xrows.dtype)
        yrows[ex * cap:ex * cap + len(pr)] = torch.tensor([b for _, b in pr], dtype=yrows.dtype)
        counts[ex] = len(pr)
    if sel is not None:
        sel[:T * k] = e.reshape(-1).to(sel.dtype)


def moe_combine_norm(y: torch.Tensor, topw: torch.Tensor, T: int, k: int, resid: torch.Tensor, alpha: float,
                     norm_w: torch.Tensor, eps: float, h: torch.Tensor):
    """moe_combine, then h[:T] = rmsnorm(resid[:T]) * norm_w (the next layer's input norm) in the same launch."""
    if y.is_cuda:
        D = resid.shape[1]
        _lib.check(_lib.lib().nls_moe_combine_norm(y.data_ptr(), topw.data_ptr(), T, k, resid.data_ptr(),
                                                   resid.stride(0), D, float(alpha), norm_w.data_ptr(), float(eps),
                                                   h.data_ptr(), h.stride(0), _stream_ptr(y)), "nls_moe_combine_norm")
        return h
    moe_combine(y, topw, T, k, resid, alpha)
    return rmsnorm(resid, norm_w, h, T, eps)


def moe_combine(y: torch.Tensor, topw: torch.Tensor, T: int, k: int, resid: torch.Tensor, alpha: float = 1.0,
                set_: bool = False):
    """resid[:T] += alpha * sum_j topw[t, j] * y[t*k + j]; set_: resid[:T] = ... (a partial combine from zero)."""
    D = resid.shape[1]
    if y.is_cuda:
        _lib.check(_lib.lib().nls_moe_combine(y.data_ptr(), topw.data_ptr(), T, k, resid.data_ptr(),
                                              resid.stride(0), D, float(alpha), int(set_), _stream_ptr(y)),
                   "nls_moe_combine")
        return
    yy = y[:T * k].float().view(T, k, D)
    c = alpha * (topw[:T * k].view(T, k, 1) * yy).sum(dim=1)
    if set_:
        resid[:T] = c
    else:
        resid[:T] += c
