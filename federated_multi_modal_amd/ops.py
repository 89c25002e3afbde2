"""Thin torch-tensor wrappers over the C ABI (include/mapfed.h).

torch supplies device memory and the current HIP stream; every compute call goes through
libmapfed.so.  Wrappers allocate outputs only when the caller passes none (the engine always
passes preallocated buffers so a whole step can be captured in a hipGraph).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

from ._lib import call

EPI_NONE, EPI_BIAS, EPI_BIAS_RESID, EPI_BIAS_GELU, EPI_DGELU, EPI_F32, EPI_RESID = range(7)


class KernelProbe:
    """Brackets every launch of the probed kernel families with HIP events on the launching stream
    (used by bench.py for the per-launch rooflines; off by default, never active during graph
    capture).  kinds: "gemm", "attention" (or one name / an iterable); each record carries a key
    ("gemm", "attention_fwd/L199", ...) so the families and towers are summarised separately."""

    def __init__(self, kinds="gemm"):
        self.kinds = {kinds} if isinstance(kinds, str) else set(kinds)
        self.kind = next(iter(self.kinds)) if len(self.kinds) == 1 else None  # single-family callers
        self.records = []  # (key, start_event, end_event, flops, bytes, meta)

    def wants(self, kind: str) -> bool:
        return kind in self.kinds

    def around(self, flops: float, nbytes: float, key: str = "gemm", meta=None):
        """meta: what the launch was (the GEMMs: (M, N, K, epilogue)), for per-shape tables."""
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        self.records.append((key, s, e, flops, nbytes, meta))
        return e

    def launches(self):
        """Per-launch records in launch order: key, duration (us), flops, algorithmic bytes, meta."""
        torch.cuda.synchronize()
        return [{"key": k, "us": 1e3 * s.elapsed_time(e), "flops": f, "bytes": b, "meta": m}
                for k, s, e, f, b, m in self.records]

    def keys(self):
        return sorted({r[0] for r in self.records})

    def summary(self, prefix: Optional[str] = None):
        torch.cuda.synchronize()
        recs = [r for r in self.records if prefix is None or r[0].startswith(prefix)]
        ms = [r[1].elapsed_time(r[2]) for r in recs]
        n = len(ms)
        tot_ms = sum(ms)
        flops = sum(r[3] for r in recs)
        nbytes = sum(r[4] for r in recs)
        return {"launches": n, "avg_us": 1e3 * tot_ms / max(n, 1), "flops_per_launch": flops / max(n, 1),
                "bytes_per_launch": nbytes / max(n, 1), "tflops": flops / (tot_ms * 1e-3) / 1e12 if n else 0.0,
                "gbs": nbytes / (tot_ms * 1e-3) / 1e9 if n else 0.0}


_PROBE: Optional[KernelProbe] = None
_TAG = ""  # the tower a probed GEMM belongs to ("vision" / "text"), set by the engine around each tower


def set_probe(probe: Optional[KernelProbe]):
    global _PROBE
    _PROBE = probe


class probe_tag:
    """with ops.probe_tag("text"): GEMM probe records are keyed "gemm/text"."""

    def __init__(self, tag: str):
        self.tag = tag

    def __enter__(self):
        global _TAG
        self.prev, _TAG = _TAG, self.tag

    def __exit__(self, *a):
        global _TAG
        _TAG = self.prev


def _gkey():
    return f"gemm/{_TAG}" if _TAG else "gemm"


def _p(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D view required"
    return t.stride(0)


def _gemm_bytes(M, N, K, C, aux=None, a_bytes=2, b_bytes=2) -> float:
    """Algorithmic bytes of one GEMM launch: A and B read once, C written once (at its element size), and
    the epilogue's aux operand (residual read, pre-activation written or read: M x N fp16) once."""
    return a_bytes * M * K + b_bytes * N * K + C.element_size() * M * N + (2.0 * M * N if aux is not None else 0.0)


def _hbm(key: str, nbytes: float):
    """HIP-event probe around a streaming (HBM-bound) kernel: algorithmic bytes per launch."""
    if _PROBE is not None and _PROBE.wants("hbm"):
        return _PROBE.around(0.0, nbytes, key)
    return None


def _rec(ev):
    if ev is not None:
        ev.record()


def gemm_nt(A, B, C=None, bias=None, aux_in=None, aux_out=None, epilogue=EPI_NONE, tile=0):
    """C[M,N] = epi(A[M,K] . B[N,K]^T)."""
    M, K = A.shape
    N, K2 = B.shape
    assert K == K2, (A.shape, B.shape)
    if C is None:
        C = torch.empty(M, N, device=A.device, dtype=torch.float32 if epilogue == EPI_F32 else torch.float16)
    aux = aux_in if aux_in is not None else aux_out
    ld_aux = _ld(aux) if aux is not None else 0
    ev = None
    if _PROBE is not None and _PROBE.wants("gemm"):
        ev = _PROBE.around(2.0 * M * N * K, _gemm_bytes(M, N, K, C, aux), _gkey(), (M, N, K, epilogue))
    call("mf_gemm_nt", _p(A), _ld(A), _p(B), _ld(B), _p(C), _ld(C), M, N, K, _p(bias), _p(aux_in), _p(aux_out),
         ld_aux, epilogue, tile, _s())
    if ev is not None:
        ev.record()
    return C


def gemm(A, B, C=None, bias=None, aux_in=None, aux_out=None, epilogue=EPI_NONE, tile=0, a_kmajor=False,
         b_kmajor=False):
    """C[M,N] = epi(op(A) . op(B)^T): A is [M,K] (or [K,M] when a_kmajor), B is [N,K] (or [K,N]
    when b_kmajor) -- the K-major forms read dY^T / X / W of the backward products in place."""
    M, Ka = (A.shape[1], A.shape[0]) if a_kmajor else A.shape
    N, Kb = (B.shape[1], B.shape[0]) if b_kmajor else B.shape
    assert Ka == Kb, (A.shape, a_kmajor, B.shape, b_kmajor)
    K = Ka
    if C is None:
        C = torch.empty(M, N, device=A.device, dtype=torch.float32 if epilogue == EPI_F32 else torch.float16)
    aux = aux_in if aux_in is not None else aux_out
    ld_aux = _ld(aux) if aux is not None else 0
    ev = None
    if _PROBE is not None and _PROBE.wants("gemm"):
        ev = _PROBE.around(2.0 * M * N * K, _gemm_bytes(M, N, K, C, aux), _gkey(), (M, N, K, epilogue))
    call("mf_gemm", _p(A), _ld(A), int(a_kmajor), _p(B), _ld(B), int(b_kmajor), _p(C), _ld(C), M, N, K, _p(bias),
         _p(aux_in), _p(aux_out), ld_aux, epilogue, tile, _s())
    if ev is not None:
        ev.record()
    return C



def gemm_splitk_ws_floats(M: int, N: int, K: int, splits: int = 0) -> int:
    n = call("mf_gemm_splitk_ws_floats", M, N, K, splits)
    if n < 0:
        raise ValueError("split-K workspace exceeds 2^31 floats")
    return n


def gemm_splitk(A, B, C, ws, splits=0, a_kmajor=False, b_kmajor=False, live=None, m_live=None):
    """C[M,N] = op(A) . op(B)^T with K split over workgroups and an fp32 workspace (mf_gemm_splitk):
    for the weight gradients, few output tiles and K = tokens.  C fp16 or fp32.
    live = (L_live, L_full): the caller's promise that A's k-rows with k % L_full >= L_live are exact zeros in the
    output rows m < m_live (default: all M); their K-tiles are skipped, the result is bit for bit the plain one
    (mf_gemm_splitk_live, both operands K-major).  The probe prices it as the full product."""
    M, Ka = (A.shape[1], A.shape[0]) if a_kmajor else A.shape
    N, Kb = (B.shape[1], B.shape[0]) if b_kmajor else B.shape
    assert Ka == Kb, (A.shape, a_kmajor, B.shape, b_kmajor)
    K = Ka
    assert ws.dtype == torch.float32 and C.dtype in (torch.float16, torch.float32)
    ev = None
    if _PROBE is not None and _PROBE.wants("gemm"):
        ev = _PROBE.around(2.0 * M * N * K, _gemm_bytes(M, N, K, C), _gkey(), (M, N, K, "splitk"))
    if live is not None:
        call("mf_gemm_splitk_live", _p(A), _ld(A), int(a_kmajor), _p(B), _ld(B), int(b_kmajor), _p(C), _ld(C), M, N,
             K, _p(ws), ws.numel(), splits, int(C.dtype == torch.float16), live[0], live[1],
             M if m_live is None else m_live, _s())
    else:
        call("mf_gemm_splitk", _p(A), _ld(A), int(a_kmajor), _p(B), _ld(B), int(b_kmajor), _p(C), _ld(C), M, N, K,
             _p(ws), ws.numel(), splits, int(C.dtype == torch.float16), _s())
    if ev is not None:
        ev.record()
    return C


def layernorm_fwd(x, gamma, beta, y=None, mean=None, rstd=None, row_index=None):
    rows = row_index.numel() if row_index is not None else x.shape[0]
    D = x.shape[1]
    if y is None:
        y = torch.empty(rows, D, device=x.device, dtype=torch.float16)
    if mean is None:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    if rstd is None:
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    # x read, y written (fp16), mean / rstd written (fp32)
    ev = _hbm(f"layernorm_fwd/D{D}", rows * D * 4.0 + rows * 8.0)
    call("mf_layernorm_fwd", _p(x), _ld(x), _p(row_index), _p(gamma), _p(beta), _p(y), _ld(y), _p(mean), _p(rstd),
         rows, D, _s())
    _rec(ev)
    return y, mean, rstd




def layernorm_fwd_inject(x, gamma, beta, y, mean, rstd, prompt, L, row0, nrows):
    """prompt_inject_fwd(x, prompt, ...) + layernorm_fwd(x, ...) in one kernel (bit-identical)."""
    rows, D = x.shape
    ev = _hbm(f"layernorm_fwd/D{D}", rows * D * 4.0 + rows * 8.0)
    call("mf_layernorm_fwd_inject", _p(x), _ld(x), _p(gamma), _p(beta), _p(y), _ld(y), _p(mean), _p(rstd), rows, D,
         _p(prompt), L, row0, nrows, _s())
    _rec(ev)
    return y, mean, rstd


def layernorm_ws_floats(rows: int, D: int) -> int:
    return 2 * call("mf_layernorm_bwd_blocks", rows) * D


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, workspace=None, dres=None, row_index=None,
                  accumulate=False):
    rows, D = dy.shape
    if workspace is None:
        workspace = torch.empty(layernorm_ws_floats(rows, D), device=dy.device, dtype=torch.float32)
    call("mf_layernorm_bwd", _p(dy), _ld(dy), _p(x), _ld(x), _p(row_index), _p(gamma), _p(mean), _p(rstd), _p(dres),
         _ld(dres) if dres is not None else 0, _p(dx), _ld(dx), _p(dgamma), _p(dbeta), _p(workspace), rows, D,
         int(accumulate), _s())
    return dx


class LNGradBatch:
    """Deferred dgamma/dbeta reductions of every LayerNorm backward of a pass: each LN param pair gets
    its own partial-sum workspace, and one mf_col_reduce_batch launch at the end of the backward
    reduces them all (instead of one reduction launch per LayerNorm).  The trainable block's bias gradients
    (colsum()) ride in the same launch."""

    def __init__(self, device):
        self.device = device
        self.ws = {}          # dgamma data_ptr -> workspace
        self.descs = []       # (part_ptr, out_ptr, nblk, C[, out_f16])
        self.keys = []
        self.dev_descs = None
        self.max_cols = 0

    def bwd(self, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dres=None, row_index=None, live=None):
        """live = (L_live, L_full): dy / x / dx are the first L_live rows of each L_full-row sequence of a tower
        whose other rows have zero gradient (mf_layernorm_bwd_live: the full tower's partials)."""
        if live is not None:
            return self._bwd_live(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dres, live, None, 0, 0)
        rows, D = dy.shape
        key = dgamma.data_ptr()
        if key not in self.ws:
            nblk = call("mf_layernorm_bwd_blocks", rows)
            w = torch.empty(2 * nblk * D, device=self.device, dtype=torch.float32)
            self.ws[key] = w
            self.descs.append((w.data_ptr(), dgamma.data_ptr(), nblk, D))
            self.descs.append((w.data_ptr() + 4 * nblk * D, dbeta.data_ptr(), nblk, D))
            self.max_cols = max(self.max_cols, D)
            self.dev_descs = None
        # dy, x (and the residual gradient) read, dx written (fp16); mean / rstd read; dgamma / dbeta partials
        ev = _hbm(f"layernorm_bwd/D{D}", rows * D * (6.0 + (2.0 if dres is not None else 0.0)) + rows * 8.0
                  + self.ws[key].numel() * 4.0)
        call("mf_layernorm_bwd", _p(dy), _ld(dy), _p(x), _ld(x), _p(row_index), _p(gamma), _p(mean), _p(rstd),
             _p(dres), _ld(dres) if dres is not None else 0, _p(dx), _ld(dx), None, None, _p(self.ws[key]), rows, D,
             0, _s())
        _rec(ev)
        return dx

    def _ws_for(self, dgamma, dbeta, rows, D):
        key = dgamma.data_ptr()
        if key not in self.ws:
            nblk = call("mf_layernorm_bwd_blocks", rows)
            w = torch.empty(2 * nblk * D, device=self.device, dtype=torch.float32)
            self.ws[key] = w
            self.descs.append((w.data_ptr(), dgamma.data_ptr(), nblk, D))
            self.descs.append((w.data_ptr() + 4 * nblk * D, dbeta.data_ptr(), nblk, D))
            self.max_cols = max(self.max_cols, D)
            self.dev_descs = None
        return self.ws[key]

    def _inj_ws_for(self, prompt_grad, n, nrows, D):
        ikey = ("inj", prompt_grad.data_ptr())
        if ikey not in self.ws:
            part = torch.empty(n * nrows * D, device=self.device, dtype=torch.float32)
            self.ws[ikey] = part
            self.descs.append((part.data_ptr(), prompt_grad.data_ptr(), n, nrows * D))
            self.max_cols = max(self.max_cols, nrows * D)
            self.dev_descs = None
        return self.ws[ikey]

    def _bwd_live(self, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dres, live, prompt_grad, row0, nrows):
        L_live, L_full = live
        rows, D = dy.shape
        assert rows % L_live == 0 and L_live <= L_full
        seqs = rows // L_live
        ws = self._ws_for(dgamma, dbeta, seqs * L_full, D)
        inj = None
        if prompt_grad is not None:
            assert prompt_grad.dtype == torch.float32 and prompt_grad.is_contiguous()
            inj = self._inj_ws_for(prompt_grad, seqs, nrows, D)
        ev = _hbm(f"layernorm_bwd/D{D}", rows * D * (6.0 + (2.0 if dres is not None else 0.0)) + rows * 8.0
                  + (ws.numel() + (inj.numel() if inj is not None else 0)) * 4.0)
        call("mf_layernorm_bwd_live", _p(dy), _ld(dy), _p(x), _ld(x), _p(gamma), _p(mean), _p(rstd), _p(dres),
             _ld(dres) if dres is not None else 0, _p(dx), _ld(dx), _p(ws), seqs, L_live, L_full, D, _p(inj), row0,
             nrows, _s())
        _rec(ev)
        return dx

    def bwd_inject(self, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dres, prompt_grad, L, row0, nrows, live=None):
        """bwd() with the deep-prompt injection backward of the same rows fused in
        (mf_layernorm_bwd_inject): prompt_grad (fp32 [nrows, D]) = sum over sequences of those rows' dx,
        reduced in finish() with the LayerNorm partials; the rows of dx are zeroed.  live: see bwd() (then
        L must be its L_live)."""
        if live is not None:
            assert L == live[0]
            return self._bwd_live(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dres, live, prompt_grad, row0, nrows)
        rows, D = dy.shape
        assert prompt_grad.dtype == torch.float32 and prompt_grad.is_contiguous() and prompt_grad.numel() == nrows * D
        key = dgamma.data_ptr()
        if key not in self.ws:
            nblk = call("mf_layernorm_bwd_blocks", rows)
            w = torch.empty(2 * nblk * D, device=self.device, dtype=torch.float32)
            self.ws[key] = w
            self.descs.append((w.data_ptr(), dgamma.data_ptr(), nblk, D))
            self.descs.append((w.data_ptr() + 4 * nblk * D, dbeta.data_ptr(), nblk, D))
            self.max_cols = max(self.max_cols, D)
            self.dev_descs = None
        ikey = ("inj", prompt_grad.data_ptr())
        if ikey not in self.ws:
            n = rows // L
            part = torch.empty(n * nrows * D, device=self.device, dtype=torch.float32)
            self.ws[ikey] = part
            self.descs.append((part.data_ptr(), prompt_grad.data_ptr(), n, nrows * D))
            self.max_cols = max(self.max_cols, nrows * D)
            self.dev_descs = None
        ev = _hbm(f"layernorm_bwd/D{D}", rows * D * (6.0 + (2.0 if dres is not None else 0.0)) + rows * 8.0
                  + (self.ws[key].numel() + self.ws[ikey].numel()) * 4.0)
        call("mf_layernorm_bwd_inject", _p(dy), _ld(dy), _p(x), _ld(x), _p(gamma), _p(mean), _p(rstd), _p(dres),
             _ld(dres) if dres is not None else 0, _p(dx), _ld(dx), _p(self.ws[key]), rows, D, _p(self.ws[ikey]), L,
             row0, nrows, _s())
        _rec(ev)
        return dx

    def colsum(self, dy, db, live=None):
        """db = colsum(dy) (a Linear's bias gradient, fp16 or fp32) with the reduction deferred to finish(): the
        partials go to this db's own workspace, and the batch kernel sums them in mf_colsum_f16's order (bit for
        bit its result).  live: see ops.colsum."""
        R, C = dy.shape
        key = ("db", db.data_ptr())
        nblk = call("mf_colsum_blocks", R)
        if key not in self.ws:
            part = torch.empty(nblk * C, device=self.device, dtype=torch.float32)
            self.ws[key] = part
            self.descs.append((part.data_ptr(), db.data_ptr(), nblk, C, int(db.dtype == torch.float16)))
            self.max_cols = max(self.max_cols, C)
            self.dev_descs = None
        assert self.ws[key].numel() == nblk * C and db.numel() == C
        colsum(dy, None, self.ws[key], live=live)

    def finish(self):
        if not self.descs:
            return
        if self.dev_descs is None:
            import numpy as np
            assert call("mf_col_reduce_desc_bytes") == 32
            arr = np.zeros(len(self.descs), dtype=np.dtype([("part", np.uint64), ("out", np.uint64),
                                                            ("nblk", np.int32), ("C", np.int32),
                                                            ("acc", np.int32), ("out_f16", np.int32)]))
            for i, (pp, op, nb, c, *f16) in enumerate(self.descs):
                arr[i] = (pp, op, nb, c, 0, f16[0] if f16 else 0)
            self.dev_descs = torch.from_numpy(arr.view(np.uint8)).to(self.device)
        call("mf_col_reduce_batch", _p(self.dev_descs), len(self.descs), self.max_cols, _s())


def attention_fwd(qkv, N, L, H, causal, out=None, lse=None, ld_lse=None):
    D = H * 64
    if out is None:
        out = torch.empty(N * L, D, device=qkv.device, dtype=torch.float16)
    if ld_lse is None:
        ld_lse = L
    if lse is None:
        lse = torch.empty(N * H * ld_lse, device=qkv.device, dtype=torch.float32)
    ev = None
    if _PROBE is not None and _PROBE.wants("attention"):
        # algorithmic: QK^T + PV = 4 * pairs * 64 flop per (sequence, head), pairs = L^2 (L(L+1)/2 under
        # the causal mask); bytes: Q, K, V read + O written (fp16) + the LSE (fp32)
        pairs = L * (L + 1) / 2 if causal else L * L
        ev = _PROBE.around(4.0 * N * H * pairs * 64, N * H * L * (2.0 * 4 * 64 + 4), f"attention_fwd/L{L}")
    call("mf_attention_fwd", _p(qkv), _ld(qkv), _p(out), _ld(out), _p(lse), ld_lse, N, L, H, int(causal), _s())
    if ev is not None:
        ev.record()
    return out, lse


def attention_fwd_rows(qkv, N, L, H, causal, q_rows, out, lse, ld_lse=None):
    """attention_fwd for query rows 0 .. q_rows-1 of every head only (their 16-row tiles are computed and stored;
    each row bit-identical to attention_fwd's): out / lse rows of the other queries are left untouched."""
    if ld_lse is None:
        ld_lse = L
    ev = None
    if _PROBE is not None and _PROBE.wants("attention"):
        rows = min(L, (q_rows + 15) // 16 * 16)
        ev = _PROBE.around(4.0 * N * H * rows * L * 64, N * H * (2.0 * 2 * 64 * L + 2.0 * 2 * 64 * rows),
                           f"attention_fwd_rows/L{L}")
    call("mf_attention_fwd_rows", _p(qkv), _ld(qkv), _p(out), _ld(out), _p(lse), ld_lse, N, L, H, int(causal), q_rows,
         _s())
    if ev is not None:
        ev.record()
    return out, lse


def qkv_attention_supported(N, L, H, causal) -> bool:
    return bool(call("mf_qkv_attention_supported", N, L, H, int(causal)))


def qkv_attention_fwd(x, w, bias, qkv, out, lse, N, L, H, causal, ld_lse=None):
    """The in-projection (qkv = x w^T + bias, fp16) and the attention forward in one launch
    (mf_qkv_attention_fwd): qkv [N*L, 3D] is written too (the backward reads it)."""
    D = H * 64
    if ld_lse is None:
        ld_lse = L
    assert x.shape[1] == D and tuple(w.shape) == (3 * D, D) and bias.numel() == 3 * D
    ev = None
    if _PROBE is not None and _PROBE.wants("attention"):
        # algorithmic: the in-projection 2 * (N*L) * 3D * D plus QK^T + PV; bytes: x and W read, qkv, O (fp16)
        # and the LSE written -- the round trip of qkv between two launches is gone
        pairs = L * (L + 1) / 2 if causal else L * L
        flops = 2.0 * N * L * 3 * D * D + 4.0 * N * H * pairs * 64
        nbytes = 2.0 * N * L * D + 2.0 * 3 * D * D + 2.0 * N * L * 3 * D + 2.0 * N * L * D + 4.0 * N * H * L
        ev = _PROBE.around(flops, nbytes, f"attention_fused_fwd/L{L}")
    call("mf_qkv_attention_fwd", _p(x), _ld(x), x.shape[0], _p(w), _p(bias), _p(qkv), _ld(qkv), _p(out), _ld(out),
         _p(lse), ld_lse, N, L, H, int(causal), _s())
    if ev is not None:
        ev.record()
    return out, lse


def attention_bwd(qkv, out, dout, lse, N, L, H, causal, dqkv=None, ws=None, ld_lse=None):
    if ld_lse is None:
        ld_lse = L
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    if ws is None:
        ws = torch.empty(N * H * ld_lse, device=qkv.device, dtype=torch.float32)
    ev = None
    if _PROBE is not None and _PROBE.wants("attention"):
        # algorithmic: dV = P^T dO, dP = dO V^T, dK = dS^T Q, dQ = dS K: 8 * pairs * 64 flop (the
        # recompute of S is not counted); bytes: Q, K, V, O, dO + LSE read, dQ, dK, dV written
        pairs = L * (L + 1) / 2 if causal else L * L
        ev = _PROBE.around(8.0 * N * H * pairs * 64, N * H * L * (2.0 * 8 * 64 + 4), f"attention_bwd/L{L}")
    call("mf_attention_bwd", _p(qkv), _ld(qkv), _p(out), _ld(out), _p(dout), _ld(dout), _p(lse), _p(ws), ld_lse,
         _p(dqkv), _ld(dqkv), N, L, H, int(causal), _s())
    if ev is not None:
        ev.record()
    return dqkv


def attention_bwd_rows(qkv, out, dout, lse, N, L, H, causal, q_rows, dqkv=None, ld_lse=None):
    """attention_bwd for a dout that is zero at query rows >= q_rows of every sequence: those rows of dout, out and
    lse are not read (they may hold stale data), dqkv is written in full, bit for bit attention_bwd's for that dout.
    Non-causal, L <= 224."""
    if ld_lse is None:
        ld_lse = L
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    ev = None
    if _PROBE is not None and _PROBE.wants("attention"):
        # the 32-query blocks below q_rows against every key (8 * 64 flop a pair); bytes: Q, dO, O of those blocks,
        # K, V read, dQ, dK, dV written
        rows = min(L, (q_rows + 31) // 32 * 32)
        ev = _PROBE.around(8.0 * N * H * rows * L * 64, N * H * (2.0 * 5 * 64 * L + 2.0 * 3 * 64 * rows),
                           f"attention_bwd_rows/L{L}")
    call("mf_attention_bwd_rows", _p(qkv), _ld(qkv), _p(out), _ld(out), _p(dout), _ld(dout), _p(lse), ld_lse,
         _p(dqkv), _ld(dqkv), N, L, H, int(causal), q_rows, _s())
    if ev is not None:
        ev.record()
    return dqkv


def im2col_patch(img, out, patch=16):
    B, C, R, R2 = img.shape
    assert C == 3 and R == R2 and img.is_contiguous()
    call("mf_im2col_patch", _p(img), int(img.dtype == torch.float32), _p(out), B, R, patch, _s())
    return out


def vision_assemble(patch, cls, pos, shared_ctx, x, B, G2, n_ctx, D):
    call("mf_vision_assemble", _p(patch), _p(cls), _p(pos), _p(shared_ctx), _p(x), B, G2, n_ctx, D, _s())
    return x


def text_assemble(prefix, ctx, suffix, pos, x, K, L, n_ctx, D):
    call("mf_text_assemble", _p(prefix), _p(ctx), _p(suffix), _p(pos), _p(x), K, L, n_ctx, D, _s())
    return x


def prompt_inject_fwd(x, prompt, N, L, row0, nrows, D):
    call("mf_prompt_inject_fwd", _p(x), _p(prompt), N, L, row0, nrows, D, _s())


def prompt_inject_bwd(dx, N, L, row0, nrows, D, out, accumulate=False, zero_rows=True):
    call("mf_prompt_inject_bwd", _p(dx), N, L, row0, nrows, D, _p(out), int(out.dtype == torch.float16),
         int(accumulate), int(zero_rows), _s())


def seq_grow(src, dst, cap, prompt, N, Lp, ncap, n_ctx, D):
    """dst [N*(Lp+ncap), D] = per sequence: src rows [0, Lp-n_ctx) | cap [ncap, D] | fp16(prompt [n_ctx, D])."""
    assert src.shape[0] == N * Lp and dst.shape[0] == N * (Lp + ncap) and prompt.dtype == torch.float32
    call("mf_seq_grow", _p(src), _p(dst), _p(cap), _p(prompt), N, Lp, ncap, n_ctx, D, _s())


def seq_scatter(src, dst, N, L_live, L_full):
    """dst rows n*L_full + t = src rows n*L_live + t (t < L_live), src's columns; dst's other rows untouched."""
    C = src.shape[1]
    assert src.shape[0] == N * L_live and dst.shape[0] >= N * L_full and dst.shape[1] >= C
    ev = _hbm("seq_scatter", 4.0 * N * L_live * C)
    call("mf_seq_scatter", _p(src), _ld(src), _p(dst), _ld(dst), N, L_live, L_full, C, _s())
    _rec(ev)
    return dst


def seq_grow_bwd(ddst, dsrc, N, Lp, ncap, n_ctx, D):
    assert ddst.shape[0] == N * (Lp + ncap) and dsrc.shape[0] == N * Lp
    call("mf_seq_grow_bwd", _p(ddst), _p(dsrc), N, Lp, ncap, n_ctx, D, _s())


def caption_pool(tokens, table, w, pooled):
    """tokens int32 [B, T] on the device, table fp32 [vocab, D], w fp16 [D] -> pooled fp16 [B, D]."""
    B, T = tokens.shape
    assert tokens.dtype == torch.int32 and table.dtype == torch.float32 and w.dtype == torch.float16
    call("mf_caption_pool", _p(tokens), B, T, _p(table), table.shape[0], _p(w), table.shape[1], _p(pooled), _s())
    return pooled


def transpose(inp, out):
    R, C = inp.shape
    call("mf_transpose_f16", _p(inp), _ld(inp), _p(out), _ld(out), R, C, _s())
    return out


def colsum_ws_floats(R: int, C: int) -> int:
    return call("mf_colsum_blocks", R) * C


def colsum(inp, out, workspace=None, live=None):
    """out[c] = sum_r inp[r, c].  out None: only the partials are written to workspace [colsum blocks of R][C] (reduced
    later: LNGradBatch.colsum).  live = (L_live, L_full): the caller's promise that rows r with r % L_full >= L_live
    are exact zeros (mf_colsum_f16_live, bit for bit the plain result)."""
    R, C = inp.shape
    if workspace is None:
        workspace = torch.empty(colsum_ws_floats(R, C), device=inp.device, dtype=torch.float32)
    f16 = int(out is not None and out.dtype == torch.float16)
    if live is not None:
        call("mf_colsum_f16_live", _p(inp), _ld(inp), R, C, _p(out), f16, _p(workspace), live[0], live[1], _s())
    else:
        call("mf_colsum_f16", _p(inp), _ld(inp), R, C, _p(out), f16, _p(workspace), _s())
    return out


def small_linear_fwd(X, W, b, Y):
    M, I = X.shape
    O = W.shape[0]
    call("mf_small_linear_fwd", _p(X), _p(W), _p(b), _p(Y), M, I, O, int(X.dtype == torch.float16), _s())
    return Y


class SmallLinearBatch:
    """A fixed set of small Linears (the prompt learner's) run as one launch per direction.  Each entry:
    X [M,I], W [O,I], b [O] or None, Y [M,O]; backward: dY [M,O], dX (accumulated when acc_dx), dW, db.
    The descriptor table is built once (static pointers, hipGraph-capturable)."""

    def __init__(self, device, entries):
        import numpy as np
        assert call("mf_small_linear_desc_bytes") == 88
        dt = np.dtype([("X", np.uint64), ("W", np.uint64), ("b", np.uint64), ("Y", np.uint64), ("dY", np.uint64),
                       ("dX", np.uint64), ("dW", np.uint64), ("db", np.uint64), ("M", np.int32), ("I", np.int32),
                       ("O", np.int32), ("is16", np.int32), ("acc", np.int32), ("pad", np.int32)])
        arr = np.zeros(len(entries), dtype=dt)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        self.max_mo = self.max_m = self.max_i = self.max_oi = 0
        for k, e in enumerate(entries):
            M, I = e["X"].shape
            O = e["W"].shape[0]
            arr[k] = (ptr(e["X"]), ptr(e["W"]), ptr(e.get("b")), ptr(e["Y"]), ptr(e.get("dY")), ptr(e.get("dX")),
                      ptr(e.get("dW")), ptr(e.get("db")), M, I, O, int(e["X"].dtype == torch.float16),
                      int(e.get("acc_dx", False)), 0)
            self.max_mo, self.max_m = max(self.max_mo, M * O), max(self.max_m, M)
            self.max_i, self.max_oi = max(self.max_i, I), max(self.max_oi, O * I)
        self.n = len(entries)
        self.descs = torch.from_numpy(arr.view(np.uint8)).to(device)

    def fwd(self):
        call("mf_small_linear_fwd_batch", _p(self.descs), self.n, self.max_mo, _s())

    def bwd(self):
        call("mf_small_linear_bwd_batch", _p(self.descs), self.n, self.max_m, self.max_i, self.max_oi, _s())


def small_linear_bwd(dY, X, W, dX=None, dW=None, db=None, accumulate_dx=False):
    M, I = X.shape
    O = W.shape[0]
    call("mf_small_linear_bwd", _p(dY), _p(X), _p(W), _p(dX), _p(dW), _p(db), M, I, O,
         int(X.dtype == torch.float16), int(accumulate_dx), _s())


def clip_head_fwd(img, txt, logit_scale, img_n, txt_n, norms, mm, logits):
    B, D = img.shape
    K = txt.shape[0]
    call("mf_clip_head_fwd", _p(img), _p(txt), B, K, D, _p(logit_scale), _p(img_n), _p(txt_n), _p(norms), _p(mm),
         _p(logits), _s())


def clip_loss_fwd_bwd(img, txt, img_n, txt_n, norms, logits, label, logit_scale, dmm, cos_ws, loss_out, dimg_n,
                      dtxt_n, dimg, dtxt):
    B, D = img.shape
    K = txt.shape[0]
    call("mf_clip_loss_fwd_bwd", _p(img), _p(txt), _p(img_n), _p(txt_n), _p(norms), _p(logits), _p(label), B, K, D,
         _p(logit_scale), _p(dmm), _p(cos_ws), _p(loss_out), _p(dimg_n), _p(dtxt_n), _p(dimg), _p(dtxt), _s())



def clip_loss_soft_fwd_bwd(img, txt, img_n, txt_n, norms, logits, label_probs, logit_scale, dmm, cos_ws, soft_ws,
                           loss_out, dimg_n, dtxt_n, dimg, dtxt):
    """Soft-label branch (trainers/maple.py:356-360): label_probs fp32 [B, K]; soft_ws fp16 >= 2*B*D."""
    B, D = img.shape
    K = txt.shape[0]
    if label_probs.dtype != torch.float32 or tuple(label_probs.shape) != (B, K) or not label_probs.is_contiguous():
        raise ValueError(f"soft labels must be contiguous fp32 [{B}, {K}], got {label_probs.dtype} "
                         f"{tuple(label_probs.shape)}")
    if soft_ws.dtype != torch.float16 or soft_ws.numel() < 2 * B * D:
        raise ValueError("soft_ws: fp16 workspace of 2*B*D elements")
    call("mf_clip_loss_soft_fwd_bwd", _p(img), _p(txt), _p(img_n), _p(txt_n), _p(norms), _p(logits),
         _p(label_probs), B, K, D, _p(logit_scale), _p(dmm), _p(cos_ws), _p(soft_ws), _p(loss_out), _p(dimg_n),
         _p(dtxt_n), _p(dimg), _p(dtxt), _s())


def argmax_correct(logits, label=None, pred=None, acc=None):
    B, K = logits.shape
    call("mf_argmax_correct", _p(logits), B, K, _p(label), _p(pred), _p(acc), _s())


def optim_chunk_elems() -> int:
    return call("mf_optim_chunk_elems")


def clip_grad_norm(g16, g32, chunks, nchunks, max_norm, part, out):
    ev = _hbm("clip_grad_norm", g16.numel() * 2.0 + g32.numel() * 4.0)  # every gradient read once
    call("mf_clip_grad_norm", _p(g16), _p(g32), _p(chunks), nchunks, float(max_norm), _p(part), _p(out), _s())
    _rec(ev)


def _sgd_call(name, p, g, buf, coef, hyper, *extra):
    # p, g, momentum read; p, momentum written (each at the parameter's element size); sgd_prox_step also reads pglob,
    # sgd_dyn_step pglob and the fp32 lam
    is16 = p.dtype == torch.float16
    ev = _hbm(f"{name}/{'f16' if is16 else 'f32'}",
              p.numel() * 5.0 * p.element_size() + sum(float(t.numel() * t.element_size()) for t in extra))
    call("mf_" + name, _p(p), _p(g), _p(buf), *map(_p, extra), p.numel(), int(is16), _p(coef), _p(hyper), _s())
    _rec(ev)


def _optimizer_call(name, p16, g16, b16, p32, g32, b32, chunks, nchunks, max_norm, part, out, hyper, halt_src,
                    input_flag, *glob):
    # every gradient read twice; p, g, momentum read and written: 5 streams per element, 6 with the two global copies,
    # and the fp32 lam of the dynamic step
    nb = (g16.numel() * 2.0 + g32.numel() * 4.0 + (p16.numel() * 2.0 + p32.numel() * 4.0) * 5.0
          + sum(float(t.numel() * t.element_size()) for t in glob))
    ev = _hbm(name, nb)
    call("mf_" + name, _p(p16), _p(g16), _p(b16), p16.numel(), _p(p32), _p(g32), _p(b32), p32.numel(), _p(chunks),
         nchunks, float(max_norm), _p(part), _p(out), _p(hyper), _p(halt_src), _p(input_flag), *map(_p, glob), _s())
    _rec(ev)


def sgd_step(p, g, buf, coef, hyper):
    """hyper: device fp32 tensor {lr, momentum, weight_decay, first_step, halt}."""
    _sgd_call("sgd_step", p, g, buf, coef, hyper)


def optimizer_step(p16, g16, b16, p32, g32, b32, chunks, nchunks, max_norm, part, out, hyper, halt_src,
                   input_flag=None):
    """clip_grad_norm + sgd_step(fp16) + sgd_step(fp32), with hyper[4] = max(hyper[4], halt_src[0], input_flag[0])
    folded in: three launches, bit-identical (mf_optimizer_step)."""
    _optimizer_call("optimizer_step", p16, g16, b16, p32, g32, b32, chunks, nchunks, max_norm, part, out, hyper,
                    halt_src, input_flag)


def _check_flat(name, t, dtype, numel=None):
    if t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        want = f"contiguous {dtype}" + (f" of {numel} elements" if numel is not None else "")
        raise ValueError(f"{name}: {want} required, got {t.dtype} {tuple(t.shape)}"
                         f"{'' if t.is_contiguous() else ' (not contiguous)'}")


def _check_prox_hyper(hyper):
    if hyper.dtype != torch.float32 or not hyper.is_contiguous() or hyper.numel() < 6:
        raise ValueError("hyper: contiguous fp32 {lr, momentum, weight_decay, first_step, halt, mu} (6 floats) "
                         f"required, got {hyper.dtype} {tuple(hyper.shape)}")


def sgd_prox_step(p, g, buf, pglob, coef, hyper):
    """sgd_step with the FedProx term mu * (p - pglob) added to the clipped gradient (mf_sgd_prox_step).
    hyper: device fp32 tensor {lr, momentum, weight_decay, first_step, halt, mu}; pglob: the last global weights,
    p's dtype and size, a buffer of its own."""
    if p.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"p: fp16 or fp32 required, got {p.dtype}")
    _check_flat("p", p, p.dtype)
    for name, t in (("g", g), ("buf", buf), ("pglob", pglob)):
        _check_flat(name, t, p.dtype, p.numel())
    if p.numel() and pglob.data_ptr() == p.data_ptr():
        raise ValueError("pglob: a buffer of its own required (it is p)")
    _check_prox_hyper(hyper)
    _sgd_call("sgd_prox_step", p, g, buf, coef, hyper, pglob)


def optimizer_step_prox(p16, g16, b16, p32, g32, b32, chunks, nchunks, max_norm, part, out, hyper, halt_src,
                        input_flag=None, glob16=None, glob32=None):
    """optimizer_step with the proximal SGD launch (mf_optimizer_step_prox): glob16 / glob32 are the last global
    weights of the two flat buffers, hyper has 6 floats (mu at [5])."""
    if glob16 is None or glob32 is None:
        raise ValueError("optimizer_step_prox: glob16 and glob32 (the global copies) are required")
    _check_flat("p16", p16, torch.float16)
    _check_flat("p32", p32, torch.float32)
    for name, t, ref in (("g16", g16, p16), ("b16", b16, p16), ("glob16", glob16, p16), ("g32", g32, p32),
                         ("b32", b32, p32), ("glob32", glob32, p32)):
        _check_flat(name, t, ref.dtype, ref.numel())
    if (p16.numel() and glob16.data_ptr() == p16.data_ptr()) or (p32.numel() and glob32.data_ptr() == p32.data_ptr()):
        raise ValueError("glob16 / glob32: buffers of their own required")
    _check_prox_hyper(hyper)
    _optimizer_call("optimizer_step_prox", p16, g16, b16, p32, g32, b32, chunks, nchunks, max_norm, part, out, hyper,
                    halt_src, input_flag, glob16, glob32)


def _check_dyn_hyper(hyper):
    if hyper.dtype != torch.float32 or not hyper.is_contiguous() or hyper.numel() < 6:
        raise ValueError("hyper: contiguous fp32 {lr, momentum, weight_decay, first_step, halt, alpha} (6 floats) "
                         f"required, got {hyper.dtype} {tuple(hyper.shape)}")


def _check_same_device(ref, named):
    for name, t in named:
        if t.device != ref.device:
            raise ValueError(f"{name}: on {t.device}, the parameters are on {ref.device}")


def sgd_dyn_step(p, g, buf, pglob, lam, coef, hyper):
    """sgd_prox_step with FedDyn's linear term (mf_sgd_dyn_step): alpha * (p - pglob) - lam joins the clipped gradient.
    hyper: device fp32 tensor {lr, momentum, weight_decay, first_step, halt, alpha}; pglob: the last global weights,
    p's dtype and size; lam: the client's correction, fp32 of p's size whatever p's dtype; both buffers of their own."""
    if p.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"p: fp16 or fp32 required, got {p.dtype}")
    _check_flat("p", p, p.dtype)
    for name, t in (("g", g), ("buf", buf), ("pglob", pglob)):
        _check_flat(name, t, p.dtype, p.numel())
    _check_flat("lam", lam, torch.float32, p.numel())
    _check_same_device(p, (("g", g), ("buf", buf), ("pglob", pglob), ("lam", lam)))
    if p.numel() and pglob.data_ptr() == p.data_ptr():
        raise ValueError("pglob: a buffer of its own required (it is p)")
    for oname, o in (("p", p), ("g", g), ("buf", buf), ("pglob", pglob)):
        if _overlap(lam, o):
            raise ValueError(f"lam: a buffer of its own required (it overlaps {oname})")
    _check_dyn_hyper(hyper)
    _sgd_call("sgd_dyn_step", p, g, buf, coef, hyper, pglob, lam)


def optimizer_step_dyn(p16, g16, b16, p32, g32, b32, chunks, nchunks, max_norm, part, out, hyper, halt_src,
                       input_flag=None, glob16=None, glob32=None, lam=None):
    """optimizer_step_prox with the dynamic SGD launch (mf_optimizer_step_dyn): hyper has 6 floats (alpha at [5]) and
    lam is fp32 of n16 + n32 elements in the bucket's order [fp16 trainables | fp32 trainables]."""
    if glob16 is None or glob32 is None or lam is None:
        raise ValueError("optimizer_step_dyn: glob16, glob32 (the global copies) and lam are required")
    _check_flat("p16", p16, torch.float16)
    _check_flat("p32", p32, torch.float32)
    for name, t, ref in (("g16", g16, p16), ("b16", b16, p16), ("glob16", glob16, p16), ("g32", g32, p32),
                         ("b32", b32, p32), ("glob32", glob32, p32)):
        _check_flat(name, t, ref.dtype, ref.numel())
    _check_flat("lam", lam, torch.float32, p16.numel() + p32.numel())
    named = (("p32", p32), ("g16", g16), ("b16", b16), ("g32", g32), ("b32", b32), ("glob16", glob16),
             ("glob32", glob32))
    _check_same_device(p16, named + (("lam", lam),))
    if (p16.numel() and glob16.data_ptr() == p16.data_ptr()) or (p32.numel() and glob32.data_ptr() == p32.data_ptr()):
        raise ValueError("glob16 / glob32: buffers of their own required")
    for oname, o in (("p16", p16),) + named:
        if _overlap(lam, o):
            raise ValueError(f"lam: a buffer of its own required (it overlaps {oname})")
    _check_dyn_hyper(hyper)
    _optimizer_call("optimizer_step_dyn", p16, g16, b16, p32, g32, b32, chunks, nchunks, max_norm, part, out, hyper,
                    halt_src, input_flag, glob16, glob32, lam)


def fedavg_pack_weighted(p16, p32, invalid_flag, weight, bucket):
    """bucket: n16 + n32 + 2 floats = [weight * trainables | weight | vote] (mf_fedavg_pack_weighted)."""
    import math
    weight = float(weight)
    if not math.isfinite(weight) or weight <= 0.0:
        raise ValueError(f"weight: finite and > 0 required, got {weight}")
    _check_flat("p16", p16, torch.float16)
    _check_flat("p32", p32, torch.float32)
    _check_flat("bucket", bucket, torch.float32, p16.numel() + p32.numel() + 2)
    call("mf_fedavg_pack_weighted", _p(p16), p16.numel(), _p(p32), p32.numel(), _p(invalid_flag), weight, _p(bucket),
         _s())


def fedavg_unpack_weighted(bucket, p16, p32, g16=None, g32=None):
    """fp16(bucket[i] / bucket[n]) into p16 / p32 and g16 / g32; vote count bucket[n+1] == 0 restores from g16 / g32."""
    _check_flat("p16", p16, torch.float16)
    _check_flat("p32", p32, torch.float32)
    if bucket.dtype != torch.float32 or not bucket.is_contiguous() or bucket.numel() < p16.numel() + p32.numel() + 2:
        raise ValueError("bucket: contiguous fp32 of at least n16 + n32 + 2 floats required")
    if g16 is not None:
        _check_flat("g16", g16, torch.float16, p16.numel())
    if g32 is not None:
        _check_flat("g32", g32, torch.float32, p32.numel())
    call("mf_fedavg_unpack_weighted", _p(bucket), _p(p16), p16.numel(), _p(p32), p32.numel(), _p(g16), _p(g32), _s())


def fedavg_pack(p16, p32, invalid_flag, bucket):
    """bucket: n16 + n32 + 1 floats (last = this client's valid vote)."""
    assert bucket.numel() == p16.numel() + p32.numel() + 1
    call("mf_fedavg_pack", _p(p16), p16.numel(), _p(p32), p32.numel(), _p(invalid_flag), _p(bucket), _s())


def fedavg_unpack(bucket, p16, p32, g16=None, g32=None):
    call("mf_fedavg_unpack", _p(bucket), _p(p16), p16.numel(), _p(p32), p32.numel(), _p(g16), _p(g32), _s())


FEDOPT_IDS = {"fedavgm": 1, "fedadagrad": 2, "fedadam": 3, "fedyogi": 4}


def _overlap(a, b) -> bool:
    if a is None or b is None or not a.numel() or not b.numel():
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_fedopt_outputs(p16, p32, g16, g32):
    _check_flat("p16", p16, torch.float16)
    _check_flat("p32", p32, torch.float32)
    _check_flat("g16", g16, torch.float16, p16.numel())
    _check_flat("g32", g32, torch.float32, p32.numel())
    if _overlap(p16, g16) or _overlap(p32, g32):
        raise ValueError("g16 / g32: buffers of their own required")


def fedopt_step(bucket, weighted, opt, beta1, beta2, tau, eta, x, m, v, p16, p32, g16, g32):
    """The FedOpt server step on the summed bucket (mf_fedopt_step).  opt: "fedavgm", "fedadagrad", "fedadam" or
    "fedyogi"; x, m, v: fp32 state of n16 + n32 elements each (v is None for fedavgm), buffers of their own; bucket:
    the plain (n + 1 floats) or, weighted=True, the weighted (n + 2 floats) layout."""
    import math
    if opt not in FEDOPT_IDS:
        raise ValueError(f"opt: one of {tuple(FEDOPT_IDS)}, got {opt!r}")
    adaptive = opt != "fedavgm"
    hp = {"beta1": float(beta1), "beta2": float(beta2), "tau": float(tau), "eta": float(eta)}
    for name, val in hp.items():
        if not math.isfinite(val):
            raise ValueError(f"{name}: finite required, got {val}")
    if adaptive and hp["tau"] <= 0.0:
        raise ValueError(f"tau: > 0 required for {opt}, got {hp['tau']}")
    _check_fedopt_outputs(p16, p32, g16, g32)
    n = p16.numel() + p32.numel()
    tail = 2 if weighted else 1
    if bucket.dtype != torch.float32 or not bucket.is_contiguous() or bucket.numel() < n + tail:
        raise ValueError(f"bucket: contiguous fp32 of at least n16 + n32 + {tail} floats required")
    if x is None or m is None or (adaptive and v is None):
        raise ValueError("x, m" + (", v" if adaptive else "") + ": the server state is required")
    state = [("x", x), ("m", m)] + ([("v", v)] if adaptive else [])
    for name, t in state:
        _check_flat(name, t, torch.float32, n)
    others = [("bucket", bucket[:n + tail]), ("p16", p16), ("p32", p32), ("g16", g16), ("g32", g32)]
    for i, (name, t) in enumerate(state):
        for oname, o in state[i + 1:] + others:
            if _overlap(t, o):
                raise ValueError(f"{name}: a buffer of its own required (it overlaps {oname})")
    # bucket read; x, m (, v) read and written; the weights and the global copy written
    nb = n * (4.0 + 8.0 * len(state)) + p16.numel() * 4.0 + p32.numel() * 8.0
    ev = _hbm(f"fedopt_step/{opt}", nb)
    call("mf_fedopt_step", _p(bucket), int(bool(weighted)), FEDOPT_IDS[opt], hp["beta1"], hp["beta2"], hp["tau"],
         hp["eta"], _p(x), _p(m), _p(v) if adaptive else None, _p(p16), p16.numel(), _p(p32), p32.numel(), _p(g16),
         _p(g32), _s())
    _rec(ev)


def fedopt_deliver(x, p16, p32, g16, g32):
    """fp16(x) into another client's trainables and global copy (mf_fedopt_deliver); x is only read."""
    _check_fedopt_outputs(p16, p32, g16, g32)
    if x is None:
        raise ValueError("x: the server state is required")
    _check_flat("x", x, torch.float32, p16.numel() + p32.numel())
    for oname, o in (("p16", p16), ("p32", p32), ("g16", g16), ("g32", g32)):
        if _overlap(x, o):
            raise ValueError(f"x: a buffer of its own required (it overlaps {oname})")
    call("mf_fedopt_deliver", _p(x), _p(p16), p16.numel(), _p(p32), p32.numel(), _p(g16), _p(g32), _s())


def _check_feddyn(bucket, alpha, h, lam, flag, p16, p32, g16, g32):
    import math
    alpha = float(alpha)
    if not math.isfinite(alpha) or alpha <= 0.0:
        raise ValueError(f"alpha: finite and > 0 required, got {alpha}")
    _check_fedopt_outputs(p16, p32, g16, g32)
    n = p16.numel() + p32.numel()
    if bucket.dtype != torch.float32 or not bucket.is_contiguous() or bucket.numel() < n + 1:
        raise ValueError("bucket: contiguous fp32 of at least n16 + n32 + 1 floats (the plain layout) required")
    if h is None or lam is None:
        raise ValueError("h, lam: the FedDyn state is required")
    _check_flat("h", h, torch.float32, n)
    _check_flat("lam", lam, torch.float32, n)
    if flag is None or flag.dtype != torch.int32 or flag.numel() < 1:
        raise ValueError("flag: the client's int32 device flag is required")
    _check_same_device(p16, (("p32", p32), ("g16", g16), ("g32", g32), ("bucket", bucket), ("h", h), ("lam", lam),
                             ("flag", flag)))
    others = [("bucket", bucket[:n + 1]), ("p16", p16), ("p32", p32), ("g16", g16), ("g32", g32)]
    for name, t, rest in (("h", h, [("lam", lam)] + others), ("lam", lam, others)):
        for oname, o in rest:
            if _overlap(t, o):
                raise ValueError(f"{name}: a buffer of its own required (it overlaps {oname})")
    return alpha, n


def feddyn_step(bucket, alpha, num_clients, h, lam, flag, p16, p32, g16, g32):
    """FedDyn's round end on the summed plain bucket (mf_feddyn_step): h, the server's mean of the num_clients
    corrections, steps; this client's lam updates unless its flag is set; fp16(mean - h / alpha) goes into its weights
    and global copy.  h, lam: fp32 of n16 + n32 elements, buffers of their own."""
    if isinstance(num_clients, bool) or int(num_clients) != num_clients or num_clients < 1:
        raise ValueError(f"num_clients: an integer >= 1 required, got {num_clients!r}")
    alpha, n = _check_feddyn(bucket, alpha, h, lam, flag, p16, p32, g16, g32)
    # bucket read; h, lam read and written; the weights and the global copy read and written
    ev = _hbm("feddyn_step", n * 20.0 + p16.numel() * 8.0 + p32.numel() * 16.0)
    call("mf_feddyn_step", _p(bucket), alpha, int(num_clients), _p(h), _p(lam), _p(flag), _p(p16), p16.numel(),
         _p(p32), p32.numel(), _p(g16), _p(g32), _s())
    _rec(ev)


def feddyn_deliver(bucket, alpha, h, lam, flag, p16, p32, g16, g32):
    """The rank's second and later clients after feddyn_step (mf_feddyn_deliver): the stepped h is only read, the same
    fp16(mean - h / alpha) delivered, this client's own lam updated."""
    alpha, n = _check_feddyn(bucket, alpha, h, lam, flag, p16, p32, g16, g32)
    ev = _hbm("feddyn_deliver", n * 16.0 + p16.numel() * 8.0 + p32.numel() * 16.0)
    call("mf_feddyn_deliver", _p(bucket), alpha, _p(h), _p(lam), _p(flag), _p(p16), p16.numel(), _p(p32), p32.numel(),
         _p(g16), _p(g32), _s())
    _rec(ev)


def fedavg_reduce_ordered(gathered, nclients, out):
    """out = sum over clients (in client order) of gathered.view(nclients, -1)[:, :out.numel()]."""
    stride = gathered.numel() // nclients
    assert gathered.numel() == stride * nclients and out.numel() <= stride
    call("mf_fedavg_reduce_ordered", _p(gathered), nclients, stride, out.numel(), _p(out), _s())


MEDIAN_TRIM = 2 ** 31 - 1  # a trim no client count reaches: mf_fedavg_reduce_trimmed degrades it to the median


def fedavg_reduce_trimmed(gathered, nclients, trim_k, count_pos, out):
    """out = the coordinate-wise trim_k-trimmed mean (median: MEDIAN_TRIM) over gathered.view(nclients, -1)[:, :n],
    n = out.numel(); a NaN is an absent client; out[count_pos] = the number of present ones (count_pos -1: none)
    (mf_fedavg_reduce_trimmed)."""
    nclients, trim_k, count_pos = int(nclients), int(trim_k), int(count_pos)
    if not 1 <= nclients <= 64:
        raise ValueError(f"nclients: 1 to 64 required, got {nclients}")
    if not 0 <= trim_k <= MEDIAN_TRIM:
        raise ValueError(f"trim_k: 0 to {MEDIAN_TRIM} required, got {trim_k}")
    for name, t in (("gathered", gathered), ("out", out)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: contiguous fp32 required, got {t.dtype} {tuple(t.shape)}")
    stride = gathered.numel() // nclients
    if gathered.numel() != stride * nclients or out.numel() > stride:
        raise ValueError(f"gathered: {nclients} rows of at least {out.numel()} floats required, got {gathered.numel()}")
    if count_pos >= out.numel():
        raise ValueError(f"count_pos: below {out.numel()} (or -1) required, got {count_pos}")
    if _overlap(gathered, out):
        raise ValueError("out: a buffer of its own required (it overlaps gathered)")
    call("mf_fedavg_reduce_trimmed", _p(gathered), nclients, stride, out.numel(), trim_k, max(count_pos, -1), _p(out),
         _s())


def fedavg_pack_robust(p16, p32, invalid_flag, bucket):
    """bucket: n16 + n32 + 2 floats = [trainables | 1 | 1], an invalid client all quiet NaNs (mf_fedavg_pack_robust)."""
    _check_flat("p16", p16, torch.float16)
    _check_flat("p32", p32, torch.float32)
    _check_flat("bucket", bucket, torch.float32, p16.numel() + p32.numel() + 2)
    call("mf_fedavg_pack_robust", _p(p16), p16.numel(), _p(p32), p32.numel(), _p(invalid_flag), _p(bucket), _s())


KRUM_MAX_CLIENTS = 64


def _check_krum_clients(nclients) -> int:
    if isinstance(nclients, bool) or int(nclients) != nclients or not 1 <= nclients <= KRUM_MAX_CLIENTS:
        raise ValueError(f"nclients: 1 to {KRUM_MAX_CLIENTS} required, got {nclients!r}")
    return int(nclients)


def krum_ws_bytes(nclients: int, n: int) -> int:
    """Bytes of workspace krum_pairwise needs for nclients rows of n coordinates (mf_krum_ws_bytes)."""
    nclients = _check_krum_clients(nclients)
    if int(n) != n or n < 0:
        raise ValueError(f"n: an integer >= 0 required, got {n!r}")
    return int(call("mf_krum_ws_bytes", nclients, int(n)))


def krum_chunk_elems() -> int:
    """Coordinates per workgroup of krum_pairwise's first launch."""
    return int(call("mf_krum_chunk_elems"))


def krum_pairwise(gathered, nclients, n, ws, dist):
    """dist[i][j] = sum over t < n of (double)(x_i[t] - x_j[t])^2 with x = gathered.view(nclients, -1): Multi-Krum's
    squared distances, fp32 subtract, fp64 square and sum, in a fixed order (mf_krum_pairwise; two launches, no host
    synchronisation).  A NaN row is an absent client: its row, column and diagonal are NaN.  ws: contiguous fp64 of at
    least krum_ws_bytes(nclients, n) bytes; dist: contiguous fp64 of nclients^2 elements; buffers of their own."""
    nclients = _check_krum_clients(nclients)
    if gathered.dtype != torch.float32 or not gathered.is_contiguous():
        raise ValueError(f"gathered: contiguous fp32 required, got {gathered.dtype} {tuple(gathered.shape)}")
    stride = gathered.numel() // nclients
    if int(n) != n or n < 0 or gathered.numel() != stride * nclients or n > stride:
        raise ValueError(f"gathered: {nclients} rows of at least n = {n} floats required, got {gathered.numel()}")
    need = krum_ws_bytes(nclients, n)
    if ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() * 8 < need:
        raise ValueError(f"ws: contiguous fp64 of at least {need} bytes required, got {ws.dtype} {tuple(ws.shape)}")
    _check_flat("dist", dist, torch.float64, nclients * nclients)
    _check_same_device(gathered, (("ws", ws), ("dist", dist)))
    for (an, a), (bn, b) in ((("ws", ws), ("gathered", gathered)), (("dist", dist), ("gathered", gathered)),
                             (("ws", ws), ("dist", dist))):
        if _overlap(a, b):
            raise ValueError(f"{an}: a buffer of its own required (it overlaps {bn})")
    ev = _hbm("krum_pairwise", nclients * int(n) * 4.0)  # the image read once (algorithmically)
    call("mf_krum_pairwise", _p(gathered), nclients, stride, int(n), _p(ws), _p(dist), _s())
    _rec(ev)


def krum_select(parts, nclients, f, m, selected, scores, counts):
    """Multi-Krum's selection from the shards' distance matrices parts ([nparts, nclients^2] fp64, added in part
    order): selected (nclients int32, 0 / 1), scores (nclients fp64, NaN for an absent client) and counts (3 int32:
    p present, the effective f', the number kept m') (mf_krum_select; one workgroup).  m = 0 keeps p - f' clients."""
    nclients = _check_krum_clients(nclients)
    for name, v in (("f", f), ("m", m)):
        if isinstance(v, bool) or int(v) != v or not 0 <= v < 2 ** 31:
            raise ValueError(f"{name}: an integer >= 0 required, got {v!r}")
    nn = nclients * nclients
    if parts.dtype != torch.float64 or not parts.is_contiguous() or parts.numel() < nn or parts.numel() % nn:
        raise ValueError(f"parts: contiguous fp64 of nparts * {nn} elements required, got {parts.dtype} "
                         f"{tuple(parts.shape)}")
    _check_flat("selected", selected, torch.int32, nclients)
    _check_flat("scores", scores, torch.float64, nclients)
    _check_flat("counts", counts, torch.int32, 3)
    _check_same_device(parts, (("selected", selected), ("scores", scores), ("counts", counts)))
    outs = (("selected", selected), ("scores", scores), ("counts", counts))
    for i, (name, t) in enumerate(outs):
        for oname, o in (("parts", parts),) + outs[i + 1:]:
            if _overlap(t, o):
                raise ValueError(f"{name}: a buffer of its own required (it overlaps {oname})")
    call("mf_krum_select", _p(parts), parts.numel() // nn, nclients, int(f), int(m), _p(selected), _p(scores),
         _p(counts), _s())


def fedavg_reduce_selected(gathered, nclients, selected, count_pos, out):
    """out = the mean, in client order, of the rows of gathered.view(nclients, -1)[:, :n] whose selected[c] (int32, read
    on the device) is non-zero, n = out.numel(); nobody selected gives +0; out[count_pos] = the number of non-NaN
    values at that coordinate (count_pos -1: none) (mf_fedavg_reduce_selected)."""
    nclients, count_pos = _check_krum_clients(nclients), int(count_pos)
    for name, t in (("gathered", gathered), ("out", out)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: contiguous fp32 required, got {t.dtype} {tuple(t.shape)}")
    stride = gathered.numel() // nclients
    if gathered.numel() != stride * nclients or out.numel() > stride:
        raise ValueError(f"gathered: {nclients} rows of at least {out.numel()} floats required, got {gathered.numel()}")
    _check_flat("selected", selected, torch.int32, nclients)
    if count_pos >= out.numel():
        raise ValueError(f"count_pos: below {out.numel()} (or -1) required, got {count_pos}")
    _check_same_device(gathered, (("selected", selected), ("out", out)))
    if _overlap(gathered, out):
        raise ValueError("out: a buffer of its own required (it overlaps gathered)")
    ev = _hbm("fedavg_reduce_selected", (nclients + 1) * out.numel() * 4.0)  # at most: unselected rows are not read
    call("mf_fedavg_reduce_selected", _p(gathered), nclients, stride, out.numel(), _p(selected), max(count_pos, -1),
         _p(out), _s())
    _rec(ev)


def dp_update_ws_floats(n16: int, n32: int) -> int:
    """Floats of workspace dp_update_scale needs for buffers of these sizes."""
    return int(call("mf_dp_update_ws_floats", int(n16), int(n32)))


def _check_dp_pairs(p16, g16, p32, g32):
    _check_flat("p16", p16, torch.float16)
    _check_flat("p32", p32, torch.float32)
    _check_flat("g16", g16, torch.float16, p16.numel())
    _check_flat("g32", g32, torch.float32, p32.numel())


def dp_update_scale(p16, g16, p32, g32, clip, ws, out):
    """out = {norm, scale, clipped} of the update [p16 | p32] - [g16 | g32]: norm = its L2 norm, scale = clip / norm
    when norm > clip, else exactly 1 (mf_dp_update_scale; two launches, no host synchronisation).  ws: fp32 of at
    least dp_update_ws_floats(n16, n32) elements; out: 3 floats; both buffers of their own."""
    import math
    clip = float(clip)
    if math.isnan(clip) or clip <= 0.0:
        raise ValueError(f"clip: > 0 required, got {clip}")
    _check_dp_pairs(p16, g16, p32, g32)
    need = dp_update_ws_floats(p16.numel(), p32.numel())
    if ws.dtype != torch.float32 or not ws.is_contiguous() or ws.numel() < need:
        raise ValueError(f"ws: contiguous fp32 of at least {need} floats required, got {ws.dtype} {tuple(ws.shape)}")
    _check_flat("out", out, torch.float32, 3)
    for name, t in (("ws", ws), ("out", out)):
        for oname, o in (("p16", p16), ("g16", g16), ("p32", p32), ("g32", g32)) + ((("out", out),) if t is ws else ()):
            if _overlap(t, o):
                raise ValueError(f"{name}: a buffer of its own required (it overlaps {oname})")
    ev = _hbm("dp_update_scale", p16.numel() * 4.0 + p32.numel() * 8.0)  # the weights and the global copy read once
    call("mf_dp_update_scale", _p(p16), _p(g16), p16.numel(), _p(p32), _p(g32), p32.numel(), clip, _p(ws), _p(out),
         _s())
    _rec(ev)


DP_LAYOUTS = {"plain": 0, "weighted": 1, "robust": 2}


def fedavg_pack_clipped(p16, p32, g16, g32, invalid_flag, scale, weight, layout, bucket):
    """The bucket of layout "plain" ([y | 1]), "weighted" ([w * y | w | 1]) or "robust" ([y | 1 | 1], an invalid
    client all quiet NaNs) with y = g + s * (float(p) - float(g)), s = scale[0] read on the device (dp_update_scale's
    out[1:2]); s >= 1 packs float(p) itself (mf_fedavg_pack_clipped).  weight is read by "weighted" only."""
    import math
    if layout not in DP_LAYOUTS:
        raise ValueError(f"layout: one of {tuple(DP_LAYOUTS)}, got {layout!r}")
    weight = 1.0 if layout != "weighted" else float(weight)
    if not math.isfinite(weight) or weight <= 0.0:
        raise ValueError(f"weight: finite and > 0 required, got {weight}")
    _check_dp_pairs(p16, g16, p32, g32)
    tail = 1 if layout == "plain" else 2
    _check_flat("bucket", bucket, torch.float32, p16.numel() + p32.numel() + tail)
    if scale is None or scale.dtype != torch.float32 or scale.numel() < 1:
        raise ValueError("scale: an fp32 tensor (dp_update_scale's out[1:2]) required")
    for oname, o in (("p16", p16), ("g16", g16), ("p32", p32), ("g32", g32), ("scale", scale)):
        if _overlap(bucket, o):
            raise ValueError(f"bucket: a buffer of its own required (it overlaps {oname})")
    call("mf_fedavg_pack_clipped", _p(p16), p16.numel(), _p(p32), p32.numel(), _p(g16), _p(g32), _p(invalid_flag),
         _p(scale), weight, DP_LAYOUTS[layout], _p(bucket), _s())


def dp_add_noise(buf, offset, seed, round_, std):
    """buf[j] += std * z(offset + j): z(i) the standard normal of global coordinate i under (seed, round), a
    counter-based stream (Philox4x32-10 + Box-Muller, include/mapfed.h), so any split of a range over calls gives the
    same bits (mf_dp_add_noise).  std = 0 launches nothing."""
    import math
    offset, seed, round_, std = int(offset), int(seed), int(round_), float(std)
    if buf.dtype != torch.float32 or not buf.is_contiguous():
        raise ValueError(f"buf: contiguous fp32 required, got {buf.dtype} {tuple(buf.shape)}")
    if not 0 <= offset <= 2 ** 63 - 1 - buf.numel():
        raise ValueError(f"offset: 0 to 2**63 - 1 - n required, got {offset}")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed: 0 to 2**64 - 1 required, got {seed}")
    if not 0 <= round_ < 2 ** 32:
        raise ValueError(f"round: 0 to 2**32 - 1 required, got {round_}")
    if not math.isfinite(std) or std < 0.0:
        raise ValueError(f"std: finite and >= 0 required, got {std}")
    ev = _hbm("dp_add_noise", buf.numel() * 8.0)  # read and written once
    call("mf_dp_add_noise", _p(buf), buf.numel(), offset, seed, round_, std, _s())
    _rec(ev)


COMPRESS_BLOCK = 256  # coordinates per block of either uplink codec: one fp32 scale (int8), k kept entries (top-k)
COMPRESS_ROUNDINGS = {"nearest": 0, "stochastic": 1}
TOPK_MAX = 64  # entries kept per block of COMPRESS_BLOCK coordinates, at most: one lane each
TOPK_LAYOUTS = ("plain", "weighted")


def _check_shard(S) -> int:
    S = int(S)
    if S <= 0 or S % COMPRESS_BLOCK:
        raise ValueError(f"S: a positive multiple of {COMPRESS_BLOCK} required, got {S}")
    return S


def _check_topk(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= TOPK_MAX:
        raise ValueError(f"k: an integer from 1 to {TOPK_MAX} required, got {k!r}")
    return k


def compress_chunk_bytes(S: int) -> int:
    """Bytes of one wire chunk of shard length S: [S int8 codes | S / 256 fp32 scales | fp32 weight | fp32 vote]
    (mf_compress_chunk_bytes)."""
    return int(call("mf_compress_chunk_bytes", _check_shard(S)))


def topk_chunk_bytes(S: int, k: int) -> int:
    """Bytes of one top-k wire chunk of shard length S: [S / 256 * k fp32 values | S / 256 * k uint8 indices | zero
    bytes to a multiple of 4 | fp32 weight | fp32 vote] (mf_topk_chunk_bytes)."""
    k = _check_topk(k)
    return int(call("mf_topk_chunk_bytes", _check_shard(S), k))


def _uplink_encode(key, symbol, chunk, codec_args, p16, p32, g16, g32, e_in, e_out, invalid_flag, weight, image, slot,
                   S):
    """What compress_quantize and topk_select share: the checks, the byte model and the call.  chunk: the codec's wire
    chunk for shard length S; codec_args: the codec's own arguments, which the entry point takes after the weight."""
    import math
    weight = 1.0 if weight is None else float(weight)
    if not math.isfinite(weight) or weight <= 0.0:
        raise ValueError(f"weight: finite and > 0 required, got {weight}")
    slot, S = int(slot), int(S)
    _check_dp_pairs(p16, g16, p32, g32)
    n = p16.numel() + p32.numel()
    if image.dtype != torch.uint8 or image.dim() != 3 or not image.is_contiguous() or image.shape[2] != chunk:
        raise ValueError(f"image: contiguous uint8 [ranks][clients][{chunk}] required, got {image.dtype} "
                         f"{tuple(image.shape)}")
    world, C = image.shape[0], image.shape[1]
    if not 0 <= slot < C:
        raise ValueError(f"slot: 0 to {C - 1} required, got {slot}")
    if world * S < n:
        raise ValueError(f"image: {world} shards of {S} hold fewer than the {n} coordinates")
    if (e_in is None) != (e_out is None):
        raise ValueError("e_in / e_out: both residual buffers or neither")
    if e_in is not None:
        _check_flat("e_in", e_in, torch.float32, n)
        _check_flat("e_out", e_out, torch.float32, n)
        if _overlap(e_in, e_out):
            raise ValueError("e_out: a buffer of its own required (it overlaps e_in)")
    if invalid_flag is None or invalid_flag.dtype != torch.int32 or invalid_flag.numel() < 1:
        raise ValueError("invalid_flag: an int32 tensor required")
    for oname, o in (("p16", p16), ("g16", g16), ("p32", p32), ("g32", g32), ("e_in", e_in), ("e_out", e_out)):
        if _overlap(image, o):
            raise ValueError(f"image: a buffer of its own required (it overlaps {oname})")
    # weights, global copy and residual read, the residual and the chunks written
    ev = _hbm(key, p16.numel() * 4.0 + p32.numel() * 8.0 + (8.0 * n if e_in is not None else 0.0)
              + world * float(chunk))
    call(symbol, _p(p16), _p(g16), p16.numel(), _p(p32), _p(g32), p32.numel(), _p(e_in), _p(e_out),
         _p(invalid_flag), weight, *codec_args, image.data_ptr() + slot * chunk, C * chunk, S, world, _s())
    _rec(ev)


def _uplink_decode(key, symbol, chunk, layouts, codec_args, image, nclients, chunk_stride, S, first, first_step, g16,
                   g32, layout, out, out_stride):
    """What compress_decode and topk_decode share.  layouts: the ones the codec's decode knows; codec_args: the
    codec's own arguments, which the entry point takes last."""
    if layout not in layouts:
        raise ValueError(f"layout: one of {tuple(layouts)}, got {layout!r}")
    nclients, chunk_stride, S, first, first_step, out_stride = (int(v) for v in (nclients, chunk_stride, S, first,
                                                                                  first_step, out_stride))
    if nclients < 1 or first < 0 or first_step < 0:
        raise ValueError(f"nclients >= 1, first >= 0 and first_step >= 0 required, got {nclients}, {first}, {first_step}")
    if chunk_stride % 4 or (nclients > 1 and (chunk_stride < chunk or out_stride < S)):
        raise ValueError(f"chunk_stride: a multiple of 4 of at least {chunk} bytes, and out_stride at least {S}, "
                         f"required, got {chunk_stride}, {out_stride}")
    if image.dtype != torch.uint8 or not image.is_contiguous() or image.numel() < (nclients - 1) * chunk_stride + chunk:
        raise ValueError(f"image: contiguous uint8 of at least {(nclients - 1) * chunk_stride + chunk} bytes required, "
                         f"got {image.dtype} {tuple(image.shape)}")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < (nclients - 1) * out_stride + S:
        raise ValueError(f"out: contiguous fp32 of at least {(nclients - 1) * out_stride + S} floats required, got "
                         f"{out.dtype} {tuple(out.shape)}")
    _check_flat("g16", g16, torch.float16)
    _check_flat("g32", g32, torch.float32)
    for oname, o in (("image", image), ("g16", g16), ("g32", g32)):
        if _overlap(out, o):
            raise ValueError(f"out: a buffer of its own required (it overlaps {oname})")
    ev = _hbm(key, nclients * (float(chunk) + 4.0 * S + 3.0 * S))  # chunk and g read, the image written
    call(symbol, _p(image), chunk_stride, nclients, S, first, first_step, _p(g16), g16.numel(), _p(g32), g32.numel(),
         DP_LAYOUTS[layout], _p(out), out_stride, *codec_args, _s())
    _rec(ev)


def compress_quantize(p16, p32, g16, g32, e_in, e_out, invalid_flag, weight, rounding, seed, round_, client, image,
                      slot, S):
    """The int8 codes, block scales and tail of the update [p16 | p32] - [g16 | g32] (+ e_in, the residual; e_out
    receives the new one; both None: no error feedback) written into image[:, slot, :], the exchange's uint8 send image
    [destination rank][local client][compress_chunk_bytes(S)] (mf_compress_quantize, include/mapfed.h).  rounding:
    "nearest" or "stochastic" (bits from (seed, round_, client, coordinate) alone); weight: the tail's weight (None: 1)."""
    if rounding not in COMPRESS_ROUNDINGS:
        raise ValueError(f"rounding: one of {tuple(COMPRESS_ROUNDINGS)}, got {rounding!r}")
    seed, round_, client = int(seed), int(round_), int(client)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed: 0 to 2**64 - 1 required, got {seed}")
    if not 0 <= round_ < 2 ** 32:
        raise ValueError(f"round: 0 to 2**32 - 1 required, got {round_}")
    if not 0 <= client < 2 ** 31:
        raise ValueError(f"client: 0 to 2**31 - 1 required, got {client}")
    _uplink_encode("compress_quantize", "mf_compress_quantize", compress_chunk_bytes(S),
                   (COMPRESS_ROUNDINGS[rounding], seed, round_, client), p16, p32, g16, g32, e_in, e_out, invalid_flag,
                   weight, image, slot, S)


def compress_decode(image, nclients, chunk_stride, S, first, first_step, g16, g32, layout, out, out_stride):
    """nclients wire chunks, image[c * chunk_stride:] (a flat uint8 tensor, bytes), decoded into out[c * out_stride:
    c * out_stride + S] (fp32): chunk c holds the global coordinates first + c * first_step + j, j < S, and out
    receives the fp32 image the reduce kernels read, in layout "plain", "weighted" or "robust" (mf_compress_decode,
    include/mapfed.h).  g16 / g32: the global copy the update was taken against."""
    _uplink_decode("compress_decode", "mf_compress_decode", compress_chunk_bytes(S), DP_LAYOUTS, (), image, nclients,
                   chunk_stride, S, first, first_step, g16, g32, layout, out, out_stride)


def topk_select(p16, p32, g16, g32, e_in, e_out, invalid_flag, weight, k, image, slot, S):
    """The k entries of largest magnitude of every block of 256 coordinates of the update [p16 | p32] - [g16 | g32]
    (+ e_in, the residual; e_out receives the new one, zero where a coordinate was sent; both None: no error feedback),
    as (uint8 index, fp32 value), and the tail, written into image[:, slot, :], the exchange's uint8 send image
    [destination rank][local client][topk_chunk_bytes(S, k)] (mf_topk_select, include/mapfed.h).  weight: the tail's
    weight (None: 1)."""
    _uplink_encode("topk_select", "mf_topk_select", topk_chunk_bytes(S, k), (k,), p16, p32, g16, g32, e_in, e_out,
                   invalid_flag, weight, image, slot, S)


def topk_decode(image, nclients, chunk_stride, S, first, first_step, g16, g32, layout, out, out_stride, k):
    """nclients top-k wire chunks, image[c * chunk_stride:] (a flat uint8 tensor, bytes), decoded into
    out[c * out_stride: c * out_stride + S] (fp32) as compress_decode does: g plus the sent value at a kept coordinate,
    g + 0 elsewhere, in layout "plain" or "weighted" (mf_topk_decode, include/mapfed.h)."""
    _uplink_decode("topk_decode", "mf_topk_decode", topk_chunk_bytes(S, k), TOPK_LAYOUTS, (k,), image, nclients,
                   chunk_stride, S, first, first_step, g16, g32, layout, out, out_stride)


def nonfinite_flag(x, flag):
    call("mf_nonfinite_flag", _p(x), x.numel(), int(x.dtype == torch.float16), _p(flag), _s())
