"""Typed Python wrappers over the libgvl C-ABI (one function per entry point of include/gvl.h).

Every wrapper takes torch tensors that already live on the current ROCm device, checks
dtype/layout on the host, and launches on torch.cuda.current_stream().  There is no CPU
path: a CPU tensor is rejected with a clear error.
"""
from __future__ import annotations

import ctypes as C
import math


import torch

from . import _lib
from ._lib import AttnBwdDesc, AttnDesc, GemmDesc

BF16 = torch.bfloat16
F32 = torch.float32


def _L():
    return _lib.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "gvl: the HIP kernel path needs tensors on a ROCm GPU (got a CPU tensor); "
                "there is no CPU fallback in the product path")


def _rowmajor(t, name):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"gvl: {name} must be a 2-D row-major view (got shape {tuple(t.shape)}, "
                         f"strides {t.stride()})")


# ------------------------------------------------------------------ live kernel timing
class KernelTimer:
    """Times every GEMM launch with a pair of HIP events (bench.py's roofline line).

    dispatch=True (default): the events are bound to the GEMM kernel's own dispatch
    (gvl_set_launch_events -> hipExtLaunchKernelGGL), so each interval is the kernel's
    execution as its dispatch records it — the quantity rocprofv3's kernel trace reports.
    dispatch=False: two stream markers around the launch (includes dispatch latency)."""

    def __init__(self, dispatch: bool = True):
        self.records = []
        self.dispatch = dispatch

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, flops in self.records:
            s = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0})
            s["launches"] += 1
            s["ms"] += e0.elapsed_time(e1)
            s["flops"] += flops
        return out


_timer = None


def set_kernel_timer(t):
    global _timer
    _timer = t


_WS = {}
GEMM_WORKSPACE_MB = 64


def _gemm_workspace(device):
    """Per-device fp32 split-K scratch, allocated once (stream-ordered reuse; allocate it
    before any hipGraph capture — bench/train warm up eagerly first)."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(GEMM_WORKSPACE_MB * 1024 * 1024 // 4, dtype=F32, device=device)
        _WS[key] = ws
    return ws


_TK = {}
GEMM_TICKETS = 1 << 16
# Arrival tickets (gvl.h ABI v5) go with every gvl_gemm call; the persistent kernel's in-launch
# two-way combine that uses them stays off for single GEMMs (decided in C, gemm_plan.hip).
# Batched weight gradients may use it (gvl_gemm_batched decides).


def _gemm_tickets(device):
    """Per-device arrival tickets of the in-launch two-way split-K combine (gvl.h ABI v5):
    zero-filled once; every GEMM call leaves them zero again."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    t = _TK.get(key)
    if t is None:
        t = torch.zeros(GEMM_TICKETS, dtype=torch.int32, device=device)
        _TK[key] = t
    return t


# ------------------------------------------------------------- device dropout offset
_SEED_OFF = {}


def seed_offset(device):
    """Per-device int64 step offset that re-keys every dropout seed on the device
    (include/gvl.h: seed_eff).  It stays 0 in eager use; gvl.graph advances it once per
    replay of a captured step so frozen host seeds still draw fresh masks."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    t = _SEED_OFF.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int64, device=device)
        _SEED_OFF[key] = t
    return t


# ------------------------------------------------------------------------------- GEMM
def _fill_desc(d, who, a, b, out, a_mn, b_mn, out_dtype=None):
    """Operand checks and the operand fields of GemmDesc d.  out_dtype None: `out` is a given
    bf16 [M, N] result (batched / grouped); else gemm's, allocated here when None.
    Returns (out, M, N, K)."""
    _dev(a, b)
    _rowmajor(a, "A")
    _rowmajor(b, "B")
    given = out_dtype is None
    if given:
        _rowmajor(out, "C")
    if a.dtype != BF16 or b.dtype != BF16 or (given and out.dtype != BF16):
        raise TypeError(f"gvl.{who}: operands must be bf16")
    M, K = (a.shape[1], a.shape[0]) if a_mn else (a.shape[0], a.shape[1])
    N, Kb = (b.shape[1], b.shape[0]) if b_mn else (b.shape[0], b.shape[1])
    if given:
        if K != Kb or tuple(out.shape) != (M, N):
            raise ValueError(f"gvl.{who}: shape mismatch")
    else:
        if K != Kb:
            raise ValueError(f"gvl.{who}: inner dims differ ({K} vs {Kb})")
        if out is None:
            out = torch.empty(M, N, dtype=out_dtype, device=a.device)
        _rowmajor(out, "C")
    d.a, d.b, d.c = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.m, d.n, d.k = M, N, K
    d.lda, d.ldb, d.ldc = a.stride(0), b.stride(0), out.stride(0)
    d.a_mn, d.b_mn = int(a_mn), int(b_mn)
    return out, M, N, K


def _batched_name():
    buf = C.create_string_buffer(128)
    _L().gvl_gemm_batched_kernel_name(buf, 128)
    return buf.value.decode()  # "" after a per-problem fallback


def _launch(call, name, flops, markers=False):
    """Runs call() -> True when it launched.  With a KernelTimer set: arms the launch events
    (dispatch mode; disarmed in `finally`) or, where `markers` allows it, records two stream
    markers around the call, then appends the record (name(), e0, e1, flops()) of what launched."""
    if _timer is None or not (_timer.dispatch or markers):
        return call()
    dispatch = _timer.dispatch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    if dispatch:
        e1.record()  # materialise both hipEvents; the launch re-records them
        _L().gvl_set_launch_events(C.c_void_p(e0.cuda_event), C.c_void_p(e1.cuda_event))
    try:
        ok = call()
    finally:
        if dispatch:
            _L().gvl_set_launch_events(None, None)
    if not dispatch:
        e1.record()
    kernel = name() if ok else ""
    if kernel:
        _timer.records.append((kernel, e0, e1, flops()))
    return ok


def gemm(a, b, *, a_mn=False, b_mn=False, out=None, alpha=1.0, alpha_ptr=None, bias=None,
         act=0, dact=0, pre_out=None, pre_in=None, residual=None, gate=None, drop_p=0.0,
         seed=0, seed_ptr=None, out_dtype=BF16):
    """C = epi(alpha * opA @ opB).  a: [M,K] (a_mn=False) or [K,M]; b: [N,K] (b_mn=False,
    nn.Linear weight) or [K,N].  Returns C [M,N]."""
    d = GemmDesc()
    out, M, N, K = _fill_desc(d, "gemm", a, b, out, a_mn, b_mn, out_dtype)
    d.alpha = float(alpha)
    d.alpha_ptr = _p(alpha_ptr)
    d.bias = _p(bias)
    d.act, d.dact = int(act), int(dact)
    d.pre_out = _p(pre_out)
    d.pre_in = _p(pre_in)
    pre = pre_out if pre_out is not None else pre_in
    d.ldp = pre.stride(0) if pre is not None else 0
    d.residual = _p(residual)
    d.ldr = residual.stride(0) if residual is not None else 0
    d.gate = _p(gate)
    d.drop_p = float(drop_p)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.seed_ptr = _p(seed_ptr)
    d.c_fp32 = int(out.dtype == F32)
    ws = _gemm_workspace(a.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    tk = _gemm_tickets(a.device)
    d.tickets, d.ticket_count = tk.data_ptr(), tk.numel()

    def call():
        _lib.check(_L().gvl_gemm(C.byref(d), _stream()), "gvl_gemm")
        return True

    def name():
        buf = C.create_string_buffer(128)
        _L().gvl_gemm_kernel_name(C.byref(d), buf, 128)
        return buf.value.decode()

    _launch(call, name, lambda: 2.0 * M * N * K, markers=True)
    return out


def linear(x2, w, bias=None, **kw):
    """y = x2 @ w.T (+bias) — nn.Linear forward on a [rows, in] view."""
    return gemm(x2, w, bias=bias, **kw)


def linear_dx(dy2, w, **kw):
    """dx = dy2 @ w — nn.Linear input gradient (w stored [out, in] is MN-major here)."""
    return gemm(dy2, w, b_mn=True, **kw)


def linear_dw(dy2, x2, **kw):
    """dW = dy2.T @ x2 — nn.Linear weight gradient ([out, in])."""
    return gemm(dy2, x2, a_mn=True, b_mn=True, **kw)


# ------------------------------------------------------- int8 weight-only decoding
I8 = torch.int8
LINEAR_W8_MAX_ROWS = _lib.LINEAR_W8_MAX_ROWS


def quantize_rows_i8(w, q=None, scale=None):
    """bf16 w [N, K] -> (int8 q [N, K], fp32 scale [N]): per-row symmetric int8 (gvl.h).  K and
    the row strides multiples of 8."""
    _dev(w, q, scale)
    _rowmajor(w, "w")
    if w.dtype != BF16:
        raise TypeError("gvl.quantize_rows_i8: w must be bf16")
    N, K = w.shape
    if q is None:
        q = torch.empty(N, K, dtype=I8, device=w.device)
    if scale is None:
        scale = torch.empty(N, dtype=F32, device=w.device)
    _rowmajor(q, "q")
    if q.dtype != I8 or scale.dtype != F32 or tuple(q.shape) != (N, K) or \
            tuple(scale.shape) != (N,) or not scale.is_contiguous():
        raise ValueError("gvl.quantize_rows_i8: q must be int8 [N, K], scale contiguous fp32 [N]")
    _lib.check(_L().gvl_quantize_rows_i8(w.data_ptr(), w.stride(0), N, K, q.data_ptr(),
                                         q.stride(0), scale.data_ptr(), _stream()),
               "gvl_quantize_rows_i8")
    return q, scale


def dequantize_rows_i8(q, scale, out=None):
    """int8 q [N, K], fp32 scale [N] -> bf16 [N, K] = bf16(fp32(q) * scale[n])."""
    _dev(q, scale, out)
    _rowmajor(q, "q")
    N, K = q.shape
    if q.dtype != I8 or scale.dtype != F32 or tuple(scale.shape) != (N,) or \
            not scale.is_contiguous():
        raise ValueError("gvl.dequantize_rows_i8: q must be int8 [N, K], scale contiguous fp32 [N]")
    if out is None:
        out = torch.empty(N, K, dtype=BF16, device=q.device)
    _rowmajor(out, "out")
    if out.dtype != BF16 or tuple(out.shape) != (N, K):
        raise ValueError("gvl.dequantize_rows_i8: out must be bf16 [N, K]")
    _lib.check(_L().gvl_dequantize_rows_i8(q.data_ptr(), q.stride(0), scale.data_ptr(), N, K,
                                           out.data_ptr(), out.stride(0), _stream()),
               "gvl_dequantize_rows_i8")
    return out


def linear_w8(x2, w, scale=None, bias=None, act=0, residual=None, gate=None, out=None):
    """y = epi(scale * (x2 @ w.T)) on the kernel for a few rows (gvl_linear_w8): x2 bf16 [M, K],
    M <= LINEAR_W8_MAX_ROWS; w int8 [N, K] with scale fp32 [N], or (scale None) a bf16 [N, K]
    weight through the same kernel.  Epilogues: plain, bias, bias + act 1, bias + residual,
    bias + gate + residual.  Returns y bf16 [M, N]."""
    _dev(x2, w, scale, bias, residual, gate, out)
    _rowmajor(x2, "x")
    _rowmajor(w, "w")
    if x2.dtype != BF16 or w.dtype != (BF16 if scale is None else I8):
        raise TypeError("gvl.linear_w8: x must be bf16, w int8 with a scale or bf16 without")
    M, K = x2.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gvl.linear_w8: inner dims differ ({K} vs {w.shape[1]})")
    if scale is not None and (scale.dtype != F32 or tuple(scale.shape) != (N,) or
                              not scale.is_contiguous()):
        raise ValueError("gvl.linear_w8: scale must be contiguous fp32 [N]")
    if bias is not None and (bias.dtype != BF16 or tuple(bias.shape) != (N,) or
                             not bias.is_contiguous()):
        raise ValueError("gvl.linear_w8: bias must be contiguous bf16 [N]")
    if gate is not None and (gate.dtype != BF16 or gate.numel() != 1):
        raise ValueError("gvl.linear_w8: gate must be one bf16 value")
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=x2.device)
    _rowmajor(out, "out")
    if out.dtype != BF16 or tuple(out.shape) != (M, N):
        raise ValueError("gvl.linear_w8: out must be bf16 [M, N]")
    if residual is not None:
        _rowmajor(residual, "residual")
        if residual.dtype != BF16 or tuple(residual.shape) != (M, N):
            raise ValueError("gvl.linear_w8: residual must be bf16 [M, N]")
    d = _lib.LinearW8Desc()
    d.x, d.w, d.scale, d.c = x2.data_ptr(), w.data_ptr(), _p(scale), out.data_ptr()
    d.m, d.n, d.k = M, N, K
    d.ldx, d.ldw, d.ldc = x2.stride(0), w.stride(0), out.stride(0)
    d.bias, d.act = _p(bias), int(act)
    d.residual = _p(residual)
    d.ldr = residual.stride(0) if residual is not None else 0
    d.gate = _p(gate)
    _lib.check(_L().gvl_linear_w8(C.byref(d), _stream()), "gvl_linear_w8")
    return out


def gemm_batched(items, *, a_mn=False, b_mn=False, dbias=None):
    """items: [(a, b, out, accumulate)] of one shape and layout: out (+)= op(a) @ op(b) for
    every item as ONE persistent launch (gvl_gemm_batched; falls back to one launch each
    when the library cannot batch them).  dbias (weight gradients only: a_mn = b_mn, every
    item accumulating): bf16 [M] bias grads, dbias[i] += column sums of items[i]'s dY, fused
    into the same launch (gvl_gemm_batched_dbias); returns False (nothing launched) when the
    batch cannot run fused."""
    n = len(items)
    if n == 0:
        return
    arr = (GemmDesc * n)()
    ws = None
    for i, (a, b, out, acc) in enumerate(items):
        d = arr[i]
        _fill_desc(d, "gemm_batched", a, b, out, a_mn, b_mn)
        d.alpha = 1.0
        if acc:
            d.residual, d.ldr = out.data_ptr(), out.stride(0)
        if ws is None:
            ws = _gemm_workspace(a.device)
            tk = _gemm_tickets(a.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        # the library may split a batch that underfills the chip in two
        d.tickets, d.ticket_count = tk.data_ptr(), tk.numel()

    def call():
        if dbias is None:
            _lib.check(_L().gvl_gemm_batched(arr, n, _stream()), "gvl_gemm_batched")
            return True
        for t in dbias:
            if t.dtype != BF16 or not t.is_contiguous():
                raise ValueError("gvl.gemm_batched: dbias must be contiguous bf16")
        da = (C.c_void_p * n)(*[t.data_ptr() for t in dbias])
        rc = _L().gvl_gemm_batched_dbias(arr, da, n, _stream())
        if rc not in (0, -1):  # -1: nothing launched, the caller runs the unfused pair
            _lib.check(rc, "gvl_gemm_batched_dbias")
        return rc == 0

    # (timed only by its own dispatch; no record after the per-problem fallback)
    return _launch(call, _batched_name, lambda: sum(2.0 * d.m * d.n * d.k for d in arr))


def gemm_grouped(items, dbias=None):
    """Weight gradients of different shapes as ONE launch (gvl_gemm_grouped): items =
    [(dy, x, out)], out += dy^T @ x (dy [K_i, M_i], x [K_i, N_i], out [M_i, N_i], bf16,
    MN-contiguous operands); an item may carry a 4th element, an fp32 device scalar (or None)
    its product is scaled by (ABI v11: one such tensor per call); dbias: None or a list with a
    bf16 [M_i] bias grad or None per item, += column sums of dy_i.  Returns False when nothing
    was launched (the caller runs the problems another way)."""
    n = len(items)
    if n == 0:
        return True
    arr = (GemmDesc * n)()
    for i, it in enumerate(items):
        a, b, out = it[:3]
        ap = it[3] if len(it) > 3 else None
        if ap is not None and (ap.dtype != torch.float32 or not ap.is_cuda):
            raise TypeError("gvl.gemm_grouped: alpha_ptr must be an fp32 device tensor")
        d = arr[i]
        _fill_desc(d, "gemm_grouped", a, b, out, True, True)
        d.alpha = 1.0
        d.alpha_ptr = _p(ap)
        d.residual, d.ldr = out.data_ptr(), out.stride(0)
    da = None
    if dbias is not None:
        for t in dbias:
            if t is not None and (t.dtype != BF16 or not t.is_contiguous()):
                raise ValueError("gvl.gemm_grouped: dbias must be contiguous bf16")
        da = (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in dbias])

    def call():
        rc = _L().gvl_gemm_grouped(arr, da, n, _stream())
        if rc not in (0, -1):
            _lib.check(rc, "gvl_gemm_grouped")
        return rc == 0

    return _launch(call, _batched_name, lambda: sum(2.0 * d.m * d.n * d.k for d in arr))


# ------------------------------------------------------------------------- LayerNorm
# Rows of up to LN_NARROW_COLS columns run the original entry points; wider ones (GPT-2 large /
# XL, up to 2048 columns) their *_wide forms.
LN_NARROW_COLS = 1024


def layernorm_fwd(x2, w, b, eps=1e-5, out=None, stats=True):
    _dev(x2)
    _rowmajor(x2, "x")
    rows, cols = x2.shape
    if out is None:
        out = torch.empty(rows, cols, dtype=BF16, device=x2.device)
    mean = torch.empty(rows, dtype=F32, device=x2.device) if stats else None
    rstd = torch.empty(rows, dtype=F32, device=x2.device) if stats else None
    name = "gvl_layernorm_fwd" if cols <= LN_NARROW_COLS else "gvl_layernorm_fwd_wide"
    _lib.check(getattr(_L(), name)(x2.data_ptr(), x2.stride(0), w.data_ptr(), b.data_ptr(),
                                   out.data_ptr(), out.stride(0), _p(mean), _p(rstd), rows, cols,
                                   float(eps), _stream()), name)
    return out, mean, rstd


def layernorm_bwd(dy2, x2, w, mean, rstd, dx=None, accumulate_dx=False, dw=None, db=None,
                  accumulate_wb=False, residual=None, defer_wb=False):
    """dx [= dx | residual] + LayerNorm backward; `residual` (a [rows, cols] bf16 operand read
    instead of dx, gvl_layernorm_bwd_res) saves the caller a copy of the residual gradient.
    defer_wb (ABI v12): the dw / db column sums are left as per-block partials; returns
    (dx, (workspace, blocks)) for a later layernorm_finalize_batched."""
    rows, cols = x2.shape
    if dx is None:
        dx = torch.empty(rows, cols, dtype=BF16, device=x2.device)
    ws = None
    if dw is not None or db is not None or defer_wb:
        n = _L().gvl_layernorm_bwd_workspace_size(rows, cols)
        ws = torch.empty(max(n, 4) // 4, dtype=F32, device=x2.device)
    if defer_wb:
        dw = db = None
        accumulate_wb = 2
    if cols > LN_NARROW_COLS:
        _lib.check(_L().gvl_layernorm_bwd_wide(
            dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0), w.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), _p(residual),
            residual.stride(0) if residual is not None else 0, dx.data_ptr(), dx.stride(0),
            int(accumulate_dx or residual is not None), _p(dw), _p(db), int(accumulate_wb), _p(ws),
            rows, cols, _stream()), "gvl_layernorm_bwd_wide")
    elif residual is not None:
        _lib.check(_L().gvl_layernorm_bwd_res(
            dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0), w.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), residual.data_ptr(), residual.stride(0),
            dx.data_ptr(), dx.stride(0), _p(dw), _p(db), int(accumulate_wb), _p(ws), rows, cols,
            _stream()), "gvl_layernorm_bwd_res")
    else:
        _lib.check(_L().gvl_layernorm_bwd(dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0),
                                          w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                          dx.stride(0), int(accumulate_dx), _p(dw), _p(db),
                                          int(accumulate_wb), _p(ws), rows, cols, _stream()),
                   "gvl_layernorm_bwd")
    if defer_wb:
        return dx, (ws, int(_L().gvl_layernorm_bwd_blocks(rows)))
    return dx


def layernorm_finalize_batched(items, cols, accumulate=True):
    """The deferred LayerNorm weight / bias gradients of one width: items = [(workspace,
    blocks, dw or None, db or None)] from layernorm_bwd(defer_wb=True); one launch per 64."""
    for i in range(0, len(items), 64):
        chunk = items[i:i + 64]
        n = len(chunk)
        ws = (C.c_void_p * n)(*[t[0].data_ptr() for t in chunk])
        nb = (C.c_int32 * n)(*[t[1] for t in chunk])
        dw = (C.c_void_p * n)(*[_p(t[2]) for t in chunk])
        db = (C.c_void_p * n)(*[_p(t[3]) for t in chunk])
        name = "gvl_layernorm_bwd_finalize_batched" + ("" if cols <= LN_NARROW_COLS else "_wide")
        _lib.check(getattr(_L(), name)(ws, nb, n, int(cols), dw, db, int(bool(accumulate)),
                                       _stream()), name)


# ------------------------------------------------------------------------- attention
def _bthd(t, T, H):
    """strides (b, t, h) of a [B, T, *] tensor whose head h occupies cols h*64..h*64+63."""
    return t.stride(0), t.stride(1), 64


def attn_desc(q, k, v, o, lse, B, H, Tq, Tk, causal, scale, drop_p=0.0, seed=0, seed_ptr=None):
    d = AttnDesc()
    d.q, d.k, d.v, d.o, d.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), _p(lse)
    d.B, d.H, d.Tq, d.Tk = B, H, Tq, Tk
    d.q_sb, d.q_st, d.q_sh = q.stride(0), q.stride(1), 64
    d.k_sb, d.k_st, d.k_sh = k.stride(0), k.stride(1), 64
    d.v_sb, d.v_st, d.v_sh = v.stride(0), v.stride(1), 64
    d.o_sb, d.o_st, d.o_sh = o.stride(0), o.stride(1), 64
    d.causal = int(causal)
    d.scale = float(scale)
    d.drop_p = float(drop_p)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.seed_ptr = _p(seed_ptr)
    return d


def attn_fwd(q, k, v, H, causal, scale=None, drop_p=0.0, seed=0, out=None, seed_ptr=None):
    """q: [B,Tq,*] view whose cols h*64.. are head h (e.g. a slice of packed qkv);
    k, v: [B,Tk,*].  Returns (o [B,Tq,H*64] bf16, lse [B,H,Tq] fp32)."""
    _dev(q, k, v)
    for t in (q, k, v):
        if t.dtype != BF16 or t.stride(2) != 1:
            raise ValueError("gvl.attn_fwd: q/k/v must be bf16 with unit last stride")
    B, Tq = q.shape[0], q.shape[1]
    Tk = k.shape[1]
    if scale is None:
        scale = 1.0 / math.sqrt(64)
    if out is None:
        out = torch.empty(B, Tq, H * 64, dtype=BF16, device=q.device)
    lse = torch.empty(B, H, Tq, dtype=F32, device=q.device)
    d = attn_desc(q, k, v, out, lse, B, H, Tq, Tk, causal, scale, drop_p, seed, seed_ptr)
    _lib.check(_L().gvl_attn_fwd(C.byref(d), _stream()), "gvl_attn_fwd")
    return out, lse


def attn_bwd(dout, q, k, v, o, lse, H, causal, dq, dk, dv, scale=None, drop_p=0.0, seed=0,
             seed_ptr=None):
    """Writes dq/dk/dv (views with the layouts of q/k/v)."""
    B, Tq = q.shape[0], q.shape[1]
    Tk = k.shape[1]
    if scale is None:
        scale = 1.0 / math.sqrt(64)
    d = attn_desc(q, k, v, o, lse, B, H, Tq, Tk, causal, scale, drop_p, seed, seed_ptr)
    g = AttnBwdDesc()
    g.dout, g.do_sb, g.do_st, g.do_sh = dout.data_ptr(), dout.stride(0), dout.stride(1), 64
    g.dq, g.dq_sb, g.dq_st, g.dq_sh = dq.data_ptr(), dq.stride(0), dq.stride(1), 64
    g.dk, g.dk_sb, g.dk_st, g.dk_sh = dk.data_ptr(), dk.stride(0), dk.stride(1), 64
    g.dv, g.dv_sb, g.dv_st, g.dv_sh = dv.data_ptr(), dv.stride(0), dv.stride(1), 64
    n = _L().gvl_attn_bwd_workspace_size(C.byref(d))
    ws = torch.empty(max(n, 4) // 4, dtype=F32, device=q.device)
    g.workspace = ws.data_ptr()
    _lib.check(_L().gvl_attn_bwd(C.byref(d), C.byref(g), _stream()), "gvl_attn_bwd")


_DECODE_SCALE = 1.0 / math.sqrt(64)


def _attn_decode_cached(name, q, k, v, H, src, gap, out, scale):
    """The checks, the allocation, the default scale and the call that attn_decode,
    attn_decode_beam and attn_decode_ragged share; name is the entry point of include/gvl.h,
    src its table or None, gap its (gap_lo, gap_hi) or None."""
    _dev(q, k, v, src, gap[0] if gap else None)
    R, Tk = q.shape[0], k.shape[1]
    tail = ()
    if gap is not None:
        gap_lo, gap_hi = gap[0], int(gap[1])
        if (gap_lo.dtype != torch.int32 or gap_lo.dim() != 1 or gap_lo.numel() != R or
                not gap_lo.is_contiguous()):
            raise ValueError("gvl: gap_lo must be a contiguous int32 [rows of q] vector")
        if not 0 <= gap_hi <= Tk:
            raise ValueError(f"gvl: gap_hi = {gap_hi} outside 0..Tk = {Tk}")
        tail = (gap_lo.data_ptr(), gap_hi)
    if src is not None:
        _rowmajor(src, "src")
        if src.dtype != torch.int32 or src.shape[0] != R:
            raise ValueError("gvl: src must be an int32 [rows of q, >= Tk] table")
        if k.shape[0] > R or v.shape[0] > R:
            raise ValueError("gvl: the cache has more rows than q; src could not name them")
    elif gap is None:
        R = k.shape[0]  # attn_decode: one sequence per cache row
    elif k.shape[0] != R or v.shape[0] != R:
        raise ValueError("gvl: without src the cache must have one row per row of q")
    if name != "gvl_attn_decode":
        tail = (_p(src), 0 if src is None else src.stride(0)) + tail
    if out is None:
        out = torch.empty(R, H * 64, dtype=BF16, device=q.device)
    if scale is None:
        scale = _DECODE_SCALE
    _lib.check(getattr(_L(), name)(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0),
                                   k.stride(1), v.data_ptr(), v.stride(0), v.stride(1),
                                   out.data_ptr(), out.stride(0), R, H, Tk, float(scale), *tail,
                                   _stream()), name)
    return out


def attn_decode(q, k, v, H, out=None, scale=None):
    """One new query per sequence over a KV cache: q [B, *] (head h at cols h*64..), k/v
    [B, Tk, *] strided views (e.g. slices of a packed [B, Tmax, 3C] cache).  -> o [B, H*64]."""
    return _attn_decode_cached("gvl_attn_decode", q, k, v, H, None, None, out, scale)


def attn_decode_beam(q, k, v, H, src, out=None, scale=None):
    """attn_decode with cache indirection (include/gvl.h gvl_attn_decode_beam): sequence r
    reads position t from cache row src[r, t].  q [R, *]; k/v [rows, Tk, *] strided views of the
    physical cache; src int32 [R, >= Tk] with entries in [0, R).  -> o [R, H*64]."""
    return _attn_decode_cached("gvl_attn_decode_beam", q, k, v, H, src, None, out, scale)


def attn_decode_ragged(q, k, v, H, gap_lo, gap_hi, src=None, out=None, scale=None):
    """attn_decode (src None) or attn_decode_beam (src given) that leaves out the keys
    [gap_lo[r], gap_hi) of sequence r (include/gvl.h gvl_attn_decode_ragged): the pad columns
    of a batch of right-padded prompts in a time-aligned cache.  gap_lo int32 [rows of q] on the
    device; 0 <= gap_hi <= Tk.  -> o [rows of q, H*64]."""
    return _attn_decode_cached("gvl_attn_decode_ragged", q, k, v, H, src, (gap_lo, gap_hi), out,
                               scale)


def _i32_vec(t, rows, name):
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != rows or not t.is_contiguous():
        raise ValueError(f"gvl: {name} must be a contiguous int32 [{rows}] vector")


def _ld(t):
    """Row stride of a row-major [rows, cols] tensor (one row: torch may report any)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def attn_decode_multi(qkv, cache, kv_len, H, out=None, scale=None):
    """Q new queries per sequence at per-sequence cache lengths, the K/V append fused
    (include/gvl.h gvl_attn_decode_multi).  qkv bf16 [B, Q, 3C] contiguous (this step's c_attn
    output, C = H*64); cache bf16 [B, Tmax, 3C] with contiguous rows; kv_len int32 [B] on the
    device.  Query j of sequence b attends positions [0, kv_len[b] + j] and its k / v land in
    cache[b, kv_len[b] + j].  -> o [B*Q, C]."""
    _dev(qkv, cache, kv_len)
    if qkv.dim() != 3 or cache.dim() != 3:
        raise ValueError("gvl: attn_decode_multi takes qkv [B, Q, 3C] and cache [B, Tmax, 3C]")
    B, Q, C3 = qkv.shape
    C = H * 64
    if qkv.dtype != BF16 or cache.dtype != BF16 or C3 != 3 * C or not qkv.is_contiguous():
        raise ValueError("gvl: qkv must be a contiguous bf16 [B, Q, 3 * H * 64] tensor")
    if (cache.shape[0] != B or cache.shape[2] != C3 or cache.stride(2) != 1 or
            cache.stride(1) != C3):
        raise ValueError("gvl: cache must be [B, Tmax, 3C] with contiguous rows")
    _i32_vec(kv_len, B, "kv_len")
    if out is None:
        out = torch.empty(B * Q, C, dtype=BF16, device=qkv.device)
    elif out.dtype != BF16 or out.shape != (B * Q, C) or out.stride(1) != 1:
        raise ValueError("gvl: attn_decode_multi writes a bf16 [B*Q, C] row-major tensor")
    if scale is None:
        scale = _DECODE_SCALE
    _lib.check(_L().gvl_attn_decode_multi(qkv.data_ptr(), cache.data_ptr(), cache.stride(0),
                                          cache.shape[1], kv_len.data_ptr(), out.data_ptr(),
                                          out.stride(0), B, H, Q, float(scale), _stream()),
               "gvl_attn_decode_multi")
    return out


def _dev_scalar(t, name):
    if t.dtype != torch.int32 or t.numel() != 1:
        raise ValueError(f"gvl: {name} must be one int32 on the device")


def attn_decode_step(qkv, cache, t, H, src=None, gap_lo=None, gap_hi=0, out=None, scale=None):
    """One new query per sequence with the K/V append fused and the column read on the device
    (include/gvl.h gvl_attn_decode_step).  qkv bf16 [R, 3C] contiguous (this step's c_attn output,
    C = H*64); cache bf16 [R, Tmax, 3C] with contiguous rows; t one int32 on the device: sequence r
    attends positions [0, t] and its k / v land in cache[r, t].  src int32 [R, >= Tmax]: the cache
    row of every earlier position (attn_decode_beam); gap_lo int32 [R], gap_hi: the skipped range
    (attn_decode_ragged).  -> o [R, C]."""
    _dev(qkv, cache, t, src, gap_lo)
    if qkv.dim() != 2 or cache.dim() != 3:
        raise ValueError("gvl: attn_decode_step takes qkv [R, 3C] and cache [R, Tmax, 3C]")
    R, C3 = qkv.shape
    C = H * 64
    if qkv.dtype != BF16 or cache.dtype != BF16 or C3 != 3 * C or not qkv.is_contiguous():
        raise ValueError("gvl: qkv must be a contiguous bf16 [R, 3 * H * 64] tensor")
    if (cache.shape[0] != R or cache.shape[2] != C3 or cache.stride(2) != 1 or
            cache.stride(1) != C3):
        raise ValueError("gvl: cache must be [R, Tmax, 3C] with contiguous rows")
    Tmax = cache.shape[1]
    _dev_scalar(t, "t")
    if src is not None:
        _rowmajor(src, "src")
        if src.dtype != torch.int32 or src.shape[0] != R or src.shape[1] < Tmax:
            raise ValueError("gvl: src must be an int32 [R, >= Tmax] table")
    if gap_lo is not None:
        _i32_vec(gap_lo, R, "gap_lo")
        if not 0 <= int(gap_hi) <= Tmax:
            raise ValueError(f"gvl: gap_hi = {gap_hi} outside 0..Tmax = {Tmax}")
    if out is None:
        out = torch.empty(R, C, dtype=BF16, device=qkv.device)
    elif out.dtype != BF16 or out.shape != (R, C) or out.stride(1) != 1:
        raise ValueError("gvl: attn_decode_step writes a bf16 [R, C] row-major tensor")
    if scale is None:
        scale = _DECODE_SCALE
    _lib.check(_L().gvl_attn_decode_step(qkv.data_ptr(), cache.data_ptr(), cache.stride(0), Tmax,
                                         t.data_ptr(), out.data_ptr(), _ld(out), R, H, float(scale),
                                         _p(src), 0 if src is None else _ld(src), _p(gap_lo),
                                         int(gap_hi) if gap_lo is not None else 0, _stream()),
               "gvl_attn_decode_step")
    return out


def _kv8_pair(kv8, kvs, rows, H, who):
    """The checks an int8 cache pair shares: kv8 int8 [rows, Tmax, 2C] and kvs fp32
    [rows, Tmax, 2H] with contiguous [Tmax, .] rows (the sequence strides are free).  -> Tmax"""
    C = H * 64
    if kv8.dim() != 3 or kvs.dim() != 3 or kv8.dtype != I8 or kvs.dtype != F32:
        raise ValueError(f"gvl: {who} takes kv8 int8 [rows, Tmax, 2C] and kvs fp32 [rows, Tmax, 2H]")
    Tmax = kv8.shape[1]
    if (tuple(kv8.shape) != (rows, Tmax, 2 * C) or tuple(kvs.shape) != (rows, Tmax, 2 * H) or
            kv8.stride(2) != 1 or kvs.stride(2) != 1 or kv8.stride(1) != 2 * C or
            kvs.stride(1) != 2 * H):
        raise ValueError(f"gvl: {who}: kv8 must be [{rows}, Tmax, {2 * C}] and kvs "
                         f"[{rows}, Tmax, {2 * H}] with contiguous rows")
    return Tmax


def _sb(t, row_elems):
    """Sequence stride of a [rows, T, cols] tensor (one sequence: torch may report any)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), row_elems)


def kv_quantize_i8(qkv, kv8, kvs, H, col0=0):
    """Quantise the k and v thirds of qkv bf16 [B, S, 3C] (a c_attn output, C = H*64; any
    sequence / position strides) into columns [col0, col0 + S) of an int8 cache pair
    (include/gvl.h gvl_kv_quantize_i8): kv8 int8 [B, Tmax, 2C], kvs fp32 [B, Tmax, 2H]."""
    _dev(qkv, kv8, kvs)
    C = H * 64
    if qkv.dim() != 3 or qkv.dtype != BF16 or qkv.shape[2] != 3 * C or qkv.stride(2) != 1:
        raise ValueError("gvl: kv_quantize_i8 takes qkv bf16 [B, S, 3 * H * 64] with contiguous rows")
    B, S, _ = qkv.shape
    Tmax = _kv8_pair(kv8, kvs, B, H, "kv_quantize_i8")
    col0 = int(col0)
    if not 0 <= col0 <= Tmax - S:
        raise ValueError(f"gvl: col0 = {col0} + S = {S} outside the cache's {Tmax} columns")
    st = qkv.stride(1) if S > 1 else max(qkv.stride(1), 3 * C)
    _lib.check(_L().gvl_kv_quantize_i8(qkv.data_ptr(), _sb(qkv, S * st), st, kv8.data_ptr(),
                                       _sb(kv8, Tmax * 2 * C), kvs.data_ptr(),
                                       _sb(kvs, Tmax * 2 * H), B, S, H, col0, _stream()),
               "gvl_kv_quantize_i8")
    return kv8, kvs


def attn_decode_q8(qkv, kv8, kvs, t, H, src=None, gap_lo=None, gap_hi=0, out=None, scale=None):
    """One new query per sequence over an int8 cache pair, the quantising append fused
    (include/gvl.h gvl_attn_decode_q8).  qkv bf16 [R, 3C] contiguous (this step's c_attn output);
    kv8 int8 [R, Tmax, 2C], kvs fp32 [R, Tmax, 2H]; t: the column of the step, a Python int or one
    int32 on the device (graph replay).  Sequence r attends positions [0, t], every one as
    fp32(q8) * scale, and its quantised k / v land in column t.  src, gap_lo, gap_hi: as in
    attn_decode_step.  -> o [R, C]."""
    t_dev = t if isinstance(t, torch.Tensor) else None
    _dev(qkv, kv8, kvs, t_dev, src, gap_lo)
    if qkv.dim() != 2:
        raise ValueError("gvl: attn_decode_q8 takes qkv [R, 3C]")
    R, C3 = qkv.shape
    C = H * 64
    if qkv.dtype != BF16 or C3 != 3 * C or not qkv.is_contiguous():
        raise ValueError("gvl: qkv must be a contiguous bf16 [R, 3 * H * 64] tensor")
    Tmax = _kv8_pair(kv8, kvs, R, H, "attn_decode_q8")
    if t_dev is not None:
        _dev_scalar(t_dev, "t")
    if src is not None:
        _rowmajor(src, "src")
        if src.dtype != torch.int32 or src.shape[0] != R or src.shape[1] < Tmax:
            raise ValueError("gvl: src must be an int32 [R, >= Tmax] table")
    if gap_lo is not None:
        _i32_vec(gap_lo, R, "gap_lo")
        if not 0 <= int(gap_hi) <= Tmax:
            raise ValueError(f"gvl: gap_hi = {gap_hi} outside 0..Tmax = {Tmax}")
    if out is None:
        out = torch.empty(R, C, dtype=BF16, device=qkv.device)
    elif out.dtype != BF16 or out.shape != (R, C) or out.stride(1) != 1:
        raise ValueError("gvl: attn_decode_q8 writes a bf16 [R, C] row-major tensor")
    if scale is None:
        scale = _DECODE_SCALE
    _lib.check(_L().gvl_attn_decode_q8(qkv.data_ptr(), kv8.data_ptr(), _sb(kv8, Tmax * 2 * C),
                                       kvs.data_ptr(), _sb(kvs, Tmax * 2 * H), Tmax,
                                       0 if t_dev is not None else int(t), _p(t_dev),
                                       out.data_ptr(), _ld(out), R, H, float(scale), _p(src),
                                       0 if src is None else _ld(src), _p(gap_lo),
                                       int(gap_hi) if gap_lo is not None else 0, _stream()),
               "gvl_attn_decode_q8")
    return out


def ngram_draft(prompt, plen, emitted, n, ngram, D, given=None, out=None):
    """Prompt-lookup draft (include/gvl.h gvl_ngram_draft): prompt int64 [B, P], plen int32 [B],
    emitted int64 [B, n_new] of which row b holds n[b] tokens (n int32 [B]), given optional int64
    [B, n_new] (-1: none).  -> draft int64 [B, D], -1 where there is no guess."""
    _dev(prompt, plen, emitted, n, given)
    _rowmajor(prompt, "prompt")
    _rowmajor(emitted, "emitted")
    B, P = prompt.shape
    n_new = emitted.shape[1]
    if prompt.dtype != torch.int64 or emitted.dtype != torch.int64 or emitted.shape[0] != B:
        raise ValueError("gvl: ngram_draft takes int64 prompt [B, P] and emitted [B, n_new]")
    _i32_vec(plen, B, "plen")
    _i32_vec(n, B, "n")
    if given is not None:
        _rowmajor(given, "given")
        if given.dtype != torch.int64 or given.shape != (B, n_new):
            raise ValueError("gvl: given must be an int64 [B, n_new] tensor")
    if out is None:
        out = torch.empty(B, int(D), dtype=torch.int64, device=prompt.device)
    elif out.dtype != torch.int64 or out.shape != (B, int(D)) or not out.is_contiguous():
        raise ValueError("gvl: ngram_draft writes a contiguous int64 [B, D] tensor")
    _lib.check(_L().gvl_ngram_draft(_p(prompt) if P > 0 else None, _ld(prompt), P,
                                    plen.data_ptr(), emitted.data_ptr(), _ld(emitted),
                                    n.data_ptr(), n_new, _p(given),
                                    0 if given is None else _ld(given), B, int(ngram), int(D),
                                    out.data_ptr(), _stream()), "gvl_ngram_draft")
    return out


def spec_accept(x, draft, n, kv_len, pos, lengths, last, out, eos=None, drafted=None,
                accepted=None):
    """Accept the drafted tokens the chosen ones confirm and advance the per-sequence state, all
    on the device (include/gvl.h gvl_spec_accept).  x int64 [B, Q]; draft int64 [B, Q - 1] (None
    with Q = 1); n, kv_len, pos, lengths int32 [B]; last int64 [B]; out int64 [B, n_new];
    drafted / accepted: optional int32 [B] counters."""
    _dev(x, draft, n, kv_len, pos, lengths, last, out, drafted, accepted)
    if x.dim() != 2 or x.dtype != torch.int64 or not x.is_contiguous():
        raise ValueError("gvl: spec_accept takes a contiguous int64 x [B, Q]")
    B, Q = x.shape
    if Q > 1 and (draft is None or draft.dtype != torch.int64 or draft.shape != (B, Q - 1) or
                  not draft.is_contiguous()):
        raise ValueError("gvl: draft must be a contiguous int64 [B, Q - 1] tensor")
    for t, name in ((n, "n"), (kv_len, "kv_len"), (pos, "pos"), (lengths, "lengths")):
        _i32_vec(t, B, name)
    for t, name in ((drafted, "drafted"), (accepted, "accepted")):
        if t is not None:
            _i32_vec(t, B, name)
    _rowmajor(out, "out")
    if (out.dtype != torch.int64 or out.shape[0] != B or last.dtype != torch.int64 or
            last.numel() != B or not last.is_contiguous()):
        raise ValueError("gvl: spec_accept takes int64 out [B, n_new] and last [B]")
    _lib.check(_L().gvl_spec_accept(x.data_ptr(), _p(draft) if Q > 1 else None, B, Q, n.data_ptr(),
                                    kv_len.data_ptr(), pos.data_ptr(), lengths.data_ptr(),
                                    last.data_ptr(), out.data_ptr(), _ld(out), out.shape[1],
                                    -1 if eos is None else int(eos), _p(drafted), _p(accepted),
                                    _stream()), "gvl_spec_accept")


def beam_step(logits2, score, flen, len_norm, src, K, step, eos, t0, out=None, workspace=None):
    """One beam-search step for B items x K beams (include/gvl.h gvl_beam_step).  logits2
    [B*K, V] bf16 / fp32; score fp32 [B*K]; flen int32 [B*K]; len_norm fp32 [>= step + 2]; src
    int32 [B*K, > t0 + step]; eos None or -1: no end token.  out: (tok int64, parent int32,
    score fp32, flen int32, src int32) to write instead of new tensors; src of `out` must not be
    the input table.  -> that tuple."""
    _dev(logits2, score, flen, len_norm, src)
    _rowmajor(logits2, "logits")
    _rowmajor(src, "src")
    R, V = logits2.shape
    if K < 1 or R % K:
        raise ValueError(f"gvl: {R} logits rows are not B x K = {K} beams")
    if (score.dtype != F32 or flen.dtype != torch.int32 or len_norm.dtype != F32 or
            src.dtype != torch.int32 or logits2.dtype not in (BF16, F32)):
        raise ValueError("gvl: beam_step takes fp32 score / len_norm, int32 flen / src and bf16 "
                         "or fp32 logits")
    if score.numel() != R or flen.numel() != R or src.shape[0] != R or len_norm.numel() < step + 2:
        raise ValueError("gvl: beam_step state does not match the logits rows / step")
    dev = logits2.device
    if out is None:
        out = (torch.empty(R, dtype=torch.int64, device=dev),
               torch.empty(R, dtype=torch.int32, device=dev),
               torch.empty(R, dtype=F32, device=dev),
               torch.empty(R, dtype=torch.int32, device=dev), torch.empty_like(src))
    tok, parent, score_o, flen_o, src_o = out
    if src_o.shape != src.shape or src_o.stride() != src.stride():
        raise ValueError("gvl: the output src table must have the input table's layout")
    nws = _L().gvl_beam_step_workspace_size(R // K, K)
    if workspace is None:
        workspace = torch.empty(max(nws, 8) // 4, dtype=F32, device=dev)
    elif workspace.numel() * workspace.element_size() < nws:
        raise ValueError(f"gvl: beam_step workspace needs {nws} bytes")
    _lib.check(_L().gvl_beam_step(logits2.data_ptr(), logits2.stride(0), int(logits2.dtype == F32),
                                  R // K, K, V, score.data_ptr(), flen.data_ptr(),
                                  len_norm.data_ptr(), int(step), -1 if eos is None else int(eos),
                                  int(t0), src.data_ptr(), src.stride(0), tok.data_ptr(),
                                  parent.data_ptr(), score_o.data_ptr(), flen_o.data_ptr(),
                                  src_o.data_ptr(), workspace.data_ptr(), _stream()),
               "gvl_beam_step")
    return out


def beam_step_dev(logits2, score, flen, len_norm, src, K, step, max_steps, eos, t0, out,
                  workspace):
    """beam_step with the step count read on the device (include/gvl.h gvl_beam_step_dev): step
    one int32 on the device, max_steps its host bound (len_norm fp32 [>= max_steps + 1], src int32
    [B*K, >= t0 + max_steps]); a step outside [0, max_steps) writes nothing.  out and workspace
    are the caller's (a replayed launch cannot allocate).  -> out."""
    _dev(logits2, score, flen, len_norm, src, step, workspace, *out)
    _rowmajor(logits2, "logits")
    _rowmajor(src, "src")
    R, V = logits2.shape
    max_steps = int(max_steps)
    if K < 1 or R % K:
        raise ValueError(f"gvl: {R} logits rows are not B x K = {K} beams")
    if (score.dtype != F32 or flen.dtype != torch.int32 or len_norm.dtype != F32 or
            src.dtype != torch.int32 or logits2.dtype not in (BF16, F32)):
        raise ValueError("gvl: beam_step_dev takes fp32 score / len_norm, int32 flen / src and "
                         "bf16 or fp32 logits")
    _dev_scalar(step, "step")
    if (score.numel() != R or flen.numel() != R or src.shape[0] != R or
            len_norm.numel() < max_steps + 1):
        raise ValueError("gvl: beam_step_dev state does not match the logits rows / max_steps")
    tok, parent, score_o, flen_o, src_o = out
    if src_o.shape != src.shape or src_o.stride() != src.stride():
        raise ValueError("gvl: the output src table must have the input table's layout")
    if (tok.dtype != torch.int64 or parent.dtype != torch.int32 or score_o.dtype != F32 or
            flen_o.dtype != torch.int32 or src_o.dtype != torch.int32 or
            min(tok.numel(), parent.numel(), score_o.numel(), flen_o.numel()) < R):
        raise ValueError("gvl: beam_step_dev writes tok int64, parent int32, score fp32, flen "
                         "int32 [B*K] and src int32")
    nws = _L().gvl_beam_step_workspace_size(R // K, K)
    if workspace.numel() * workspace.element_size() < nws:
        raise ValueError(f"gvl: beam_step workspace needs {nws} bytes")
    _lib.check(_L().gvl_beam_step_dev(logits2.data_ptr(), logits2.stride(0),
                                      int(logits2.dtype == F32), R // K, K, V, score.data_ptr(),
                                      flen.data_ptr(), len_norm.data_ptr(), step.data_ptr(),
                                      max_steps, -1 if eos is None else int(eos), int(t0),
                                      src.data_ptr(), src.stride(0), tok.data_ptr(),
                                      parent.data_ptr(), score_o.data_ptr(), flen_o.data_ptr(),
                                      src_o.data_ptr(), workspace.data_ptr(), _stream()),
               "gvl_beam_step_dev")
    return out


def logits_process_dev(logits2, hist, step, hist_cap, *, src=None, t0=0, prompt=None,
                       rows_per_item=1, repetition_penalty=1.0, no_repeat_ngram_size=0, eos=None,
                       min_new=0, bad_tokens=None, flen=None):
    """logits_process with the step count read on the device (include/gvl.h
    gvl_logits_process_dev): step one int32 on the device, n_hist = clamp(step, 0, hist_cap), eos
    banned while step < min_new.  hist int64 [>= hist_cap, >= R]; src int32
    [R, >= t0 + hist_cap]; the rest as logits_process.  -> logits2."""
    _dev(logits2, hist, step, src, prompt, bad_tokens, flen)
    _rowmajor(logits2, "logits")
    R, V = logits2.shape
    hist_cap = int(hist_cap)
    if logits2.dtype not in (BF16, F32):
        raise ValueError("gvl: logits_process_dev takes bf16 or fp32 logits")
    _dev_scalar(step, "step")
    hist_ld = 0
    if hist_cap > 0:
        if hist is None:
            raise ValueError(f"gvl: logits_process_dev needs hist for hist_cap = {hist_cap}")
        _rowmajor(hist, "hist")
        if hist.dtype != torch.int64 or hist.shape[0] < hist_cap or hist.shape[1] < R:
            raise ValueError("gvl: hist must be an int64 [>= hist_cap, >= rows of logits] tensor")
        hist_ld = hist.stride(0)
    if src is not None:
        _rowmajor(src, "src")
        if src.dtype != torch.int32 or src.shape[0] != R or src.shape[1] < t0 + hist_cap:
            raise ValueError("gvl: src must be an int32 [rows of logits, >= t0 + hist_cap] table")
    P = 0
    if prompt is not None:
        _rowmajor(prompt, "prompt")
        if (prompt.dtype != torch.int64 or rows_per_item < 1 or
                prompt.shape[0] * rows_per_item != R):
            raise ValueError("gvl: prompt must be an int64 [rows of logits / rows_per_item, P] "
                             "tensor")
        P = prompt.shape[1]
    if bad_tokens is not None and (bad_tokens.dtype != torch.int32 or bad_tokens.dim() != 1 or
                                   not bad_tokens.is_contiguous()):
        raise ValueError("gvl: bad_tokens must be a contiguous int32 vector")
    if flen is not None and (flen.dtype != torch.int32 or flen.numel() != R or
                             not flen.is_contiguous()):
        raise ValueError("gvl: flen must be a contiguous int32 [rows of logits] vector")
    n_bad = 0 if bad_tokens is None else bad_tokens.numel()
    _lib.check(_L().gvl_logits_process_dev(
        logits2.data_ptr(), logits2.stride(0), int(logits2.dtype == F32), R, V,
        _p(hist) if hist_cap > 0 else None, hist_ld, step.data_ptr(), hist_cap, _p(src),
        0 if src is None else src.stride(0), int(t0), _p(prompt) if P > 0 else None,
        0 if P == 0 else prompt.stride(0), P, int(rows_per_item), float(repetition_penalty),
        int(no_repeat_ngram_size), -1 if eos is None else int(eos), int(min_new),
        _p(bad_tokens) if n_bad > 0 else None, n_bad, _p(flen), _stream()),
        "gvl_logits_process_dev")
    return logits2


def logits_process(logits2, hist, n_hist, *, src=None, t0=0, prompt=None, rows_per_item=1,
                   repetition_penalty=1.0, no_repeat_ngram_size=0, eos=None, ban_eos=False,
                   bad_tokens=None, flen=None):
    """Repetition penalty, no-repeat n-gram, end-token and bad-token bans on logits2 [R, V] bf16 /
    fp32, in place (include/gvl.h gvl_logits_process).  hist int64 [>= n_hist, >= R]: the
    generated tokens, one step per row (None with n_hist = 0); src int32 [R, >= t0 + n_hist]: the
    beam table a row's history is read through (None: its own column); prompt int64
    [R / rows_per_item, P]; bad_tokens int32 [n]; flen int32 [R]: rows with flen > 0 are left
    alone.  -> logits2."""
    _dev(logits2, hist, src, prompt, bad_tokens, flen)
    _rowmajor(logits2, "logits")
    R, V = logits2.shape
    n_hist = int(n_hist)
    if logits2.dtype not in (BF16, F32):
        raise ValueError("gvl: logits_process takes bf16 or fp32 logits")
    hist_ld = 0
    if n_hist > 0:
        if hist is None:
            raise ValueError(f"gvl: logits_process needs hist for n_hist = {n_hist}")
        _rowmajor(hist, "hist")
        if hist.dtype != torch.int64 or hist.shape[0] < n_hist or hist.shape[1] < R:
            raise ValueError("gvl: hist must be an int64 [>= n_hist, >= rows of logits] tensor")
        hist_ld = hist.stride(0)
    if src is not None:
        _rowmajor(src, "src")
        if src.dtype != torch.int32 or src.shape[0] != R or src.shape[1] < t0 + n_hist:
            raise ValueError("gvl: src must be an int32 [rows of logits, >= t0 + n_hist] table")
    P = 0
    if prompt is not None:
        _rowmajor(prompt, "prompt")
        if (prompt.dtype != torch.int64 or rows_per_item < 1 or
                prompt.shape[0] * rows_per_item != R):
            raise ValueError("gvl: prompt must be an int64 [rows of logits / rows_per_item, P] "
                             "tensor")
        P = prompt.shape[1]
    if bad_tokens is not None and (bad_tokens.dtype != torch.int32 or bad_tokens.dim() != 1 or
                                   not bad_tokens.is_contiguous()):
        raise ValueError("gvl: bad_tokens must be a contiguous int32 vector")
    if flen is not None and (flen.dtype != torch.int32 or flen.numel() != R or
                             not flen.is_contiguous()):
        raise ValueError("gvl: flen must be a contiguous int32 [rows of logits] vector")
    n_bad = 0 if bad_tokens is None else bad_tokens.numel()
    _lib.check(_L().gvl_logits_process(
        logits2.data_ptr(), logits2.stride(0), int(logits2.dtype == F32), R, V,
        _p(hist) if n_hist > 0 else None, hist_ld, n_hist, _p(src),
        0 if src is None else src.stride(0), int(t0), _p(prompt) if P > 0 else None,
        0 if P == 0 else prompt.stride(0), P, int(rows_per_item), float(repetition_penalty),
        int(no_repeat_ngram_size), -1 if eos is None else int(eos), int(bool(ban_eos)),
        _p(bad_tokens) if n_bad > 0 else None, n_bad, _p(flen), _stream()), "gvl_logits_process")
    return logits2


def sample(logits2, u, temperature=1.0, top_k=0, top_p=1.0, out=None):
    """Fused temperature / top-k / top-p draw per row (include/gvl.h gvl_sample); u [rows]
    fp32 uniforms in [0, 1) on the device.  -> int64 [rows]."""
    _dev(logits2, u)
    _rowmajor(logits2, "logits")
    rows, V = logits2.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=logits2.device)
    _lib.check(_L().gvl_sample(logits2.data_ptr(), logits2.stride(0), int(logits2.dtype == F32),
                               rows, V, float(temperature), int(top_k), float(top_p),
                               u.data_ptr(), out.data_ptr(), _stream()), "gvl_sample")
    return out


def _score_out(t, n, dtype, device, name):
    """An optional output of the scoring launchers: True allocates it, None / False leaves it
    out, a tensor (contiguous, n elements of dtype) is written."""
    if t is None or t is False:
        return None
    if t is True:
        return torch.empty(n, dtype=dtype, device=device)
    _dev(t)
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"gvl: {name} must be a contiguous {dtype} tensor of {n} elements")
    return t


def _score_mask(mask, n):
    if mask is None:
        return None
    _dev(mask)
    mk = mask.reshape(-1)
    if mk.dtype != torch.uint8:
        mk = mk.to(torch.uint8)
    if mk.numel() != n:
        raise ValueError(f"gvl: mask must have {n} elements")
    return mk.contiguous()


def token_logprobs(logits2, targets, mask=None, *, vocab=None, logp=True, lse=True, argmax=True,
                   rank=True):
    """Per row of logits2 [rows, >= V] bf16 / fp32 and its target (include/gvl.h
    gvl_token_logprobs): logp = x[t] - lse, lse, argmax (first maximum) and the target's rank (0:
    it is the argmax).  targets int64 [rows] (-100: skipped); mask [rows], 0: skipped; `vocab` <
    logits2.shape[1] marks the trailing columns as padding.  Each output: True allocates it, None
    leaves it out, a tensor is written in place.  -> (logp fp32, lse fp32, argmax int32, rank
    int32), None where left out."""
    _dev(logits2, targets)
    _rowmajor(logits2, "logits")
    if logits2.dtype not in (BF16, F32):
        raise ValueError("gvl: token_logprobs takes bf16 or fp32 logits")
    rows = logits2.shape[0]
    V = logits2.shape[1] if vocab is None else int(vocab)
    if V > logits2.shape[1]:
        raise ValueError(f"gvl: vocab = {V} exceeds the {logits2.shape[1]} logits columns")
    tg = targets.reshape(-1)
    if tg.dtype != torch.int64:
        tg = tg.long()
    tg = tg.contiguous()
    if tg.numel() != rows:
        raise ValueError(f"gvl: {tg.numel()} targets for {rows} logits rows")
    mk = _score_mask(mask, rows)
    dev = logits2.device
    logp = _score_out(logp, rows, F32, dev, "logp")
    lse = _score_out(lse, rows, F32, dev, "lse")
    argmax = _score_out(argmax, rows, torch.int32, dev, "argmax")
    rank = _score_out(rank, rows, torch.int32, dev, "rank")
    _lib.check(_L().gvl_token_logprobs(logits2.data_ptr(), logits2.stride(0),
                                       int(logits2.dtype == F32), rows, V, tg.data_ptr(), _p(mk),
                                       _p(logp), _p(lse), _p(argmax), _p(rank), _stream()),
               "gvl_token_logprobs")
    return logp, lse, argmax, rank


def sequence_score(logp, mask=None, group=1):
    """Per-sequence and per-example reduction of token log-probabilities (include/gvl.h
    gvl_sequence_score).  logp fp32 [N, T]; mask [N, T] of 0 / 1 (None: every position counts);
    `group` consecutive sequences form an example.  -> (sum_nll fp32 [N], count int32 [N],
    mean_nll fp32 [N], pred_norm int32 [N / group], pred int32 [N / group])."""
    _dev(logp)
    if logp.dim() != 2 or logp.dtype != F32:
        raise ValueError("gvl: sequence_score takes fp32 logp [N, T]")
    logp = logp.contiguous()
    N, T = logp.shape
    group = int(group)
    if group < 1 or N % group:
        raise ValueError(f"gvl: group = {group} does not divide the {N} sequences")
    mk = _score_mask(mask, N * T)
    dev = logp.device
    i32 = torch.int32
    out = (torch.empty(N, dtype=F32, device=dev), torch.empty(N, dtype=i32, device=dev),
           torch.empty(N, dtype=F32, device=dev), torch.empty(N // group, dtype=i32, device=dev),
           torch.empty(N // group, dtype=i32, device=dev))
    if N == 0:
        return out
    _lib.check(_L().gvl_sequence_score(logp.data_ptr(), _p(mk), N, T, group,
                                       *[t.data_ptr() for t in out], _stream()),
               "gvl_sequence_score")
    return out


# ---------------------------------------------------------------------- cross entropy
def cross_entropy(logits2, targets, *, rows_per_group=None, group_stride=0, row_offset=0,
                  mask=None, mask_mode=False, want_grad=True, vocab=None, dlogits=None):
    """Returns (loss_and_inv [2] fp32 device tensor, dlogits [rows, V] bf16 or None).
    `vocab` < logits2.shape[1] marks the trailing columns as padding (V % 8 != 0): the kernel
    writes the gradient of columns [0, ceil(vocab / 8) * 8), zero past `vocab`; any further
    padding columns of the returned dlogits are zeroed here, so all of it can feed a GEMM.
    `dlogits`: a caller's [rows, >= ceil(vocab / 8) * 8] bf16 row-major view to write instead
    (only those columns of it are written)."""
    _dev(logits2, targets)
    Vp = logits2.shape[1]
    V = Vp if vocab is None else int(vocab)
    rows = targets.numel()
    if rows_per_group is None:
        rows_per_group = max(rows, 1)
    tg = targets.reshape(-1)
    if tg.dtype != torch.int64:
        tg = tg.long()
    tg = tg.contiguous()
    mk = None
    if mask is not None:
        mk = mask.reshape(-1).to(torch.uint8).contiguous()
    row_loss = torch.empty(max(rows, 1), dtype=F32, device=logits2.device)
    dl = None
    if dlogits is not None:
        _rowmajor(dlogits, "dlogits")
        if dlogits.dtype != BF16 or dlogits.shape[0] != rows:
            raise ValueError("gvl.cross_entropy: dlogits must be bf16 with one row per target")
        dl = dlogits
    elif want_grad:
        dl = torch.empty(rows, Vp, dtype=BF16, device=logits2.device)
        vpad = (V + 7) // 8 * 8
        if Vp > vpad:  # never in the product (pad_vocab pads to 8): the kernel stops at vpad
            dl[:, vpad:].zero_()
    out = torch.empty(2, dtype=F32, device=logits2.device)
    _lib.check(_L().gvl_cross_entropy(logits2.data_ptr(), logits2.stride(0), rows, V,
                                      rows_per_group, group_stride, row_offset, tg.data_ptr(),
                                      _p(mk), int(mask_mode), row_loss.data_ptr(), _p(dl),
                                      dl.stride(0) if dl is not None else 0, out.data_ptr(),
                                      _stream()), "gvl_cross_entropy")
    return out, dl


# -------------------------------------------------------------------------- embedding
def embedding_fwd(idx, wte, wpe, out, T, out_rows_per_seq, out_offset):
    _dev(idx, wte, wpe, out)
    idx = idx.contiguous()
    V, C_ = wte.shape
    _lib.check(_L().gvl_embedding_fwd(idx.data_ptr(), wte.data_ptr(), wpe.data_ptr(),
                                      out.data_ptr(), idx.numel(), T, C_, V, out_rows_per_seq,
                                      out_offset, _stream()), "gvl_embedding_fwd")
    return out


def embedding_fwd_pos(idx, pos, wte, wpe, out=None):
    """out[r] = wte[idx[r]] + wpe[pos[r]] (include/gvl.h gvl_embedding_fwd_pos): idx int64 [n],
    pos int32 [n] on the device, out bf16 [n, C] contiguous.  -> out."""
    _dev(idx, pos, wte, wpe, out)
    n = idx.numel()
    V, C_ = wte.shape
    if idx.dtype != torch.int64 or pos.dtype != torch.int32 or pos.numel() != n:
        raise ValueError("gvl: embedding_fwd_pos takes int64 ids and as many int32 positions")
    if wte.dtype != BF16 or wpe.dtype != BF16 or wpe.shape[1] != C_ or \
            not (wte.is_contiguous() and wpe.is_contiguous()):
        raise ValueError("gvl: embedding_fwd_pos takes contiguous bf16 wte [V, C] and wpe [T, C]")
    if out is None:
        out = torch.empty(n, C_, dtype=BF16, device=idx.device)
    elif out.dtype != BF16 or out.numel() != n * C_ or not out.is_contiguous():
        raise ValueError("gvl: embedding_fwd_pos writes a contiguous bf16 [n, C] tensor")
    idx, pos = idx.contiguous(), pos.contiguous()
    _lib.check(_L().gvl_embedding_fwd_pos(idx.data_ptr(), pos.data_ptr(), wte.data_ptr(),
                                          wpe.data_ptr(), out.data_ptr(), n, C_, V, wpe.shape[0],
                                          _stream()), "gvl_embedding_fwd_pos")
    return out


def embedding_bwd(idx, dout, dwte_acc, dwpe_acc, T, out_rows_per_seq, out_offset, C_, V):
    idx = idx.contiguous()
    _lib.check(_L().gvl_embedding_bwd(idx.data_ptr(), dout.data_ptr(), _p(dwte_acc),
                                      _p(dwpe_acc), idx.numel(), T, C_, V, out_rows_per_seq,
                                      out_offset, _stream()), "gvl_embedding_bwd")


def copy_rows(src, dst, T, G, src_rows, src_off, dst_rows, dst_off, zero_rest=False):
    """Grouped row copy (gvl_copy_rows) between row-major bf16 2-D views: dst row
    (g*dst_rows + dst_off + t) = src row (g*src_rows + src_off + t); zero_rest zeroes the
    other rows of every dst group.  src_rows = 0 broadcasts T rows to all G groups."""
    _dev(src, dst)
    if src.dtype != BF16 or dst.dtype != BF16 or src.stride(-1) != 1 or dst.stride(-1) != 1:
        raise TypeError("gvl.copy_rows: bf16 row-major views expected")
    _lib.check(_L().gvl_copy_rows(src.data_ptr(), src.stride(0), src_rows, src_off,
                                  dst.data_ptr(), dst.stride(0), dst_rows, dst_off, T, G,
                                  dst.shape[-1], int(zero_rest), _stream()), "gvl_copy_rows")
    return dst


_EMB_KEYS = {}


def embedding_bwd_det(idx, dout, dwte, dwpe, T, out_rows_per_seq, out_offset, C_, V):
    """Deterministic embedding backward into bf16 gradients, accumulating in place
    (gvl_embedding_bwd_det): dwte [V, C] += per-id row sums, dwpe [P, C] += per-position sums."""
    _dev(idx, dout)
    idx = idx.contiguous()
    n = idx.numel()
    for t in (dwte, dwpe):
        if t is not None and (t.dtype != BF16 or not t.is_contiguous()):
            raise TypeError("gvl.embedding_bwd_det: gradients must be contiguous bf16")
    keys = None
    if dwte is not None:
        need = int(_L().gvl_embedding_bwd_workspace(n))
        key = (dout.device, torch.cuda.current_stream(dout.device).cuda_stream)
        keys = _EMB_KEYS.get(key)
        if keys is None or keys.numel() < need:
            keys = torch.empty(max(need, 1), dtype=torch.int32, device=dout.device)
            _EMB_KEYS[key] = keys
    _lib.check(_L().gvl_embedding_bwd_det(idx.data_ptr(), dout.data_ptr(), _p(dwte), _p(dwpe), n,
                                          T, C_, V, out_rows_per_seq, out_offset, _p(keys),
                                          0 if keys is None else keys.numel(), _stream()),
               "gvl_embedding_bwd_det")


# ------------------------------------------------------------------------------- pool
def pool_clip(tokens, out_dtype=None, normalize=True):
    """[B, 1+s*s, D] -> [B, 33, D]: CLS + adaptive-avg (4,8) (+ L2 normalise)."""
    _dev(tokens)
    t = tokens.contiguous()
    if t.dtype not in (F32, BF16):
        t = t.float()
    B, L, D = t.shape
    out_dtype = out_dtype or t.dtype
    out = torch.empty(B, 33, D, dtype=out_dtype, device=t.device)
    _lib.check(_L().gvl_pool_clip_ex(t.data_ptr(), int(t.dtype == F32), out.data_ptr(),
                                     int(out_dtype == F32), B, L, D, int(normalize), _stream()),
               "gvl_pool_clip")
    return out


def l2_normalize_rows(x, out=None):
    """F.normalize(x, dim=-1, eps=1e-12) for bf16 / fp32 rows (D <= 1024)."""
    _dev(x)
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    D = x.shape[-1]
    _lib.check(_L().gvl_l2_normalize_rows(x.data_ptr(), out.data_ptr(), int(x.dtype == F32),
                                          x.numel() // D, D, _stream()), "gvl_l2_normalize_rows")
    return out


# ------------------------------------------------------------------------- optimizer
def grad_norm(g_flat, max_norm, out=None):
    _dev(g_flat)
    n = g_flat.numel()
    ws = torch.empty(max(_L().gvl_grad_norm_workspace_size(n), 4) // 4, dtype=F32,
                     device=g_flat.device)
    if out is None:
        out = torch.empty(2, dtype=F32, device=g_flat.device)
    _lib.check(_L().gvl_grad_norm(g_flat.data_ptr(), n, float(max_norm), ws.data_ptr(),
                                  out.data_ptr(), _stream()), "gvl_grad_norm")
    return out


def adamw_dev(p, g, m, v, n_decay, hyper, beta1, beta2, eps, wd, grad_scale=None):
    """AdamW with lr / step read on the device from hyper[0:2] (graph-capturable)."""
    _dev(p, g, m, v, hyper)
    _lib.check(_L().gvl_adamw_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                  p.numel(), int(n_decay), hyper.data_ptr(), float(beta1),
                                  float(beta2), float(eps), float(wd), _p(grad_scale), _stream()),
               "gvl_adamw_dev")


def adamw_master_dev(p, p_master, g, m, v, n_decay, hyper, beta1, beta2, eps, wd,
                     grad_scale=None):
    """Mixed-precision AdamW: fp32 master / moments, bf16 compute copy p (gvl.h)."""
    _dev(p, p_master, g, m, v, hyper)
    if p_master.dtype != F32 or m.dtype != F32 or v.dtype != F32:
        raise TypeError("gvl.adamw_master_dev: master / moments must be fp32")
    _lib.check(_L().gvl_adamw_master_dev(p.data_ptr(), p_master.data_ptr(), g.data_ptr(),
                                         m.data_ptr(), v.data_ptr(), p.numel(), int(n_decay),
                                         hyper.data_ptr(), float(beta1), float(beta2), float(eps),
                                         float(wd), _p(grad_scale), _stream()),
               "gvl_adamw_master_dev")


def adamw(p, g, m, v, n_decay, lr, beta1, beta2, eps, wd, step, grad_scale=None):
    _dev(p, g, m, v)
    _lib.check(_L().gvl_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                              int(n_decay), float(lr), float(beta1), float(beta2), float(eps),
                              float(wd), int(step), _p(grad_scale), _stream()), "gvl_adamw")


# ------------------------------------------------------------------------- elementwise
def colsum(x2, out=None, accumulate=False):
    rows, cols = x2.shape
    if out is None:
        out = torch.empty(cols, dtype=BF16, device=x2.device)
    ws = torch.empty(max(_L().gvl_colsum_workspace_size(rows, cols), 4) // 4, dtype=F32,
                     device=x2.device)
    _lib.check(_L().gvl_colsum(x2.data_ptr(), rows, cols, x2.stride(0), out.data_ptr(),
                               int(accumulate), ws.data_ptr(), _stream()), "gvl_colsum")
    return out


def colsum_batched(xs, outs, accumulate=False):
    """outs[i] (+)= column sums of xs[i] (one shape, <= 16 problems) in one launch pair."""
    n = len(xs)
    rows, cols = xs[0].shape
    for x, o in zip(xs, outs):
        _dev(x)
        if tuple(x.shape) != (rows, cols) or x.stride(0) != xs[0].stride(0) or x.stride(1) != 1:
            raise ValueError("gvl.colsum_batched: problems must share shape and row stride")
        if o.dtype != BF16 or o.numel() != cols or not o.is_contiguous():
            raise ValueError("gvl.colsum_batched: bad output")
    ws = torch.empty(max(_L().gvl_colsum_batched_workspace_size(n, rows, cols), 4) // 4,
                     dtype=F32, device=xs[0].device)
    xa = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    oa = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    _lib.check(_L().gvl_colsum_batched(xa, oa, n, rows, cols, xs[0].stride(0), int(accumulate),
                                       ws.data_ptr(), _stream()), "gvl_colsum_batched")


def dropout_mask_apply(x2, p, seed, out=None, seed_ptr=None):
    rows, cols = x2.shape
    if out is None:
        out = torch.empty(rows, cols, dtype=BF16, device=x2.device)
    _lib.check(_L().gvl_dropout_mask_apply(x2.data_ptr(), x2.stride(0), out.data_ptr(),
                                           out.stride(0), rows, cols, float(p),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, _p(seed_ptr),
                                           _stream()),
               "gvl_dropout_mask_apply")
    return out


def gate_bwd(dx, y, gate, gate_grad_f32=None, grad_bf16=None):
    """dy = tanh(gate) * dx; the gate gradient (1 - tanh^2) * sum(dx * y) added into
    gate_grad_f32 (fp32 scalar) or, with grad_bf16, into that bf16 scalar with autograd's
    roundings (ABI v13)."""
    n = dx.numel()
    dy = torch.empty_like(dx)
    ws = torch.empty(max(_L().gvl_gate_bwd_workspace_size(n), 4) // 4, dtype=F32,
                     device=dx.device)
    if grad_bf16 is not None:
        if grad_bf16.dtype != BF16 or grad_bf16.numel() != 1:
            raise TypeError("gvl.gate_bwd: grad_bf16 must be a bf16 scalar")
        _lib.check(_L().gvl_gate_bwd_acc_bf16(dx.data_ptr(), y.data_ptr(), gate.data_ptr(),
                                              dy.data_ptr(), grad_bf16.data_ptr(), n, ws.data_ptr(),
                                              _stream()), "gvl_gate_bwd_acc_bf16")
        return dy
    _lib.check(_L().gvl_gate_bwd(dx.data_ptr(), y.data_ptr(), gate.data_ptr(), dy.data_ptr(),
                                 gate_grad_f32.data_ptr(), n, ws.data_ptr(), _stream()),
               "gvl_gate_bwd")
    return dy


def f32_to_bf16(x, out, accumulate=False):
    _lib.check(_L().gvl_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), int(accumulate),
                                    _stream()), "gvl_f32_to_bf16")
    return out
