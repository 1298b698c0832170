"""CPU restatement of int8 weight-only decoding (include/gvl.h, csrc/linear_w8.hip): the
quantiser, the dequantiser and the float64 reference of gvl_linear_w8 with its error scale.

Format: per row n of a weight [N, K]: scale[n] = absmax_n / 127 (fp32 division), q[n, k] =
clamp(round_half_even(fp32(w) / scale[n]), -127, 127); a zero row has scale 0 and q 0; the
dequantised weight is bf16(fp32(q) * scale[n]).
Linear: y[m, n] = epi(scale[n] * sum_k x[m, k] q[n, k]), the scale applied once after the sum and
before the bias, then gemm_common.h's epilogue (tests/gemm_ref.py epilogue64).  Error scale:
gemm_ref.scale on (|x| @ |q|^T) * scale[n].  Slack: gemm_ref's rule, four times the worse of two
fp32 emulations in this arithmetic (torch's blocked sum and the 32-deep K-step order, each
followed by * scale and gemm_ref.epilogue32); it never comes from the kernel.  scale None: w is a
bf16 weight, no scale (the kernel's bf16 instance)."""
import numpy as np
import torch

from tests import gemm_ref as G
from tests.helpers import assert_bf16_rounded, err_units, f64

F32 = np.float32
BF = torch.bfloat16
CAP = 256  # GVL_LINEAR_W8_MAX_ROWS

# the five epilogues of a decode step: which operands each takes
EPIS = {
    "plain": (),
    "bias": ("bias",),
    "bias_gelu": ("bias", "act"),
    "bias_res": ("bias", "residual"),
    "bias_gate_res": ("bias", "gate", "residual"),
}
LINEAR_EPIS = ("plain", "bias", "bias_res")  # exact on exact inputs: bit for bit


def quantize(w):
    """bf16 (or fp32) CPU weight [N, K] -> (q int8 [N, K], scale fp32 [N])."""
    wf = w.detach().to("cpu", torch.float32)
    absmax = wf.abs().amax(dim=1)
    scale = absmax / torch.full_like(absmax, 127.0)  # tensor / tensor: one rounded division
    zero = scale == 0
    q = (wf / torch.where(zero, torch.ones_like(scale), scale)[:, None]).round()
    q = q.clamp_(-127, 127).to(torch.int8)
    q[zero] = 0
    return q, scale


def dequantize(q, scale):
    """bf16 [N, K] = bf16_rne(fp32(q) * scale[n])."""
    return (q.to(torch.float32) * scale.to(torch.float32)[:, None]).to(BF)


def products(x, w, scale=None):
    """What every epilogue of one (x, w, scale) shares: the float64 product, the sum of absolute
    terms, and the two fp32 emulations of the scaled sum."""
    X, Wm = f64(x), f64(w)
    s = np.ones(Wm.shape[0]) if scale is None else f64(scale)
    x32, w32 = X.astype(F32), Wm.astype(F32)
    h1 = (torch.from_numpy(x32) @ torch.from_numpy(w32).t()).numpy()
    h2 = G.matmul32_seq(x32, np.ascontiguousarray(w32.T))
    if scale is not None:
        s32 = s.astype(F32)[None, :]
        h1, h2 = h1 * s32, h2 * s32
    return dict(h=(X @ Wm.T) * s[None, :], absh=(np.abs(X) @ np.abs(Wm).T) * np.abs(s)[None, :],
                emu=(h1, h2))


def epi_kw(bias=None, act=0, residual=None, gate=None):
    kw = dict(act=int(act))
    if bias is not None:
        kw["bias"] = f64(bias)
    if residual is not None:
        kw["residual"] = f64(residual)
    if gate is not None:
        kw["gate"] = float(gate.float().reshape(-1)[0]) if isinstance(gate, torch.Tensor) \
            else float(gate)
    return kw


def reference(prod, **epi):
    """dict(ref float64 [M, N], E, emu, slack) of one epilogue over products()."""
    kw = epi_kw(**epi)
    ref, _ = G.epilogue64(prod["h"], **kw)
    E, _ = G.scale(prod["absh"], h=prod["h"], **kw)
    emu = max(err_units(G.epilogue32(h, **kw)[0], ref, E) for h in prod["emu"])
    return dict(ref=ref, E=E, emu=emu, slack=4 * emu)


def linear_reference(x, w, scale=None, **epi):
    return reference(products(x, w, scale), **epi)


def check(got, R, name=""):
    """got bf16 [M, N] against reference R per element (tests/helpers.py assert_bf16_rounded)."""
    return assert_bf16_rounded(got, R["ref"], R["E"], R["slack"], name)


def _bf(a):
    return torch.from_numpy(np.asarray(a, dtype=F32)).to(BF)


def inputs(kind, M, N, K, seed=0):
    """Seeded operands of one case: x bf16 [M, K], w bf16 [N, K] (the bf16 instance's weight), q
    int8 / scale fp32 (the int8 instance's: w quantised; `exact`: drawn directly), bias [N],
    residual [M, N], gate.
      random  N(0, 1)
      scaled  rows of x and rows of w times 2**-6 .. 2**6 (the scales then span 12 binades)
      exact   x in -2 .. 2, q in -9 .. 9 with a +-127 per row, scale a power of two 2**-3 .. 2**3,
              w in -2 .. 2, bias / residual integers of magnitude <= 64: every partial sum is an
              integer multiple of 2**-3 below 2**21, exact in fp32 in any order"""
    g = np.random.default_rng(7919 * seed + 131 * M + 17 * N + K)
    if kind == "exact":
        x = g.integers(-2, 3, (M, K)).astype(F32)
        w = g.integers(-2, 3, (N, K)).astype(F32)
        q = g.integers(-9, 10, (N, K)).astype(np.int8)
        q[np.arange(N), g.integers(0, K, N)] = np.where(g.random(N) < 0.5, -127, 127)
        scale = np.exp2(g.integers(-3, 4, N)).astype(F32)
        bias = g.integers(-64, 65, N).astype(F32)
        res = g.integers(-64, 65, (M, N)).astype(F32)
        out = dict(q=torch.from_numpy(q), scale=torch.from_numpy(scale))
    else:
        x = g.standard_normal((M, K)).astype(F32)
        w = g.standard_normal((N, K)).astype(F32)
        bias = g.standard_normal(N).astype(F32)
        res = g.standard_normal((M, N)).astype(F32)
        if kind == "scaled":
            rs = np.exp2(g.integers(-6, 7, M)).astype(F32)
            cs = np.exp2(g.integers(-6, 7, N)).astype(F32)
            x *= rs[:, None]
            w *= cs[:, None]
            sk = F32(2.0 ** round(np.log2(np.sqrt(K))))
            bias *= cs * sk * np.median(rs)
            res *= rs[:, None] * cs[None, :] * sk
        out = {}
    out.update(x=_bf(x), w=_bf(w), bias=_bf(bias), residual=_bf(res),
               gate=_bf(np.array([0.75], dtype=F32)))
    if "q" not in out:
        out["q"], out["scale"] = quantize(out["w"])
    return out


def epi_operands(epi, ins):
    """The keyword operands (torch tensors) epilogue `epi` takes from inputs()."""
    names = EPIS[epi]
    kw = {}
    if "bias" in names:
        kw["bias"] = ins["bias"]
    if "act" in names:
        kw["act"] = 1
    if "residual" in names:
        kw["residual"] = ins["residual"]
    if "gate" in names:
        kw["gate"] = ins["gate"]
    return kw
