"""float64 reference, per-element error scales and an fp32 emulation of the GEMM family
(csrc/gemm*.hip, gemm_common.h gemm_epi_vals), bf16-exact input builders, descriptors and the
case table: one small case per kernel instance of tests/data/gemm_routes.json.  Shared by
test_gemm_ref_cpu.py, which shows that the per-element bound rejects doctored outputs the
max-norm comparison accepts and holds the table to the built library, and test_gpu_gemm.py,
which holds the HIP kernels to it.  Everything here runs on the CPU and reads the same bf16
values the kernels read; nothing reads a kernel's output."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from tests.attn_ref import drop_scale, mix64, seed_eff  # noqa: F401  (one restatement of the hash)
from tests.helpers import F32_UNIT, err_units, f64, ulp_bf16

BF = torch.bfloat16
F32 = np.float32

# ------------------------------------------------------------------------------ dropout
def keep_mask(seed, M, N, p, row_len=None):
    """bool [M, N]: common.h rng_keep on element index m * N + n (attn_ref.keep_mask on one
    [1, 1, M, N] plane); the threshold is the host's (uint32)(p * 2**32)."""
    from tests.attn_ref import keep_mask as km
    return km(seed, 1, 1, M, N, p, row_len=row_len)[0, 0]


# ---------------------------------------------------------------- exact activations, float64
_K0 = math.sqrt(2.0 / math.pi)


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + np.tanh(_K0 * (x + 0.044715 * x ** 3)))


def dgelu_tanh64(x):
    u = _K0 * (x + 0.044715 * x ** 3)
    t = np.tanh(u)
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _K0 * (1.0 + 3 * 0.044715 * x * x)


def gelu_erf64(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def dgelu_erf64(x):
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def quick_gelu64(x):
    return x / (1.0 + np.exp(-1.702 * x))


# ------------------------------------------- common.h formulas restated in float32 numpy
def _f(x):
    return np.asarray(x, dtype=F32)


def fast_sigmoid32(z):
    with np.errstate(over="ignore"):
        return F32(1) / (F32(1) + np.exp2(F32(-1.4426950408889634) * _f(z)))


def gelu_tanh_sig32(x, x2):
    A = F32(F32(2) * F32(0.7978845608028654) * F32(1.4426950408889634))
    B = F32(A * F32(0.044715))
    with np.errstate(over="ignore"):
        return F32(1) / (F32(1) + np.exp2(-_f(x) * (B * _f(x2) + A)))


def gelu_tanh32(x):
    x = _f(x)
    return x * gelu_tanh_sig32(x, x * x)


def quick_gelu32(x):
    x = _f(x)
    A = F32(F32(1.702) * F32(1.4426950408889634))
    with np.errstate(over="ignore"):
        return x * (F32(1) / (F32(1) + np.exp2(-A * x)))


def dgelu_tanh32(x):
    x = _f(x)
    Cc = F32(F32(2) * F32(0.7978845608028654))
    D = F32(F32(3) * F32(0.044715) * Cc)
    x2 = x * x
    s = gelu_tanh_sig32(x, x2)
    return x * s * (F32(1) - s) * (D * x2 + Cc) + s


def fast_erf32(x, worse=1.0):
    """Abramowitz-Stegun 7.1.26 as common.h fast_erf writes it.  `worse`: the polynomial's error
    term scaled (doctored-output tests: 10 = a version with ten times its error)."""
    x = _f(x)
    a = np.abs(x)
    t = F32(1) / (F32(1) + F32(0.3275911) * a)
    poly = t * (F32(0.254829592) + t * (F32(-0.284496736) + t * (F32(1.421413741) + t * (
        F32(-1.453152027) + t * F32(1.061405429)))))
    r = F32(1) - poly * np.exp2(F32(-1.4426950408889634) * a * a)
    if worse != 1.0:
        exact = _erf(a.astype(np.float64))
        r = (exact + worse * (r.astype(np.float64) - exact)).astype(F32)
    return np.copysign(r, x)


def gelu_erf32(x, worse=1.0):
    x = _f(x)
    return F32(0.5) * x * (F32(1) + fast_erf32(x * F32(0.7071067811865476), worse))


def dgelu_erf32(x):
    x = _f(x)
    return F32(0.5) * (F32(1) + fast_erf32(x * F32(0.7071067811865476))) + \
        x * F32(0.3989422804014327) * np.exp2(F32(-0.7213475204444817) * x * x)


# ------------------------------------------------------------------- epilogue kinds
# name -> the descriptor's epilogue fields (tools/gemm_routes.py EPIS, by operand not address)
EPIS = {
    "plain": {},
    "bias": dict(bias=1),
    "bias_res": dict(bias=1, residual=1),
    "res_inplace": dict(residual="c"),
    "bias_act1": dict(bias=1, act=1, pre_out=1),
    "bias_act2": dict(bias=1, act=2, pre_out=1),
    "bias_act_d": dict(bias=1, act=3, pre_out=1),
    "bias_act_erf_d": dict(bias=1, act=4, pre_out=1),
    "dact": dict(dact=1, pre_in=1),
    "dact_erf": dict(dact=2, pre_in=1),
    "mul": dict(dact=3, pre_in=1),
    "drop_res": dict(bias=1, residual=1, drop=1),
    "gate_res": dict(bias=1, residual=1, gate=1, pre_out=1),
    "qgelu": dict(bias=1, act=5),
    "c_fp32": dict(c_fp32=1),
    # the runtime-flag epilogue (EPI_GEN): no compile-time kind has these combinations
    "gen_act_res": dict(bias=1, act=1, pre_out=1, residual=1),
    "gen_gate_drop": dict(bias=1, residual=1, gate=1, pre_out=1, drop=1),
}
ACT_EPIS = ("bias_act1", "bias_act2", "bias_act_d", "bias_act_erf_d", "dact", "dact_erf", "qgelu",
            "gen_act_res")
# bitwise on the *exact* inputs: every value on the way is an integer below 2**24 (alpha and
# drop_scale powers of two), so the correctly rounded result does not depend on the route
BITWISE_EPIS = ("plain", "bias", "bias_res", "res_inplace", "drop_res", "c_fp32", "mul")
DROP_P = 0.1
SEED = 0x5EED0000


def epilogue64(h, *, alpha=1.0, alpha_dev=None, bias=None, act=0, dact=0, pre_in=None, keep=None,
               drop_p=0.0, gate=None, residual=None):
    """gemm_common.h gemm_epi_vals in float64, in its order: x alpha (x *alpha_ptr), + bias,
    x dgelu(pre_in) or x pre_in, activation (pre_out <- x or gelu'(x)), dropout, gate (pre_out <-
    the un-gated branch when there is no activation), + residual.  h = A @ B in float64; bias [N],
    pre_in / residual [M, N], keep a bool [M, N], gate the bf16 scalar.  Returns (C, side): side
    is None where the epilogue stores none."""
    a = float(alpha) if alpha_dev is None else float(F32(alpha) * F32(alpha_dev))
    v = f64(h) * a
    side = None
    if bias is not None:
        v = v + f64(bias)[None, :]
    if dact:
        x = f64(pre_in)
        v = v * (dgelu_tanh64(x) if dact == 1 else dgelu_erf64(x) if dact == 2 else x)
    if act == 5:
        v = quick_gelu64(v)
    elif act:
        x = v
        v = gelu_tanh64(x) if act in (1, 3) else gelu_erf64(x)
        side = x if act in (1, 2) else (dgelu_tanh64(x) if act == 3 else dgelu_erf64(x))
    if drop_p > 0:
        v = np.where(keep, v * drop_scale(drop_p), 0.0)  # drop_scale: 1.f / (1.f - p) in fp32
    if gate is not None:
        if not act:
            side = v
        v = v * math.tanh(float(gate))
    if residual is not None:
        v = v + f64(residual)
    return v, side


def scale(absAB, *, alpha=1.0, alpha_dev=None, bias=None, act=0, dact=0, pre_in=None, keep=None,
          drop_p=0.0, gate=None, residual=None, h=None):
    """Per-element error scale (E, E_side): the sum of the absolute values of the terms added to
    form each output, so that an fp32 evaluation in any order is off by a few 2**-24 * E.
    absAB = |A| @ |B| (float64), h = A @ B (needed for the activations and dact)."""
    a = float(alpha) if alpha_dev is None else float(F32(alpha) * F32(alpha_dev))
    E = abs(a) * f64(absAB)  # h = sum_k a_k b_k: every add is within 2**-24 of the sum of the |a_k b_k|
    x = None if h is None else a * f64(h)  # the value in front of dact / the activation
    Es = None
    if bias is not None:
        E = E + np.abs(f64(bias))[None, :]  # one more term
        x = None if x is None else x + f64(bias)[None, :]
    if dact in (1, 2):
        # v = x * g, g = dgelu(pre_in): the error of x scales by |g|; the formula's own absolute
        # error (a few 2**-24, |g| <= 1.13) is carried by |x|
        g = dgelu_tanh64(f64(pre_in)) if dact == 1 else dgelu_erf64(f64(pre_in))
        E = E * np.abs(g) + np.abs(x)
    elif dact == 3:
        E = E * np.abs(f64(pre_in))  # an exact bf16 factor: one more rounding of the product
    if act:
        Ex = E
        # gelu(x + e) - gelu(x) <= 1.13 |e| (|gelu'| <= 1.13, quick-GELU's <= 1.10); the formulas'
        # own error is absolute in x (A-S 7.1.26: <= 4.5 * 2**-24 * |x|), carried by |x|
        E = 1.13 * Ex + np.abs(x)
        if act in (1, 2):
            Es = Ex  # pre_out <- x
        elif act in (3, 4):
            Es = 0.8 * Ex + 1.0  # |gelu''| <= 0.8; gelu' is O(1) with an absolute formula error
    if drop_p > 0:
        E = np.where(keep, E * drop_scale(drop_p), 0.0)  # a dropped element is exactly zero
    if gate is not None:
        if not act:
            Es = E
        E = E * abs(math.tanh(float(gate)))
    if residual is not None:
        E = E + np.abs(f64(residual))
    return E, Es


def matmul32_seq(A, B, step=32):
    """A @ B in fp32 as the kernels order it: one 32-deep K-step after the other into an fp32
    accumulator."""
    A, B = _f(A), _f(B)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=F32)
    for k0 in range(0, A.shape[1], step):
        acc += A[:, k0:k0 + step] @ B[k0:k0 + step]
    return acc


def epilogue32(h32, *, alpha=1.0, alpha_dev=None, bias=None, act=0, dact=0, pre_in=None, keep=None,
               drop_p=0.0, gate=None, residual=None, erf_worse=1.0):
    """gemm_epi_vals in float32 numpy with the common.h formulas -> (C, side) in fp32."""
    a = F32(alpha) if alpha_dev is None else F32(F32(alpha) * F32(alpha_dev))
    v = _f(h32) * a
    side = None
    if bias is not None:
        v = v + _f(bias)[None, :]
    if dact:
        x = _f(pre_in)
        v = v * (dgelu_tanh32(x) if dact == 1 else dgelu_erf32(x) if dact == 2 else x)
    if act == 5:
        v = quick_gelu32(v)
    elif act:
        x = v
        v = gelu_tanh32(x) if act in (1, 3) else gelu_erf32(x, erf_worse)
        side = x if act in (1, 2) else (dgelu_tanh32(x) if act == 3 else dgelu_erf32(x))
    if drop_p > 0:
        v = np.where(keep, v * F32(drop_scale(drop_p)), F32(0))
    if gate is not None:
        if not act:
            side = v
        v = v * F32(math.tanh(float(gate)))
    if residual is not None:
        v = v + _f(residual)
    return v, side


def emulate32(A, B, **epi):
    """The same operation in fp32 on the CPU, the matmul two ways (torch's blocked fp32 sum and
    the kernels' K-step order) -> [(C, side), (C, side)]."""
    A32, B32 = _f(A), _f(B)
    h1 = (torch.from_numpy(A32) @ torch.from_numpy(B32)).numpy()
    return [epilogue32(h1, **epi), epilogue32(matmul32_seq(A32, B32), **epi)]


def slack_of(emus, ref64, E, margin=4):
    """margin x the worse emulation's error in units of 2**-24 * E over the whole tensor."""
    return margin * max(err_units(e, ref64, E) for e in emus)


def round_bf16(x64):
    """The correctly rounded (RNE) bf16 of float64 values that are exact in fp32."""
    return torch.from_numpy(np.asarray(x64, dtype=F32)).to(BF)


def slack_ulps(slack, ref64, E):
    """The slack term of assert_bf16_rounded per element, in bf16 ulps of the reference."""
    return slack * F32_UNIT * np.abs(f64(E)) / ulp_bf16(ref64)


# ------------------------------------------------------------------------ input builders
KINDS = ("random", "scaled", "exact", "act")


def _bf(a):
    return torch.from_numpy(np.asarray(a, dtype=F32)).to(BF)


def inputs(kind, M, N, K, epi, seed=0):
    """bf16-exact, seeded operands of one case: dict with A [M, K], B [K, N] and, as the epilogue
    `epi` needs them, bias [N], residual / pre_in [M, N], gate (bf16 scalar), all torch bf16.
      random  N(0, 1) everywhere
      scaled  rows of A and columns of B times powers of two 2**-6 .. 2**6 (outputs span 24
              binades; bias, residual and pre_in follow their column's / element's scale)
      exact   integers: A, B in -2 .. 2, bias / residual of magnitude <= 64, pre_in in -2 .. 2:
              every partial sum is an integer below 2**24 for K <= 4096, exact in fp32 in any order
      act     x = AB + bias covers [-8, 8]: bias runs over it, B's columns have their own width,
              whole columns lie beyond +-4; pre_in covers [-8, 8] as well"""
    f = EPIS[epi]
    g = np.random.default_rng(1000003 * seed + 7 * M + 3 * N + K)
    out = {}
    if kind == "exact":
        A = g.integers(-2, 3, (M, K)).astype(F32)
        B = g.integers(-2, 3, (K, N)).astype(F32)
        bias = g.integers(-64, 65, N).astype(F32)
        res = g.integers(-64, 65, (M, N)).astype(F32)
        pre = g.integers(-2, 3, (M, N)).astype(F32)
    else:
        A = g.standard_normal((M, K)).astype(F32)
        B = g.standard_normal((K, N)).astype(F32)
        bias = g.standard_normal(N).astype(F32)
        res = g.standard_normal((M, N)).astype(F32)
        pre = (2 * g.standard_normal((M, N))).astype(F32)
        if kind == "scaled":
            rs = np.exp2(g.integers(-6, 7, M)).astype(F32)
            cs = np.exp2(g.integers(-6, 7, N)).astype(F32)
            A *= rs[:, None]
            B *= cs[None, :]
            sk = F32(2.0 ** round(math.log2(math.sqrt(K))))  # the scale of a K-term sum
            bias *= cs * sk * np.median(rs)
            res *= rs[:, None] * cs[None, :] * sk
            if f.get("dact") == 3:
                pre *= np.exp2(g.integers(-3, 4, (M, N))).astype(F32)
        elif kind == "act":
            width = np.exp2(g.integers(-3, 2, N)).astype(F32)  # column widths 1/8 .. 2
            B *= (width / F32(math.sqrt(K)))[None, :]
            bias = g.permutation(np.linspace(-8.0, 8.0, N)).astype(F32) if f.get("act") else bias
            pre = np.clip(3 * g.standard_normal((M, N)), -8, 8).astype(F32)
            pre[:, ::7] = np.where(pre[:, ::7] < 0, -4.0, 4.0) + pre[:, ::7] / 2  # tails
    out["A"], out["B"] = _bf(A), _bf(B)
    if f.get("bias"):
        out["bias"] = _bf(bias)
    if f.get("residual"):
        out["residual"] = _bf(res)
    if f.get("pre_in"):
        out["pre_in"] = _bf(pre)
    if f.get("gate"):
        out["gate"] = _bf(np.array([0.75], dtype=F32))
    return out


def epi_args(case, ins, seed_off=None):
    """The keyword arguments of epilogue64 / scale / epilogue32 for a case and its inputs."""
    f = EPIS[case["epi"]]
    kw = dict(alpha=case.get("alpha", 1.0), alpha_dev=case.get("alpha_dev"),
              act=f.get("act", 0), dact=f.get("dact", 0))
    for k in ("bias", "residual", "pre_in"):
        if k in ins:
            kw[k] = f64(ins[k])
    if "gate" in ins:
        kw["gate"] = float(ins["gate"].float()[0])
    if f.get("drop"):
        p = case.get("drop_p", DROP_P)
        kw["drop_p"] = p
        kw["keep"] = keep_mask(seed_eff(SEED, seed_off), case["M"], case["N"], p)
    return kw


def reference(case, ins, seed_off=None, emulate=True):
    """Everything the tests need of one case: dict with ref (C in float64), side, E, E_side and,
    with emulate, slack / slack_side (4 x the fp32 emulations' own error) and emu, emu_side (the
    worse emulation's error in units of 2**-24 * E)."""
    A, B = f64(ins["A"]), f64(ins["B"])
    kw = epi_args(case, ins, seed_off)
    h = A @ B
    ref, side = epilogue64(h, **kw)
    E, Es = scale(np.abs(A) @ np.abs(B), h=h, **kw)
    out = dict(ref=ref, side=side, E=E, E_side=Es, kw=kw)
    if emulate:
        emus = emulate32(A, B, **kw)
        out["emu"] = max(err_units(c, ref, E) for c, _ in emus)
        out["slack"] = 4 * out["emu"]
        if side is not None:
            out["emu_side"] = max(err_units(s, side, Es) for _, s in emus)
            out["slack_side"] = 4 * out["emu_side"]
    return out


# ------------------------------------------------------------------------- descriptors
# dummy operands of the name query (distinct 16-byte aligned addresses, never dereferenced)
DUMMY = dict(a=0x100000, b=0x200000, c=0x300010, aux=0x400010, aux2=0x500010, bias=0x600000,
             gate=0x700000, ws=0x800000, tickets=0x900000, alpha_ptr=0xA00000, seed_ptr=0xB00000)
WS_BYTES = 64 << 20
TICKETS = 1 << 16


def lds_of(case):
    """(lda, ldb, ldc, ld_aux): every [M, N] operand's row stride is N + pad > N."""
    M, N, K = case["M"], case["N"], case["K"]
    pad = case.get("pad", 8)
    return (M if case["a_mn"] else K), (N if case["b_mn"] else K), N + pad, N + pad


def fill_desc(case, ptr=None):
    """The gvl_gemm_desc of a case.  ptr: operand addresses (a, b, c, aux = residual or pre_in,
    aux2 = pre_out, bias, gate, alpha_ptr, seed_ptr, ws, tickets); default: the dummies."""
    from gvl import _lib
    p = dict(DUMMY if ptr is None else ptr)
    f = EPIS[case["epi"]]
    d = _lib.GemmDesc()
    d.a, d.b, d.c = p["a"], p["b"], p["c"]
    d.m, d.n, d.k = case["M"], case["N"], case["K"]
    d.lda, d.ldb, d.ldc, ld = lds_of(case)
    d.a_mn, d.b_mn = case["a_mn"], case["b_mn"]
    d.alpha = case.get("alpha", 1.0)
    if case.get("alpha_dev") is not None:
        d.alpha_ptr = p["alpha_ptr"]
    if f.get("bias"):
        d.bias = p["bias"]
    d.act, d.dact = f.get("act", 0), f.get("dact", 0)
    if f.get("pre_in"):
        d.pre_in, d.ldp = p["aux"], ld
    if f.get("pre_out"):
        d.pre_out, d.ldp = p["aux2"], ld
    if f.get("residual"):
        d.residual, d.ldr = (p["c"], d.ldc) if f["residual"] == "c" else (p["aux"], ld)
    if f.get("gate"):
        d.gate = p["gate"]
    if f.get("drop"):
        d.drop_p, d.seed = case.get("drop_p", DROP_P), SEED
        if case.get("seed_off") is not None:
            d.seed_ptr = p["seed_ptr"]
    d.c_fp32 = f.get("c_fp32", 0)
    if case["ws"]:
        d.workspace, d.workspace_bytes = p["ws"], WS_BYTES
        d.tickets, d.ticket_count = p["tickets"], TICKETS
    return d


def kernel_name(lib, case, ptr=None):
    """gvl_gemm_kernel_name of a case under its tune setting (restored to (3, -1))."""
    lib.gvl_gemm_tune(*case["tune"])
    buf = C.create_string_buffer(128)
    try:
        lib.gvl_gemm_kernel_name(C.byref(fill_desc(case, ptr)), buf, 128)
    finally:
        lib.gvl_gemm_tune(3, -1)
    return buf.value.decode()


COST_CAP = 4e9  # M * N * K per case


def cost(case):
    return case["M"] * case["N"] * case["K"]


def kinds_of(case):
    """The input kinds a case runs: activations on the *act* inputs, the rest alternately on the
    *random* and the *scaled* ones, and everything on the *exact* ones too."""
    if "kinds" in case:
        return case["kinds"]
    first = "act" if case["epi"] in ACT_EPIS else ("random", "scaled")[case["i"] % 2]
    return (first, "exact")


def bitwise(case):
    """On the *exact* inputs the correctly rounded result is unique, whatever the route."""
    a = case.get("alpha", 1.0) * (case.get("alpha_dev") or 1.0)
    return (case["epi"] in BITWISE_EPIS and math.log2(abs(a)).is_integer() and case["K"] <= 4096
            and (case["epi"] != "drop_res" or case.get("drop_p", DROP_P) == 0.5))


def _case(i, t):
    name, tune, ws, M, N, K, a_mn, b_mn, epi = t[:9]
    c = dict(i=i, name=name, tune=tuple(tune), ws=int(ws), M=M, N=N, K=K, a_mn=a_mn, b_mn=b_mn, epi=epi)
    c.update(t[9] if len(t) > 9 else {})
    c["id"] = "%03d-%s-%d:%d-%s-%dx%dx%d-%d%d-%s" % (
        i, name.split("_kernel")[0][5:], c["tune"][0], c["tune"][1], "ws" if ws else "nows", M, N, K,
        a_mn, b_mn, epi)
    return c


# ---------------------------------------------------------------------------- the cases
# (kernel instance, tune setting, workspace + tickets, M, N, K, a_mn, b_mn, epilogue[, options]).
# One row per name of tests/data/gemm_routes.json: the cheapest descriptor the planner admits
# among shapes of at least two tile rows and two tile columns whose M is no multiple of a tile
# height (8 x an odd number: MN-contiguous A needs M % 8 == 0), whose N is no multiple of the tile
# width and N % 8 == 4 where the route stores 8 bytes at a time (a 192-wide persistent tile needs
# N % 64 == 0 and N >= 384; 256 rows beside 192 columns need more than 256 tiles of 128 x 192:
# M = 6536, which also leaves tiles_m % group != 0), ldc = ldr = ldp = N + 8, K one 32-deep
# step for every other name and an odd number of steps (96: no multiple of 64) for the rest where
# the instance admits it (the four-wave kernels need K % 192 == 0, the LDS-DMA kernel K % 64 == 0).
# Found by asking gvl_gemm_kernel_name over a grid of shapes; test_gemm_ref_cpu.py re-queries
# every row.
_ROUTE_CASES = [
    ("gemm_pp3_kernel<4, false, false, 0, 192, 256>", (3, 3), 0, 6536, 832, 32, 0, 0, "plain"),
    ("gemm_w4d_kernel<false, 0>", (3, -1), 1, 12296, 264, 384, 0, 0, "plain"),
    ("gemm_w4x_kernel<256, 192, false, false, 0, false>", (3, 12), 1, 12296, 776, 96, 0, 0, "plain"),
    ("gemm_pp_kernel<4, false, false>", (3, -1), 0, 12296, 776, 96, 0, 0, "gate_res"),
    ("gemm_ring_kernel<64, 128, 1, 2, 4, 1, false, false>", (2, 6), 1, 328, 260, 32, 0, 0, "plain"),
    ("gemm_ring_kernel<192, 128, 2, 2, 4, 2, false, false>", (2, 7), 1, 328, 260, 96, 0, 0, "plain"),
    ("gemm_ring_kernel<192, 256, 2, 2, 4, 2, false, false>", (2, 8), 0, 328, 260, 32, 0, 0, "plain"),
    ("gemm_ring_kernel<128, 192, 2, 2, 4, 1, false, false>", (2, 9), 1, 328, 260, 96, 0, 0, "plain"),
    ("gemm_lds_kernel<256, 256, 2, 4, false, false>", (1, -1), 1, 16136, 2312, 64, 0, 0, "plain"),
    ("gemm_bf16_kernel<false, false>", (1, -1), 0, 328, 260, 96, 0, 0, "plain"),
    ("gemm_pp3_kernel<4, false, false, 1, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 0, "bias"),
    ("gemm_w4d_kernel<false, 1>", (3, -1), 1, 12296, 264, 384, 0, 0, "bias"),
    ("gemm_lds_kernel<128, 128, 2, 2, false, false>", (1, -1), 0, 328, 260, 64, 0, 0, "plain"),
    ("gemm_w4x_kernel<256, 192, false, false, 2, false>", (3, 12), 1, 12296, 776, 96, 0, 0, "bias_res"),
    ("gemm_pp3_kernel<4, false, false, 2, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 0, "bias_res"),
    ("gemm_w4d_kernel<false, 2>", (3, -1), 0, 12296, 264, 384, 0, 0, "bias_res"),
    ("gemm_pp3_kernel<4, false, false, 12, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 0, "drop_res"),
    ("gemm_w4d_kernel<false, 12>", (3, -1), 1, 12296, 264, 384, 0, 0, "drop_res"),
    ("gemm_w4_kernel<3, false, 13>", (3, -1), 0, 12296, 264, 192, 0, 0, "gate_res"),
    ("gemm_pp3_kernel<4, false, false, 1, 256, 256>", (3, 3), 1, 328, 264, 96, 0, 0, "bias"),
    ("gemm_pp3_kernel<4, false, false, 3, 256, 256>", (3, 3), 1, 328, 264, 32, 0, 0, "bias_act1"),
    ("gemm_w4_kernel<3, false, 3>", (3, -1), 0, 12296, 264, 192, 0, 0, "bias_act1"),
    ("gemm_pp3_kernel<4, false, false, 7, 256, 256>", (3, 3), 1, 328, 264, 32, 0, 0, "bias_act2"),
    ("gemm_w4_kernel<3, false, 7>", (3, -1), 1, 12296, 264, 192, 0, 0, "bias_act2"),
    ("gemm_pp3_kernel<4, false, false, 9, 256, 256>", (3, 3), 0, 328, 264, 32, 0, 0, "bias_act_d"),
    ("gemm_w4_kernel<3, false, 9>", (3, -1), 1, 12296, 264, 192, 0, 0, "bias_act_d"),
    ("gemm_pp3_kernel<4, false, false, 10, 256, 256>", (3, 3), 1, 328, 264, 32, 0, 0, "bias_act_erf_d"),
    ("gemm_w4_kernel<3, false, 10>", (3, -1), 0, 12296, 264, 192, 0, 0, "bias_act_erf_d"),
    ("gemm_pp3_kernel<4, false, false, 14, 256, 256>", (3, 3), 1, 328, 264, 32, 0, 0, "qgelu"),
    ("gemm_pp3_kernel<4, false, false, 0, 256, 256>", (3, 3), 1, 328, 264, 96, 0, 0, "plain"),
    ("gemm_w4x_kernel<256, 192, false, true, 0, false>", (3, 12), 0, 12296, 776, 96, 0, 1, "plain"),
    ("gemm_pp3_kernel<4, false, true, 0, 192, 256>", (3, 3), 1, 6536, 832, 96, 0, 1, "plain"),
    ("gemm_w4d_kernel<true, 0>", (3, -1), 1, 12296, 264, 384, 0, 1, "plain"),
    ("gemm_pp_kernel<4, false, true>", (3, -1), 0, 12296, 776, 96, 0, 1, "gate_res"),
    ("gemm_ring_kernel<64, 128, 1, 2, 4, 1, false, true>", (2, 6), 1, 328, 264, 32, 0, 1, "plain"),
    ("gemm_ring_kernel<192, 128, 2, 2, 4, 2, false, true>", (2, 7), 1, 328, 264, 96, 0, 1, "plain"),
    ("gemm_ring_kernel<192, 256, 2, 2, 4, 2, false, true>", (2, 8), 0, 328, 264, 32, 0, 1, "plain"),
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, true>", (3, -1), 1, 328, 264, 96, 0, 1, "plain"),
    ("gemm_lds_kernel<128, 128, 2, 2, false, true>", (1, -1), 1, 328, 264, 64, 0, 1, "plain"),
    ("gemm_bf16_kernel<false, true>", (1, -1), 0, 328, 264, 96, 0, 1, "plain"),
    ("gemm_pp3_kernel<4, false, true, 6, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 1, "res_inplace"),
    ("gemm_w4d_kernel<true, 6>", (3, -1), 1, 12296, 264, 384, 0, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, false, true, 0, 256, 256>", (3, 3), 0, 328, 264, 32, 0, 1, "plain"),
    ("gemm_lds_kernel<256, 256, 2, 4, false, true>", (1, -1), 1, 16136, 2312, 64, 0, 1, "plain"),
    ("gemm_pp3_kernel<4, false, true, 6, 256, 256>", (3, 3), 1, 328, 264, 32, 0, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, false, true, 4, 256, 256>", (3, 3), 0, 328, 264, 96, 0, 1, "dact"),
    ("gemm_w4_kernel<3, true, 4>", (3, -1), 1, 12296, 264, 192, 0, 1, "dact"),
    ("gemm_pp3_kernel<4, false, true, 8, 256, 256>", (3, 3), 1, 328, 264, 96, 0, 1, "dact_erf"),
    ("gemm_w4_kernel<3, true, 8>", (3, -1), 0, 12296, 264, 192, 0, 1, "dact_erf"),
    ("gemm_pp3_kernel<4, false, true, 11, 256, 256>", (3, 3), 1, 328, 264, 96, 0, 1, "mul"),
    ("gemm_w4_kernel<3, true, 11>", (3, -1), 1, 12296, 264, 192, 0, 1, "mul"),
    ("gemm_pp3_kernel<4, true, true, 0, 256, 256>", (3, 3), 0, 328, 264, 96, 1, 1, "plain"),
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, true, true>", (3, -1), 1, 328, 264, 32, 1, 1, "plain"),
    ("gemm_lds_kernel<128, 128, 2, 2, true, true>", (1, -1), 1, 328, 264, 64, 1, 1, "plain"),
    ("gemm_bf16_kernel<true, true>", (1, -1), 0, 328, 264, 32, 1, 1, "plain"),
    ("gemm_pp3_kernel<4, true, true, 0, 192, 128>", (3, 3), 1, 328, 448, 96, 1, 1, "plain"),
    ("gemm_pp3_kernel<4, true, true, 6, 192, 128>", (3, 3), 1, 328, 448, 32, 1, 1, "res_inplace"),
    ("gemm_pp_kernel<4, true, true>", (3, -1), 0, 12296, 776, 96, 1, 1, "gate_res"),
    ("gemm_lds_kernel<256, 256, 2, 4, true, true>", (1, -1), 1, 16136, 2312, 64, 1, 1, "plain"),
    ("gemm_pp3_kernel<4, true, true, 6, 256, 256>", (3, 3), 0, 328, 264, 32, 1, 1, "res_inplace"),
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 328, 260, 96, 0, 0, "plain"),
    ("gemm_pp3_kernel<4, false, false, 1, 192, 128>", (3, 3), 1, 328, 448, 32, 0, 0, "bias"),
    ("gemm_pp3_kernel<4, false, false, 2, 192, 128>", (3, 3), 0, 328, 448, 96, 0, 0, "bias_res"),
    ("gemm_w4x_kernel<128, 192, false, false, 2, false>", (3, 12), 1, 328, 264, 96, 0, 0, "bias_res"),
    ("gemm_pp3_kernel<4, false, false, 12, 192, 128>", (3, 3), 1, 328, 448, 96, 0, 0, "drop_res"),
    ("gemm_pp3_kernel<4, false, false, 3, 192, 256>", (3, 3), 0, 6536, 832, 32, 0, 0, "bias_act1"),
    ("gemm_pp3_kernel<4, false, false, 7, 192, 256>", (3, 3), 1, 6536, 832, 96, 0, 0, "bias_act2"),
    ("gemm_pp3_kernel<4, false, false, 9, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 0, "bias_act_d"),
    ("gemm_pp3_kernel<4, false, false, 10, 192, 256>", (3, 3), 0, 6536, 832, 96, 0, 0, "bias_act_erf_d"),
    ("gemm_pp3_kernel<4, false, false, 14, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 0, "qgelu"),
    ("gemm_w4r_kernel<3, true, 0>", (3, 10), 1, 328, 264, 192, 0, 1, "plain"),
    ("gemm_w4x_kernel<128, 192, false, true, 0, false>", (3, 12), 0, 328, 264, 96, 0, 1, "plain"),
    ("gemm_pp3_kernel<4, false, true, 0, 192, 128>", (3, 3), 1, 328, 448, 96, 0, 1, "plain"),
    ("gemm_w4m_kernel<3, true, 6>", (3, 10), 1, 328, 264, 192, 0, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, false, true, 6, 192, 128>", (3, 3), 0, 328, 448, 96, 0, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, false, true, 4, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 1, "dact"),
    ("gemm_pp3_kernel<4, false, true, 8, 192, 256>", (3, 3), 1, 6536, 832, 96, 0, 1, "dact_erf"),
    ("gemm_pp3_kernel<4, false, true, 11, 192, 256>", (3, 3), 0, 6536, 832, 32, 0, 1, "mul"),
    ("gemm_w4n_kernel<3, false, 0>", (3, 10), 1, 328, 392, 192, 0, 0, "plain"),
    ("gemm_pp3_kernel<4, false, false, 0, 192, 128>", (3, 3), 1, 328, 448, 32, 0, 0, "plain"),
    ("gemm_w4x_kernel<128, 192, false, false, 0, false>", (3, 12), 0, 328, 264, 96, 0, 0, "plain"),
    ("gemm_w4n_kernel<3, false, 1>", (3, 10), 1, 328, 392, 192, 0, 0, "bias"),
    ("gemm_w4n_kernel<3, false, 2>", (3, 10), 1, 328, 392, 192, 0, 0, "bias_res"),
    ("gemm_w4n_kernel<3, false, 12>", (3, 10), 0, 328, 392, 192, 0, 0, "drop_res"),
    ("gemm_w4n_kernel<3, false, 13>", (3, 10), 1, 328, 392, 192, 0, 0, "gate_res"),
    ("gemm_w4m_kernel<3, true, 0>", (3, -1), 1, 6536, 392, 192, 0, 1, "plain"),
    ("gemm_w4x_kernel<256, 192, false, true, 2, false>", (3, 12), 0, 12296, 776, 96, 0, 1, "bias_res"),
    ("gemm_pp3_kernel<4, false, true, 2, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 1, "bias_res"),
    ("gemm_w4d_kernel<true, 2>", (3, -1), 1, 12296, 264, 384, 0, 1, "bias_res"),
    ("gemm_pp3_kernel<4, false, false, 2, 256, 256>", (3, 3), 0, 328, 264, 32, 0, 0, "bias_res"),
    ("gemm_pp3_kernel<4, false, true, 2, 256, 256>", (3, 3), 1, 328, 264, 96, 0, 1, "bias_res"),
    ("gemm_w4x_kernel<128, 192, false, true, 2, false>", (3, 12), 1, 328, 264, 96, 0, 1, "bias_res"),
    ("gemm_pp3_kernel<4, false, true, 2, 192, 128>", (3, 3), 0, 328, 448, 96, 0, 1, "bias_res"),
    ("gemm_pp3_kernel<4, true, true, 6, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, true, false, 0, 192, 256>", (3, 3), 0, 6536, 832, 32, 1, 0, "plain"),
    ("gemm_pp_kernel<4, true, false>", (3, -1), 1, 12296, 776, 96, 1, 0, "gate_res"),
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, true, false>", (3, -1), 1, 328, 260, 32, 1, 0, "plain"),
    ("gemm_lds_kernel<128, 128, 2, 2, true, false>", (1, -1), 0, 328, 260, 64, 1, 0, "plain"),
    ("gemm_bf16_kernel<true, false>", (1, -1), 1, 328, 260, 32, 1, 0, "plain"),
    ("gemm_pp3_kernel<4, true, true, 0, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 1, "plain"),
    ("gemm_pp3_kernel<4, true, false, 0, 256, 256>", (3, 3), 0, 328, 264, 32, 1, 0, "plain"),
    ("gemm_pp3_kernel<4, true, false, 0, 192, 128>", (3, 3), 1, 328, 448, 96, 1, 0, "plain"),
    ("gemm_w4d_kernel<false, 6>", (3, -1), 1, 12296, 264, 384, 0, 0, "res_inplace"),
    ("gemm_pp3_kernel<4, false, false, 6, 192, 256>", (3, 3), 0, 6536, 832, 96, 0, 0, "res_inplace"),
    ("gemm_pp3_kernel<4, false, false, 6, 192, 128>", (3, 3), 1, 328, 448, 32, 0, 0, "res_inplace"),
    ("gemm_pp3_kernel<4, false, false, 9, 192, 128>", (3, 3), 1, 328, 448, 96, 0, 0, "bias_act_d"),
    ("gemm_w4_kernel<3, false, 11>", (3, -1), 0, 12296, 264, 192, 0, 0, "mul"),
    ("gemm_pp3_kernel<4, false, false, 11, 192, 256>", (3, 3), 1, 6536, 832, 96, 0, 0, "mul"),
    ("gemm_pp3_kernel<4, false, false, 11, 192, 128>", (3, 3), 1, 328, 448, 32, 0, 0, "mul"),
    ("gemm_w4_kernel<3, false, 4>", (3, -1), 0, 12296, 264, 192, 0, 0, "dact"),
    ("gemm_pp3_kernel<4, false, false, 4, 192, 256>", (3, 3), 1, 6536, 832, 32, 0, 0, "dact"),
    ("gemm_pp3_kernel<4, false, false, 4, 192, 128>", (3, 3), 1, 328, 448, 96, 0, 0, "dact"),
    ("gemm_w4_kernel<3, true, 9>", (3, -1), 0, 12296, 264, 192, 0, 1, "bias_act_d"),
    ("gemm_pp3_kernel<4, false, true, 9, 192, 256>", (3, 3), 1, 6536, 832, 96, 0, 1, "bias_act_d"),
    ("gemm_pp3_kernel<4, false, true, 9, 192, 128>", (3, 3), 1, 328, 448, 32, 0, 1, "bias_act_d"),
    ("gemm_pp3_kernel<4, false, true, 11, 192, 128>", (3, 3), 0, 328, 448, 96, 0, 1, "mul"),
    ("gemm_pp3_kernel<4, false, true, 4, 192, 128>", (3, 3), 1, 328, 448, 32, 0, 1, "dact"),
    ("gemm_pp3_kernel<4, true, false, 2, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 0, "bias_res"),
    ("gemm_pp3_kernel<4, true, false, 2, 192, 128>", (3, 3), 0, 328, 448, 32, 1, 0, "bias_res"),
    ("gemm_pp3_kernel<4, true, false, 6, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 0, "res_inplace"),
    ("gemm_pp3_kernel<4, true, false, 6, 192, 128>", (3, 3), 1, 328, 448, 32, 1, 0, "res_inplace"),
    ("gemm_pp3_kernel<4, true, false, 9, 192, 256>", (3, 3), 0, 6536, 832, 96, 1, 0, "bias_act_d"),
    ("gemm_pp3_kernel<4, true, false, 9, 192, 128>", (3, 3), 1, 328, 448, 32, 1, 0, "bias_act_d"),
    ("gemm_pp3_kernel<4, true, false, 11, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 0, "mul"),
    ("gemm_pp3_kernel<4, true, false, 11, 192, 128>", (3, 3), 0, 328, 448, 32, 1, 0, "mul"),
    ("gemm_pp3_kernel<4, true, false, 4, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 0, "dact"),
    ("gemm_pp3_kernel<4, true, false, 4, 192, 128>", (3, 3), 1, 328, 448, 32, 1, 0, "dact"),
    ("gemm_pp3_kernel<4, true, true, 2, 192, 256>", (3, 3), 0, 6536, 832, 96, 1, 1, "bias_res"),
    ("gemm_pp3_kernel<4, true, true, 2, 192, 128>", (3, 3), 1, 328, 448, 32, 1, 1, "bias_res"),
    ("gemm_pp3_kernel<4, true, true, 9, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 1, "bias_act_d"),
    ("gemm_pp3_kernel<4, true, true, 9, 192, 128>", (3, 3), 0, 328, 448, 32, 1, 1, "bias_act_d"),
    ("gemm_pp3_kernel<4, true, true, 11, 192, 256>", (3, 3), 1, 6536, 832, 96, 1, 1, "mul"),
    ("gemm_pp3_kernel<4, true, true, 11, 192, 128>", (3, 3), 1, 328, 448, 32, 1, 1, "mul"),
    ("gemm_pp3_kernel<4, true, true, 4, 192, 256>", (3, 3), 0, 6536, 832, 96, 1, 1, "dact"),
    ("gemm_pp3_kernel<4, true, true, 4, 192, 128>", (3, 3), 1, 328, 448, 32, 1, 1, "dact"),
    ("gemm_w4_kernel<3, false, 8>", (3, -1), 1, 12296, 264, 192, 0, 0, "dact_erf"),
    ("gemm_pp3_kernel<4, false, false, 8, 192, 256>", (3, 3), 0, 6536, 832, 32, 0, 0, "dact_erf"),
    ("gemm_pp3_kernel<4, false, false, 8, 192, 128>", (3, 3), 1, 328, 448, 96, 0, 0, "dact_erf"),
    ("gemm_w4d_kernel<true, 1>", (3, -1), 1, 12296, 264, 384, 0, 1, "bias"),
    ("gemm_pp3_kernel<4, false, true, 1, 192, 256>", (3, 3), 0, 6536, 832, 96, 0, 1, "bias"),
    ("gemm_pp3_kernel<4, false, true, 1, 192, 128>", (3, 3), 1, 328, 448, 32, 0, 1, "bias"),
    ("gemm_pp3_kernel<4, false, true, 8, 192, 128>", (3, 3), 1, 328, 448, 96, 0, 1, "dact_erf"),
    ("gemm_w4_kernel<3, false, 0>", (3, -1), 0, 12296, 264, 192, 0, 0, "plain"),
    ("gemm_w4_kernel<3, false, 1>", (3, -1), 1, 12296, 264, 192, 0, 0, "bias"),
    ("gemm_w4_kernel<3, false, 2>", (3, -1), 1, 12296, 264, 192, 0, 0, "bias_res"),
    ("gemm_pp3_kernel<4, false, false, 6, 256, 256>", (3, 3), 0, 328, 264, 96, 0, 0, "res_inplace"),
    ("gemm_w4_kernel<3, false, 6>", (3, -1), 1, 12296, 264, 192, 0, 0, "res_inplace"),
    ("gemm_pp3_kernel<4, false, false, 11, 256, 256>", (3, 3), 1, 328, 264, 96, 0, 0, "mul"),
    ("gemm_pp3_kernel<4, false, false, 8, 256, 256>", (3, 3), 0, 328, 264, 32, 0, 0, "dact_erf"),
    ("gemm_w4_kernel<3, true, 0>", (3, -1), 1, 12296, 264, 192, 0, 1, "plain"),
    ("gemm_pp3_kernel<4, false, true, 1, 256, 256>", (3, 3), 1, 328, 264, 32, 0, 1, "bias"),
    ("gemm_w4_kernel<3, true, 1>", (3, -1), 0, 12296, 264, 192, 0, 1, "bias"),
    ("gemm_w4_kernel<3, true, 2>", (3, -1), 1, 12296, 264, 192, 0, 1, "bias_res"),
    ("gemm_w4_kernel<3, true, 6>", (3, -1), 1, 12296, 264, 192, 0, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, false, true, 9, 256, 256>", (3, 3), 0, 328, 264, 32, 0, 1, "bias_act_d"),
    ("gemm_w4n_kernel<3, false, 6>", (3, 10), 1, 328, 392, 192, 0, 0, "res_inplace"),
    ("gemm_w4n_kernel<3, false, 9>", (3, 10), 1, 328, 392, 192, 0, 0, "bias_act_d"),
    ("gemm_w4n_kernel<3, false, 11>", (3, 10), 0, 328, 392, 192, 0, 0, "mul"),
    ("gemm_w4n_kernel<3, false, 8>", (3, 10), 1, 328, 392, 192, 0, 0, "dact_erf"),
    ("gemm_w4m_kernel<3, true, 1>", (3, 10), 1, 328, 264, 192, 0, 1, "bias"),
    ("gemm_w4m_kernel<3, true, 2>", (3, 10), 0, 328, 264, 192, 0, 1, "bias_res"),
    ("gemm_w4m_kernel<3, true, 9>", (3, 10), 1, 328, 264, 192, 0, 1, "bias_act_d"),
    ("gemm_w4m_kernel<3, true, 11>", (3, 10), 1, 328, 264, 192, 0, 1, "mul"),
    ("gemm_w4m_kernel<3, true, 8>", (3, 10), 0, 328, 264, 192, 0, 1, "dact_erf"),
    ("gemm_w4m_kernel<3, false, 0>", (3, 10), 1, 328, 264, 192, 0, 0, "plain"),
    ("gemm_w4m_kernel<3, false, 1>", (3, 10), 1, 328, 264, 192, 0, 0, "bias"),
    ("gemm_w4m_kernel<3, false, 2>", (3, 10), 0, 328, 264, 192, 0, 0, "bias_res"),
    ("gemm_w4m_kernel<3, false, 6>", (3, 10), 1, 328, 264, 192, 0, 0, "res_inplace"),
    ("gemm_w4m_kernel<3, false, 9>", (3, 10), 1, 328, 264, 192, 0, 0, "bias_act_d"),
    ("gemm_w4m_kernel<3, false, 11>", (3, 10), 0, 328, 264, 192, 0, 0, "mul"),
    ("gemm_w4m_kernel<3, false, 8>", (3, 10), 1, 328, 264, 192, 0, 0, "dact_erf"),
    ("gemm_w4m_kernel<3, false, 13>", (3, 10), 1, 328, 264, 192, 0, 0, "gate_res"),
    ("gemm_pp3_kernel<4, true, false, 6, 256, 256>", (3, 3), 0, 328, 264, 32, 1, 0, "res_inplace"),
]

# Further cases: work the instance table does not force.
_EXTRA_CASES = [
    # persistent loop: 260 tiles of 256 x 256 on 256 CUs, tiles_m % group = 4
    ("gemm_pp3_kernel<4, false, false, 2, 256, 256>", (3, -1), 1, 5000, 3080, 96, 0, 0, "bias_res"),
    # persistent loop, MN-contiguous B, 5 K-steps
    ("gemm_pp3_kernel<4, false, true, 0, 256, 256>", (3, -1), 1, 5000, 3080, 160, 0, 1, "plain", dict(kinds=('scaled',))),
    # slab split-K + gemm_splitk_reduce, persistent kernel
    ("gemm_pp3_kernel<4, false, false, 0, 256, 256>", (3, 3), 1, 328, 264, 2048, 0, 0, "bias_res"),
    # slab split-K of a weight gradient, C += AB
    ("gemm_pp3_kernel<4, true, true, 0, 256, 256>", (3, 3), 1, 520, 392, 4096, 1, 1, "res_inplace"),
    # slab split-K, ring kernel: the reduce runs the activation
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, 11), 1, 328, 264, 2048, 0, 0, "bias_act1"),
    # slab split-K, ping-pong kernel
    ("gemm_pp_kernel<4, false, true>", (2, 4), 1, 328, 264, 2048, 0, 1, "bias"),
    # slab split-K, LDS-DMA kernel, dropout in the reduce
    ("gemm_lds_kernel<128, 128, 2, 2, false, false>", (1, -1), 1, 328, 264, 2048, 0, 0, "drop_res"),
    # in-launch two-way combine: the tickets return to zero
    ("gemm_pp3_kernel<4, false, false, 2, 256, 256>", (3, 13), 1, 5000, 1032, 512, 0, 0, "bias_res"),
    # in-launch combine, MN-contiguous B
    ("gemm_pp3_kernel<4, false, true, 0, 256, 256>", (3, 13), 1, 5000, 1032, 576, 0, 1, "plain", dict(kinds=('scaled', 'exact'))),
    # fp32 C, N % 8 == 4
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 328, 260, 96, 0, 0, "c_fp32"),
    # fp32 C without workspace
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, true>", (3, -1), 0, 520, 264, 160, 0, 1, "c_fp32"),
    # alpha and alpha_ptr (powers of two: the exact inputs stay exact)
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 328, 264, 96, 0, 0, "bias", dict(alpha=0.5, alpha_dev=0.25)),
    # alpha and alpha_ptr, persistent kernel
    ("gemm_pp3_kernel<4, false, false, 2, 192, 128>", (3, 3), 1, 328, 448, 96, 0, 0, "bias_res", dict(alpha=-1.5, alpha_dev=0.75)),
    # alpha in front of an activation, four-wave kernel
    ("gemm_w4m_kernel<3, false, 7>", (3, 10), 1, 328, 264, 192, 0, 0, "bias_act2", dict(alpha=0.375)),
    # generic epilogue: activation and residual
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 328, 264, 96, 0, 0, "gen_act_res"),
    # generic epilogue: dropout, gate, residual, 8-byte stores
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 328, 260, 160, 0, 0, "gen_gate_drop"),
    # generic epilogue asked of the persistent kernel
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, 3), 1, 328, 448, 96, 0, 0, "gen_gate_drop"),
    # dropout re-keyed through seed_ptr
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 328, 264, 96, 0, 0, "drop_res", dict(seed_off=12345)),
    # dropout re-keyed through seed_ptr, four-wave kernel
    ("gemm_w4m_kernel<3, false, 12>", (3, 10), 1, 328, 264, 192, 0, 0, "drop_res", dict(seed_off=7)),
    # ldc % 8 == 4: no 16-byte row stores
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 328, 264, 96, 0, 0, "bias_res", dict(pad=4)),
    # K % 32 != 0: the register-staged kernel, a K tail
    ("gemm_bf16_kernel<false, false>", (3, -1), 1, 520, 264, 72, 0, 0, "bias_res"),
    # K % 32 != 0, both operands MN-contiguous
    ("gemm_bf16_kernel<true, true>", (3, -1), 1, 520, 264, 72, 1, 1, "res_inplace"),
    # register-staged kernel, long K with a tail, gate
    ("gemm_bf16_kernel<false, false>", (0, -1), 1, 328, 260, 1000, 0, 0, "gate_res"),
]

# Instances whose planner admits nothing under the cost cap, with the condition: they run the
# *exact* inputs only, against an fp32 reference, at the smallest shape admitted.
_EXCLUDED = [
    # the single weight gradient on the AGPR kernel: gemm_w4x_plan needs K >= 4096 and w4x_dw_plan
    # >= 230 tiles of 256 x 256 / 256 x 192 (90 % of the CUs); 256-wide: 64 x 4 tiles
    ("gemm_w4x_kernel<256, 256, true, true, 6, false>", (3, -1), 1, 16136, 776, 4096, 1, 1, "res_inplace"),
    # the same with 256 x 192 tiles: 49 x 5 = 245 tiles fill the last round better than 49 x 4
    ("gemm_w4x_kernel<256, 192, true, true, 6, false>", (3, -1), 1, 12296, 776, 4096, 1, 1, "res_inplace"),
]

CASES = [_case(i, t) for i, t in enumerate(_ROUTE_CASES + _EXTRA_CASES)]
EXCLUDED_CASES = [_case(800 + i, t) for i, t in enumerate(_EXCLUDED)]
EXCLUDED = [c["name"] for c in EXCLUDED_CASES]
# tune settings under which one K-contiguous descriptor takes different routes (route agreement)
AGREE_TUNES = [(3, -1), (3, 3), (3, 12), (2, 6), (2, 4), (2, 0), (2, 1), (1, -1), (0, -1)]
