"""Int8 weight-only decoding without a GPU: the properties of the quantiser's CPU restatement
(tests/quant_ref.py), the linear reference's power to reject doctored outputs that a max-norm
comparison accepts, the host-side refusals of the three entry points (nothing is launched, every
sentinel-filled output stays untouched), and the `weights` argument check of gvl.decode."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quant_ref as Q
from tests.gemm_ref import round_bf16
from tests.helpers import TINY, f64, rel_err, ulp_bf16
from tests.test_capi import SENT16, _host

BF = torch.bfloat16


def _w(N=24, K=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, K, generator=g).to(BF)


# ------------------------------------------------------------------------- the quantiser
def test_dequantised_weight_within_half_a_scale():
    w = _w()
    q, s = Q.quantize(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    err = (q.double() * s.double()[:, None] - w.double()).abs()
    # |q - w / s| <= 1/2 + the rounding of the fp32 quotient, itself <= 127 * 2**-24 < 2**-17
    assert (err <= s.double()[:, None] / 2 * (1 + 2.0 ** -16)).all()
    # and the bf16 the prefill multiplies by is that product, rounded once
    assert torch.equal(Q.dequantize(q, s), (q.float() * s[:, None]).to(BF))


def test_absmax_maps_to_127_either_sign_any_column():
    w = _w(8, 64)
    w[0, 5], w[1, 63], w[2, 0], w[3, 63] = 9.0, -9.0, -9.0, 9.0  # last column, negative
    q, s = Q.quantize(w)
    assert q[0, 5] == 127 and q[1, 63] == -127 and q[2, 0] == -127 and q[3, 63] == 127
    assert (q.abs().amax(1) == 127).all() and int(q.min()) >= -127
    assert torch.equal(s[:4], torch.full((4,), 9.0) / torch.full((4,), 127.0))


def test_zero_row_has_zero_scale_and_values():
    w = _w(8, 64)
    w[3] = 0
    w[5] = -0.0
    q, s = Q.quantize(w)
    assert s[3] == 0 and s[5] == 0 and (q[3] == 0).all() and (q[5] == 0).all()
    assert (Q.dequantize(q, s)[3] == 0).all()


def test_ties_round_to_even_on_a_power_of_two_scale():
    w = torch.zeros(8, 64, dtype=BF)
    w[0, 0] = 127.0 * 0.25      # absmax: scale = 0.25 exactly
    w[0, 1], w[0, 2] = 2.5 * 0.25, 3.5 * 0.25
    w[0, 3], w[0, 4] = -2.5 * 0.25, -0.5 * 0.25
    q, s = Q.quantize(w)
    assert s[0] == 0.25
    assert q[0, :5].tolist() == [127, 2, 4, -2, 0]


# --------------------------------------------------- the linear reference rejects doctoring
def _case(epi="bias"):
    M, N, K = 5, 24, 64
    ins = Q.inputs("random", M, N, K, seed=3)
    w = ins["w"].clone()
    w[:, 0] = 4.0          # every row's absmax ...
    w[1, 0] = 4.0625       # ... but row 1's: neighbouring scales 1.6 % apart
    ins["w"] = w
    ins["q"], ins["scale"] = Q.quantize(w)
    ins["bias"] = (ins["bias"].float() * 0.125).to(BF)
    kw = Q.epi_operands(epi, ins)
    return ins, kw, Q.linear_reference(ins["x"], ins["q"], ins["scale"], **kw)


def _maxnorm_accepts(got, R):
    return rel_err(f64(got), R["ref"]) < 3e-2  # the decoder tests' max-norm bound


def test_reference_accepts_the_correctly_rounded_result():
    for epi in Q.EPIS:
        ins, kw, R = _case(epi)
        assert R["slack"] < 8, R  # a handful of fp32 roundings, as gemm_ref's cases
        Q.check(round_bf16(R["ref"]), R, epi)


def test_reference_rejects_one_element_one_ulp_off():
    ins, kw, R = _case()
    got = round_bf16(R["ref"]).clone()
    i = (2, 7)
    bits = got.view(torch.int16)
    bits[i] += 1  # the next bf16 away from zero
    assert abs(float(got[i]) - R["ref"][i]) >= 0.99 * ulp_bf16(R["ref"][i]) / 2
    assert _maxnorm_accepts(got, R)
    with pytest.raises(AssertionError, match="out of tolerance"):
        Q.check(got, R)


def test_reference_rejects_a_neighbours_scale():
    ins, kw, R = _case()
    s = ins["scale"].clone()
    assert s[0] != s[1]
    s[1] = s[0]
    wrong = Q.linear_reference(ins["x"], ins["q"], s, **kw)["ref"]
    got = round_bf16(wrong)
    assert _maxnorm_accepts(got, R)
    with pytest.raises(AssertionError, match="out of tolerance"):
        Q.check(got, R)


def test_reference_rejects_the_bias_added_before_the_scale():
    ins, kw, R = _case()
    h = f64(ins["x"]) @ f64(ins["q"]).T
    wrong = (h + f64(ins["bias"])[None, :]) * f64(ins["scale"])[None, :]
    got = round_bf16(wrong)
    assert _maxnorm_accepts(got, R)
    with pytest.raises(AssertionError, match="out of tolerance"):
        Q.check(got, R)


def test_exact_inputs_leave_no_slack_on_the_linear_epilogues():
    ins = Q.inputs("exact", 5, 24, 128, seed=1)
    for wt in ("i8", "bf16"):
        P = Q.products(ins["x"], ins["q"] if wt == "i8" else ins["w"],
                       ins["scale"] if wt == "i8" else None)
        for epi in Q.LINEAR_EPIS:
            assert Q.reference(P, **Q.epi_operands(epi, ins))["slack"] == 0


# ------------------------------------------------------------------ host-side refusals
def _lib():
    from gvl import _lib
    return _lib, _lib.load()


def test_linear_w8_refuses_bad_arguments_before_any_launch():
    """Every GVL_REQUIRE of gvl_linear_w8: K = 96, N = 12, a misaligned c, M above the cap, the
    unsupported epilogues, null operands, bad leading dimensions: -1 with its message, and the
    sentinel-filled output is untouched (host memory stands in for the device's: a call that got
    past its check would fail with the launch's error instead)."""
    L, lib = _lib()
    M, N, K = 4, 16, 64
    x = _host(300 * 128, np.uint16, 0x3F80)
    w = _host(64 * 128, np.int8, 1)
    scale = _host(64, np.float32, 1.0)
    bias = _host(64, np.uint16, 0x3F80)
    res = _host(300 * 64, np.uint16, 0x3F80)
    gate = _host(8, np.uint16, 0x3F80)
    c = _host(300 * 64 + 8, np.uint16, SENT16)
    P = lambda a, off=0: a.ctypes.data + off

    def call(m=M, n=N, k=K, ldx=None, ldw=None, ldc=None, ldr=None, xp=P(x), wp=P(w), cp=P(c),
             sp=P(scale), bp=None, act=0, rp=None, gp=None, desc=True):
        d = L.LinearW8Desc()
        d.x, d.w, d.scale, d.c = xp, wp, sp, cp
        d.m, d.n, d.k = m, n, k
        d.ldx, d.ldw, d.ldc = ldx or k, ldw or k, ldc or n
        d.bias, d.act, d.residual, d.gate = bp, act, rp, gp
        d.ldr = (ldr or n) if rp else 0
        return lib.gvl_linear_w8(ctypes.byref(d) if desc else None, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (c == SENT16).all()

    refused(call(k=96), b"K must be a multiple of 64")
    refused(call(k=0), b"K must be a multiple of 64")
    refused(call(n=12), b"N must be a multiple of 8")
    refused(call(n=0), b"N must be a multiple of 8")
    refused(call(m=L.LINEAR_W8_MAX_ROWS + 1), b"outside 1..256 rows")
    refused(call(m=0), b"outside 1..256 rows")
    align = b"operands must be 16-byte aligned"
    refused(call(cp=P(c, 8)), align)
    refused(call(cp=P(c, 2)), align)
    refused(call(xp=P(x, 8)), align)
    refused(call(wp=P(w, 8)), align)
    refused(call(sp=P(scale, 4)), align)
    refused(call(bp=P(bias, 2)), align)
    refused(call(bp=P(bias), rp=P(res, 8)), align)
    null = b"null operand"
    refused(call(xp=None), null)
    refused(call(wp=None), null)
    refused(call(cp=None), null)
    refused(call(desc=False), b"null descriptor")
    epi = b"unsupported epilogue"
    refused(call(act=1), epi)                                  # GELU without a bias
    refused(call(bp=P(bias), act=2), epi)                      # erf-GELU
    refused(call(rp=P(res)), epi)                              # residual without a bias
    refused(call(bp=P(bias), gp=P(gate)), epi)                 # gate without a residual
    refused(call(bp=P(bias), act=1, rp=P(res)), epi)           # GELU + residual
    refused(call(gp=P(gate)), epi)
    ld = b"bad leading dimension"
    refused(call(ldx=72 - 4), ld)      # ldx % 8
    refused(call(ldx=56), ld)          # ldx < K
    refused(call(ldw=72), ld)          # int8 rows: ldw % 16
    refused(call(sp=None, ldw=68), ld)  # bf16 rows: ldw % 8
    refused(call(ldc=18), ld)
    refused(call(ldc=8), ld)           # ldc < N
    refused(call(bp=P(bias), rp=P(res), ldr=18), ld)


def test_quantiser_and_dequantiser_refuse_bad_arguments_before_any_launch():
    L, lib = _lib()
    w = _host(8 * 128, np.uint16, 0x3F80)
    q = _host(8 * 128 + 16, np.int8, 7)
    scale = _host(16, np.float32, 7.0)
    out = _host(8 * 128 + 8, np.uint16, SENT16)
    P = lambda a, off=0: a.ctypes.data + off

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (q == 7).all() and (scale == 7.0).all() and (out == SENT16).all()

    qz = lambda wp=P(w), ldw=64, n=8, k=64, qp=P(q), ldq=64, sp=P(scale): \
        lib.gvl_quantize_rows_i8(wp, ldw, n, k, qp, ldq, sp, None)
    refused(qz(wp=None), b"gvl_quantize_rows_i8: null operand")
    refused(qz(qp=None), b"gvl_quantize_rows_i8: null operand")
    refused(qz(sp=None), b"gvl_quantize_rows_i8: null operand")
    shape = b"gvl_quantize_rows_i8: shape unsupported"
    refused(qz(k=60), shape)
    refused(qz(k=0), shape)
    refused(qz(n=0), shape)
    refused(qz(ldw=68), shape)
    refused(qz(ldq=56), shape)
    refused(qz(qp=P(q, 8)), b"gvl_quantize_rows_i8: operands must be 16-byte aligned")
    refused(qz(wp=P(w, 2)), b"gvl_quantize_rows_i8: operands must be 16-byte aligned")

    dq = lambda qp=P(q), ldq=64, sp=P(scale), n=8, k=64, op=P(out), ldo=64: \
        lib.gvl_dequantize_rows_i8(qp, ldq, sp, n, k, op, ldo, None)
    refused(dq(qp=None), b"gvl_dequantize_rows_i8: null operand")
    refused(dq(op=None), b"gvl_dequantize_rows_i8: null operand")
    shape = b"gvl_dequantize_rows_i8: shape unsupported"
    refused(dq(k=60), shape)
    refused(dq(ldo=68), shape)
    refused(dq(ldq=32), shape)
    refused(dq(op=P(out, 8)), b"gvl_dequantize_rows_i8: operands must be 16-byte aligned")
    refused(dq(sp=P(scale, 4)), b"gvl_dequantize_rows_i8: operands must be 16-byte aligned")


# --------------------------------------------------------------- the weights argument
def test_unknown_weights_value_raises_before_touching_a_device():
    import gvl.gpt2 as g2
    from gvl import decode as D
    model = g2.GPT(g2.GPTConfig(**TINY))  # on the CPU: any launch would raise its own error
    ids = torch.zeros(1, 4, dtype=torch.int64)
    for call in (lambda: D.generate(model, ids, 4, weights="int4"),
                 lambda: D.generate(model, ids, 4, weights="int4", graph=True),
                 lambda: D.beam_search(model, ids, 4, weights="int4"),
                 lambda: D.speculative_generate(model, ids, 4, weights=8),
                 lambda: D.KVDecoder(model, 1, 4, weights="fp8"),
                 lambda: D.BeamDecoder(model, 1, 2, 4, weights="INT8"),
                 lambda: D.GraphedGenerate(model, 4, 4, weights="int4"),
                 lambda: D.GraphedBeamSearch(model, 4, 4, weights="int4")):
        with pytest.raises(ValueError, match='"int8"'):
            call()
