"""Per-element parity of the row-wise and element-wise kernels on the MI355X.

tests/helpers.py::rel_err divides by the largest element of the whole tensor, which hides almost
everything in outputs that span orders of magnitude (AdamW state, softmax gradients, LayerNorm
rows of different scale) and, in a GEMM output, a truncating final rounding, bf16 split-K
partials and wrong rows or columns of small scale (tests/test_gemm_ref_cpu.py; the GEMMs are
held per element by tests/test_gpu_gemm.py).  Here every element is compared with a
float64 CPU reference that reads the same bf16 / fp32 inputs as the kernel, one step from given
inputs: bf16 outputs to one bf16 ulp (helpers.assert_bf16_close), fp32 outputs to a count of
fp32 roundings (helpers.assert_f32_close) taken from the same formula in fp32 torch on the CPU
times four, row movers bit for bit.  tests/test_helpers_cpu.py shows that these assertions
reject the doctored outputs rel_err accepts.  The measured margins go to
profiles/rowwise_margins.json through helpers.margins_out."""
import math

import numpy as np
import pytest
import torch

from tests import rowwise_ref as R
from tests.helpers import (F32_UNIT, assert_bf16_close, assert_f32_close, f64, margins_out,
                           ulp_bf16)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
SENT = 7.0

_MARGINS = {}


def _record(key, rec):
    _MARGINS[key] = rec
    margins_out("rowwise_margins", _MARGINS)


def _k():
    from gvl import kernels as K
    return K


def _arena(t, cuda):
    """t at a 16-byte-aligned, non-zero offset inside a sentinel-filled buffer on the device:
    (the view the kernel gets, a check that nothing outside it was written)."""
    off, n = 16 // t.element_size(), t.numel()
    big = torch.full((n + 2 * off,), SENT, dtype=t.dtype)
    big[off:off + n] = t
    big = big.to(cuda)

    def untouched():
        return bool(torch.all(big[:off] == SENT)) and bool(torch.all(big[off + n:] == SENT))

    return big[off:off + n], untouched


def _bound_used(got, ref64, scale, slack):
    """The worst |got - ref| as a fraction of assert_bf16_close's bound (what the margins file
    keeps next to the error in ulps, which says little where the reference cancels to ~0)."""
    tol = ulp_bf16(ref64) + slack * F32_UNIT * np.abs(f64(scale))
    return float((np.abs(f64(got) - f64(ref64)) / tol).max()) if np.size(ref64) else 0.0


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------ AdamW
def _adam_run(cuda, entry, n, step, nd):
    """One step of entry point `entry` from rowwise_ref.adam_inputs -> (outputs on the CPU,
    float64 reference)."""
    K_ = _k()
    h = R.ADAM
    p32, g, m32, v32 = R.adam_inputs(n)
    gs = R.adam_scaled_grad(g)
    gd, g_ok = _arena(g, cuda)
    scale = torch.tensor([h["gscale"]], dtype=F32, device=cuda)
    hyper = torch.tensor([h["lr"], float(step)], dtype=F32, device=cuda)
    hp = (h["b1"], h["b2"], h["eps"], h["wd"])
    if entry == "adamw_master_dev":
        ref = R.adamw_ref64(p32, gs, m32, v32, nd, step)
        pd, p_ok = _arena(torch.full((n,), float("nan"), dtype=BF), cuda)  # output only
        wd_, w_ok = _arena(p32, cuda)
        md, m_ok = _arena(m32, cuda)
        vd, v_ok = _arena(v32, cuda)
        K_.adamw_master_dev(pd, wd_, gd, md, vd, nd, hyper, *hp, grad_scale=scale)
        got = dict(p=wd_.cpu(), m=md.cpu(), v=vd.cpu(), p_bf16=pd.cpu())
        assert w_ok()
    else:
        p, m, v = p32.to(BF), m32.to(BF), v32.to(BF)
        ref = R.adamw_ref64(p, gs, m, v, nd, step)
        pd, p_ok = _arena(p, cuda)
        md, m_ok = _arena(m, cuda)
        vd, v_ok = _arena(v, cuda)
        if entry == "adamw_dev":
            K_.adamw_dev(pd, gd, md, vd, nd, hyper, *hp, grad_scale=scale)
        else:
            K_.adamw(pd, gd, md, vd, nd, h["lr"], *hp, step, scale)
        got = dict(p=pd.cpu(), m=md.cpu(), v=vd.cpu())
        ref["before"] = dict(p=p, m=m, v=v)
    torch.cuda.synchronize()
    assert p_ok() and m_ok() and v_ok() and g_ok(), "a store outside the arena"
    assert torch.equal(gd.cpu(), g)
    return got, ref


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("n", R.ADAM_SIZES)
@pytest.mark.parametrize("entry", ["adamw", "adamw_dev"])
def test_adamw_bf16_per_element(cuda, entry, n, step):
    """gvl_adamw / gvl_adamw_dev (bf16 p, m, v): every element of p, m and v within one bf16 ulp
    of the float64 step (+ 4 x the CPU fp32 baseline of rowwise_ref.adam_baseline in
    2**-24 * (sum of |terms|), which matters only where 0.9 m + 0.1 g or p - update cancel),
    for n_decay in {0, 3, n - 3, n}; n = 5 is tail only, 8 one vector, 6149 three blocks + tail.
    The reference itself moves >= 95 % of m and v (and of p at step 1; >= 90 % later: 93.0 %
    measured on the reference) by a bf16 ulp or more, so a kernel that does nothing fails.
    Measured on the MI355X: worst error 0.49998 ulp (p), 0.50001 (m), 0.50001 (v): correctly
    rounded but for near-ties, for both entry points alike."""
    base = R.adam_baseline()
    worst = dict(p=0.0, m=0.0, v=0.0)
    for nd in R.adam_decays(n):
        got, ref = _adam_run(cuda, entry, n, step, nd)
        for k in "pmv":
            e = assert_bf16_close(got[k], ref[k], scale=ref["scale_" + k], slack=4 * base[k],
                                  name=f"{entry} n={n} step={step} n_decay={nd} {k}")
            worst[k] = max(worst[k], e)
        if n == R.ADAM_BIG:
            b = ref["before"]
            assert R.moved_fraction(b["p"], ref["p"]) >= (0.95 if step == 1 else 0.90)
            assert R.moved_fraction(b["m"], ref["m"]) >= 0.95
            assert R.moved_fraction(b["v"], ref["v"]) >= 0.95
    print(f"{entry} n={n} step={step}: worst error in bf16 ulps {worst}")
    _record(f"{entry}:n{n}:step{step}", dict(worst_ulp=worst, cpu_baseline_units=base))


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adamw_master_per_element(cuda, n, step):
    """gvl_adamw_master_dev: the fp32 master weights and moments within 4 x the CPU baseline
    of 2**-24 * (sum of |terms|) of the float64 step (the same formula in fp32 torch on the CPU
    is off by at most 3.17 - 3.86 such units for p, depending on the host's pow, 1.62 for m, 2.16
    for v; the device's powf, sqrtf and division need not round like the host's), and the bf16
    copy equal to the rounded master bit for bit.  This is the path that can see the n_decay
    boundary: lr * wd = 1e-4 relative is far below a bf16 ulp.
    Measured on the MI355X: p 2.83, m 1.54, v 2.16 units, against bounds of 12.7, 6.5 and 8.6."""
    base = R.adam_baseline()
    worst = dict(p=0.0, m=0.0, v=0.0)
    for nd in R.adam_decays(n):
        got, ref = _adam_run(cuda, "adamw_master_dev", n, step, nd)
        for k in "pmv":
            e = assert_f32_close(got[k], ref[k], ref["scale_" + k], 4 * base[k],
                                 name=f"master n={n} step={step} n_decay={nd} {k}")
            worst[k] = max(worst[k], e)
        assert torch.equal(_bits(got["p_bf16"]), _bits(got["p"].to(BF)))
    print(f"adamw_master_dev n={n} step={step}: measured {worst} of 4 x baseline {base}")
    _record(f"adamw_master_dev:n{n}:step{step}",
            dict(kernel_units=worst, cpu_baseline_units=base,
                 bound_units={k: 4 * x for k, x in base.items()}))


@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adamw_dev_matches_host_bias_correction(cuda, n):
    """Step 1: gvl_adamw_dev (lr / step read on the device, powf) and gvl_adamw (bias
    corrections from the host's double pow) agree to one bf16 ulp on every output."""
    for nd in (0, n):
        a, _ = _adam_run(cuda, "adamw", n, 1, nd)
        b, _ = _adam_run(cuda, "adamw_dev", n, 1, nd)
        for k in "pmv":
            assert_bf16_close(b[k], f64(a[k]), name=f"adamw_dev vs adamw n={n} {k}")


# -------------------------------------------------------------------------- grad_norm
@pytest.mark.parametrize("n", [8 * 256 * 1024 + 8 * 300 + 5, 5])
def test_grad_norm_grid_stride_and_tail(cuda, n):
    """More vectors than RED_MAXB blocks hold in one trip (the grid-stride loop) plus a ragged
    tail, and a tail-only input: the norm to 1e-6 of the float64 norm, the clip coefficient
    min(1, max / (norm + 1e-6)) on both sides of the clip (three fp32 roundings from the
    kernel's own norm)."""
    K_ = _k()
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(BF)
    want = math.sqrt(float((f64(g) ** 2).sum()))
    gd = g.to(cuda)
    for max_norm, clipped in ((0.25 * want, True), (4.0 * want, False)):
        out = K_.grad_norm(gd, max_norm).cpu()
        nrm, coef = float(out[0]), float(out[1])
        assert abs(nrm - want) / want < 1e-6, (nrm, want)
        if clipped:
            c = float(np.float32(max_norm)) / (nrm + 1e-6)
            assert abs(coef - c) <= 3 * 2.0 ** -24 * c and coef < 1.0, (coef, c)
            assert abs(coef - 0.25) < 1e-6
        else:
            assert coef == 1.0


# -------------------------------------------------------------------------- LayerNorm
def _ln_slacks(base=None):
    base = base or R.ln_baseline()
    # y = (x - mean) * rstd * w + b: the errors of mean and rstd, then a subtraction, two
    # products and a sum (one fp32 rounding each)
    return base, 4 * base["mean"], 4 * base["rstd"], 4 * (base["mean"] + base["rstd"]) + 4


def _ln_check_fwd(x, w, b, y, mean, rstd, name, base=None):
    base, sm, sr, sy = _ln_slacks(base)
    ref = R.ln_ref64(x, w, b)
    em = assert_f32_close(mean.cpu(), ref["mean"], ref["scale_mean"], sm, name=name + " mean")
    er = assert_f32_close(rstd.cpu(), ref["rstd"], ref["scale_rstd"], sr, name=name + " rstd")
    assert_bf16_close(y.cpu(), ref["y"], scale=ref["scale_y"], slack=sy, name=name + " y")
    return ref, em, er


@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_layernorm_per_row(cuda, rows, C):
    """Rows scaled by 2**-6 .. 2**6 (a global max-norm sees only the largest): mean and rstd
    against float64 within 4 x the CPU fp32 baseline (two-pass torch: 0.90 units of
    2**-24 * mean|x| for the mean, 2.53 units of 2**-24 * rstd for rstd), y per element to one
    bf16 ulp, dx (plain, and accumulated in place over the residual) per element as in
    test_layernorm_bwd_dx_every_route.  Then x and y as column slices (ld = C + 8) of
    sentinel-filled buffers with stats=False: the same y bit for bit, nothing outside the slice
    written, NaNs next to x never read.  C = 8 is the minimum, 776 the first width of the
    IT = 4 instantiation; 9 and 37 rows leave half-filled forward blocks.
    Measured on the MI355X: mean at most 0.50, rstd 1.68 units, against bounds of 3.6 and 10.1."""
    K_ = _k()
    x, w, b, dy, prev = R.ln_inputs(rows, C)
    xd, wd_, bd, dyd = x.to(cuda), w.to(cuda), b.to(cuda), dy.to(cuda)
    y, mean, rstd = K_.layernorm_fwd(xd, wd_, bd, eps=R.LN_EPS)
    name = f"layernorm {rows}x{C}"
    ref, em, er = _ln_check_fwd(x, w, b, y, mean, rstd, name)
    print(f"{name}: mean {em:.2f} rstd {er:.2f} units; CPU baseline {R.ln_baseline()}")
    _record(f"layernorm:{rows}x{C}", dict(kernel_units=dict(mean=em, rstd=er),
                                          cpu_baseline_units=R.ln_baseline()))
    # backward from the kernel's own statistics (what the product feeds it)
    slack = R.ln_bwd_slack()["dx"]
    want, scale = R.ln_bwd_dx_ref64(dy, x, w, mean.cpu(), rstd.cpu())
    dx = K_.layernorm_bwd(dyd, xd, wd_, mean, rstd)
    assert_bf16_close(dx.cpu(), want, scale=scale, slack=slack, name=name + " dx")
    acc = prev.to(cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dx=acc, accumulate_dx=True)  # dx aliases the residual
    wantp, scalep = R.ln_bwd_dx_ref64(dy, x, w, mean.cpu(), rstd.cpu(), prev)
    assert_bf16_close(acc.cpu(), wantp, scale=scalep, slack=slack, name=name + " dx += ")
    # strided views, no statistics
    xbuf = torch.full((rows, C + 8), float("nan"), dtype=BF, device=cuda)
    xbuf[:, 8:] = xd
    ybuf = torch.full((rows + 1, C + 8), SENT, dtype=BF, device=cuda)
    y2, m2, r2 = K_.layernorm_fwd(xbuf[:, 8:], wd_, bd, eps=R.LN_EPS, out=ybuf[:rows, :C],
                                  stats=False)
    assert m2 is None and r2 is None
    assert torch.equal(_bits(ybuf[:rows, :C]), _bits(y))
    assert torch.all(ybuf[:, C:] == SENT) and torch.all(ybuf[rows:] == SENT)
    dbuf = torch.full((rows + 1, C + 8), SENT, dtype=BF, device=cuda)
    K_.layernorm_bwd(dyd, xbuf[:, 8:], wd_, mean, rstd, dx=dbuf[:rows, 8:])
    assert torch.equal(_bits(dbuf[:rows, 8:]), _bits(dx))
    assert torch.all(dbuf[:, :8] == SENT) and torch.all(dbuf[rows:] == SENT)


@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_layernorm_constant_and_offset_rows(cuda, C):
    """A row of zero variance: rstd = 1 / sqrt(eps) and y = b exactly.  Rows x = +-(256 +
    {0, 2, 4}), exact in bf16: a one-pass variance E[x^2] - mean^2 in fp32 loses rstd on them
    (tests/test_helpers_cpu.py), the two-pass form stays within the same bound as above.
    Measured on the MI355X: mean 0.90 (its final rounding at C = 776, as on the CPU), rstd 2.68
    units (C = 1024), against bounds of 3.6 and 10.1."""
    K_ = _k()
    x = R.ln_special_rows(C)
    _, w, b, _, _ = R.ln_inputs(3, C, seed=1)
    y, mean, rstd = K_.layernorm_fwd(x.to(cuda), w.to(cuda), b.to(cuda), eps=R.LN_EPS)
    _, em, er = _ln_check_fwd(x, w, b, y, mean, rstd, f"layernorm special rows C={C}")
    _record(f"layernorm:special:{C}", dict(kernel_units=dict(mean=em, rstd=er),
                                           cpu_baseline_units=R.ln_baseline()))
    assert float(mean[0]) == 3.25
    want = 1.0 / math.sqrt(float(np.float32(R.LN_EPS)))
    assert abs(float(rstd[0]) - want) <= _ln_slacks()[2] * 2.0 ** -24 * want
    assert torch.equal(_bits(y[0]), _bits(b))


@pytest.mark.parametrize("rows,C", R.LN_FWD_TALL)
def test_layernorm_fwd_second_persistent_pass(cuda, rows, C):
    """More than LN_FWD_MAXB * 8 = 8192 rows: the half-waves of the persistent forward take a
    second row (8192: the last size with one pass; 8193: one half-wave alone in the second;
    8203: a full block and a partial one).  Same bounds as test_layernorm_per_row from a CPU
    baseline of these shapes' own (rowwise_ref.ln_fwd_tall_baseline: mean 0.98, rstd 4.14
    units).
    Measured on the MI355X: mean at most 0.90, rstd 3.38 units, against bounds of 3.9 and 16.6."""
    K_ = _k()
    x, w, b, _, _ = R.ln_inputs(rows, C)
    y, mean, rstd = K_.layernorm_fwd(x.to(cuda), w.to(cuda), b.to(cuda), eps=R.LN_EPS)
    base = R.ln_fwd_tall_baseline()
    _, em, er = _ln_check_fwd(x, w, b, y, mean, rstd, f"layernorm {rows}x{C}", base=base)
    _record(f"layernorm:tall:{rows}x{C}", dict(kernel_units=dict(mean=em, rstd=er),
                                               cpu_baseline_units=base))


# ----------------------------------------------------------------- LayerNorm backward
def _ln_stats(cuda, x, w, b):
    """The kernel's own fp32 statistics (what the product feeds the backward; exact inputs of
    the reference) -> (x, w on the device, mean, rstd)."""
    xd, wd_ = x.to(cuda), w.to(cuda)
    _, mean, rstd = _k().layernorm_fwd(xd, wd_, b.to(cuda), eps=R.LN_EPS)
    return xd, wd_, mean, rstd


def _nan_view(t, cuda, ld, off):
    """t as columns off .. off + C of a NaN-filled [rows, ld] buffer on the device."""
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=cuda)
    buf[:, off:off + t.shape[1]] = t.to(cuda)
    return buf[:, off:off + t.shape[1]]


def _ln_bwd_dx_routes(cuda, x, w, b, dy, prev, name):
    """dx on the three routes and the strided run -> (worst error in bf16 ulps, worst fraction
    of the bound used)."""
    K_ = _k()
    rows, C = x.shape
    slack = R.ln_bwd_slack()["dx"]
    xd, wd_, mean, rstd = _ln_stats(cuda, x, w, b)
    dyd = dy.to(cuda)
    want, scale = R.ln_bwd_dx_ref64(dy, x, w, mean.cpu(), rstd.cpu())
    wantp, scalep = want + f64(prev), scale + np.abs(f64(prev))
    dx = torch.full((rows, C), float("nan"), dtype=BF, device=cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dx=dx)
    e1 = assert_bf16_close(dx.cpu(), want, scale=scale, slack=slack, name=name + " dx")
    u1 = _bound_used(dx.cpu(), want, scale, slack)
    acc = prev.to(cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dx=acc, accumulate_dx=True)
    e2 = assert_bf16_close(acc.cpu(), wantp, scale=scalep, slack=slack, name=name + " dx +=")
    u2 = _bound_used(acc.cpu(), wantp, scalep, slack)
    prev_d = prev.to(cuda)
    dx2 = torch.full((rows, C), float("nan"), dtype=BF, device=cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dx=dx2, residual=prev_d)
    assert torch.equal(_bits(dx2), _bits(acc)), name + ": residual route differs from in place"
    assert torch.equal(_bits(prev_d), _bits(prev)), name + ": the residual was written"
    # four leading dimensions at once; NaN next to every operand, sentinels around dx
    dbuf = torch.full((rows + 1, C + 32), SENT, dtype=BF, device=cuda)
    K_.layernorm_bwd(_nan_view(dy, cuda, C + 8, 8), _nan_view(x, cuda, C + 16, 16), wd_, mean, rstd,
                     dx=dbuf[:rows, 16:16 + C], residual=_nan_view(prev, cuda, C + 24, 8))
    assert torch.equal(_bits(dbuf[:rows, 16:16 + C]), _bits(dx2)), name + ": strided run differs"
    assert torch.all(dbuf[:, :16] == SENT) and torch.all(dbuf[:, 16 + C:] == SENT)
    assert torch.all(dbuf[rows:] == SENT)
    return max(e1, e2), max(u1, u2)


@pytest.mark.parametrize("rows,C", R.LN_BWD_SHAPES)
def test_layernorm_bwd_dx_every_route(cuda, rows, C):
    """Every element of dx within one bf16 ulp + 4 x max(CPU baseline, 1) fp32 roundings of the
    added terms, rstd * (|g| + mean|g| + |xh| mean|g xh|) + |prev|, of the float64 backward from
    the kernel's own statistics: stored, accumulated in place over prev, and with prev as a
    separate residual (the last two bit-identical, the residual's bits kept).  Then dy, x, the
    residual and dx with four different leading dimensions, the inputs inside NaN-filled
    buffers, dx inside sentinels: the same bits, nothing else written.  Widths 256 / 264 / 520
    end exactly at, inside the second and inside the third 4-column chunk of a lane; 1 .. 9 rows
    leave waves of the block idle, 129 and 136 rows are 17 blocks; 4088 / 4096 / 4099 rows are
    511 blocks, the 512-block cap with two rows per wave, and a third pass for three waves (the
    prefetch guard row + stride < rows).  The CPU baseline (rowwise_ref.ln_bwd_baseline, fp32
    torch) is 4.76 units, so the slack is 19 fp32 roundings: 2**-20 of the terms, nothing unless
    they cancel.
    Measured on the MI355X: no element of any shape or route uses more than 0.500 of its bound
    (correctly rounded but for near-ties).  In ulps of the reference the worst is 46.5 (136 x
    520), at an element that cancels to almost nothing, where the slack term is the bound."""
    x, w, b, dy, prev = R.ln_inputs(rows, C)
    e, u = _ln_bwd_dx_routes(cuda, x, w, b, dy, prev, f"layernorm_bwd {rows}x{C}")
    base = R.ln_bwd_baseline()["cases"][f"{rows}x{C}"]["dx"]
    _record(f"layernorm_bwd_dx:{rows}x{C}", dict(worst_ulp=e, bound_used=u, cpu_baseline_units=base,
                                                 slack_units=R.ln_bwd_slack()["dx"]))


def _pair(dw, db, cuda):
    """[pad | dw | db | pad] in one sentinel-filled device buffer; a tensor goes in as it is,
    None leaves sentinels where it would stand -> (dw view or None, db view or None, buffer)."""
    C = (dw if dw is not None else db).numel()
    buf = torch.full((2 * C + 16,), SENT, dtype=BF)
    if dw is not None:
        buf[8:8 + C] = dw
    if db is not None:
        buf[8 + C:8 + 2 * C] = db
    buf = buf.to(cuda)
    return (buf[8:8 + C] if dw is not None else None,
            buf[8 + C:8 + 2 * C] if db is not None else None, buf)


def _pair_untouched(buf, C, dw, db):
    ok = bool(torch.all(buf[:8] == SENT)) and bool(torch.all(buf[8 + 2 * C:] == SENT))
    if dw is None:
        ok = ok and bool(torch.all(buf[8:8 + C] == SENT))
    if db is None:
        ok = ok and bool(torch.all(buf[8 + C:8 + 2 * C] == SENT))
    return ok


def _ln_bwd_wb_variants(cuda, x, w, b, dy, name, db_prev=None):
    """dw / db stored, accumulated, and each alone -> (dict(worst_ulp, bound_used) per
    quantity, the stored and the accumulated db on the CPU)."""
    K_ = _k()
    rows, C = x.shape
    S = R.ln_bwd_slack()
    xd, wd_, mean, rstd = _ln_stats(cuda, x, w, b)
    dyd = dy.to(cuda)
    dwp, dbp = R.ln_wb_prev(C)
    if db_prev is not None:
        dbp = db_prev
    ref = R.ln_bwd_wb_ref64(dy, x, mean.cpu(), rstd.cpu())
    refp = R.ln_bwd_wb_ref64(dy, x, mean.cpu(), rstd.cpu(), dwp, dbp)
    nan = torch.full((C,), float("nan"), dtype=BF)
    worst, used = dict(dw=0.0, db=0.0), dict(dw=0.0, db=0.0)

    def check(got, r, k, what):
        e = assert_bf16_close(got.cpu(), r[k], scale=r["scale_" + k], slack=S[k],
                              name=f"{name} {k} {what}")
        worst[k] = max(worst[k], e)
        used[k] = max(used[k], _bound_used(got.cpu(), r[k], r["scale_" + k], S[k]))

    dwd, dw_ok = _arena(nan, cuda)
    dbd, db_ok = _arena(nan, cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dw=dwd, db=dbd)
    assert dw_ok() and db_ok(), name + ": a store outside dw / db"
    check(dwd, ref, "dw", "store"), check(dbd, ref, "db", "store")
    dwa, dwa_ok = _arena(dwp, cuda)
    dba, dba_ok = _arena(dbp, cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dw=dwa, db=dba, accumulate_wb=True)
    assert dwa_ok() and dba_ok(), name + ": a store outside dw / db"
    check(dwa, refp, "dw", "+="), check(dba, refp, "db", "+=")
    for k in ("dw", "db"):
        vw, vb, buf = _pair(nan if k == "dw" else None, nan if k == "db" else None, cuda)
        K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dw=vw, db=vb)
        assert _pair_untouched(buf, C, vw, vb), f"{name}: {k} alone wrote outside {k}"
        one, both = (vw, dwd) if k == "dw" else (vb, dbd)
        check(one, ref, k, "alone")
        assert torch.equal(_bits(one), _bits(both)), f"{name}: {k} alone differs"
    return dict(worst_ulp=worst, bound_used=used), dbd.cpu(), dba.cpu()


@pytest.mark.parametrize("rows,C", R.LN_BWD_SHAPES)
def test_layernorm_bwd_dw_db_per_column(cuda, rows, C):
    """Every column of dw = sum_r dy * xh and db = sum_r dy within one bf16 ulp + 4 x max(CPU
    baseline, 1) fp32 roundings of sum_r |dy * xh| resp. sum_r |dy| (+ |prev|) of the float64
    sums (the global max-norm of test_gpu_kernels.py accepts a dw that lost one of 4099 rows:
    tests/test_helpers_cpu.py): stored into NaN-filled outputs between sentinels, accumulated
    over random bf16 values (one rounding of sum + prev), and dw alone / db alone with
    sentinels where the other would stand.  Shapes as test_layernorm_bwd_dx_every_route: 16,
    17, 511 and 512 blocks walk the finalize's 16 partial groups (k = g + 16 j) and its cap.
    CPU baseline (row-by-row fp32 sums): dw 3.48, db 0.77 units.
    Measured on the MI355X: dw at most 0.79 ulp (8 x 1024), db 0.50 ulp (exact ties of a few
    rows); no column of any shape or variant uses more than 0.500 of its bound."""
    x, w, b, dy, _ = R.ln_inputs(rows, C)
    rec, _, _ = _ln_bwd_wb_variants(cuda, x, w, b, dy, f"layernorm_bwd {rows}x{C}")
    base = R.ln_bwd_baseline()["cases"][f"{rows}x{C}"]
    _record(f"layernorm_bwd_wb:{rows}x{C}",
            dict(**rec, cpu_baseline_units=dict(dw=base["dw"], db=base["db"]),
                 slack_units={k: R.ln_bwd_slack()[k] for k in ("dw", "db")}))


@pytest.mark.parametrize("rows,C", R.LN_COUNT_SHAPES)
def test_layernorm_bwd_counts_every_row_once(cuda, rows, C):
    """dy[r, c] = 1 where c == r % C: db[c] is the number of rows congruent to c (+ a small
    integer previous value), below 256 and so exact in fp32 and bf16.  db bit for bit, stored
    and accumulated: a dropped, doubled or misattributed row changes a count by one and no
    tolerance is there to absorb it.  dx and dw of the same inputs go through the per-element
    checks above.  4099 rows: the 512-block cap and the third pass; 137 x 264: 18 blocks (the
    finalize's second trip over its groups) and a width that ends inside a lane's second chunk.
    Measured on the MI355X: db exact at all three shapes; dx and dw at most 0.500 of their bound."""
    x, w, b, dy, prev, db_prev, counts = R.ln_count_inputs(rows, C)
    name = f"layernorm_bwd count {rows}x{C}"
    rec, db, dba = _ln_bwd_wb_variants(cuda, x, w, b, dy, name, db_prev=db_prev)
    assert torch.equal(_bits(db), _bits(counts.to(BF))), name + ": db is not the row count"
    assert torch.equal(_bits(dba), _bits((counts + db_prev.float()).to(BF))), name + ": db +="
    e, u = _ln_bwd_dx_routes(cuda, x, w, b, dy, prev, name)
    base = R.ln_bwd_baseline()["cases"][f"count:{rows}x{C}"]
    _record(f"layernorm_bwd_count:{rows}x{C}",
            dict(worst_ulp=dict(dx=e, **rec["worst_ulp"]),
                 bound_used=dict(dx=u, **rec["bound_used"]), cpu_baseline_units=base))


_FIN_POOLS = {}


def _fin_pool(cuda, C):
    if C not in _FIN_POOLS:
        _FIN_POOLS.clear()  # one width on the device at a time
        _FIN_POOLS[C] = R.ln_fin_pool(C).to(cuda)
    return _FIN_POOLS[C]


@pytest.mark.parametrize("count", R.LN_FIN_COUNTS)
@pytest.mark.parametrize("nblk", R.LN_FIN_NBLK)
@pytest.mark.parametrize("C", R.LN_FIN_WIDTHS)
def test_layernorm_finalize_synthetic_partials(cuda, C, nblk, count):
    """gvl_layernorm_bwd_finalize_batched on fp32 [nblk, 2C] partials made here (columns scaled
    by 2**(c % 9 - 4), every seventh cancelling): every dw / db column within one bf16 ulp +
    4 x max(baseline, 1) roundings of sum |partial| + |prev| of the float64 column sum, the
    baseline being a running fp32 sum on the CPU of the same item.  nblk 15 / 16 / 17 end a
    trip over the 16 partial groups, 511 / 512 the last one; 0 gives 0 when storing and prev
    when accumulating; C = 72 leaves a 16-column last block.  Items after the first walk the
    nblk list, every fourth has no dw and every fourth no db (their places keep sentinels, as
    does everything around the outputs); the 65th item is the wrapper's second launch.
    Measured on the MI355X: no column uses more than 0.500 of its bound; 632 ulps of the
    reference at one cancelling column (C = 776, 15 blocks), where the slack term is the bound."""
    K_ = _k()
    pool, pd = R.ln_fin_pool(C), _fin_pool(cuda, C)
    items = R.ln_fin_items(nblk, C, count)
    worst, used, wbase = 0.0, 0.0, 0.0
    for acc in (False, True):
        out = torch.full((count, 2, C + 16), SENT, dtype=BF)
        for i, (s, n, hw, hb, pw, pb) in enumerate(items):
            if hw:
                out[i, 0, 8:8 + C] = pw if acc else float("nan")
            if hb:
                out[i, 1, 8:8 + C] = pb if acc else float("nan")
        od = out.to(cuda)
        # (an empty view has no data pointer: nblk = 0 still gets a real workspace)
        K_.layernorm_finalize_batched(
            [(pd[s:s + max(n, 1)], n, od[i, 0, 8:8 + C] if hw else None,
              od[i, 1, 8:8 + C] if hb else None) for i, (s, n, hw, hb, _, _) in enumerate(items)],
            C, accumulate=acc)
        got = od.cpu()
        assert torch.all(got[:, :, :8] == SENT) and torch.all(got[:, :, 8 + C:] == SENT)
        for i, (s, n, hw, hb, pw, pb) in enumerate(items):
            ref, E, base = R.ln_fin_ref(pool[s:s + n], torch.cat([pw, pb]) if acc else None)
            slack = 4 * max(base, 1.0)
            wbase = max(wbase, base)
            for k, has, p in ((0, hw, pw), (1, hb, pb)):
                o, rk, Ek = got[i, k, 8:8 + C], ref[k * C:(k + 1) * C], E[k * C:(k + 1) * C]
                if not has:
                    assert torch.all(o == SENT), f"item {i}: a null output was written"
                    continue
                e = assert_bf16_close(o, rk, scale=Ek, slack=slack,
                                      name=f"finalize C={C} item {i} nblk={n} "
                                           f"{'db' if k else 'dw'} acc={acc}")
                worst = max(worst, e)
                used = max(used, _bound_used(o, rk, Ek, slack))
                if n == 0:
                    assert torch.equal(_bits(o), _bits(p if acc else torch.zeros(C, dtype=BF)))
    _record(f"layernorm_finalize:C{C}:nblk{nblk}:count{count}",
            dict(worst_ulp=worst, bound_used=used, cpu_baseline_units=wbase))


def test_layernorm_deferred_finalize_matches_in_place_at_the_cap(cuda):
    """4099 x 128, 512 blocks: the partials left in the workspace and reduced by the batched
    finalize give the bits of the in-place finalize (they share ln_fin_block), and dx does not
    depend on the route."""
    K_ = _k()
    rows, C = 4099, 128
    x, w, b, dy, _ = R.ln_inputs(rows, C)
    xd, wd_, mean, rstd = _ln_stats(cuda, x, w, b)
    dyd = dy.to(cuda)
    dwp, dbp = R.ln_wb_prev(C)
    dx1, (ws, nblk) = K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, defer_wb=True)
    assert nblk == 512
    dwb, dbb = dwp.to(cuda), dbp.to(cuda)
    K_.layernorm_finalize_batched([(ws, nblk, dwb, dbb)], C, accumulate=True)
    dwr, dbr = dwp.to(cuda), dbp.to(cuda)
    dx2 = K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dw=dwr, db=dbr, accumulate_wb=True)
    assert torch.equal(_bits(dwb), _bits(dwr)) and torch.equal(_bits(dbb), _bits(dbr))
    assert torch.equal(_bits(dx1), _bits(dx2))


# ---------------------------------------------------------------------- cross entropy
CE_ROWS = 6


def _ce_logits(V, seed):
    """Six rows: random, +-80, -inf outside the target, all equal, random (ignored target),
    random (masked in the second call)."""
    gen = torch.Generator().manual_seed(3000 + seed)
    lg = torch.randn(CE_ROWS, V, generator=gen) * 3
    tg = torch.randint(0, V, (CE_ROWS,), generator=gen)
    lg[1] = torch.where(torch.rand(V, generator=gen) > 0.5, 80.0, -80.0)
    lg[1, 0], tg[1] = 80.0, 0
    lg[2, torch.rand(V, generator=gen) > 0.5] = float("-inf")
    lg[2, tg[2]] = 1.25
    lg[3] = 1.5
    tg[4] = -100
    return lg.to(BF), tg


@pytest.mark.parametrize("V,ld", [(8, 8), (4104, 4104), (50257, 50264), (50257, 50304),
                                  (65529, 65536), (65536, 65536)])
def test_cross_entropy_per_element(cuda, V, ld):
    """Loss (1e-5, the existing bar) and every dlogits element (one bf16 ulp of softmax - onehot
    in float64; fp32 rounded to bf16 stays within 0.5 ulp at these V) at one chunk per row, past
    4096 columns (the second trip of the register row buffer), the default vocabulary (V % 8 != 0:
    the masked tail chunk, `vocab=`) in buffers padded to 8 and to 64, and the largest supported
    row.  The logits' padding columns hold NaN / 3e38; the gradient's padding columns up to the
    next multiple of 8 must be exactly 0 and the rest of the ld-wide buffer keep its sentinel.
    Rows: random, +-80, -inf outside the target, all equal, an ignored target (zero row); a
    second call masks the last row out."""
    K_ = _k()
    lg, tg = _ce_logits(V, V + ld)
    vpad = (V + 7) // 8 * 8
    buf = torch.empty(CE_ROWS, ld, dtype=BF)
    buf[0::2] = float("nan")
    buf[1::2] = 3e38
    buf[:, :V] = lg
    lgd, tgd = buf.to(cuda), tg.to(cuda)
    loss, want = R.ce_ref64(lg, tg)
    for mask in (None, torch.tensor([1, 1, 1, 1, 1, 0], dtype=torch.bool)):
        if mask is not None:
            loss, want = R.ce_ref64(lg, tg, mask)
        valid = (tg != -100) if mask is None else ((tg != -100) & mask)
        dl = torch.full((CE_ROWS, ld), SENT, dtype=BF, device=cuda)
        out, got = K_.cross_entropy(lgd, tgd, vocab=V, dlogits=dl,
                                    mask=None if mask is None else mask.to(cuda))
        assert got is dl
        ref_loss = loss[valid.numpy()].mean()
        assert abs(float(out[0]) - ref_loss) / ref_loss < 1e-5
        assert abs(float(out[1]) - 1.0 / int(valid.sum())) < 1e-7
        dlc = dl.cpu()
        assert_bf16_close(dlc[:, :V], want, name=f"dlogits V={V} ld={ld}")
        assert torch.all(dlc[:, V:vpad] == 0) and not torch.any(_bits(dlc[:, V:vpad]) != 0)
        assert torch.all(dlc[:, vpad:] == SENT)
        assert not torch.any(_bits(dlc[~valid, :vpad]) != 0)


def test_cross_entropy_zeroes_padding_it_allocates(cuda):
    """kernels.cross_entropy returns a dlogits as wide as the logits; the kernel writes only
    ceil(vocab / 8) * 8 columns of it, so with logits padded further (never in the product:
    pad_vocab pads to 8) the wrapper zeroes the rest: all of it can feed the backward GEMM."""
    K_ = _k()
    V, Vp = 50257, 50304
    lg, tg = _ce_logits(V, 1)
    buf = torch.zeros(CE_ROWS, Vp, dtype=BF)
    buf[:, :V] = lg
    junk = torch.full((CE_ROWS, Vp), SENT, dtype=BF, device=cuda)  # what torch.empty may hand back
    del junk
    out, dl = K_.cross_entropy(buf.to(cuda), tg.to(cuda), vocab=V)
    assert tuple(dl.shape) == (CE_ROWS, Vp)
    _, want = R.ce_ref64(lg, tg)
    assert_bf16_close(dl[:, :V].cpu(), want)
    assert not torch.any(_bits(dl[:, V:]) != 0)


def test_cross_entropy_row_mapping_gradients(cuda):
    """The caption layout (loss rows are logits[:, M:M+T] of a [B, S, V] tensor) at V = 50304:
    the gradient rows, not only the loss, come from the mapped rows."""
    K_ = _k()
    B, S, M, T, V = 2, 5, 2, 3, 50304
    gen = torch.Generator().manual_seed(11)
    lg = (torch.randn(B, S, V, generator=gen) * 3).to(BF)
    tg = torch.randint(0, 50257, (B, T), generator=gen)
    tg[1, 1] = -100
    out, dl = K_.cross_entropy(lg.view(B * S, V).to(cuda), tg.to(cuda), rows_per_group=T,
                               group_stride=S, row_offset=M)
    loss, want = R.ce_ref64(lg[:, M:M + T].reshape(B * T, V), tg.reshape(-1))
    ref = loss[(tg.reshape(-1) != -100).numpy()].mean()
    assert abs(float(out[0]) - ref) / ref < 1e-5
    assert tuple(dl.shape) == (B * T, V)
    assert_bf16_close(dl.cpu(), want, name="row-mapped dlogits")


def test_cross_entropy_finalize_cases(cuda):
    """An out-of-range target poisons the loss (NaN) and leaves a zero gradient row; all rows
    ignored give NaN as torch does; mask_mode with an all-zero mask gives 0 with out[1] = 1."""
    K_ = _k()
    V = 520
    gen = torch.Generator().manual_seed(12)
    lg = (torch.randn(4, V, generator=gen) * 3).to(BF)
    lgd = lg.to(cuda)
    tg = torch.tensor([3, V, 17, -5])
    dl = torch.full((4, V), SENT, dtype=BF, device=cuda)
    out, _ = K_.cross_entropy(lgd, tg.to(cuda), dlogits=dl)
    assert math.isnan(float(out[0]))
    _, want = R.ce_ref64(lg[[0, 2]], tg[[0, 2]])
    assert_bf16_close(dl[[0, 2]].cpu(), want)
    assert not torch.any(_bits(dl[[1, 3]]) != 0)
    out, dl = K_.cross_entropy(lgd, torch.full((4,), -100).to(cuda))
    assert math.isnan(float(out[0]))
    assert not torch.any(_bits(dl) != 0)
    out, dl = K_.cross_entropy(lgd, torch.tensor([3, 5, 17, 9]).to(cuda),
                               mask=torch.zeros(4, dtype=torch.bool, device=cuda), mask_mode=True)
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0
    assert not torch.any(_bits(dl) != 0)


# -------------------------------------------------------------------------- row movers
@pytest.mark.parametrize("cols", [8, 512, 520, 1024])
@pytest.mark.parametrize("G,T,src_rows,src_off,dst_rows,dst_off", [
    (1, 1, 1, 0, 1, 0),    # one row: a quarter of a block
    (2, 2, 2, 0, 2, 0),    # four rows: one full block
    (1, 5, 6, 1, 8, 3),    # five rows (zero_rest: eight) over two blocks, offsets on both sides
    (3, 2, 0, 0, 5, 3),    # src_rows = 0: the same T rows broadcast to every group
    (2, 0, 3, 0, 3, 0),    # T = 0: nothing copied
])
@pytest.mark.parametrize("zero_rest", [False, True])
def test_copy_rows_exact(cuda, cols, G, T, src_rows, src_off, dst_rows, dst_off, zero_rest):
    """gvl_copy_rows bit for bit against a host loop, between strided views inside
    sentinel-filled buffers: 8 columns (one lane), 512 (one trip of the column loop), 520 and
    1024 (a second trip), with and without zeroing the other rows of each group."""
    K_ = _k()
    gen = torch.Generator().manual_seed(cols + G + T)
    n_src = max((G - 1) * src_rows + src_off + T, 1)
    sbuf = torch.randn(n_src, cols + 8, generator=gen).to(BF)
    dbuf = torch.full((G * dst_rows + 2, cols + 16), SENT, dtype=BF)
    want = dbuf.clone()
    for g in range(G):
        for r in range(dst_rows):
            t = r - dst_off
            if 0 <= t < T:
                want[1 + g * dst_rows + r, 8:8 + cols] = sbuf[g * src_rows + src_off + t, 8:]
            elif zero_rest:
                want[1 + g * dst_rows + r, 8:8 + cols] = 0
    sd, dd = sbuf.to(cuda), dbuf.to(cuda)
    K_.copy_rows(sd[:, 8:], dd[1:-1, 8:8 + cols], T, G, src_rows, src_off, dst_rows, dst_off,
                 zero_rest=zero_rest)
    assert torch.equal(_bits(dd), _bits(want))


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 3])
@pytest.mark.parametrize("acc", [False, True])
def test_f32_to_bf16_exact(cuda, n, acc):
    """Round-to-nearest-even of x (+ the bf16 value already there), bit for bit, up to more
    elements than one trip of the 4096-block grid covers; nothing past n is written."""
    K_ = _k()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    x[0] = 1.00390625  # a tie: rounds to even (1.0)
    o0 = torch.randn(n + 8, generator=gen).to(BF)
    o0[n:] = SENT
    od = o0.to(cuda)
    K_.f32_to_bf16(x.to(cuda), od[:n], accumulate=acc)
    want = o0.clone()
    want[:n] = ((x + o0[:n].float()) if acc else x).to(BF)
    assert torch.equal(_bits(od), _bits(want))


@pytest.mark.parametrize("C", [8, 520, 768, 1024])
def test_embedding_fwd_exact(cuda, C):
    """wte[id] + wpe[t] added in fp32 and rounded once, bit for bit, at widths that need the
    second trip of the 512-column loop (every model width does); an id outside [0, V) embeds
    as row 0; five rows straddle the four-rows-per-block grid; the rows in front of the
    offset keep their contents."""
    K_ = _k()
    V, T, M = 11, 5, 2
    gen = torch.Generator().manual_seed(C)
    wte = torch.randn(V, C, generator=gen).to(BF)
    wpe = torch.randn(T + 2, C, generator=gen).to(BF)
    idx = torch.tensor([[4, V + 3, 0, -1, 10]])
    out = torch.full((1, M + T, C), SENT, dtype=BF, device=cuda)
    K_.embedding_fwd(idx.to(cuda), wte.to(cuda), wpe.to(cuda), out, T, M + T, M)
    ids = torch.where((idx >= 0) & (idx < V), idx, torch.zeros_like(idx))
    want = (wte.float()[ids[0]] + wpe.float()[:T]).to(BF)
    assert torch.equal(_bits(out[0, M:]), _bits(want))
    assert torch.all(out[0, :M] == SENT)


@pytest.mark.parametrize("D", [8, 768, 1024])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_l2_normalize_rows(cuda, D, dtype):
    """F.normalize(x, dim=-1, eps=1e-12) against float64: bf16 rows to one bf16 ulp, fp32 rows
    within 12 fp32 roundings of |ref| (the sum of squares: a product, three adds per thread and
    an 8-level tree, halved by the square root: 6.5; then sqrtf, the reciprocal and the product,
    allowed 2 + 2 + 1); a zero row gives zeros (no NaN); a row of norm 1e-20 (fp32) is divided
    by eps, as torch does."""
    K_ = _k()
    gen = torch.Generator().manual_seed(D)
    x = torch.randn(5, D, generator=gen) * torch.tensor([1.0, 1e-3, 300.0, 0.0, 1.0])[:, None]
    x[3] = 0.0  # (+0: the product above leaves -0 too)
    if dtype == F32:
        x[4] = x[4] / x[4].norm() * 1e-20
    x = x.to(dtype)
    got = K_.l2_normalize_rows(x.to(cuda)).cpu()
    x64 = f64(x)
    want = x64 / np.maximum(np.sqrt((x64 * x64).sum(axis=1, keepdims=True)), 1e-12)
    assert not torch.any(_bits(got[3]) != 0)
    if dtype == BF:
        assert_bf16_close(got, want, name=f"l2_normalize bf16 D={D}")
    else:
        assert_f32_close(got, want, np.abs(want), 12, name=f"l2_normalize fp32 D={D}")
        assert abs(float(got[4].double().norm()) - 1e-8) < 1e-13
