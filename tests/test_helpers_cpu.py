"""The per-element closeness helpers are not vacuous: each accepts an fp32 torch evaluation of
the operation (rounded to bf16 where the kernel's output is bf16) and rejects every doctored
output a max-norm comparison lets through.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from tests import rowwise_ref as R
from tests.helpers import (assert_bf16_close, assert_f32_close, f64, rel_err, rel_err_rows,
                           ulp_bf16)

BF = torch.bfloat16


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


def test_ulp_bf16():
    x = np.array([1.0, 1.99, 2.0, -3.5, 0.02, 0.0, 1e-45])
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -13, 2.0 ** -133, 2.0 ** -133]
    assert np.array_equal(ulp_bf16(x), np.array(want))
    # the spacing of bf16 itself
    t = torch.tensor([1.0, 0.02, 3.5]).to(BF)
    nxt = (t.view(torch.int16) + 1).view(BF)
    assert np.array_equal(f64(nxt) - f64(t), ulp_bf16(f64(t)))


def test_close_helpers_edges():
    ref = np.array([1.0, -2.0, 0.0])
    assert_bf16_close(ref + np.array([2.0 ** -7, 2.0 ** -6, 0.0]), ref)  # exactly one ulp
    _rejects(assert_bf16_close, ref + np.array([0.0, 1.01 * 2.0 ** -6, 0.0]), ref)
    _rejects(assert_bf16_close, np.array([1.0, -2.0, np.nan]), ref)
    _rejects(assert_bf16_close, np.array([1.0, -2.0, 1e-30]), ref)
    assert_bf16_close(np.array([np.inf, np.nan]), np.array([np.inf, np.nan]))
    _rejects(assert_bf16_close, np.array([1e38, 0.0]), np.array([np.inf, 0.0]))
    with pytest.raises(AssertionError, match=r"worst at \(1,\): got -2.5 want -2.0"):
        assert_bf16_close(np.array([1.0, -2.5, 0.0]), ref, name="x")
    s = np.array([1.0, 4.0, 0.0])
    assert assert_f32_close(ref + np.array([2.0 ** -24, 0.0, 0.0]), ref, s, 1) == 1.0
    _rejects(assert_f32_close, ref + np.array([0.0, 2.0 ** -21, 0.0]), ref, s, 1.5)
    _rejects(assert_f32_close, ref + np.array([0.0, 0.0, 1e-40]), ref, s, 100)  # scale 0: exact
    a = np.array([[1.0, 2.0], [1e-3, 2e-3]])
    assert rel_err_rows(a, a) == 0.0
    assert rel_err_rows(a * np.array([[1.0], [1.5]]), a) == pytest.approx(0.5)


# ------------------------------------------------------------------------------ AdamW
def _adam_case(step, master):
    n = R.ADAM_BIG
    p, g, m, v = R.adam_inputs(n)
    if not master:
        p, m, v = p.to(BF), m.to(BF), v.to(BF)
    return n, p, R.adam_scaled_grad(g), m, v


@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_adamw_bf16_rejects_noop_and_wrong_bias_correction(step):
    n, p, gs, m, v = _adam_case(step, master=False)
    base = R.adam_baseline()
    ref = R.adamw_ref64(p, gs, m, v, n, step)
    for dev in (False, True):
        good = R.adamw_f32(p, gs, m, v, n, step, dev=dev)
        for k in "pmv":
            assert_bf16_close(good[k].to(BF), ref[k], scale=ref["scale_" + k], slack=4 * base[k],
                              name=k)
    # the kernel did nothing
    for k, t in (("p", p), ("m", m), ("v", v)):
        _rejects(assert_bf16_close, t, ref[k], scale=ref["scale_" + k], slack=4 * base[k])
    if step == 7:  # the bias correction of step 1 at step 7
        bad = R.adamw_ref64(p, gs, m, v, n, step, bias_step=1)
        _rejects(assert_bf16_close, torch.from_numpy(bad["p"]).to(BF), ref["p"],
                 scale=ref["scale_p"], slack=4 * base["p"])


def test_adamw_reference_moves_its_inputs():
    """The condition the GPU test asserts too: on these inputs the reference moves at least
    95 % of p (step 1), m and v by a bf16 ulp or more, so a no-op cannot pass."""
    for step in R.ADAM_STEPS:
        n, p, gs, m, v = _adam_case(step, master=False)
        ref = R.adamw_ref64(p, gs, m, v, n, step)
        assert R.moved_fraction(p, ref["p"]) >= (0.95 if step == 1 else 0.90)
        assert R.moved_fraction(m, ref["m"]) >= 0.95
        assert R.moved_fraction(v, ref["v"]) >= 0.95


def test_adamw_master_rejects_decay_past_the_boundary():
    """Decay applied to all n elements where n_decay = n - 3: lr * wd = 1e-4 relative, far
    below half a bf16 ulp (2**-9), so only the fp32 master weights can show it."""
    n, p, gs, m, v = _adam_case(7, master=True)
    base = R.adam_baseline()
    ref = R.adamw_ref64(p, gs, m, v, n - 3, 7)
    good = R.adamw_f32(p, gs, m, v, n - 3, 7, dev=True)
    bad = R.adamw_f32(p, gs, m, v, n, 7, dev=True)
    for k in "pmv":
        assert_f32_close(good[k], ref[k], ref["scale_" + k], 4 * base[k], name=k)
    with pytest.raises(AssertionError, match=rf"worst at \(({n - 3}|{n - 2}|{n - 1}),\)"):
        assert_f32_close(bad["p"], ref["p"], ref["scale_p"], 4 * base["p"])
    assert rel_err(f64(bad["p"]), ref["p"]) < 1e-4  # invisible to the max-norm figure


# ---------------------------------------------------------------------- cross entropy
def test_cross_entropy_dlogits_rejects_doctored():
    rows, V, vpad = 6, 4101, 4104
    gen = torch.Generator().manual_seed(3)
    lg = (torch.randn(rows, V, generator=gen) * 3).to(BF)
    tg = torch.randint(0, V, (rows,), generator=gen)
    _, ref = R.ce_ref64(lg, tg)
    ref = np.pad(ref, ((0, 0), (0, vpad - V)))
    pad = lambda t: torch.nn.functional.pad(t, (0, vpad - V))
    good = pad(R.ce_f32(lg, tg))
    assert assert_bf16_close(good, ref) <= 0.5 + 1e-3  # correctly rounded but for fp32 near-ties
    bad = good.clone()
    bad[2, 2048:2056] = 0  # one 8-column chunk of probabilities dropped
    _rejects(assert_bf16_close, bad, ref)
    assert rel_err(f64(bad), ref) < 8e-3  # the existing bar passes it
    p = torch.softmax(lg.float(), -1) * 1.01  # every probability 1 % high
    p[torch.arange(rows), tg] -= 1.0
    _rejects(assert_bf16_close, pad(p.to(BF)), ref)
    assert rel_err(f64(pad(p.to(BF))), ref) < 8e-3
    bad = good.clone()
    bad[4, V + 1] = 1e-30  # a padding column that is not exactly zero
    _rejects(assert_bf16_close, bad, ref)


# -------------------------------------------------------------------------- LayerNorm
def test_layernorm_rejects_lost_row_and_one_pass_variance():
    rows, C = 9, 768
    x, w, b, dy, _ = R.ln_inputs(rows, C)
    base = R.ln_baseline()
    ref = R.ln_ref64(x, w, b)
    mean, rstd = R.ln_f32(x)
    assert_f32_close(mean, ref["mean"], ref["scale_mean"], 4 * base["mean"])
    assert_f32_close(rstd, ref["rstd"], ref["scale_rstd"], 4 * base["rstd"])
    dx = R.ln_bwd_ref64(dy, x, w, mean, rstd)
    xr = x.float().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (C,), w.float(), b.float(), R.LN_EPS).backward(dy.float())
    good = xr.grad.to(BF)
    assert rel_err_rows(good, dx) < 1e-2
    small = int(np.argmin(np.abs(dx).max(axis=1)))  # the row with the smallest gradient
    bad = good.clone()
    bad[small] = 0
    assert rel_err_rows(bad, dx) >= 1.0
    assert rel_err(f64(bad), dx) < 1e-2  # the global max-norm hides it
    # offset rows: the two-pass statistics pass, E[x^2] - mean^2 in fp32 does not
    xs = R.ln_special_rows(C)
    ref = R.ln_ref64(xs, torch.ones(C), torch.zeros(C))
    m2, r2 = R.ln_f32(xs)
    assert_f32_close(m2, ref["mean"], ref["scale_mean"], 4 * base["mean"])
    assert_f32_close(r2, ref["rstd"], ref["scale_rstd"], 4 * base["rstd"])
    _, r1 = R.ln_f32(xs, one_pass=True)
    _rejects(assert_f32_close, r1[1:], ref["rstd"][1:], ref["scale_rstd"][1:], 4 * base["rstd"])


# ----------------------------------------------------------------- LayerNorm backward
def _bf(a):
    return torch.from_numpy(np.asarray(a)).to(BF)


def test_layernorm_bwd_f32_passes_at_every_shape():
    """The condition that keeps the float64 reference inside its own bound on these inputs:
    the kernel's formulas in fp32 torch (rowwise_ref.ln_bwd_f32), rounded to bf16, pass every
    check of tests/test_gpu_rowwise.py at every shape it runs, storing and accumulating."""
    S = R.ln_bwd_slack()
    base = R.ln_bwd_baseline()
    assert set(base["cases"]) >= {f"{r}x{c}" for r, c in R.LN_BWD_SHAPES}
    assert all(4 * max(base[k], 1.0) == S[k] for k in S)
    for key, (x, w, dy, prev) in R.ln_bwd_cases():
        C = x.shape[1]
        mean, rstd = R.ln_f32(x)
        dwp, dbp = R.ln_wb_prev(C)
        f = R.ln_bwd_f32(dy, x, w, mean, rstd)
        fa = R.ln_bwd_f32(dy, x, w, mean, rstd, prev, dwp, dbp)
        dx, sdx = R.ln_bwd_dx_ref64(dy, x, w, mean, rstd)
        dxa, sdxa = R.ln_bwd_dx_ref64(dy, x, w, mean, rstd, prev)
        assert_bf16_close(f["dx"].to(BF), dx, scale=sdx, slack=S["dx"], name=key + " dx")
        assert_bf16_close(fa["dx"].to(BF), dxa, scale=sdxa, slack=S["dx"], name=key + " dx +=")
        r, ra = R.ln_bwd_wb_ref64(dy, x, mean, rstd), R.ln_bwd_wb_ref64(dy, x, mean, rstd, dwp, dbp)
        for k in ("dw", "db"):
            assert_bf16_close(f[k].to(BF), r[k], scale=r["scale_" + k], slack=S[k],
                              name=f"{key} {k}")
            assert_bf16_close(fa[k].to(BF), ra[k], scale=ra["scale_" + k], slack=S[k],
                              name=f"{key} {k} +=")
    for rows, C in R.LN_COUNT_SHAPES:  # the counting inputs: db is exact, in any order
        x, w, _, dy, _, db_prev, counts = R.ln_count_inputs(rows, C)
        f = R.ln_bwd_f32(dy, x, w, *R.ln_f32(x), db_prev=db_prev)
        assert torch.equal(f["db"], counts + db_prev.float())
        assert torch.equal(f["db"].to(BF).float(), f["db"])


def test_layernorm_bwd_rejects_lost_and_doubled_rows():
    """dw / db of 4099 x 8 with the last row left out, or counted twice, rounded to bf16: the
    per-column bound rejects both; the global max-norm of test_gpu_kernels.py accepts the dw
    that lost a row (0.0085 < 1e-2), which is the gap the per-column tests close."""
    rows, C = 4099, 8
    x, w, _, dy, _ = R.ln_inputs(rows, C)
    mean, rstd = R.ln_f32(x)
    S = R.ln_bwd_slack()
    ref = R.ln_bwd_wb_ref64(dy, x, mean, rstd)
    lost = R.ln_bwd_wb_ref64(dy[:-1], x[:-1], mean[:-1], rstd[:-1])
    last = R.ln_bwd_wb_ref64(dy[-1:], x[-1:], mean[-1:], rstd[-1:])
    for k in ("dw", "db"):
        assert_bf16_close(_bf(ref[k]), ref[k], scale=ref["scale_" + k], slack=S[k])
        _rejects(assert_bf16_close, _bf(lost[k]), ref[k], scale=ref["scale_" + k], slack=S[k])
        _rejects(assert_bf16_close, _bf(ref[k] + last[k]), ref[k], scale=ref["scale_" + k],
                 slack=S[k])
    assert rel_err(f64(_bf(lost["dw"])), ref["dw"]) < 1e-2


def test_layernorm_bwd_dx_rejects_missing_mean_and_wrong_rstd():
    """dx without its - mean(g) term, and dx with one row scaled by its neighbour's rstd (rows
    differ by powers of two in scale): both fail the per-element bound at every shape kind."""
    S = R.ln_bwd_slack()
    for rows, C in ((9, 8), (37, 768), (136, 264)):
        x, w, _, dy, _ = R.ln_inputs(rows, C)
        mean, rstd = R.ln_f32(x)
        dx, sdx = R.ln_bwd_dx_ref64(dy, x, w, mean, rstd)
        assert_bf16_close(_bf(dx), dx, scale=sdx, slack=S["dx"])
        g = f64(dy) * f64(w)
        no_mean = dx + f64(rstd)[:, None] * g.mean(axis=1, keepdims=True)
        _rejects(assert_bf16_close, _bf(no_mean), dx, scale=sdx, slack=S["dx"])
        r2 = rstd.clone()
        r2[rows - 1] = rstd[rows - 2]
        wrong = R.ln_bwd_ref64(dy, x, w, mean, r2)
        assert np.array_equal(wrong[:-1], dx[:-1])
        with pytest.raises(AssertionError, match=rf"worst at \({rows - 1}, "):
            assert_bf16_close(_bf(wrong), dx, scale=sdx, slack=S["dx"])


@pytest.mark.parametrize("C", R.LN_FIN_WIDTHS)
def test_layernorm_finalize_check_rejects_ignored_partials(C):
    """A finalize that sums only the first trip over its 16 partial groups (k < 16): equal to
    the reference up to 16 blocks, rejected from 17 on; a running fp32 sum rounded to bf16
    passes at every block count, storing and accumulating."""
    pool = R.ln_fin_pool(C)
    prev = R.ln_fin_items(512, C, 1)[0]
    prev = torch.cat([prev[4], prev[5]])
    for n in R.LN_FIN_NBLK:
        for p in (None, prev):
            ref, E, base = R.ln_fin_ref(pool[:n], p)
            slack = 4 * max(base, 1.0)
            s32 = pool[:n].cumsum(dim=0)[-1] if n else torch.zeros(2 * C)
            s32 = s32 if p is None else s32 + p.float()
            assert_bf16_close(s32.to(BF), ref, scale=E, slack=slack, name=f"C={C} nblk={n}")
            bad = R.ln_fin_ref(pool[:n], p, first=16)[0]
            if n <= 16:
                assert np.array_equal(bad, ref)
            else:
                _rejects(assert_bf16_close, _bf(bad), ref, scale=E, slack=slack)
