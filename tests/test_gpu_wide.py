"""The GPT-2 large / XL widths on the MI355X: the wide row kernels (1024 < cols <= 2048) per
element against the float64 references of tests/rowwise_ref.py with their own CPU baselines
(tests/wide_ref.py), the deterministic embedding backward bit for bit, the GEMM instances the wide
LM shapes reach with their ragged tiles, the three model kinds at 1280 / 20 and 1600 / 25 against
fp32 CPU fixtures, and KV-cached decoding at 1280.  The rules are those of test_gpu_rowwise.py,
test_gpu_kernels.py, test_gpu_gemm.py, test_gpu_models.py and test_gpu_decode.py; the measured
margins go to profiles/wide_margins.json through helpers.margins_out."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import rowwise_ref as R
from tests import wide_ref as WR
from tests.helpers import (F32_UNIT, assert_bf16_close, f64, margins_out,
                           ulp_bf16)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
SENT = 7.0

_MARGINS = {}


def _record(key, rec):
    _MARGINS[key] = rec
    margins_out("wide_margins", _MARGINS)


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
    tol = ulp_bf16(ref64) + slack * F32_UNIT * np.abs(f64(scale))
    return float((np.abs(f64(got) - f64(ref64)) / tol).max()) if np.size(ref64) else 0.0


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------- LayerNorm forward
def _ln_check_fwd(x, w, b, y, mean, rstd, name, base):
    """test_gpu_rowwise's rule (mean / rstd within 4 x the CPU baseline, y to one bf16 ulp + their
    errors and four roundings) on the wide baseline -> (mean, rstd) errors in units."""
    from tests.test_gpu_rowwise import _ln_check_fwd as check
    _, em, er = check(x, w, b, y, mean, rstd, name, base=base)
    return em, er


@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("C", WR.WIDE_WIDTHS)
def test_layernorm_fwd_wide_per_row(cuda, rows, C):
    """gvl_layernorm_fwd_wide through K.layernorm_fwd: rows scaled by 2**-6 .. 2**6, mean and rstd
    against float64 within 4 x the wide CPU baseline (mean 0.88, rstd 2.58 units), y per element
    to one bf16 ulp.  Then x and y as column slices (ld = C + 8) of a NaN-filled and a sentinel-
    filled buffer with stats=False: the same y bit for bit, nothing outside the slice written.
    1536 / 1544 are the last width of the IT = 3 instance and the first of IT = 4; 7, 9 and 37
    rows leave partly filled 4-row blocks.
    Measured on the MI355X (special rows included): mean at most 0.88, rstd 2.52 units, against
    bounds of 3.5 and 10.3."""
    K_ = _k()
    x, w, b, _, _ = R.ln_inputs(rows, C)
    xd, wd_, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    y, mean, rstd = K_.layernorm_fwd(xd, wd_, bd, eps=R.LN_EPS)
    name = f"layernorm wide {rows}x{C}"
    base = WR.wide_ln_baseline()
    em, er = _ln_check_fwd(x, w, b, y, mean, rstd, name, base)
    print(f"{name}: mean {em:.2f} rstd {er:.2f} units; CPU baseline {base}")
    _record(f"layernorm:{rows}x{C}", dict(kernel_units=dict(mean=em, rstd=er),
                                          cpu_baseline_units=base))
    xbuf = torch.full((rows, C + 8), float("nan"), dtype=BF, device=cuda)
    xbuf[:, 8:] = xd
    ybuf = torch.full((rows + 1, C + 8), SENT, dtype=BF, device=cuda)
    _, m2, r2 = K_.layernorm_fwd(xbuf[:, 8:], wd_, bd, eps=R.LN_EPS, out=ybuf[:rows, :C], stats=False)
    assert m2 is None and r2 is None
    assert torch.equal(_bits(ybuf[:rows, :C]), _bits(y))
    assert torch.all(ybuf[:, C:] == SENT) and torch.all(ybuf[rows:] == SENT)


@pytest.mark.parametrize("C", WR.WIDE_WIDTHS)
def test_layernorm_fwd_wide_constant_and_offset_rows(cuda, C):
    """A row of zero variance: rstd = 1 / sqrt(eps) and y = b exactly.  Rows x = +-(256 +
    {0, 2, 4}): the two-pass variance stays within the bound a one-pass form misses."""
    K_ = _k()
    x = R.ln_special_rows(C)
    _, w, b, _, _ = R.ln_inputs(3, C, seed=1)
    y, mean, rstd = K_.layernorm_fwd(x.to(cuda), w.to(cuda), b.to(cuda), eps=R.LN_EPS)
    base = WR.wide_ln_baseline()
    em, er = _ln_check_fwd(x, w, b, y, mean, rstd, f"layernorm wide special rows C={C}", base)
    _record(f"layernorm:special:{C}", dict(kernel_units=dict(mean=em, rstd=er),
                                           cpu_baseline_units=base))
    assert float(mean[0]) == 3.25
    want = 1.0 / math.sqrt(float(np.float32(R.LN_EPS)))
    assert abs(float(rstd[0]) - want) <= 4 * base["rstd"] * 2.0 ** -24 * want
    assert torch.equal(_bits(y[0]), _bits(b))


@pytest.mark.parametrize("rows,C", WR.WIDE_FWD_TALL)
def test_layernorm_fwd_wide_second_persistent_pass(cuda, rows, C):
    """4097 rows: one row more than the 1024 blocks x 4 waves of the persistent forward hold, so
    one wave takes a second row while the others read row 0 and store nothing."""
    K_ = _k()
    x, w, b, _, _ = R.ln_inputs(rows, C)
    y, mean, rstd = K_.layernorm_fwd(x.to(cuda), w.to(cuda), b.to(cuda), eps=R.LN_EPS)
    base = WR.wide_ln_tall_baseline()
    em, er = _ln_check_fwd(x, w, b, y, mean, rstd, f"layernorm wide {rows}x{C}", base)
    _record(f"layernorm:tall:{rows}x{C}", dict(kernel_units=dict(mean=em, rstd=er),
                                               cpu_baseline_units=base))


# --------------------------------------------------------------- LayerNorm backward
def _ln_stats(cuda, x, w, b):
    xd, wd_ = x.to(cuda), w.to(cuda)
    _, mean, rstd = _k().layernorm_fwd(xd, wd_, b.to(cuda), eps=R.LN_EPS)
    return xd, wd_, mean, rstd


def _nan_view(t, cuda, ld, off):
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=cuda)
    buf[:, off:off + t.shape[1]] = t.to(cuda)
    return buf[:, off:off + t.shape[1]]


def _ln_bwd_dx_routes(cuda, x, w, b, dy, prev, name):
    """dx stored, accumulated in place, with a separate residual, and strided -> (worst error in
    bf16 ulps, worst fraction of the bound used).  Each launch runs twice: the same bits."""
    K_ = _k()
    rows, C = x.shape
    slack = WR.wide_bwd_slack()["dx"]
    xd, wd_, mean, rstd = _ln_stats(cuda, x, w, b)
    dyd = dy.to(cuda)
    want, scale = R.ln_bwd_dx_ref64(dy, x, w, mean.cpu(), rstd.cpu())
    wantp, scalep = want + f64(prev), scale + np.abs(f64(prev))
    dx = torch.full((rows, C), float("nan"), dtype=BF, device=cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dx=dx)
    e1 = assert_bf16_close(dx.cpu(), want, scale=scale, slack=slack, name=name + " dx")
    u1 = _bound_used(dx.cpu(), want, scale, slack)
    again = K_.layernorm_bwd(dyd, xd, wd_, mean, rstd)
    assert torch.equal(_bits(again), _bits(dx)), name + ": two calls differ"
    acc = prev.to(cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dx=acc, accumulate_dx=True)
    e2 = assert_bf16_close(acc.cpu(), wantp, scale=scalep, slack=slack, name=name + " dx +=")
    u2 = _bound_used(acc.cpu(), wantp, scalep, slack)
    prev_d = prev.to(cuda)
    dx2 = torch.full((rows, C), float("nan"), dtype=BF, device=cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dx=dx2, residual=prev_d)
    assert torch.equal(_bits(dx2), _bits(acc)), name + ": residual route differs from in place"
    assert torch.equal(_bits(prev_d), _bits(prev)), name + ": the residual was written"
    dbuf = torch.full((rows + 1, C + 32), SENT, dtype=BF, device=cuda)
    K_.layernorm_bwd(_nan_view(dy, cuda, C + 8, 8), _nan_view(x, cuda, C + 16, 16), wd_, mean, rstd,
                     dx=dbuf[:rows, 16:16 + C], residual=_nan_view(prev, cuda, C + 24, 8))
    assert torch.equal(_bits(dbuf[:rows, 16:16 + C]), _bits(dx2)), name + ": strided run differs"
    assert torch.all(dbuf[:, :16] == SENT) and torch.all(dbuf[:, 16 + C:] == SENT)
    assert torch.all(dbuf[rows:] == SENT)
    return max(e1, e2), max(u1, u2)


@pytest.mark.parametrize("rows,C", WR.WIDE_BWD_SHAPES)
def test_layernorm_bwd_wide_dx_every_route(cuda, rows, C):
    """gvl_layernorm_bwd_wide: every element of dx within one bf16 ulp + 4 x max(wide CPU
    baseline, 1) fp32 roundings (baseline 1.97: 7.9 roundings) of the added terms of the float64
    backward from the kernel's own statistics: stored, accumulated in place, with a separate
    residual (the last two bit-identical, the residual's bits kept), then with four different
    leading dimensions inside NaN-filled / sentinel-filled buffers.  Two waves share a row: 1 row
    leaves the block's second pair idle, 3 and 5 give the pairs unequal trip counts behind the
    shared barrier.
    Measured on the MI355X: no element of any shape or route uses more than 0.500 of its bound;
    29.9 ulps of the reference at an element that cancels to almost nothing."""
    x, w, b, dy, prev = R.ln_inputs(rows, C)
    e, u = _ln_bwd_dx_routes(cuda, x, w, b, dy, prev, f"layernorm_bwd wide {rows}x{C}")
    base = WR.wide_bwd_baseline()["cases"][f"{rows}x{C}"]["dx"]
    _record(f"layernorm_bwd_dx:{rows}x{C}", dict(worst_ulp=e, bound_used=u, cpu_baseline_units=base,
                                                 slack_units=WR.wide_bwd_slack()["dx"]))


def _pair(dw, db, cuda):
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
    """dw / db stored, accumulated, and each alone -> (dict(worst_ulp, bound_used) per quantity,
    the stored and the accumulated db on the CPU)."""
    K_ = _k()
    rows, C = x.shape
    S = WR.wide_bwd_slack()
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
    dw2, db2 = torch.empty(C, dtype=BF, device=cuda), torch.empty(C, dtype=BF, device=cuda)
    K_.layernorm_bwd(dyd, xd, wd_, mean, rstd, dw=dw2, db=db2)
    assert torch.equal(_bits(dw2), _bits(dwd)) and torch.equal(_bits(db2), _bits(dbd)), \
        name + ": two calls differ"
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


@pytest.mark.parametrize("rows,C", WR.WIDE_BWD_SHAPES)
def test_layernorm_bwd_wide_dw_db_per_column(cuda, rows, C):
    """Every column of dw = sum_r dy * xh and db = sum_r dy within one bf16 ulp + 4 x max(wide CPU
    baseline, 1) fp32 roundings (dw 4.05: 16.2, db 0.69: 4) of sum_r |dy * xh| resp. sum_r |dy|
    (+ |prev|) of the float64 sums: stored into NaN-filled outputs between sentinels,
    accumulated over random bf16 values, and dw alone / db alone with sentinels where the other
    would stand; the stored pair of a second call bit for bit.
    Measured on the MI355X: at most 1.90 ulp, no column above 0.500 of its bound."""
    x, w, b, dy, _ = R.ln_inputs(rows, C)
    rec, _, _ = _ln_bwd_wb_variants(cuda, x, w, b, dy, f"layernorm_bwd wide {rows}x{C}")
    base = WR.wide_bwd_baseline()["cases"][f"{rows}x{C}"]
    _record(f"layernorm_bwd_wb:{rows}x{C}",
            dict(**rec, cpu_baseline_units=dict(dw=base["dw"], db=base["db"]),
                 slack_units={k: WR.wide_bwd_slack()[k] for k in ("dw", "db")}))


@pytest.mark.parametrize("rows,C", WR.WIDE_COUNT_SHAPES)
def test_layernorm_bwd_wide_counts_every_row_once(cuda, rows, C):
    """dy[r, c] = 1 where c == r % C: db[c] is the number of rows congruent to c (+ a small
    integer previous value), exact in fp32 and bf16.  db bit for bit, stored and accumulated: a
    dropped, doubled or misattributed row changes a count by one.  dx and dw of the same inputs go
    through the per-element checks.  4099 x 1032: the 512-block cap and a fifth pass for three
    rows; 137 x 2040: 18 blocks and a width that ends inside the last chunk."""
    x, w, b, dy, prev, db_prev, counts = R.ln_count_inputs(rows, C)
    name = f"layernorm_bwd wide count {rows}x{C}"
    rec, db, dba = _ln_bwd_wb_variants(cuda, x, w, b, dy, name, db_prev=db_prev)
    assert torch.equal(_bits(db), _bits(counts.to(BF))), name + ": db is not the row count"
    assert torch.equal(_bits(dba), _bits((counts + db_prev.float()).to(BF))), name + ": db +="
    e, u = _ln_bwd_dx_routes(cuda, x, w, b, dy, prev, name)
    _record(f"layernorm_bwd_count:{rows}x{C}",
            dict(worst_ulp=dict(dx=e, **rec["worst_ulp"]), bound_used=dict(dx=u, **rec["bound_used"])))


def test_layernorm_wide_deferred_finalize_matches_in_place_at_the_cap(cuda):
    """4099 x 1032, 512 blocks: the partials left in the workspace and reduced by
    gvl_layernorm_bwd_finalize_batched_wide give the bits of the in-place finalize (they share
    ln_fin_block), and dx does not depend on the route."""
    K_ = _k()
    rows, C = 4099, 1032
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


_FIN_POOLS = {}


def _fin_pool(cuda, C):
    if C not in _FIN_POOLS:
        _FIN_POOLS.clear()  # one width on the device at a time
        _FIN_POOLS[C] = R.ln_fin_pool(C).to(cuda)
    return _FIN_POOLS[C]


@pytest.mark.parametrize("count", WR.WIDE_FIN_COUNTS)
@pytest.mark.parametrize("nblk", WR.WIDE_FIN_NBLK)
@pytest.mark.parametrize("C", WR.WIDE_FIN_WIDTHS)
def test_layernorm_finalize_wide_synthetic_partials(cuda, C, nblk, count):
    """gvl_layernorm_bwd_finalize_batched_wide on fp32 [nblk, 2C] partials made here, by
    test_layernorm_finalize_synthetic_partials' rule: every dw / db column within one bf16 ulp +
    4 x max(baseline, 1) roundings of sum |partial| + |prev| of the float64 column sum, the
    baseline being a running fp32 sum on the CPU of the same item; null outputs and everything
    around the outputs keep their sentinels; the 65th item is the wrapper's second launch."""
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
                                      name=f"finalize wide C={C} item {i} nblk={n} "
                                           f"{'db' if k else 'dw'} acc={acc}")
                worst = max(worst, e)
                used = max(used, _bound_used(o, rk, Ek, slack))
                if n == 0:
                    assert torch.equal(_bits(o), _bits(p if acc else torch.zeros(C, dtype=BF)))
    _record(f"layernorm_finalize:C{C}:nblk{nblk}:count{count}",
            dict(worst_ulp=worst, bound_used=used, cpu_baseline_units=wbase))


# ------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("C", WR.WIDE_EMB_WIDTHS)
def test_embedding_fwd_wide_exact(cuda, C):
    """test_embedding_fwd_exact at the wide widths: wte[id] + wpe[t] rounded once, bit for bit."""
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


@pytest.mark.parametrize("with_pe", [True, False])
@pytest.mark.parametrize("C", WR.WIDE_EMB_WIDTHS)
def test_embedding_bwd_det_wide_bit_exact(cuda, C, with_pe):
    """gvl_embedding_bwd_det past 1024 columns (two slabs of the row, the second partly filled
    at 1032 / 1280 / 1600), by test_embedding_bwd_det_bit_exact's host emulation: per-id fp32
    sums in token order and one bf16 update per row, bit for bit, with a hot id (every second
    token), ids out of range (skipped), dwpe over 5 sequences (the four-row load group and its
    tail) or null, and nothing written to the rows of untouched ids."""
    K_ = _k()
    V, G, T, M = 37, 5, 13, 3
    gen = torch.Generator().manual_seed(11 + C)
    idx = torch.randint(0, V - 4, (G, T), generator=gen)   # ids V-4 .. V-1 never occur
    idx[:, ::2] = 7
    idx[1, 5] = V + 3
    idx[2, 9] = -1
    dout = torch.randn(G, M + T, C, generator=gen).to(BF)
    w0 = torch.randn(V, C, generator=gen).to(BF)
    p0 = torch.randn(T + 5, C, generator=gen).to(BF)
    gte, gpe = w0.to(cuda), p0.to(cuda)
    K_.embedding_bwd_det(idx.to(cuda), dout.to(cuda), gte, gpe if with_pe else None, T, M + T, M,
                         C, V)
    ids = idx.reshape(-1).numpy()
    rows = dout[:, M:].reshape(-1, C).float().numpy()
    ok = (ids >= 0) & (ids < V)
    acc = np.zeros((V, C), np.float32)
    np.add.at(acc, ids[ok], rows[ok])
    touched = np.unique(ids[ok])
    upd = w0.float().numpy()
    upd[touched] = upd[touched] + acc[touched]
    assert torch.equal(_bits(gte), _bits(torch.from_numpy(upd).to(BF)))
    assert torch.equal(_bits(gte[V - 4:]), _bits(w0[V - 4:]))
    if with_pe:
        ps = np.zeros((T, C), np.float32)
        for g in range(G):
            ps += dout[g, M:].float().numpy()
        wp = p0.float().numpy().copy()
        wp[:T] += ps
        assert torch.equal(_bits(gpe), _bits(torch.from_numpy(wp).to(BF)))
    else:
        assert torch.equal(_bits(gpe), _bits(p0))
    again = w0.to(cuda)
    K_.embedding_bwd_det(idx.to(cuda), dout.to(cuda), again, None, T, M + T, M, C, V)
    assert torch.equal(_bits(again), _bits(gte))


# --------------------------------------------------------------------------- models
WIDE_CFG = {
    "wide1280": dict(block_size=64, vocab_size=512, n_layer=2, n_head=20, n_embd=1280),
    "wide1600": dict(block_size=64, vocab_size=512, n_layer=1, n_head=25, n_embd=1600),
}
ENC = 768  # the vision tokens keep the CLIP width
KINDS = ("gpt", "qformer", "cross")
# tests/test_gpu_models.py's bounds for its tiny fixtures
TINY_BOUNDS = dict(loss=2e-3, logits=3e-2, grads=1.2e-1, params=8e-2, train_losses=3e-3,
                   train_norms=3e-2)
_YARD = {}
_RECIPE = {}


def _bound(tag, kind, what):
    """The larger of the tiny-fixture bound and twice the yardstick: what the reference's own bf16
    path (tools/make_wide_fixtures.py, on the CPU) shows against its fp32 path on these inputs."""
    if not _YARD:
        from tests.conftest import GOLDEN
        with open(os.path.join(GOLDEN, "wide_yardstick.json")) as f:
            _YARD.update(json.load(f))
    return max(TINY_BOUNDS[what], 2.0 * _YARD[f"{tag}:{kind}"][what])


def _build_wide(kind, tag):
    import gvl.caption as cap
    import gvl.cross_att as xa
    import gvl.gpt2 as g2
    cfg = WIDE_CFG[tag]
    if kind == "gpt":
        return g2.GPT(g2.GPTConfig(**cfg))
    if kind == "qformer":
        return cap.QFormerCaption(enc_dim=ENC, lm=cap.GPT_previous(g2.GPTConfig(**cfg)), m_vis_tokens=32)
    return xa.GPT(xa.GPTConfig(**cfg, img_embd=ENC))


def _wide_model(kind, tag, cuda):
    """A fresh model with the recipe weights (made once per kind and config), bf16, eval."""
    from tests.helpers import recipe_params
    m = _build_wide(kind, tag)
    sd = m.state_dict()
    if (kind, tag) not in _RECIPE:
        _RECIPE.clear()  # one set of recipe weights in host memory at a time
        _RECIPE[(kind, tag)] = recipe_params([(k, tuple(v.shape)) for k, v in sd.items()])
    P = _RECIPE[(kind, tag)]
    m.load_state_dict({k: (P[k] if k in P else v) for k, v in sd.items()}, strict=True)
    return m.to(cuda).to(BF).eval()


def _wide_loss(kind, m, fx, cuda):
    from gvl.caption import pool_clip_197_to_33_avg_with_cls as pool
    from oracle import weights as W
    t = lambda k: torch.from_numpy(fx[k]).to(cuda)
    if kind == "gpt":
        return m(t("x"), t("y"))
    shape = tuple(int(s) for s in fx["z_shape"])
    z_raw = torch.from_numpy(W.make_normal_like(int(np.prod(shape)), int(fx["z_seed"]))).view(shape)
    z = pool(z_raw.to(cuda))
    if kind == "qformer":
        return m(z, t("x"), labels=t("labels"))
    return m(t("x"), z=z, targets=t("y"), target_mask=t("mask"))


def _trainable(fx):
    return sorted(k[len("grad:"):-len("#sq")] for k in fx if k.startswith("grad:") and k.endswith("#sq"))


def _summary_err(fx, name, t):
    """helpers.check_summary's two figures as one: the (sampled) max-norm error and half the
    relative error of the sum of squares, both held to rtol there."""
    from tests.helpers import rel_err
    a = t.detach().to(torch.float64).cpu().numpy().reshape(-1)
    e = rel_err(a, fx[name + "#full"]) if name + "#full" in fx else rel_err(a[fx[name + "#idx"]], fx[name + "#val"])
    sq = float(fx[name + "#sq"])
    return max(e, 0.5 * abs((a * a).sum() - sq) / max(sq, 1e-30))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", list(WIDE_CFG))
def test_wide_forward_loss_and_logits(cuda, golden, tag, kind):
    """Loss and logits of the bf16 HIP path at n_embd 1280 / 1600 against the reference's fp32
    CPU path (tests/golden/KIND_wide*.npz), each within the larger of test_gpu_models.py's
    tiny-fixture bound and twice the reference's own bf16-against-fp32 yardstick.
    Measured on the MI355X: loss at most 1.8e-4 (bound 2e-3), logits 9.6e-3 (bound 3e-2); gradients
    at most 2.4e-2 (bound 1.2e-1); after three AdamW steps parameters 5.5e-2 (qformer, bound
    1.26e-1, yardstick 6.3e-2), train losses 1.4e-2 (gpt, bound 2.8e-2, yardstick 1.4e-2), norms
    3.6e-2 (cross at 1600, bound 1.5e-1)."""
    from tests.helpers import rel_err
    fx = golden(f"{kind}_{tag}")
    m = _wide_model(kind, tag, cuda)
    with torch.no_grad():
        logits, loss = _wide_loss(kind, m, fx, cuda)
    e = abs(loss.item() - float(fx["loss"])) / abs(float(fx["loss"]))
    el = rel_err(logits.float().cpu().numpy(), fx["logits"])
    print(f"{tag} {kind}: loss {loss.item():.6f} ref {float(fx['loss']):.6f} rel {e:.2e} "
          f"(bound {_bound(tag, kind, 'loss'):.2e}); logits {el:.2e} (bound {_bound(tag, kind, 'logits'):.2e})")
    _record(f"model:{tag}:{kind}:forward", dict(loss=e, logits=el, bounds=dict(
        loss=_bound(tag, kind, "loss"), logits=_bound(tag, kind, "logits"))))
    assert e < _bound(tag, kind, "loss")
    assert el < _bound(tag, kind, "logits")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", list(WIDE_CFG))
def test_wide_backward_grads(cuda, golden, tag, kind):
    """Every trainable gradient by helpers.check_summary; frozen parameters get none."""
    from tests.helpers import check_summary
    fx = golden(f"{kind}_{tag}")
    m = _wide_model(kind, tag, cuda)
    _, loss = _wide_loss(kind, m, fx, cuda)
    loss.backward()
    params = dict(m.named_parameters())
    names = _trainable(fx)
    assert names
    bound = _bound(tag, kind, "grads")
    errs = {n: _summary_err(fx, "grad:" + n, params[n].grad.float()) for n in names
            if params[n].grad is not None}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{tag} {kind}: worst gradient {worst[1]:.2e} ({worst[0]}), bound {bound:.2e}")
    _record(f"model:{tag}:{kind}:grads", dict(worst=worst[1], tensor=worst[0], bound=bound))
    for n in names:
        assert params[n].grad is not None, n
        check_summary(fx, "grad:" + n, params[n].grad.float(), bound)
    for n, p in params.items():
        if n not in names:
            assert p.grad is None, n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", list(WIDE_CFG))
def test_wide_three_adamw_steps(cuda, golden, tag, kind):
    from gvl.train import train_step
    from tests.helpers import check_summary, lr_caption, lr_cross, lr_lm, rel_err
    fx = golden(f"{kind}_{tag}")
    m = _wide_model(kind, tag, cuda)
    opt = m.configure_optimizers(weight_decay=0.1, learning_rate=1e-3, device="cuda")
    lr_of = {"gpt": lr_lm, "qformer": lr_caption, "cross": lr_cross}[kind]
    losses, norms = [], []
    for it in range(3):
        r = train_step(m, opt, [None], lambda mm, _b: _wide_loss(kind, mm, fx, cuda)[1], lr_of(it))
        losses.append(r.loss.item())
        norms.append(r.norm.item())
    params = dict(m.named_parameters())
    names = _trainable(fx)
    el, en = rel_err(losses, fx["train_losses"]), rel_err(norms, fx["train_norms"])
    ep = max(_summary_err(fx, "step3:" + n, params[n].float()) for n in names)
    b = {k: _bound(tag, kind, k) for k in ("train_losses", "train_norms", "params")}
    print(f"{tag} {kind}: losses {el:.2e} norms {en:.2e} params {ep:.2e}; bounds {b}")
    _record(f"model:{tag}:{kind}:adamw3", dict(train_losses=el, train_norms=en, params=ep, bounds=b))
    assert el < b["train_losses"]
    assert en < b["train_norms"]
    for n in names:
        check_summary(fx, "step3:" + n, params[n].float(), b["params"])


# ---------------------------------------------------------------------------- decode
DEC_B, DEC_P, DEC_NEW = 2, 8, 8
_DEC = {}


def _decode_case(kind, cuda):
    """(model at 1280 / 20, prompt [2, 8], z or None), one kind on the device at a time."""
    if kind not in _DEC:
        from tests.test_gpu_parity_full import _z
        _DEC.clear()
        model = _wide_model(kind, "wide1280", cuda)
        g = torch.Generator().manual_seed(77)
        prompt = torch.randint(0, 512, (DEC_B, DEC_P), generator=g).to(cuda)
        z = None if kind == "gpt" else _z(5, DEC_B, ENC, cuda)
        _DEC[kind] = (model, prompt, z)
    return _DEC[kind]


@pytest.mark.parametrize("kind", ["gpt", "qformer"])
def test_wide_kv_decode_matches_full_forward(cuda, kind):
    """KVDecoder's prefill and three cached steps at n_embd = 1280 against the model's own full
    forward at the same positions: rel_err < 3e-2, test_gpu_decode.py's bound."""
    from gvl.decode import generate
    model, prompt, z = _decode_case(kind, cuda)
    toks, lg = generate(model, prompt, 4, z=z, greedy=True, return_logits=True)
    with torch.no_grad():
        seq = torch.cat([prompt, toks[:, :-1]], 1)
        full = (model(seq)[0] if kind == "gpt" else model(z, seq)[0]).float()
    P = DEC_P + full.shape[1] - seq.shape[1]  # caption logits lead with M image rows
    ref = full[:, P - 1:P - 1 + 4]
    err = (lg.float() - ref).abs().max().item() / ref.abs().max().item()
    print(f"wide decode {kind}: logits rel {err:.2e}")
    _record(f"decode:{kind}", dict(logits_rel=err))
    assert lg.shape == (DEC_B, 4, 512)
    assert err < 3e-2


def _same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (i, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(_bits(a) if a.is_floating_point() else a,
                           _bits(b) if b.is_floating_point() else b), f"output {i} differs"


@pytest.mark.parametrize("kind", ["gpt", "qformer"])
def test_wide_graph_replay_equals_eager(cuda, kind):
    """generate(graph=True) and beam_search(graph=True) at n_embd = 1280: the eager calls' ids,
    logits, lengths and scores bit for bit."""
    from gvl.decode import beam_search, generate
    model, prompt, z = _decode_case(kind, cuda)
    kw = dict(z=z, greedy=True, return_logits=True, return_lengths=True)
    _same(generate(model, prompt, DEC_NEW, graph=True, **kw), generate(model, prompt, DEC_NEW, **kw))
    kw = dict(z=z, num_beams=3, eos=None, return_all=True)
    _same(beam_search(model, prompt, DEC_NEW, graph=True, **kw), beam_search(model, prompt, DEC_NEW, **kw))


@pytest.mark.parametrize("kind", ["gpt", "qformer"])
def test_wide_speculative_equals_generate_greedy(cuda, kind):
    from gvl.decode import generate, speculative_generate
    model, prompt, z = _decode_case(kind, cuda)
    want, lg = generate(model, prompt, DEC_NEW, z=z, greedy=True, return_logits=True)
    top2 = lg.float().topk(2, dim=-1).values
    print(f"wide spec {kind}: smallest greedy margin {float((top2[..., 0] - top2[..., 1]).min()):.3f}")
    got = speculative_generate(model, prompt, DEC_NEW, z=z, greedy=True, draft_len=3)
    assert torch.equal(got, want), (got.tolist(), want.tolist())


# ------------------------------------------------------------------------------ GEMM
# (kernel instance, tune setting, workspace + tickets, M, N, K, a_mn, b_mn, epilogue): the instances
# the LM products of n_embd 1280 / 1600 reach (tests/data/gemm_routes_wide.json), N and K (for the
# weight-gradient layouts M and N) at the model's values with their ragged tiles: 1600 = 6 x 256 +
# 64, 4800 = 18 x 256 + 192, 6400 % 192 = 64, 1280 % 192 = 128.  The other extent is the smallest
# the planner takes to the instance (8 x an odd number for a row count, a multiple of 32 / 192 for
# a depth), found with gvl_gemm_kernel_name on the CPU; the asserted name is part of the case.
_GEMM_ROWS = [
    ("gemm_pp3_kernel<4, false, false, 2, 256, 256>", (3, -1), 1, 7176, 1600, 1600, 0, 0, "bias_res"),
    ("gemm_pp3_kernel<4, false, true, 6, 256, 256>", (3, -1), 1, 7176, 1600, 6400, 0, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, false, true, 4, 256, 256>", (3, -1), 1, 1800, 6400, 1600, 0, 1, "dact"),
    ("gemm_pp3_kernel<4, true, true, 6, 192, 256>", (3, -1), 1, 4800, 1600, 32, 1, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, true, true, 6, 192, 256>", (3, -1), 1, 6400, 1600, 32, 1, 1, "res_inplace"),
    ("gemm_w4x_kernel<256, 192, true, true, 6, false>", (3, -1), 1, 1600, 6400, 4224, 1, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, true, true, 6, 192, 128>", (3, -1), 1, 3840, 1280, 32, 1, 1, "res_inplace"),
    ("gemm_pp3_kernel<4, false, false, 2, 192, 256>", (3, 3), 0, 4616, 1280, 1280, 0, 0, "bias_res"),
    ("gemm_ring_kernel<128, 128, 2, 2, 4, 1, false, false>", (3, -1), 1, 64, 4800, 1600, 0, 0, "bias"),
    ("gemm_pp3_kernel<4, false, false, 0, 256, 256>", (3, 3), 1, 8, 4800, 1600, 0, 0, "plain"),
    ("gemm_pp3_kernel<4, false, false, 1, 256, 256>", (3, -1), 1, 1800, 6400, 1600, 0, 0, "bias"),
    ("gemm_pp3_kernel<4, false, false, 9, 256, 256>", (3, -1), 1, 1800, 6400, 1600, 0, 0, "bias_act_d"),
    ("gemm_bf16_kernel<true, true>", (3, -1), 1, 3840, 1280, 8, 1, 1, "res_inplace"),
    ("gemm_w4x_kernel<256, 256, true, true, 6, false>", (3, -1), 1, 11784, 1280, 4096, 1, 1, "res_inplace"),
]


def _gemm_cases():
    from tests import gemm_ref as G
    cases = []
    for i, t in enumerate(_GEMM_ROWS):
        c = G._case(900 + i, t)
        if G.cost(c) > G.COST_CAP:
            # one input set where the float64 reference of two would take over ten seconds: the exact
            # integers where the instance must then be bit-exact, else the case's first kind
            c["kinds"] = ("exact",) if G.bitwise(c) else G.kinds_of(c)[:1]
        cases.append(c)
    return cases


_GEMM_CASES = _gemm_cases()


@pytest.mark.parametrize("case", _GEMM_CASES, ids=[c["id"] for c in _GEMM_CASES])
def test_wide_gemm_instances(cuda, case):
    """test_gpu_gemm.py's per-element check (Run / Arena, the references and bounds of
    tests/gemm_ref.py, the instance name asserted first) at the wide LM shapes: one case per
    instance of the wide route table's default routes (two for pp3<4, true, true, 6, 192, 256>:
    4800 and 6400 rows).  w4x<256, 256> needs K >= 4096 and 47 tile rows at N = 1280; at K = 4096
    the in-place accumulation is bit-exact on the integer inputs."""
    from tests import gemm_ref as G
    from tests import test_gpu_gemm as TG
    for kind in G.kinds_of(case):
        TG._check_case(case, kind, cuda)
        tag = f"{case['id']}/{kind}"
        if tag in TG._MARGINS:
            _record("gemm:" + tag, TG._MARGINS[tag])
