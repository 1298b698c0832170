"""tests/misc_ref.py on the CPU: each float64 reference against torch or oracle/ops.py, the
input conditions the GPU tests rely on, and the doctored outputs that the per-element
assertions reject although helpers.rel_err < 8e-3 (the earlier bar) accepts them."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import misc_ref as M
from tests.helpers import (assert_bf16_close, assert_bf16_rounded, assert_f32_close, f64, rel_err,
                           ulp_bf16)

BF = torch.bfloat16
F32 = torch.float32


def _trunc_bf16(x64):
    """float64 -> bf16 by truncation of the fp32 bits (the doctored rounding)."""
    b = torch.from_numpy(np.asarray(x64, dtype=np.float32)).view(torch.int32) & ~0xFFFF
    return b.view(F32).to(BF)


# ------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("rows,cols", [(17, 136), (129, 264), M.COLSUM_TALL])
def test_colsum_reference_and_conditions(rows, cols):
    x = M.colsum_input(rows, cols)
    ref, E, base = M.colsum_ref(x)
    assert np.allclose(ref, x.double().sum(0).numpy(), rtol=1e-13, atol=0)
    assert np.isfinite(base) and base < 64
    if rows >= 16:
        cancel = np.arange(cols) % 7 == 3
        if cancel.any():  # the scale term matters: the sum is far below the sum of |x|
            assert (np.abs(ref[cancel]) < E[cancel] / 16).all()
        assert (np.abs(ref[~cancel]) > 0).all()
    if cols >= 9:  # columns differ in scale by 2**8
        m = np.abs(f64(x)).max(axis=0)
        assert m.max() / m.min() > 64
    prev = torch.ones(cols, dtype=BF)
    ref2, E2, _ = M.colsum_ref(x, prev)
    assert np.allclose(ref2, ref + 1.0) and np.allclose(E2, E + 1.0)


def test_colsum_rejects_a_zeroed_small_column():
    """Column 9 (scale 2**-4, 2**8 below the largest) zeroed: rel_err accepts, the per-column
    assertion does not; the correctly rounded sums pass."""
    x = M.colsum_input(129, 264)
    ref, E, base = M.colsum_ref(x)
    good = torch.from_numpy(ref).to(BF)
    assert_bf16_close(good, ref, scale=E, slack=M.slack_of(base))
    bad = good.clone()
    bad[9] = 0
    assert rel_err(bad.float().numpy(), ref) < 8e-3
    with pytest.raises(AssertionError):
        assert_bf16_close(bad, ref, scale=E, slack=M.slack_of(base))


# ----------------------------------------------------------------------------- dropout
def test_dropout_reference():
    x = (torch.randn(37, 45, generator=torch.Generator().manual_seed(0)) * 3).to(BF)
    want, keep = M.dropout_ref(x, 0.0, 5)
    assert bool(keep.all()) and torch.equal(M.bits(want), M.bits(x))
    want, keep = M.dropout_ref(x, 0.1, 5)
    frac = 1 - float(keep.float().mean())
    assert 0.05 < frac < 0.15
    near = x.double() / 0.9
    assert float(((want.double() - near).abs()[keep] / near.abs()[keep]).max()) < 2.0 ** -8
    assert not torch.any(M.bits(want)[~keep] != 0)
    # the keep index is r * cols + c of the logical tensor: another row length moves the mask
    _, keep48 = M.dropout_ref(torch.zeros(37, 48, dtype=BF), 0.1, 5)
    assert not torch.equal(keep[:, :45], keep48[:, :45])
    _, keep_off = M.dropout_ref(x, 0.1, 5, offset=3)
    assert not torch.equal(keep, keep_off)
    want999, keep999 = M.dropout_ref(x, 0.999, 5)
    assert float(keep999.float().mean()) < 0.01


# -------------------------------------------------------------------------------- gate
@pytest.mark.parametrize("gate", M.GATES)
def test_gate_reference_matches_autograd(gate):
    dx, y = M.gate_inputs(2049, cancel=False)
    g = torch.tensor(gate).to(BF)
    ref = M.gate_ref(dx, y, g)
    gg = g.double().clone().requires_grad_(True)
    yy = y.double().clone().requires_grad_(True)
    (torch.tanh(gg) * yy).backward(dx.double())
    assert np.allclose(ref["dy"], yy.grad.numpy(), rtol=1e-14, atol=0)
    # (autograd's 1 - tanh^2 cancels at gate 9: 1e-8 relative there, exact elsewhere)
    assert abs(ref["dg"] - float(gg.grad)) <= (1e-7 if gate == 9.0 else 1e-12) * ref["E"]
    assert np.isfinite(ref["base"])


def test_gate_cancelling_input_cancels():
    dx, y = M.gate_inputs(2048, cancel=True)
    ref = M.gate_ref(dx, y, torch.tensor(0.3).to(BF))
    assert abs(ref["dg"]) < ref["E"] / 16


def test_gate_rejects_truncated_rounding():
    """dy truncated to bf16 instead of rounded: within one ulp (assert_bf16_close and
    rel_err < 8e-3 accept it), but not correctly rounded."""
    dx, y = M.gate_inputs(2049)
    ref = M.gate_ref(dx, y, torch.tensor(0.3).to(BF))
    good = torch.from_numpy(ref["dy"]).to(BF)
    assert_bf16_rounded(good, ref["dy"], np.abs(ref["dy"]), 2)
    bad = _trunc_bf16(ref["dy"])
    assert rel_err(bad.float().numpy(), ref["dy"]) < 8e-3
    assert_bf16_close(bad, ref["dy"])
    with pytest.raises(AssertionError):
        assert_bf16_rounded(bad, ref["dy"], np.abs(ref["dy"]), 2)


def test_bf16_accumulator_two_roundings():
    g0 = torch.tensor([0.75], dtype=BF)
    got = M.bf16_add_two_roundings(g0, 0.00390625 * 1.4)  # bf16(dg) first, then the sum
    d = torch.tensor(0.00390625 * 1.4).to(BF).float()
    assert torch.equal(got, (g0.float() + d).to(BF))


# -------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("side", M.POOL_SIDES)
def test_pool_reference_is_the_oracle(side):
    tok = M.pool_input(2, side, 260, F32)
    ref, scale, base = M.pool_ref(tok, 1)
    assert rel_err(ref, O.pool_clip(tok).numpy()) < 1e-6
    z32, _ = M._pool(tok, 1, F32)
    assert torch.equal(z32, O.pool_clip(tok))  # the baseline IS oracle.pool_clip in fp32
    assert np.allclose(np.linalg.norm(ref, axis=-1), 1.0, atol=1e-12)
    raw, scale0, _ = M.pool_ref(tok, 0)
    assert np.allclose(raw[:, 0], f64(tok[:, 0]))
    assert np.isfinite(base) and base < 64
    # the 33 rows differ in scale: CLS 2**10 above, window 5 2**10 below the rest
    m = scale0.mean(axis=(0, 2))
    if side >= 8:
        assert m[0] / np.median(m) > 500 and np.median(m) / m[6] > 500


def test_pool_routes_cover_every_kernel_instance():
    table = {("pool4<8>", 16, 768, True, True), ("pool4<16>", 14, 768, True, True),
             ("pool<float>-unrolled", 16, 6, True, True), ("pool<float>-unrolled", 16, 768, True, False),
             ("pool<float>-loop", 24, 260, True, True), ("pool<bf16>-unrolled", 16, 768, False, True),
             ("pool<bf16>-loop", 24, 768, False, True), ("pool<bf16>-loop", 14, 768, False, True)}
    for want, side, D, f32, aligned in table:
        assert M.pool_route(side, D, f32, aligned) == want
    assert len(M.pool_windows(7)) == 32 and M.pool_windows(7)[0] == (0, 2, 0, 1)


def test_pool_rejects_a_dropped_window_row():
    """Window 5 (scale 2**-10) averaged without its last patch row: rel_err accepts, the
    per-row scale does not."""
    tok = M.pool_input(1, 16, 768, F32)
    ref, scale, base = M.pool_ref(tok, 0)
    good = torch.from_numpy(ref).float()
    assert_f32_close(good, ref, scale, M.slack_of(base))
    r0, r1, c0, c1 = M.pool_windows(16)[5]
    grid = tok[:, 1:].view(1, 16, 16, 768).double()
    bad = good.clone()
    bad[:, 6] = (grid[:, r0:r1 - 1, c0:c1].sum(dim=(1, 2)) / ((r1 - r0) * (c1 - c0))).float()
    assert rel_err(bad.numpy(), ref) < 8e-3
    with pytest.raises(AssertionError):
        assert_f32_close(bad, ref, scale, M.slack_of(base))
    with pytest.raises(AssertionError):
        assert_bf16_close(bad.to(BF), ref, scale=scale, slack=M.slack_of(base))


# ------------------------------------------------------------------ embedding backward
def _emb_case():
    C = 130
    idx, dout, T, S, off, V, n = M.emb_case(C)
    return idx, dout, T, S, off, C, V, n


def test_embedding_bwd_reference_matches_autograd():
    idx, dout, T, S, off, C, V, n = _emb_case()
    ref = M.emb_bwd_ref(idx, dout, T, S, off, C, V, n, torch.zeros(V, C), torch.zeros(T + 2, C))
    ids = idx.view(-1)[:n]
    ok = (ids >= 0) & (ids < V)
    r = torch.arange(n)
    rows = dout.double().view(-1, C)[(r // T) * S + off + r % T]
    wte = torch.zeros(V, C, dtype=torch.float64, requires_grad=True)
    wpe = torch.zeros(T + 2, C, dtype=torch.float64, requires_grad=True)
    emb = wte[ids.clamp(0, V - 1)] * ok[:, None] + wpe[r % T]
    (emb * rows).sum().backward()
    assert np.allclose(ref["dwte"], wte.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(ref["dwpe"], wpe.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert ref["S_dwte"][7, 0] >= 502 and ref["S_dwte"][V - 1, 0] == 2
    assert n % 4 != 0 and int((ids == V + 3).sum()) == 1 and int((ids == -1).sum()) == 1
    assert M.emb_bwd_ref(idx, dout, T, S, off, C, V, n, None, torch.zeros(T + 2, C))["dwte"] is None


def test_embedding_bwd_rejects_a_dropped_hot_token():
    """One of the 500 tokens of the hot id left out of its row: 1 / 500 of a row whose norm
    dominates, so rel_err accepts; the per-element bound (terms + 1 fp32 roundings) does not."""
    idx, dout, T, S, off, C, V, n = _emb_case()
    w0 = torch.randn(V, C, generator=torch.Generator().manual_seed(1))
    ref = M.emb_bwd_ref(idx, dout, T, S, off, C, V, n, w0, None)
    good = torch.from_numpy(ref["dwte"]).float()
    assert_f32_close(good, ref["dwte"], ref["E_dwte"] * ref["S_dwte"], 1)
    first = int(np.nonzero(idx.view(-1).numpy()[:n] == 7)[0][0])
    row = dout.double().view(-1, C)[(first // T) * S + off + first % T]
    bad = good.clone()
    bad[7] = (torch.from_numpy(ref["dwte"][7]) - row).float()
    assert rel_err(bad.numpy(), ref["dwte"]) < 8e-3
    with pytest.raises(AssertionError):
        assert_f32_close(bad, ref["dwte"], ref["E_dwte"] * ref["S_dwte"], 1)
