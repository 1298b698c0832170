"""tests/attn_ref.py checked on the CPU: the closed-form gradients equal float64 autograd, the
case list reaches every route of the dispatch, the bf16-rounding emulation passes the bounds
test_gpu_attention.py holds the kernels to, and those bounds reject doctored outputs that the
max-norm comparison of test_gpu_kernels._attn_case (rel_err < 1.2e-2 for o, 2.5e-2 for the
gradients) accepts.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from tests import attn_ref as A
from tests.helpers import assert_attn_close, assert_attn_tight, assert_f32_close, rel_err

BF = torch.bfloat16
F64 = torch.float64
OLD_TOL = dict(o=1.2e-2, dq=2.5e-2, dk=2.5e-2, dv=2.5e-2)


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


def _hard(got, ref, E, n, **kw):
    return assert_attn_close(got, ref[n], E[n], A.HARD_UNITS[n], slack=4 * A.baseline()[n], **kw)


# ---------------------------------------------------------------------------- reference
@pytest.mark.parametrize("causal,p", [(False, 0.0), (True, 0.0), (True, 0.1), (False, 0.1)])
def test_closed_form_equals_float64_autograd(causal, p):
    B, H, Tq, Tk = 2, 3, 37, 70
    x = A.inputs(B, H, Tq, Tk)
    keep = A.keep_mask(11, B, H, Tq, Tk, p) if p else None
    ref, _, _ = A.attention_ref(*x, causal, 0.2, p, keep)
    q, k, v, dO = (t.to(F64) for t in x)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * float(np.float32(0.2))
    s = s.masked_fill(~A.visible(Tq, Tk, causal), float("-inf"))
    P = torch.softmax(s, -1)
    if p:
        P = P * torch.from_numpy(keep).to(F64) * A.drop_scale(p)
    o = P @ v
    o.backward(dO)
    for n, t in (("o", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad),
                 ("lse", torch.logsumexp(s, -1).detach())):
        np.testing.assert_allclose(ref[n], t.numpy(), rtol=1e-12, atol=1e-13, err_msg=n)


def test_seed_eff_and_keep_mask():
    from tests.test_gpu_kernels import keep_mask
    assert A.seed_eff(5) == A.seed_eff(5, 0) == 5
    assert A.seed_eff(5, 1) == 5 ^ A.mix64(1) != 5
    B, H, Tq, Tk = 2, 3, 5, 7
    m = A.keep_mask(4242, B, H, Tq, Tk, 0.1)
    assert np.array_equal(m.reshape(-1), keep_mask(4242, np.arange(B * H * Tq * Tk), 0.1))
    big = A.keep_mask(1, 2, 2, 300, 300, 0.1)
    assert abs(big.mean() - 0.9) < 5e-3


# ------------------------------------------------------------------------------- routes
def test_cases_reach_every_route():
    """Every (forward kernel, backward path) pair the dispatch can reach, with and without
    dropout, is reached by the sweep's shapes, causal and not (the mask does not route); the
    classes are those of attention.hip at the time of writing: moving a 32 / 64 threshold there
    without restating it in attn_ref.routes leaves the kernel-level expectations below wrong."""
    for drop in (False, True):
        reach = {A.routes(tq, tk, drop) for tq in range(1, 200) for tk in range(1, 200)}
        for causal in (False, True):
            got = {A.routes(tq, tk, p > 0) for tq, tk, c, p in A.cases() if c == causal and (p > 0) == drop}
            if causal:  # the long case is causal only and adds no class
                assert got == reach, (drop, sorted(reach - got))
            assert got >= reach, (drop, causal, sorted(reach - got))
        fwd = {f for f, _ in reach}
        assert {b for _, b in reach} == set(A.BWD_CLASSES)
        assert fwd == (set(A.FWD_CLASSES) - {"dma<2>", "dma<1>"} if drop else set(A.FWD_CLASSES) - {"fwd<1>"})
    assert {A.routes(*s, False)[1] for s in A.PATH_SHAPES.values()} == set(A.BWD_CLASSES)
    for path, s in A.PATH_SHAPES.items():
        assert A.routes(*s, True)[1] == path
    # the combinations no kernel-level test ran before
    assert A.routes(100, 33, False) == ("fwd<2>", "dq<2>+dkdv")
    assert A.routes(40, 130, True) == ("fwd<1>", "dq<1>+dkdv")


# ----------------------------------------------------------- the reference alone passes
def _emulation_passes(x, causal, scale, p, keep, name):
    ref, E, emu = A.attention_ref(*x, causal, scale, p, keep)
    worst = {}
    for n in A.OUTS:
        worst[n] = assert_attn_close(emu[n], ref[n], E[n], A.HARD_UNITS[n], name=f"{name} {n}")
    for n in ("dq", "dk"):
        assert_attn_tight(emu[n], ref[n], E[n], emu[n], name=f"{name} {n}")
    f32 = A.attention_f32(*x, causal, scale, p, keep)
    for n in A.OUTS:  # an fp32 evaluation rounded to bf16
        _hard(torch.from_numpy(f32[n]).to(BF), ref, E, n, name=f"{name} fp32 {n}")
    return worst


def test_emulation_inside_hard_bounds_sweep():
    worst = dict.fromkeys(A.OUTS, 0.0)
    for c in A.cases():
        x, keep, ref, E, emu = A.case_data(*c)
        for n in A.OUTS:
            worst[n] = max(worst[n], assert_attn_close(emu[n], ref[n], E[n], A.HARD_UNITS[n],
                                                       name=f"{c} {n}"))
        assert_f32_close(A.attention_f32(*x, c[2], 0.125, c[3], keep)["lse"], ref["lse"], E["lse"],
                         4 * A.baseline()["lse"], name=f"{c} lse")
    print("emulation, worst over the sweep, units of 2**-8 E:", worst)
    assert 0.5 < worst["o"] and 0.5 < worst["dv"] and 0.1 < worst["dq"] and 0.1 < worst["dk"]


@pytest.mark.parametrize("kind", A.STRUCTURED)
def test_emulation_inside_hard_bounds_structured(kind):
    for (Tq, Tk) in A.STRUCT_SHAPES:
        for scale in A.STRUCT_SCALES:
            for causal in (False, True):
                x = A.structured_inputs(kind, *A.bh(Tq, Tk), Tq, Tk, scale)
                _emulation_passes(x, causal, scale, 0.0, None, f"{kind} {Tq}x{Tk} {scale} {causal}")


def test_structured_inputs_are_what_they_claim():
    Tq, Tk = 130, 257
    for scale in A.STRUCT_SCALES:
        mk = lambda kind: A.structured_inputs(kind, 2, 3, Tq, Tk, scale)
        s = lambda x: float(np.float32(scale)) * (x[0].to(F64) @ x[1].to(F64).transpose(-1, -2))
        rise = s(mk("rising"))
        tile_max = torch.stack([rise[..., i:i + 64].amax(-1) for i in range(0, Tk - 63, 64)], -1)
        assert (tile_max.diff(dim=-1) > 0.5).all()  # every row's maximum moves in every full key tile
        assert (rise[..., -1] > tile_max[..., -1] - 4.0).all()  # (the one-key last tile: no rescale)
        sp = s(mk("span60"))
        assert sp.max() > 60 and sp.min() < -60
        assert torch.softmax(sp, -1).amax(-1).median() > 0.9  # nearly one-hot rows
        assert s(mk("low")).max() < -100
        same = mk("same")
        assert (same[1] == same[1][:, :, :1]).all()
        assert not mk("dO0")[3].any()


# ----------------------------------------------------------------------- doctored outputs
def _old_inputs(B, H, Tq, Tk):
    """test_gpu_kernels._attn_case's own inputs, as [B, H, T, 64]."""
    torch.manual_seed(B * 100 + Tq + Tk)
    C = H * 64
    q, k, v = (torch.randn(B, T, C).to(BF) for T in (Tq, Tk, Tk))
    dO = torch.randn(B, Tq, C).to(BF)
    return tuple(t.reshape(B, t.shape[1], H, 64).permute(0, 2, 1, 3) for t in (q, k, v, dO))


@pytest.fixture(scope="module")
def lm1024():
    x = _old_inputs(1, 2, 1024, 1024)
    return (x,) + A.attention_ref(*x, True, 0.125)


def _old_accepts(bad, ref, n):
    e = rel_err(bad, ref[n])
    assert e < OLD_TOL[n], f"the max-norm comparison rejects it too ({e})"


@pytest.mark.parametrize("n,first", [("dv", 918), ("dk", 986)])
def test_rejects_doubled_last_key_rows(lm1024, n, first):
    """Causal B = 1, H = 2, T = 1024, the existing test's inputs: dv of every key >= 918 (dk:
    >= 986) doubled or zeroed passes rel_err < 2.5e-2; the per-element bound rejects either, and
    a x1.25 error on the single row `first`."""
    x, ref, E, emu = lm1024
    _hard(emu[n], ref, E, n)
    for f in (2.0, 0.0):
        bad = emu[n].copy()
        bad[:, :, first:] *= f
        _old_accepts(bad, ref, n)
        _rejects(_hard, bad, ref, E, n)
    bad = emu[n].copy()
    bad[:, :, first] *= 1.25
    _old_accepts(bad, ref, n)
    _rejects(_hard, bad, ref, E, n)
    if n == "dk":  # the bound the emulation sets is tighter still
        bad = emu[n].copy()
        bad[:, :, first] *= 1.05
        _hard(bad, ref, E, n)
        _rejects(assert_attn_tight, bad, ref[n], E[n], emu[n], slack=4 * A.baseline()[n])


def test_rejects_scaled_late_row_of_o_and_shifted_lse(lm1024):
    x, ref, E, emu = lm1024
    late = 512 + int(np.abs(ref["o"][0, 0, 512:]).max(-1).argmin())  # a quiet row of the second half
    bad = emu["o"].copy()
    bad[0, 0, late] *= 1.25
    _old_accepts(bad, ref, "o")
    _rejects(_hard, bad, ref, E, "o")
    base = 4 * A.baseline()["lse"]
    f32 = A.attention_f32(*x, True, 0.125)["lse"]
    assert_f32_close(f32, ref["lse"], E["lse"], base)
    _rejects(assert_f32_close, ref["lse"] + 1e-3, ref["lse"], E["lse"], base)
    one = ref["lse"].copy()
    one[0, 1, 700] += 1e-3
    _rejects(assert_f32_close, one, ref["lse"], E["lse"], base)
    # the sum of the bf16-rounded exponentials in place of the fp32 one: up to 2**-8 relative
    s = 0.125 * (x[0].to(F64) @ x[1].to(F64).transpose(-1, -2))
    s = s.masked_fill(~A.visible(1024, 1024, True), float("-inf"))
    m = s.amax(-1, keepdim=True)
    rounded = (m + torch.log(A._bf(torch.exp(s - m)).sum(-1, keepdim=True))).squeeze(-1)
    _rejects(assert_f32_close, rounded.numpy(), ref["lse"], E["lse"], base)


def test_rejects_a_dropped_last_key():
    """(130, 257) with key Tk - 1 left out (a `<` for a `<=` in the ragged last tile).  (At this
    size the max-norm comparison notices too: one key in 257 moves o by 12 % and dq by 15 % of
    their largest elements; it is listed because the per-element bound must not lose that.)"""
    Tq, Tk = 130, 257
    x, keep, ref, E, emu = A.case_data(Tq, Tk, False, 0.0)
    q, k, v, dO = x
    _, _, short = A.attention_ref(q, k[:, :, :-1], v[:, :, :-1], dO, False, 0.125)
    for n in A.OUTS:
        bad = short[n]
        if n in ("dk", "dv"):  # the last key's gradient rows never written: zero
            bad = np.concatenate([bad, np.zeros_like(bad[:, :, :1])], axis=2)
        _rejects(_hard, bad, ref, E, n)


def test_rejects_a_mask_of_the_wrong_row_length():
    """Dropout keyed on (row * (Tk + 1) + k): right for row 0 of the first head, wrong after."""
    Tq, Tk = 300, 300
    x, keep, ref, E, emu = A.case_data(Tq, Tk, True, A.DROP_P)
    B, H = A.bh(Tq, Tk)
    wrong = A.keep_mask(A.SEED, B, H, Tq, Tk, A.DROP_P, row_len=Tk + 1)
    assert np.array_equal(wrong[0, 0, 0], keep[0, 0, 0]) and not np.array_equal(wrong, keep)
    _, _, bad = A.attention_ref(*x, True, 0.125, A.DROP_P, wrong)
    for n in A.OUTS:
        _hard(emu[n], ref, E, n)
        _rejects(_hard, bad[n], ref, E, n)
