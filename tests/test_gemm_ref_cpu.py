"""The GEMM reference of tests/gemm_ref.py, checked on the CPU: epilogue64 against an independent
torch restatement; assert_bf16_rounded against doctored outputs that rel_err < 8e-3 accepts (all
doctoring is done on reference arrays); the case table against the built library and the route
table; and the emulation's slack, which must stay a small fraction of a bf16 ulp or the bound
would not be a rounding test.  No GPU: the name query touches no device."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as G
from tests.helpers import assert_bf16_close, assert_bf16_rounded, f64, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "gemm_routes.json")
BF = torch.bfloat16
M, N, K = 130, 264, 1000


def _bf64(x):
    """float64 values rounded to bf16 (through fp32), back in float64."""
    return f64(G.round_bf16(np.asarray(x, dtype=np.float32)))


def _trunc_bf16(x64):
    u = np.asarray(x64, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


# ------------------------------------------------------------ epilogue64 vs torch
def _torch_epilogue(h, kw):
    """The same epilogue from torch's own functions: F.gelu in both modes, autograd derivatives."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    a = kw.get("alpha", 1.0) * (kw["alpha_dev"] if kw.get("alpha_dev") is not None else 1.0)
    v = t(h) * a
    side = None

    def dgelu(x, mode):
        x = x.clone().requires_grad_(True)
        F.gelu(x, approximate=mode).sum().backward()
        return x.grad

    if kw.get("bias") is not None:
        v = v + t(kw["bias"])
    d = kw.get("dact", 0)
    if d:
        x = t(kw["pre_in"])
        v = v * (x if d == 3 else dgelu(x, "tanh" if d == 1 else "none"))
    act = kw.get("act", 0)
    if act == 5:
        v = v * torch.sigmoid(1.702 * v)
    elif act:
        mode = "tanh" if act in (1, 3) else "none"
        side = v if act in (1, 2) else dgelu(v, mode)
        v = F.gelu(v, approximate=mode)
    if kw.get("drop_p", 0) > 0:
        scale = float(np.float32(1) / (np.float32(1) - np.float32(kw["drop_p"])))
        v = torch.where(torch.from_numpy(kw["keep"]), v * scale, torch.zeros_like(v))
    if kw.get("gate") is not None:
        if not act:
            side = v
        v = v * math.tanh(kw["gate"])
    if kw.get("residual") is not None:
        v = v + t(kw["residual"])
    return v.numpy(), None if side is None else side.detach().numpy()


@pytest.mark.parametrize("epi", sorted(G.EPIS))
def test_epilogue64_matches_torch(epi):
    case = dict(M=40, N=24, K=64, epi=epi, alpha=0.75, alpha_dev=0.5)
    ins = G.inputs("act" if epi in G.ACT_EPIS else "random", 40, 24, 64, epi, seed=3)
    kw = G.epi_args(case, ins)
    h = f64(ins["A"]) @ f64(ins["B"])
    c, s = G.epilogue64(h, **kw)
    ct, st = _torch_epilogue(h, kw)
    np.testing.assert_allclose(c, ct, rtol=1e-12, atol=1e-14)
    assert (s is None) == (st is None) == (not G.EPIS[epi].get("pre_out"))
    if s is not None:
        np.testing.assert_allclose(s, st, rtol=1e-12, atol=1e-14)


def test_dropout_hash_is_the_kernel_tests_restatement():
    from tests.test_gpu_kernels import keep_mask
    assert np.array_equal(G.keep_mask(77, 13, 20, 0.1), keep_mask(77, np.arange(260), 0.1).reshape(13, 20))
    assert G.seed_eff(77, 0) == 77 and G.seed_eff(77, 5) != 77


def test_float32_restatements_match_float64_formulas():
    """fast_erf: absolute error <= 4.5 * 2**-24 |x| in gelu_erf, exact to 0.15 ulp down to -4, no
    relative accuracy below (the value the |x| term of E states)."""
    x = np.linspace(-8, 8, 4001)
    x32 = x.astype(np.float32).astype(np.float64)
    g = G.gelu_erf32(x32).astype(np.float64)
    assert np.all(np.abs(g - G.gelu_erf64(x32)) <= 4.5 * 2.0 ** -24 * np.abs(x32) + 1e-45)
    assert G.gelu_erf32(np.float32(-5.6)) == 0 and abs(G.gelu_erf64(np.array(-5.6)) + 6e-8) < 1e-8
    for f32, f64_ in [(G.gelu_tanh32, G.gelu_tanh64), (G.dgelu_tanh32, G.dgelu_tanh64),
                      (G.dgelu_erf32, G.dgelu_erf64), (G.quick_gelu32, G.quick_gelu64)]:
        assert np.all(np.abs(f32(x32).astype(np.float64) - f64_(x32)) <= 16 * 2.0 ** -24 * (np.abs(x32) + 1))


# ----------------------------------------------------------------- doctored outputs
def _honest(case, ins):
    r = G.reference(case, ins)
    kw = r["kw"]
    c32, s32 = G.epilogue32(G.matmul32_seq(f64(ins["A"]), f64(ins["B"])), **kw)
    return r, kw, _bf64(c32), None if s32 is None else _bf64(s32)


def _rejects(bad, r, what, side=False):
    ref, E, slack = (r["side"], r["E_side"], r["slack_side"]) if side else (r["ref"], r["E"], r["slack"])
    assert rel_err(bad, ref) < 8e-3, f"{what}: rel_err is meant to accept this"
    with pytest.raises(AssertionError):
        assert_bf16_rounded(bad, ref, E, slack, what)


def _case(epi, **kw):
    return dict(M=M, N=N, K=K, epi=epi, i=0, **kw)


def test_bound_accepts_the_honest_result_and_rejects_truncation():
    case = _case("plain")
    ins = G.inputs("random", M, N, K, "plain", seed=1)
    r, kw, good, _ = _honest(case, ins)
    assert rel_err(good, r["ref"]) < 8e-3
    assert_bf16_rounded(good, r["ref"], r["E"], r["slack"], "honest")
    bad = _trunc_bf16(G.matmul32_seq(f64(ins["A"]), f64(ins["B"])))
    # within one ulp everywhere: the one-ulp bound accepts it
    assert_bf16_close(bad, r["ref"], scale=r["E"], slack=r["slack"])
    _rejects(bad, r, "truncation")


def test_bound_rejects_bf16_split_k_partials():
    case = _case("plain")
    ins = G.inputs("random", M, N, K, "plain", seed=2)
    r, _, _, _ = _honest(case, ins)
    A, B = f64(ins["A"]), f64(ins["B"])
    h = K // 2
    parts = [_bf64(G.matmul32_seq(A[:, :h], B[:h])), _bf64(G.matmul32_seq(A[:, h:], B[h:]))]
    _rejects(_bf64(parts[0] + parts[1]), r, "bf16 partials")


def test_bound_rejects_rotated_small_rows():
    case = _case("plain")
    ins = G.inputs("random", M, N, K, "plain", seed=3)
    A = ins["A"].float()
    A[1::2] *= 2.0 ** -8
    ins["A"] = A.to(BF)
    r, _, good, _ = _honest(case, ins)
    bad = good.copy()
    bad[1::2] = np.roll(good[1::2], 4, axis=1)
    _rejects(bad, r, "rotated small rows")


def test_bound_rejects_a_neighbour_quad_bias_on_small_columns():
    case = _case("bias")
    ins = G.inputs("random", M, N, K, "bias", seed=4)
    cs = np.where(np.arange(N) < 64, 2.0 ** -6, 1.0).astype(np.float32)
    ins["B"] = (ins["B"].float() * torch.from_numpy(cs)).to(BF)
    ins["bias"] = (ins["bias"].float() * torch.from_numpy(cs) * 8).to(BF)
    r, kw, good, _ = _honest(case, ins)
    bias = f64(ins["bias"]).copy()
    bias[:60] = bias[4:64]  # the next quad's bias, inside the small-scale columns
    bad, _ = G.epilogue32(G.matmul32_seq(f64(ins["A"]), f64(ins["B"])), **{**kw, "bias": bias})
    _rejects(_bf64(bad), r, "neighbour-quad bias")


def test_bound_rejects_pre_out_taken_after_the_activation():
    case = _case("bias_act2")
    ins = G.inputs("random", M, N, K, "bias_act2", seed=5)
    ins["B"] = (ins["B"].float() * (0.05 / math.sqrt(K))).to(BF)
    ins["bias"] = torch.linspace(2.2, 8.0, N).to(BF)  # x in [2, 8]: gelu(x) is x to 6e-3 of the largest
    r, _, good, side = _honest(case, ins)
    assert_bf16_rounded(side, r["side"], r["E_side"], r["slack_side"], "honest pre_out")
    _rejects(good, r, "pre_out after the activation", side=True)  # gelu(x) stored where x belongs


def test_bound_rejects_one_flipped_dropout_bit():
    case = _case("drop_res")
    ins = G.inputs("scaled", M, N, K, "drop_res", seed=6)
    r, kw, good, _ = _honest(case, ins)
    assert_bf16_rounded(good, r["ref"], r["E"], r["slack"], "honest dropout")
    mag = np.abs(r["ref"])
    small = np.argwhere((mag < np.quantile(mag, 0.2)) & (mag > 0))
    for want in (True, False):  # one kept element dropped, one dropped element kept
        i, j = next((i, j) for i, j in small if kw["keep"][i, j] == want)
        keep = kw["keep"].copy()
        keep[i, j] = not want
        bad, _ = G.epilogue32(G.matmul32_seq(f64(ins["A"]), f64(ins["B"])), **{**kw, "keep": keep})
        _rejects(_bf64(bad), r, "flipped dropout bit")


def test_bound_rejects_an_erf_with_ten_times_the_error():
    case = _case("bias_act2")
    ins = G.inputs("act", M, N, K, "bias_act2", seed=7)
    # x = bias + a small product, in the negative tail -4.5 .. -3: E is about 2 |x|, gelu(x) is
    # small beside it (its ulp is a few units of 2**-24 E), so the formula's error is what is
    # measured; around 0 the same error hides in the rounding of a result of the size of x
    ins["B"] = (ins["B"].float() * 2.0 ** -7).to(BF)
    ins["bias"] = torch.linspace(-4.5, -3.0, N).to(BF)
    r, kw, good, _ = _honest(case, ins)
    assert_bf16_rounded(good, r["ref"], r["E"], r["slack"], "honest gelu_erf")
    bad, _ = G.epilogue32(G.matmul32_seq(f64(ins["A"]), f64(ins["B"])), erf_worse=10.0, **kw)
    _rejects(_bf64(bad), r, "fast_erf with 10x its error")


# -------------------------------------------------------------------- the case table
def test_every_instance_of_the_route_table_has_a_case():
    names = json.load(open(TABLE))["names"]
    have = {c["name"] for c in G.CASES}
    assert len(G.EXCLUDED) <= 8 and set(G.EXCLUDED) <= set(names)
    missing = [n for n in names if n not in have and n not in G.EXCLUDED]
    assert not missing, missing
    assert not have & set(G.EXCLUDED)


def test_every_case_reaches_its_instance_within_the_cost_cap():
    from gvl import _lib
    lib = _lib.load()
    assert len({c["id"] for c in G.CASES}) == len(G.CASES)
    for c in G.CASES + G.EXCLUDED_CASES:
        assert G.kernel_name(lib, c) == c["name"], c["id"]
        ldc = G.lds_of(c)[2]
        assert ldc > c["N"] and (not c["a_mn"] or c["M"] % 8 == 0)
    for c in G.CASES:
        assert G.cost(c) <= G.COST_CAP, c["id"]
    for c in G.EXCLUDED_CASES:
        assert G.cost(c) > G.COST_CAP and c["K"] <= 4096, c["id"]  # exact inputs stay exact to K = 4096


def test_the_table_has_the_shapes_it_promises():
    cs = G.CASES
    assert any(c["M"] >= 12288 for c in cs + G.EXCLUDED_CASES)  # group = 4
    assert any(math.ceil(c["M"] / 256) * math.ceil(c["N"] / 256) >= 260 for c in cs)  # persistent loop
    assert any(c["tune"] == (3, 13) for c in cs) and any(c["epi"] == "c_fp32" for c in cs)
    assert any(c.get("alpha_dev") for c in cs) and any(c.get("seed_off") for c in cs)
    assert {(c["a_mn"], c["b_mn"]) for c in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c["K"] == 32 for c in cs) and any((c["K"] // 32) % 2 == 1 and c["K"] > 32 for c in cs)
    assert any(c["K"] % 32 for c in cs) and any(c["N"] % 8 == 4 for c in cs) and any(not c["ws"] for c in cs)
    assert all(c["M"] % 64 for c in cs) and sum(c["N"] % 64 == 0 for c in cs) < len(cs)


_SLACK_CASES = [c for c in G.CASES if G.kinds_of(c)[0] in ("random", "scaled")]


@pytest.mark.parametrize("part", range(4))
def test_slack_is_a_small_fraction_of_an_ulp(part):
    """For the random and scaled cases the emulation's slack is finite and its term stays below a
    quarter ulp for at least 95 % of the elements.  Rows beyond the first 1000 are left out here:
    the row count does not enter an element's error, and the GPU test computes every case whole."""
    assert len(_SLACK_CASES) >= 100
    med = []
    for c in _SLACK_CASES[part::4]:
        kind = G.kinds_of(c)[0]
        c = dict(c, M=min(c["M"], 1000))
        ins = G.inputs(kind, c["M"], c["N"], c["K"], c["epi"], seed=c["i"])
        r = G.reference(c, ins, seed_off=c.get("seed_off"))
        for s, ref, E in [(r["slack"], r["ref"], r["E"])] + ([(r["slack_side"], r["side"], r["E_side"])]
                                                              if r["side"] is not None else []):
            assert np.isfinite(s), c["id"]
            u = G.slack_ulps(s, ref, E)[ref != 0]
            assert (u < 0.25).mean() >= 0.95, (c["id"], float((u < 0.25).mean()))
            med.append(float(np.median(u)))
    assert np.median(med) < 0.02
