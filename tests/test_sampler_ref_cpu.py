"""tests/sampler_ref.py on the CPU: the draw predicate against the oracle's inverse CDF, the
doctored draw it rejects and the earlier rule accepted, the fp32 restatement of the sampler's
block scan (the boundary sweep meets its gaps; the owner rule has none), and the input
conditions of every edge case of tests/test_gpu_sampler.py."""
import numpy as np
import pytest

from oracle import ops as O
from tests import sampler_ref as S


def _sweep_ref():
    row = S.sweep_row()
    dist = O.sampling_distribution(S.row_values(row))
    return row, dist, S.cdf64(dist)


def test_predicate_accepts_the_oracle_and_its_fp32_neighbours():
    """The float64 inverse CDF satisfies the predicate for random and for boundary uniforms, with
    no filter and with top-k / top-p (zero-probability tokens between kept ones); so does the
    neighbouring kept token when u is within tol of the shared boundary, and no other."""
    row, dist, cdf = _sweep_ref()
    rng = np.random.default_rng(0)
    for d in (dist, O.sampling_distribution(S.row_values(row), 0.8, 40, 0.9)):
        c = S.cdf64(d)
        u = np.concatenate([rng.random(2000), S.boundary_sweep(c)[0][::37].astype(np.float64)])
        got = S.oracle_draws(d, u)
        assert got[::50].tolist() == [O.inverse_cdf_index(d, float(x)) for x in u[::50]]
        assert S.draw_ok(d, c, got, u).all()
        kept = np.nonzero(d > 0)[0]
        pos = np.searchsorted(kept, got)
        nxt = kept[np.minimum(pos + 1, kept.size - 1)]
        near = np.abs(c[got] - u) <= S.TOL
        ok_next = S.draw_ok(d, c, nxt, u)
        assert (ok_next == (near | (nxt == got))).all()
        assert not S.draw_ok(d, c, np.full(u.size, -1), u).any()
        assert not S.draw_ok(d, c, np.full(u.size, d.size), u).any()
        if (d == 0).any():
            assert not S.draw_ok(d, c, np.full(u.size, np.nonzero(d == 0)[0][0]), u).any()


def test_predicate_rejects_the_fallback_draw_the_old_rule_accepted():
    """The doctored output: the last kept token for a mid-range u that sits on a CDF boundary.
    The rule test_sampler_matches_reference_distribution had (u within 1e-5 of ANY boundary)
    accepts every one of them; the predicate rejects every one."""
    _, dist, cdf = _sweep_ref()
    u, bi = S.boundary_sweep(cdf)
    mid = (u > 0.05) & (u < 0.95)
    last = np.full(int(mid.sum()), dist.size - 1)
    assert mid.sum() > 20000
    assert S.old_boundary_rule(cdf, u[mid]).all()
    assert not S.draw_ok(dist, cdf, last, u[mid]).any()


def test_boundary_sweep_shape():
    _, dist, cdf = _sweep_ref()
    u, bi = S.boundary_sweep(cdf)
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
    assert 32000 < u.size <= 999 * 33
    # 33 consecutive floats around every boundary
    first = u[bi == 500]
    assert first.size == 33 and first[16] == np.float32(cdf[500])
    assert (np.diff(first.view(np.int32)) == 1).all()
    big = S.sweep_big_boundaries()
    assert big.size == 2000 and np.unique(big).size == 2000 and big.max() < S.SWEEP_BIG_V - 1
    tb = S.thread_boundaries()
    assert tb.size == 1005 and tb[0] == 49 and tb[-1] == 50249


def test_sweep_meets_gaps_of_the_fp32_scan():
    """The condition that the sweep's input is able to fail: in the fp32 restatement of the
    draw as it was (per-thread claim pre <= target < pre + s), some of the sweep's uniforms are
    claimed by no thread and fall back to token 999, far from u; every such draw breaks the
    predicate.  With the owner rule (the last thread with pre <= target) none falls back and
    every draw satisfies it."""
    row, dist, cdf = _sweep_ref()
    u, _ = S.boundary_sweep(cdf)
    em = S.ScanEmulation(row.numpy())
    tok, fell = em.draw(u, fixed=False)
    ok = S.draw_ok(dist, cdf, tok, u)
    print(f"claim rule: {int(fell.sum())} of {u.size} uniforms unclaimed, {int((~ok).sum())} draws rejected")
    assert fell.sum() >= 1
    assert (tok[fell] == 999).all() and not ok[fell & (u < 0.99)].any()
    assert ok[~fell].all()
    tok, fell = em.draw(u, fixed=True)
    assert not fell.any() and S.draw_ok(dist, cdf, tok, u).all()
    # and both forms agree with the oracle away from the boundaries
    um = np.random.default_rng(1).random(3000).astype(np.float32)
    for fixed in (False, True):
        t, _ = em.draw(um, fixed)
        assert S.draw_ok(dist, cdf, t, um).all()
        assert (t == S.oracle_draws(dist, um)).mean() > 0.99


def test_emulation_handles_many_tokens_per_thread():
    """E = 50 with ragged last threads: the owner rule tiles [0, tot) at the thread boundaries
    (a sample of them), the claim rule does not."""
    row = S.sweep_row(S.SWEEP_BIG_V, S.BF)
    dist = O.sampling_distribution(S.row_values(row))
    cdf = S.cdf64(dist)
    u, _ = S.boundary_sweep(cdf, S.thread_boundaries()[::4])
    em = S.ScanEmulation(row.float().numpy())
    assert em.E == 50 and em.s[1005] > 0 and not em.s[1006:].any()
    tok, fell = em.draw(u, fixed=True)
    assert not fell.any() and S.draw_ok(dist, cdf, tok, u).all()
    _, fell = em.draw(u, fixed=False)
    assert fell.any()


CASES = S.edge_cases()


def test_case_names_are_unique_and_cover_the_sizes():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    assert {c[1].numel() for c in CASES} >= {1, 63, 1000, 1024, 1025, 50257, 65536}
    for c in CASES:  # the values are exact in bf16, so fp32 and bf16 runs read the same row
        assert (c[1].to(S.BF).float() == c[1]).all()
        if c[1].numel() > 1025:  # (1025 unfiltered is still wide everywhere: two tokens a thread)
            assert 0 < c[3] <= 64


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_conditions(case):
    """Every kept interval is wider than 4 tol (in the peaked row: the narrow ones hold less
    than tol / 100 together, so they cannot move a wide token's midpoint); every top-k cut is an
    exact tie or clear by more than 1e-3 relative; the sorted cumulative probability stays more
    than 1e-4 away from top_p; u = 0 and u -> 1 belong to the first and the last kept token."""
    name, logits, temperature, top_k, top_p, narrow_ok = case
    cond = S.case_conditions(case)
    ref = S.case_reference(case)
    if narrow_ok:
        assert cond["narrow_count"] > 0 and cond["narrow_mass"] < S.TOL / 100
        assert ref["wide"].size == 5
    else:
        assert cond["narrow_count"] == 0
        assert ref["first"] == ref["kept"][0] and ref["last"] == ref["kept"][-1]
    assert cond["topk_tie"] or cond["topk_gap"] > 1e-3
    assert cond["topp_gap"] > 1e-4
    assert ref["wide"].size >= 1 and abs(ref["cdf"][-1] - 1.0) < 1e-12
    mids = ref["mids"]
    assert (S.oracle_draws(ref["dist"], mids) == ref["wide"]).all()


def test_tie_cases_keep_the_lowest_indices():
    """What the reference keeps in the tie rows (the GPU test asks the kernel for the same)."""
    by = {c[0]: S.case_reference(c)["kept"].tolist() for c in CASES}
    assert by["topk-tie5-keep2-V1000"] == [3, 17, 70, 333, 555, 901]
    assert by["topk-1-on-a-tie"] == [100]
    assert by["topp-cross-mid-tie"] == [10, 80, 150, 500]
    assert by["topp-cross-first-of-tie"] == [10, 500]
    assert by["topp-only-top"] == [500]
    assert by["topk5-topp0.6-tie"] == [10, 80, 500]
    assert len(by["topk-V-1"]) == 62 and 31 not in by["topk-V-1"]
    assert len(by["neginf-single-finite"]) == 1
