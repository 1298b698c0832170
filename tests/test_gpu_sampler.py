"""gvl_sample's draw per token on the MI355X (csrc/decode.hip sample_kernel).

tests/test_gpu_decode.py holds the sampler on Gaussian rows with random uniforms, where a draw
next to a CDF boundary is a one-in-10^5 event.  Here the uniforms are placed: on and around
every boundary of a row (the inverse-CDF draw: per-thread intervals from a block scan must tile
[0, total) without gaps), and at the midpoint of every kept token's interval of rows built to
sit on the edges of the kept-set logic (ties at the top-k and top-p cuts, -inf logits, padded
rows, V around the block size and at its limit).  Every draw is judged by
tests/sampler_ref.py::draw_ok against the float64 distribution of oracle/ops.py; the counts and
the worst boundary distance go to profiles/misc_margins.json."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import sampler_ref as S
from tests.misc_ref import record as _record

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
PAD = 1e30     # the padding columns of a strided row: drawn at once if ever read
SENT = -7      # around the int64 output

def _out_arena(n, cuda):
    big = torch.full((n + 16,), SENT, dtype=torch.int64, device=cuda)

    def untouched():
        return bool(torch.all(big[:8] == SENT)) and bool(torch.all(big[8 + n:] == SENT))

    return big[8:8 + n], untouched


def _sweep(cuda, V, dtype, which, tag=""):
    import gvl.kernels as K
    row = S.sweep_row(V, dtype)
    dist = O.sampling_distribution(S.row_values(row))
    cdf = S.cdf64(dist)
    u, _ = S.boundary_sweep(cdf, which)
    out, untouched = _out_arena(u.size, cuda)
    K.sample(row.to(cuda).expand(u.size, V), torch.from_numpy(u).to(cuda), 1.0, 0, 1.0, out=out)
    got = out.cpu().numpy()
    assert untouched(), "a store outside the output"
    ok = S.draw_ok(dist, cdf, got, u)
    differs = got != S.oracle_draws(dist, u)
    worst = float(S.edge_distance(dist, cdf, got[differs & ok], u[differs & ok]).max()) \
        if (differs & ok).any() else 0.0
    bad = np.nonzero(~ok)[0]
    last = int(np.nonzero(dist > 0)[0][-1])
    print(f"boundary sweep V={V} {dtype}: {u.size} draws, {int(differs.sum())} differ from the "
          f"float64 inverse CDF, worst |u - nearer edge| among the accepted {worst:.3g}; "
          f"{bad.size} rejected, {int((got[bad] == last).sum())} of them the last kept token")
    _record(f"sweep:V{V}:{'fp32' if dtype == F32 else 'bf16'}{tag}",
            dict(draws=int(u.size), differ=int(differs.sum()), rejected=int(bad.size),
                 rejected_last_token=int((got[bad] == last).sum()),
                 worst_edge_distance=worst, tol=S.TOL))
    lo, hi = S.draw_edges(dist, cdf, np.clip(got[bad[:5]], 0, V - 1))
    assert bad.size == 0, (
        f"{bad.size} of {u.size} draws outside their token's CDF interval; first (u, token, "
        f"interval): {[(float(u[i]), int(got[i]), (float(a), float(b))) for i, a, b in zip(bad[:5], lo, hi)]}")


def test_boundary_sweep_fp32(cuda):
    """Every fl32(cdf[i]), i < 999, of a 1000-token fp32 row (one token per thread) and its 16
    fp32 neighbours on each side, ~33k uniforms in one launch: every draw within 1e-5 of its
    token's float64 interval.  Before the owner of the draw was defined by `the last thread with
    pre <= target`, a target in the gap between fl(pre_i + s_i) and pre_{i+1} was claimed by no
    thread and drew token 999; tests/test_sampler_ref_cpu.py shows that this sweep meets such
    gaps in the fp32 restatement of the scan.
    Measured on the MI355X: with the per-thread claim 119 of the 32,967 draws returned token 999
    (u from 0.0015 up; the restatement with numpy's exp predicts 121); with the owner rule none,
    585 draws differ from the float64 inverse CDF, each within 1.1e-7 of its token's interval."""
    _sweep(cuda, S.SWEEP_V, F32, None)


def test_boundary_sweep_bf16_ragged(cuda):
    """The same at V = 50257 in bf16: 50 tokens per thread, thread 1005 holds 7 and the rest
    none; 2000 boundaries from a seeded permutation."""
    _sweep(cuda, S.SWEEP_BIG_V, BF, S.sweep_big_boundaries())


def test_boundary_sweep_bf16_thread_boundaries(cuda):
    """V = 50257 in bf16 again, at the 1005 boundaries where one thread's 50 tokens end and the
    next thread's begin: a seeded choice of 2000 of 50256 boundaries meets about 40 of them
    (and met no gap).  Measured on the MI355X: with the per-thread claim 155 of the 33,165
    draws returned token 50256; with the owner rule none, the worst distance is 3.8e-7."""
    _sweep(cuda, S.SWEEP_BIG_V, BF, S.thread_boundaries(), tag=":thread-boundaries")


CASES = S.edge_cases()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kept_set_and_token_cdf(cuda, case, dtype):
    """One draw at the midpoint of every kept token's float64 CDF interval (wider than 4e-5)
    must return exactly that token, u = 0 the first kept token and u = nextafter(1, 0) the
    last; no draw has dist == 0.  (The peaked row at temperature 0.05 has kept tokens of mass
    1e-37 .. 1e-6 in front of and behind its five wide ones, below what an fp32 prefix sum
    resolves: there the two end draws are held to draw_ok alone.)  Each draw reads its own row
    of a [draws, V + 3] buffer whose padding columns hold +1e30.  The cases and the conditions that make fp32 and float64 agree
    on the kept set are in tests/sampler_ref.py (asserted by tests/test_sampler_ref_cpu.py)."""
    import gvl.kernels as K
    name, logits, temperature, top_k, top_p, narrow_ok = case
    ref = S.case_reference(case)
    V = logits.numel()
    u = np.concatenate([ref["mids"], [0.0, S.U_LAST]])
    u = u.astype(np.float32)
    want = np.concatenate([ref["wide"], [ref["first"], ref["last"]]])
    buf = torch.full((u.size, V + 3), PAD, dtype=dtype)
    buf[:, :V] = logits.to(dtype)
    out, untouched = _out_arena(u.size, cuda)
    K.sample(buf.to(cuda)[:, :V], torch.from_numpy(u).to(cuda), temperature, top_k, top_p,
             out=out)
    got = out.cpu().numpy()
    assert untouched(), "a store outside the output"
    assert ((got >= 0) & (got < V)).all(), f"{name}: a token outside [0, V): {got[(got < 0) | (got >= V)][:5]}"
    assert (ref["dist"][got] > 0).all(), \
        f"{name}: drew tokens outside the kept set: {got[ref['dist'][got] == 0][:5]}"
    exact = np.ones(u.size, dtype=bool)
    exact[-2:] = not narrow_ok
    wrong = np.nonzero((got != want) & exact)[0]
    assert wrong.size == 0, (f"{name}: {wrong.size} of {u.size} draws; first (u, got, want): "
                             f"{[(float(u[i]), int(got[i]), int(want[i])) for i in wrong[:5]]}")
    assert S.draw_ok(ref["dist"], ref["cdf"], got, u).all()
    _record(f"edge:{name}:{'fp32' if dtype == F32 else 'bf16'}", dict(draws=int(u.size)))
