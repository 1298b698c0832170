"""CPU proof of the scoring references and assertions (tests/score_ref.py):

  * token_ref64 against an independent statement (F.log_softmax + gather, torch.logsumexp,
    torch.argmax, a stable-sort rank) and sequence_ref64's pred_norm against
    gvl.data.get_most_likely_row itself;
  * the assertions used on the GPU pass the fp32 CPU baseline and reject doctored outputs;
  * the baseline error of logp and lse, and the host-side argument checks of both entry points
    (no device needed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import score_ref as S
from tests.helpers import F32_UNIT

SMALL = [s for s in S.TOKEN_SHAPES if s[0] <= 50257]


def _slack():
    base = S.token_baseline()
    return {k: S.MARGIN * v for k, v in base.items()}


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("variant", S.TOKEN_VARIANTS)
@pytest.mark.parametrize("V,ld", SMALL)
def test_token_ref_matches_log_softmax_and_sort(V, ld, variant, f32):
    c = S.token_case(V, ld, f32, variant)
    ref = S.token_ref64(c["logits"], V, c["targets"], c["mask"])
    x = c["logits"][:, :V].double()
    t = torch.from_numpy(c["targets"])
    lsm = F.log_softmax(x, dim=-1)
    lse = torch.logsumexp(x, dim=-1)
    am = torch.argmax(x, dim=-1)
    order = torch.sort(-x, dim=-1, stable=True).indices  # descending, ties: lower index first
    for r in range(x.shape[0]):
        if ref["skipped"][r]:
            assert (ref["logp"][r], ref["lse"][r], ref["argmax"][r], ref["rank"][r]) == (0, 0, -1, -1)
            continue
        assert ref["argmax"][r] == int(am[r])
        assert abs(ref["lse"][r] - float(lse[r])) <= 1e-12 * max(1.0, abs(float(lse[r])))
        if not 0 <= t[r] < V:
            assert np.isnan(ref["logp"][r]) and ref["rank"][r] == -1
            continue
        want = float(lsm[r, t[r]])
        if np.isinf(want):
            assert ref["logp"][r] == want  # -inf exactly, never NaN
        else:
            assert abs(ref["logp"][r] - want) <= 1e-12 * max(1.0, abs(want))
        assert ref["rank"][r] == int((order[r] == t[r]).nonzero()[0, 0])
        assert (ref["rank"][r] == 0) == (ref["argmax"][r] == t[r])


def test_token_case_holds_the_edge_rows():
    V, ld = 509, 512
    c = S.token_case(V, ld, False, "targets5")
    ref = S.token_ref64(c["logits"], V, c["targets"])
    x = c["logits"][:, :V].float().numpy()
    assert list(c["targets"][:3]) == [0, V - 1, S.ragged_target(V)] and S.ragged_target(V) >= 504
    t = c["targets"][3]
    top = np.flatnonzero(x[3] == x[3].max())
    assert len(top) == 2 and top[0] < t < top[1] and ref["argmax"][3] == top[0]
    same = np.flatnonzero(x[3] == x[3, t])
    assert len(same) == 3 and same[0] < t < same[2]
    assert ref["rank"][3] == int((x[3] > x[3, t]).sum()) + 1  # the equal one in front counts
    assert ref["logp"][4] == -np.inf and np.isfinite(ref["lse"][4])
    c = S.token_case(V, ld, False, "special5")
    ref = S.token_ref64(c["logits"], V, c["targets"], c["mask"])
    assert list(ref["skipped"]) == [True, True, False, False, False]
    assert np.isnan(ref["logp"][2]) and ref["rank"][2] == -1 and ref["argmax"][2] >= 0
    assert (c["logits"][:, V:] == S.SENTINEL).all()


@pytest.mark.parametrize("seed", range(4))
def test_sequence_ref_matches_get_most_likely_row(seed):
    from gvl.data import get_most_likely_row
    g = torch.Generator().manual_seed(seed)
    E, T, V = 4, 12, 40
    logits = torch.randn(E, T, V, generator=g) * 2
    tokens = torch.randint(0, V, (E, T), generator=g)
    mask = torch.zeros(E, T, dtype=torch.long)
    for e in range(E):
        mask[e, 3 + e % 2:7 + e] = 1
    tok = S.token_ref64(logits[:, :-1].reshape(-1, V), V, tokens[:, 1:].reshape(-1).numpy())
    ref = S.sequence_ref64(tok["logp"].reshape(E, T - 1), mask[:, 1:].numpy(), E)
    assert ref["pred_norm"][0] == get_most_likely_row(tokens, mask, logits)
    losses = F.cross_entropy(logits[:, :-1].reshape(-1, V).double(), tokens[:, 1:].reshape(-1),
                             reduction="none").view(E, T - 1)
    want = (losses * mask[:, 1:]).sum(dim=1)
    assert np.allclose(ref["sum"], want.numpy(), rtol=1e-12)
    assert np.array_equal(ref["count"], mask[:, 1:].sum(dim=1).numpy())
    assert ref["pred"][0] == int(want.argmin())


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("N,T,group", S.SEQ_SHAPES)
def test_sequence_cases_are_decided_and_hold_ties(N, T, group, masked):
    c = S.seq_case(N, T, group, masked)
    ref = S.sequence_ref64(c["logp"], c["mask"], group)
    assert S.sequence_decided(ref, T, group).all()
    if group >= 3:  # the equal pair (1, group - 1) wins example 0: the first of them
        assert np.array_equal(c["logp"][1], c["logp"][group - 1])
        assert ref["mean"][1] == ref["mean"][group - 1] and ref["pred_norm"][0] == 1
    if masked and N >= 3 and N // group != 1:
        assert ref["count"][N - 1] == 0 and ref["pred_norm"][-1] == -1 and ref["pred"][-1] == -1
        assert np.isnan(ref["mean"][N - 1])
    got = S.sequence_f32(c["logp"], c["mask"])
    S.check_sequence_outputs(dict(sum=got["sum"].numpy(), mean=got["mean"].numpy(),
                                  count=ref["count"], pred_norm=ref["pred_norm"],
                                  pred=ref["pred"]), ref, T, group)


# ------------------------------------------------------------------ the assertions reject
def _good(V, ld, f32, variant):
    """The reference rounded to fp32: what a correct kernel may return."""
    c = S.token_case(V, ld, f32, variant)
    ref = S.token_ref64(c["logits"], V, c["targets"], c["mask"])
    got = dict(logp=ref["logp"].astype(np.float32), lse=ref["lse"].astype(np.float32),
               argmax=ref["argmax"].copy(), rank=ref["rank"].copy())
    return c, ref, got


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("variant", S.TOKEN_VARIANTS)
def test_assertions_pass_the_reference_and_the_fp32_baseline(variant, f32):
    c, ref, got = _good(509, 512, f32, variant)
    S.check_token_outputs(got, ref, _slack(), "rounded reference")
    ok = ~ref["skipped"] & (ref["rank"] >= 0)
    base = S.token_f32(c["logits"][torch.from_numpy(ok)], 509, c["targets"][ok])
    for k in ("logp", "lse"):
        got[k][ok] = base[k].numpy()
    S.check_token_outputs(got, ref, _slack(), "fp32 baseline")


def test_rejects_logp_off_by_twice_the_bound():
    c, ref, got = _good(509, 512, False, "targets5")
    slack = _slack()
    for k in ("logp", "lse"):
        bad = dict(got)
        v = ref[k].copy()
        v[1] += 2 * slack[k] * F32_UNIT * ref["scale_" + k][1]
        bad[k] = v.astype(np.float32)
        with pytest.raises(AssertionError, match=r"worst at \(1,\)"):
            S.check_token_outputs(bad, ref, slack, k)


def test_rejects_rank_off_by_one():
    c, ref, got = _good(509, 512, False, "targets5")
    for d in (1, -1):
        bad = dict(got, rank=got["rank"].copy())
        bad["rank"][3] += d  # the row with ties on both sides of the target
        with pytest.raises(AssertionError, match="rank"):
            S.check_token_outputs(bad, ref, _slack())


def test_rejects_argmax_of_the_last_maximum():
    c, ref, got = _good(509, 512, False, "targets5")
    x = c["logits"][3, :509].float().numpy()
    last = int(np.flatnonzero(x == x.max())[-1])
    assert last != ref["argmax"][3]
    bad = dict(got, argmax=got["argmax"].copy())
    bad["argmax"][3] = last
    with pytest.raises(AssertionError, match="argmax"):
        S.check_token_outputs(bad, ref, _slack())


@pytest.mark.parametrize("V,ld", [(8, 12), (12, 16), (509, 512)])
def test_rejects_a_pad_column_read_as_a_logit(V, ld):
    c, ref, got = _good(V, ld, False, "one")
    for cols in (V + 1, ld):  # one pad column, all of them
        wrong = S.token_ref64(c["logits"], cols, c["targets"], c["mask"])
        bad = dict(got, logp=wrong["logp"].astype(np.float32), lse=wrong["lse"].astype(np.float32))
        with pytest.raises(AssertionError, match="out of tolerance"):
            S.check_token_outputs(bad, ref, _slack())
        with pytest.raises(AssertionError, match="argmax"):
            S.check_token_outputs(dict(argmax=wrong["argmax"]), ref, _slack())


def test_rejects_a_skipped_row_written():
    c, ref, got = _good(509, 512, False, "special5")
    full = S.token_ref64(c["logits"], 509, np.where(ref["skipped"], 5, c["targets"]))
    for r in (0, 1):  # the ignored row, the masked row
        for k in ("logp", "lse", "argmax", "rank"):
            bad = dict(got)
            bad[k] = got[k].copy()
            bad[k][r] = full[k][r]
            with pytest.raises(AssertionError):
                S.check_token_outputs(bad, ref, _slack())
    bad = dict(got, logp=got["logp"].copy())
    bad["logp"][2] = 0.0  # the out-of-range row must be NaN
    with pytest.raises(AssertionError):
        S.check_token_outputs(bad, ref, _slack())
    c4, ref4, got4 = _good(509, 512, False, "targets5")
    got4["logp"][4] = np.nan  # a -inf target must give -inf, not NaN
    with pytest.raises(AssertionError):
        S.check_token_outputs(got4, ref4, _slack())


def test_sequence_assertions_reject_doctored_outputs():
    N, T, group = 6, 63, 3
    c = S.seq_case(N, T, group)
    ref = S.sequence_ref64(c["logp"], c["mask"], group)
    good = dict(sum=ref["sum"].astype(np.float32), mean=ref["mean"].astype(np.float32),
                count=ref["count"], pred_norm=ref["pred_norm"], pred=ref["pred"])
    S.check_sequence_outputs(good, ref, T, group)
    bad = dict(good, sum=good["sum"].copy())
    bad["sum"][0] += np.float32(2 * T * F32_UNIT * ref["scale"][0])
    with pytest.raises(AssertionError, match="sum_nll"):
        S.check_sequence_outputs(bad, ref, T, group)
    bad = dict(good, count=good["count"] + np.int32(1))
    with pytest.raises(AssertionError, match="count"):
        S.check_sequence_outputs(bad, ref, T, group)
    bad = dict(good, pred_norm=np.asarray([group - 1, -1], dtype=np.int32))  # the later twin
    with pytest.raises(AssertionError, match="pred_norm"):
        S.check_sequence_outputs(bad, ref, T, group)
    bad = dict(good, pred=np.asarray([ref["pred"][0], 0], dtype=np.int32))  # an empty sequence
    with pytest.raises(AssertionError, match="pred"):
        S.check_sequence_outputs(bad, ref, T, group)
    unmasked = S.sequence_ref64(c["logp"], None, group)  # the mask ignored
    bad = dict(good, sum=unmasked["sum"].astype(np.float32))
    with pytest.raises(AssertionError):
        S.check_sequence_outputs(bad, ref, T, group)


# ------------------------------------------------------------------ the model-level inputs
@pytest.mark.parametrize("kind", S.MODEL_KINDS)
def test_oracle_decides_every_model_example(kind):
    """At MODEL_SEED the fp32 CPU oracle separates the best ending of every example from the
    runner-up by more than twice the GEMM-route bound, for every model kind: the GPU test may
    leave none out."""
    from oracle import ops as O
    from oracle import weights as W
    from tests.helpers import TINY, recipe_params
    from tests.test_gpu_parity_full import _build_tiny
    sd = _build_tiny(kind).state_dict()
    P = recipe_params([(k, tuple(v.shape)) for k, v in sd.items()])
    tokens, mask = S.model_inputs(TINY["vocab_size"])
    z = None
    if kind != "gpt":
        D = TINY["n_embd"]
        z = O.pool_clip(torch.from_numpy(W.make_normal_like(S.MODEL_N * 257 * D, S.Z_SEED))
                        .view(S.MODEL_N, 257, D))
    logits = S.oracle_text_logits(kind, P, tokens, z, TINY)
    assert tuple(logits.shape) == (S.MODEL_N, S.MODEL_T, TINY["vocab_size"])
    ref = S.model_reference(logits, tokens, mask)
    means = ref["seq"]["mean"].reshape(-1, S.MODEL_GROUP)
    gaps = np.sort(means, axis=1)
    print(f"{kind}: gaps {(gaps[:, 1] - gaps[:, 0]).tolist()} against twice the bounds "
          f"{(2 * ref['seq_bound'].reshape(-1, S.MODEL_GROUP).max(axis=1)).tolist()}")
    assert ref["decided"].all()
    assert (ref["seq"]["count"] > 0).all() and (ref["seq"]["count"] < S.MODEL_T - 1).all()


# ------------------------------------------------------------------ the baseline, on record
def test_token_baseline_is_recorded():
    """fp32 torch on the CPU against the float64 reference over every GPU test case, in units of
    2**-24 * scale: a few roundings of the operands of lse = max + ln s and logp = x_t - lse."""
    base = S.token_baseline()
    print(f"token_logprobs CPU fp32 baseline: logp {base['logp']:.3f} lse {base['lse']:.3f} units; "
          f"the kernel gets {S.MARGIN} x")
    for k in ("logp", "lse"):
        assert 0.0 < base[k] <= 4.0, base


# ------------------------------------------------------------------ host-side checks
def _token_call(lib, **over):
    a = dict(logits=16, ld=512, f32=0, rows=4, V=509, targets=16, mask=None, logp=16, lse=None,
             argmax=None, rank=None)
    a.update(over)
    return lib.gvl_token_logprobs(a["logits"], a["ld"], a["f32"], a["rows"], a["V"], a["targets"],
                                  a["mask"], a["logp"], a["lse"], a["argmax"], a["rank"], None)


def _seq_call(lib, **over):
    a = dict(logp=16, mask=None, N=8, T=5, group=4, sum=16, count=16, mean=16, pn=16, p=16)
    a.update(over)
    return lib.gvl_sequence_score(a["logp"], a["mask"], a["N"], a["T"], a["group"], a["sum"],
                                  a["count"], a["mean"], a["pn"], a["p"], None)


def test_entry_points_reject_bad_arguments_without_gpu():
    """Fake non-null device pointers, never dereferenced: every call is rejected on the host."""
    from gvl import _lib
    lib = _lib.load()

    def rejected(rc, who, word):
        err = lib.gvl_last_error()
        assert rc == -1 and err.startswith(who) and word in err, (rc, err)

    for V in (0, -1, 65537):
        rejected(_token_call(lib, V=V, ld=1 << 20), b"gvl_token_logprobs", b"V=%d" % V)
    rejected(_token_call(lib, ld=508), b"gvl_token_logprobs", b"ld=508")
    rejected(_token_call(lib, logits=None), b"gvl_token_logprobs", b"null logits")
    rejected(_token_call(lib, targets=None), b"gvl_token_logprobs", b"null targets")
    rejected(_token_call(lib, rows=-1), b"gvl_token_logprobs", b"rows=-1")
    assert _token_call(lib, rows=0) == 0  # nothing to launch
    for g in (0, 17, -2):
        rejected(_seq_call(lib, group=g, N=0), b"gvl_sequence_score", b"group=%d" % g)
    rejected(_seq_call(lib, group=3), b"gvl_sequence_score", b"N=8")
    rejected(_seq_call(lib, logp=None), b"gvl_sequence_score", b"null logp")
    for name in ("sum", "count", "mean", "pn", "p"):
        rejected(_seq_call(lib, **{name: None}), b"gvl_sequence_score", b"null output")
    rejected(_seq_call(lib, T=-1), b"gvl_sequence_score", b"T=-1")
    assert _seq_call(lib, N=0) == 0


def test_public_names_are_exported():
    import gvl
    import gvl.score as sc
    from gvl import kernels
    from gvl.dist import all_reduce_sum_
    assert gvl.most_likely_row is sc.most_likely_row
    assert gvl.evaluate_hellaswag is sc.evaluate_hellaswag
    assert callable(sc.score) and callable(kernels.token_logprobs) and callable(kernels.sequence_score)
    t = torch.tensor([1, 2, 3])
    assert all_reduce_sum_(t) is t and t.tolist() == [1, 2, 3]  # no process group: unchanged
    for m in (sc._text_hidden,):
        with pytest.raises(TypeError, match="unsupported model"):
            m(torch.nn.Linear(2, 2), torch.zeros(1, 2, dtype=torch.long), None)
