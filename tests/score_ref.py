"""float64 references (and the same formulas in fp32 torch, the CPU baseline) of the scoring
kernels gvl_token_logprobs and gvl_sequence_score (include/gvl.h), the test inputs, and the
assertions that hold the HIP kernels to them.  Shared by test_score_cpu.py, which proves the
references against independent statements and that the assertions reject doctored outputs, and
test_gpu_score.py.  Every reference reads the same bf16 / fp32 values the kernel reads."""
from __future__ import annotations

import numpy as np
import torch

from tests.helpers import F32_UNIT, assert_f32_close, err_units, f64, ulp_bf16

BF = torch.bfloat16
F32 = torch.float32
SENTINEL = 16384.0  # in the pad columns [V, ld): a kernel that reads one moves lse to ~16384
TOKEN_SHAPES = ((8, 8), (8, 12), (12, 16), (509, 512), (50257, 50304), (65536, 65536))
TOKEN_VARIANTS = ("one", "targets5", "special5")  # rows 1, 5, 5
MARGIN = 4  # what the row-wise tests give a device's exp / log over the host's


# ------------------------------------------------------------------ token_logprobs
def ragged_target(V):
    """A column inside the last 8-column chunk of the row (ragged when V % 8 != 0)."""
    last = (V - 1) // 8 * 8
    return last + ((V - 1) - last) // 2


def token_case(V, ld, f32, variant, seed=0):
    """CPU inputs of one launch: logits [rows, ld] (bf16 or fp32, pad columns = SENTINEL),
    targets int64 [rows], mask uint8 [rows] or None.
      one:      a single row, random target;
      targets5: targets at column 0, at V - 1, in the last 8-column chunk; a row whose maximum
                stands on both sides of the target (and the target's own value on both sides of
                it too); a row whose target logit is -inf;
      special5: an ignored row (-100), a masked row, an out-of-range row (target V: the first pad
                column), two ordinary rows."""
    rows = 1 if variant == "one" else 5
    g = torch.Generator().manual_seed(7000 + 31 * seed + V + 3 * ld + (1 if f32 else 0) + rows)
    x = torch.randn(rows, V, generator=g) * 2.0
    x[:, V // 3] += 3.0
    x = x.to(F32 if f32 else BF)
    tg = torch.randint(0, V, (rows,), generator=g).numpy().astype(np.int64)
    mask = None
    if variant == "targets5":
        tg[0], tg[1], tg[2] = 0, V - 1, ragged_target(V)
        t = V // 2
        lo, hi = max(t - 3, 0), min(t + 2, V - 1)          # the maximum, twice
        lo2, hi2 = max(t - 2, 0), min(t + 1, V - 1)        # the target's value, twice more
        tg[3] = t
        top = (x[3].float().max() + 1.0).to(x.dtype)
        x[3, lo2] = x[3, hi2] = x[3, t]
        x[3, lo] = x[3, hi] = top
        tg[4] = V // 4 + (1 if V // 4 == V // 3 else 0)  # not the boosted column
        x[4, tg[4]] = float("-inf")
    elif variant == "special5":
        tg[0] = -100
        mask = np.ones(rows, dtype=np.uint8)
        mask[1] = 0
        tg[2] = V
    buf = torch.full((rows, ld), SENTINEL, dtype=x.dtype)
    buf[:, :V] = x
    return dict(logits=buf, V=V, targets=tg, mask=mask)


def token_ref64(logits, V, targets, mask=None):
    """float64 reference of gvl_token_logprobs over logits[:, :V].  -> dict(logp, lse, argmax,
    rank, skipped, scale_logp = |x_t| + |max| + |ln s|, scale_lse = |max| + |ln s|); the scales
    are 1 where the reference is not finite (those elements must match exactly)."""
    x = f64(logits)[:, :V]
    t = np.asarray(targets, dtype=np.int64)
    rows = x.shape[0]
    skipped = t == -100
    if mask is not None:
        skipped |= np.asarray(mask) == 0
    inr = (t >= 0) & (t < V)
    mx = x.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.exp(x - mx[:, None]).sum(axis=1)
        lns = np.log(s)
        lse = mx + lns
        xt = np.where(inr, x[np.arange(rows), np.where(inr, t, 0)], np.nan)
        logp = xt - lse
    argmax = x.argmax(axis=1).astype(np.int32)  # numpy: the first maximum, like torch
    above = (x > xt[:, None]).sum(axis=1)
    before = ((x == xt[:, None]) & (np.arange(V)[None, :] < t[:, None])).sum(axis=1)
    rank = np.where(inr, above + before, -1).astype(np.int32)
    logp = np.where(skipped, 0.0, logp)
    lse = np.where(skipped, 0.0, lse)
    argmax = np.where(skipped, -1, argmax).astype(np.int32)
    rank = np.where(skipped, -1, rank).astype(np.int32)
    with np.errstate(invalid="ignore"):
        s_lse = np.abs(mx) + np.abs(lns)
        s_logp = np.abs(xt) + s_lse
    s_lse = np.where(np.isfinite(lse) & ~skipped, s_lse, 1.0)
    s_logp = np.where(np.isfinite(logp) & ~skipped, s_logp, 1.0)
    return dict(logp=logp, lse=lse, argmax=argmax, rank=rank, skipped=skipped,
                scale_logp=s_logp, scale_lse=s_lse)


def token_f32(logits, V, targets):
    """The kernel's formulas in fp32 torch on the CPU (rows with a target in [0, V) only):
    lse = max + log(sum exp(x - max)), logp = x_t - lse."""
    x = logits[:, :V].float()
    mx = x.max(dim=1).values
    s = torch.exp(x - mx[:, None]).sum(dim=1)
    lse = mx + torch.log(s)
    xt = x[torch.arange(x.shape[0]), torch.as_tensor(targets, dtype=torch.int64)]
    return dict(logp=xt - lse, lse=lse)


def _finite_units(got, ref, scale):
    fin = np.isfinite(f64(ref))
    return err_units(f64(got)[fin], f64(ref)[fin], f64(scale)[fin])


_TOKEN_BASE = {}


def token_baseline():
    """Worst error of token_f32 against token_ref64 over every test case (shape, dtype, variant),
    in units of 2**-24 * scale: the CPU baseline the kernel gets MARGIN times of."""
    if not _TOKEN_BASE:
        base = dict(logp=0.0, lse=0.0)
        for V, ld in TOKEN_SHAPES:
            for f32 in (False, True):
                for variant in TOKEN_VARIANTS:
                    c = token_case(V, ld, f32, variant)
                    ref = token_ref64(c["logits"], V, c["targets"], c["mask"])
                    ok = ~ref["skipped"] & (ref["rank"] >= 0)
                    got = token_f32(c["logits"][torch.from_numpy(ok)], V, c["targets"][ok])
                    for k in base:
                        u = _finite_units(got[k], ref[k][ok], ref["scale_" + k][ok])
                        base[k] = max(base[k], u)
        _TOKEN_BASE.update(base)
    return dict(_TOKEN_BASE)


def check_token_outputs(got, ref, slack, name=""):
    """The per-element assertions on gvl_token_logprobs' outputs.  got: dict with any of logp,
    lse, argmax, rank (arrays [rows]); slack: dict(logp, lse) in units of 2**-24 * scale.
    argmax, rank and every output of a skipped row must be exact; a non-finite reference (NaN
    for an out-of-range target, -inf for a banned one) must be matched exactly.  -> the measured
    units of logp and lse over the finite elements."""
    units = {}
    for k in ("argmax", "rank"):
        if k in got:
            g = np.asarray(got[k])
            assert g.dtype == np.int32 and np.array_equal(g, ref[k]), \
                f"{name}: {k} {g.tolist()} != {ref[k].tolist()}"
    for k in ("logp", "lse"):
        if k in got:
            g = f64(got[k])
            sk = ref["skipped"]
            assert np.array_equal(g[sk], ref[k][sk]), f"{name}: {k} of a skipped row was written"
            with np.errstate(invalid="ignore"):  # inf - inf where both are the same infinity
                assert_f32_close(g, ref[k], ref["scale_" + k], slack[k], name=f"{name} {k}")
            units[k] = _finite_units(g, ref[k], ref["scale_" + k])
    return units


# ------------------------------------------------------------------ sequence_score
SEQ_SHAPES = ((1, 1, 1), (4, 7, 4), (6, 63, 3), (16, 1, 16), (3, 1025, 1))


def seq_case(N, T, group, masked=True, seed=0):
    """logp fp32 [N, T] (negative) and mask uint8 [N, T] or None.  Where the shape allows: two
    equal sequences that are the best of their example (a tie: the first must win), and, with a
    mask, one sequence whose mask is all zero (its example predicts -1)."""
    g = torch.Generator().manual_seed(9000 + seed + 17 * N + T + 5 * group)
    logp = -(torch.randn(N, T, generator=g).abs() * 3.0 + 0.01)
    mask = None
    if masked:
        mask = (torch.rand(N, T, generator=g) < 0.6).to(torch.uint8)
        mask[:, 0] = 1  # every sequence counts something unless zeroed below
    if group >= 3:  # sequences 1 and group - 1 of example 0: equal and closest to zero
        a, b = 1, group - 1
        logp[a] *= 0.05
        logp[b] = logp[a]
        if mask is not None:
            mask[b] = mask[a]
    if masked and N >= 3 and N // group != 1:  # an all-zero sequence outside example 0
        mask[N - 1] = 0
    return dict(logp=logp.to(F32), mask=None if mask is None else mask.numpy())


def sequence_ref64(logp, mask, group):
    """float64 reference of gvl_sequence_score.  -> dict(sum, count, mean, pred_norm, pred,
    scale = sum of |terms| per sequence)."""
    lp = f64(logp)
    N, T = lp.shape
    m = np.ones((N, T), dtype=bool) if mask is None else np.asarray(mask) != 0
    terms = np.where(m, -lp, 0.0)
    s = terms.sum(axis=1)
    scale = np.abs(terms).sum(axis=1)
    cnt = m.sum(axis=1).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / cnt
    pn, ps = [], []
    for e in range(N // group):
        sl = slice(e * group, (e + 1) * group)
        if (cnt[sl] == 0).any():
            pn.append(-1)
            ps.append(-1)
        else:
            pn.append(int(np.argmin(mean[sl])))
            ps.append(int(np.argmin(s[sl])))
    return dict(sum=s, count=cnt, mean=mean, pred_norm=np.asarray(pn, dtype=np.int32),
                pred=np.asarray(ps, dtype=np.int32), scale=scale)


def sequence_f32(logp, mask):
    """The same sums in fp32 torch on the CPU."""
    lp = logp.float()
    m = torch.ones_like(lp, dtype=torch.bool) if mask is None else torch.as_tensor(mask) != 0
    s = torch.where(m, -lp, torch.zeros_like(lp)).sum(dim=1)
    return dict(sum=s, mean=s / m.sum(dim=1))


def sequence_bounds(ref, T):
    """The worst-case fp32 error of a T-term sum in any order, T * 2**-24 * sum |terms|, per
    sequence, and of the mean: that over count, plus the division's one rounding."""
    b_sum = T * F32_UNIT * ref["scale"]
    with np.errstate(invalid="ignore", divide="ignore"):
        b_mean = b_sum / ref["count"] + F32_UNIT * np.abs(ref["mean"])
    return b_sum, b_mean


def sequence_decided(ref, T, group):
    """Per example: True when the float64 gaps decide both predictions, i.e. every sequence whose
    value differs from the winner's at all is worse by more than the two error bounds (equal
    sequences are exact ties in fp32 as well and must resolve to the first)."""
    b_sum, b_mean = sequence_bounds(ref, T)
    out = []
    for e in range(len(ref["pred"])):
        sl = slice(e * group, (e + 1) * group)
        ok = True
        if ref["pred"][e] >= 0:
            for v, b, p in ((ref["sum"][sl], b_sum[sl], ref["pred"][e]),
                            (ref["mean"][sl], b_mean[sl], ref["pred_norm"][e])):
                other = v != v[p]
                ok &= bool(np.all(v[other] - v[p] > b[other] + b[p]))
        out.append(ok)
    return np.asarray(out)


def check_sequence_outputs(got, ref, T, group, name=""):
    """got: dict(sum, count, mean, pred_norm, pred) arrays.  count exact; sum within T units of
    2**-24 * sum |terms|; mean within that over count plus one unit of |mean| (NaN where count
    is 0); both predictions exact (the input must be decided, asserted).  -> measured units."""
    assert np.asarray(got["count"]).dtype == np.int32
    assert np.array_equal(got["count"], ref["count"]), f"{name}: count"
    u = assert_f32_close(got["sum"], ref["sum"], ref["scale"], T, name=f"{name} sum_nll")
    b_sum, b_mean = sequence_bounds(ref, T)
    gm, rm = f64(got["mean"]), ref["mean"]
    empty = ref["count"] == 0
    assert np.isnan(gm[empty]).all(), f"{name}: mean of an empty sequence must be NaN"
    assert np.all(np.abs(gm[~empty] - rm[~empty]) <= b_mean[~empty]), f"{name}: mean_nll"
    assert sequence_decided(ref, T, group).all(), \
        f"{name}: invalid input, the reference's own ranking is too close to call"
    for k in ("pred_norm", "pred"):
        assert np.asarray(got[k]).dtype == np.int32
        assert np.array_equal(got[k], ref[k]), f"{name}: {k} {got[k]} != {ref[k]}"
    return u


# ------------------------------------------------------------------ model level
MODEL_KINDS = ("gpt", "linear", "qformer", "cross")
MODEL_N, MODEL_T, MODEL_GROUP = 8, 24, 4
# Of seeds 1..39 the one whose smallest gap (best ending to runner-up, over all kinds and examples,
# by the fp32 CPU oracle) is widest against twice the GEMM-route bound: 4.6 times it.
# test_score_cpu.py asserts that the oracle decides every example at it.
MODEL_SEED = 38
Z_SEED = 3


def model_inputs(V, seed=MODEL_SEED):
    """tokens int64 [8, 24] and a HellaSwag-shaped mask [8, 24]: zeros over a context of 6..8
    tokens, ones over an ending of 5..14, zeros over the padding behind it."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, V, (MODEL_N, MODEL_T), generator=g)
    mask = torch.zeros(MODEL_N, MODEL_T, dtype=torch.int64)
    for n in range(MODEL_N):
        ctx = 6 + n % 3
        mask[n, ctx:ctx + 5 + 3 * (n % 4)] = 1
    return tokens, mask


def oracle_text_logits(kind, P, tokens, z, cfg):
    """The fp32 CPU oracle's logits over the text positions [N, T, V] (oracle/models.py)."""
    from oracle import models as OM
    L, H = cfg["n_layer"], cfg["n_head"]
    if kind == "gpt":
        return OM.gpt_forward(P, tokens, L, H)[0]
    if kind == "cross":
        return OM.cross_att_forward(P, tokens, z, L, H)[0]
    return OM.caption_forward(P, kind, z, tokens, L, H, cfg["block_size"])[0][:, -tokens.shape[1]:]


def model_reference(logits, tokens, mask, group=MODEL_GROUP):
    """From text logits [N, T, V] (bf16 or fp32 values): the float64 per-token reference of the
    shifted rows, the sequence reference, the per-token bound of logp_route_bound, per sequence
    its mean over the masked tokens, and per example whether the gap from the best mean_nll to
    the runner-up exceeds twice the largest such bound of the example."""
    N, T, V = logits.shape
    tg = np.asarray(tokens)[:, 1:].reshape(-1)
    sm = np.asarray(mask)[:, 1:] != 0
    rows = logits[:, :-1].reshape(N * (T - 1), V)
    tok = token_ref64(rows, V, tg)
    seq = sequence_ref64(tok["logp"].reshape(N, T - 1), sm, group)
    bound = logp_route_bound(rows, V, tg).reshape(N, T - 1)
    seq_bound = np.where(sm, bound, 0.0).sum(axis=1) / sm.sum(axis=1)
    decided = []
    for e in range(N // group):
        sl = slice(e * group, (e + 1) * group)
        m = np.sort(seq["mean"][sl])
        decided.append(bool(m[1] - m[0] > 2 * seq_bound[sl].max()))
    return dict(tok=tok, seq=seq, bound=bound, seq_bound=seq_bound, decided=np.asarray(decided),
                smask=sm)


def logp_route_bound(logits, V, targets):
    """Per row: ulp_bf16(x_t) + max_v ulp_bf16(x_v), what two GEMM routes that round an fp32
    accumulation to neighbouring bf16 values may move logp by (each logit by at most one bf16
    ulp, lse by at most the largest such move)."""
    x = f64(logits)[:, :V]
    t = np.asarray(targets, dtype=np.int64)
    xt = x[np.arange(x.shape[0]), t]
    return ulp_bf16(xt) + ulp_bf16(x).max(axis=1)
