"""Scoring of given token sequences on the MI355X (gvl_token_logprobs, gvl_sequence_score,
gvl.score), held to tests/score_ref.py:

  1. the token kernel per element: argmax, rank and skipped rows exact, logp and lse within 4 x
     the fp32 CPU baseline's measured error (in units of 2**-24 * (|x_t| + |max| + |ln s|)), on
     bf16 and fp32 logits whose pad columns hold a sentinel; every single-output call; guards;
  2. the sequence kernel: counts exact, sums within the worst-case fp32 summation bound,
     predictions exact on decided inputs, ties to the first;
  3. gvl.score on the tiny models of every kind against the references applied to the model's
     own logits, masked against all, against get_most_likely_row, the rows the lm_head sees,
     evaluate_hellaswag, and forward / generate / get_most_likely_row unchanged by it.

Measured units go to profiles/score_margins.json through helpers.margins_out."""
import functools

import numpy as np
import pytest
import torch

from tests import score_ref as S
from tests.helpers import TINY, margins_out
from tests.test_gpu_beam import _tiny
from tests.test_gpu_parity_full import _z

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
GUARD = 4
FILL = {torch.float32: 77.5, torch.int32: 12345}
OUT_DTYPES = dict(logp=F32, lse=F32, argmax=torch.int32, rank=torch.int32)

_MARGINS = {}


def _record(key, rec):
    _MARGINS[key] = rec
    margins_out("score_margins", _MARGINS)


def _slack():
    return {k: S.MARGIN * v for k, v in S.token_baseline().items()}


def _guarded(rows, dtype, cuda):
    """(buffer of rows + 2 * GUARD elements filled with a sentinel, its middle rows)."""
    buf = torch.full((rows + 2 * GUARD,), FILL[dtype], dtype=dtype, device=cuda)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    fill = FILL[buf.dtype]
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + rows:] == fill).all())


def _bits(t):
    return t.view(torch.int32) if t.dtype == F32 else t


# ------------------------------------------------------------------ 1. the token kernel
@functools.lru_cache(maxsize=None)
def _token_case(V, ld, f32, variant):
    c = S.token_case(V, ld, f32, variant)
    return c, S.token_ref64(c["logits"], V, c["targets"], c["mask"])


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("variant", S.TOKEN_VARIANTS)
@pytest.mark.parametrize("V,ld", S.TOKEN_SHAPES)
def test_token_logprobs_per_element(cuda, V, ld, variant, f32):
    import gvl.kernels as K
    c, ref = _token_case(V, ld, f32, variant)
    rows = c["logits"].shape[0]
    logits = c["logits"].to(cuda)[:, :V]  # row stride ld, the pad columns behind the view
    assert logits.stride(0) == ld
    targets = torch.from_numpy(c["targets"]).to(cuda)
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(cuda)
    bufs = {k: _guarded(rows, dt, cuda) for k, dt in OUT_DTYPES.items()}
    K.token_logprobs(logits, targets, mask, **{k: v[1] for k, v in bufs.items()})
    torch.cuda.synchronize()
    got = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    name = f"V{V}-ld{ld}-{'fp32' if f32 else 'bf16'}-{variant}"
    slack = _slack()
    print(f"{name}: logp {got['logp'].tolist()} rank {got['rank'].tolist()} "
          f"argmax {got['argmax'].tolist()}")
    units = S.check_token_outputs(got, ref, slack, name)
    print(f"{name}: measured units logp {units['logp']:.3f} lse {units['lse']:.3f} "
          f"(allowed {slack['logp']:.3f} / {slack['lse']:.3f})")
    _record(f"token_logprobs:{name}", dict(kernel_units=units, cpu_baseline_units=S.token_baseline(),
                                           allowed_units=slack))
    for k, (buf, _) in bufs.items():
        assert _guards_intact(buf, rows), f"{name}: {k} written outside its {rows} rows"
    # every call with a single non-null output gives that output's bits again
    for k, dt in OUT_DTYPES.items():
        buf, view = _guarded(rows, dt, cuda)
        out = K.token_logprobs(logits, targets, mask,
                               **{j: (view if j == k else None) for j in OUT_DTYPES})
        assert [o is not None for o in out] == [j == k for j in OUT_DTYPES]
        assert torch.equal(_bits(view), _bits(bufs[k][1])), f"{name}: {k} alone differs"
        assert _guards_intact(buf, rows), f"{name}: {k} alone wrote outside its rows"


def test_token_logprobs_vocab_argument_and_allocation(cuda):
    """`vocab` marks trailing columns of a contiguous [rows, ld] tensor as padding, and outputs
    left at True are allocated: the same bits as the strided view."""
    import gvl.kernels as K
    c, ref = _token_case(509, 512, False, "targets5")
    full = c["logits"].to(cuda)
    tg = torch.from_numpy(c["targets"]).to(cuda)
    a = K.token_logprobs(full, tg, vocab=509)
    b = K.token_logprobs(full[:, :509], tg)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))
    S.check_token_outputs(dict(zip(("logp", "lse", "argmax", "rank"), (t.cpu().numpy() for t in a))),
                          ref, _slack(), "vocab=")
    with pytest.raises(ValueError, match="vocab"):
        K.token_logprobs(full, tg, vocab=513)


# ------------------------------------------------------------------ 2. the sequence kernel
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N,T,group", S.SEQ_SHAPES)
def test_sequence_score(cuda, N, T, group, masked):
    import gvl.kernels as K
    c = S.seq_case(N, T, group, masked)
    ref = S.sequence_ref64(c["logp"], c["mask"], group)
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(cuda)
    out = K.sequence_score(c["logp"].to(cuda), mask, group)
    torch.cuda.synchronize()
    got = dict(zip(("sum", "count", "mean", "pred_norm", "pred"), (t.cpu().numpy() for t in out)))
    name = f"N{N}-T{T}-g{group}-{'mask' if masked else 'nomask'}"
    print(f"{name}: sum {got['sum'].tolist()} count {got['count'].tolist()} "
          f"pred_norm {got['pred_norm'].tolist()} pred {got['pred'].tolist()}")
    u = S.check_sequence_outputs(got, ref, T, group, name)
    print(f"{name}: sum_nll measured {u:.3f} units of 2**-24 * sum|terms| (allowed {T})")
    _record(f"sequence_score:{name}", dict(kernel_units=u, allowed_units=T))
    if group >= 3:
        assert got["pred_norm"][0] == 1, "the tie between sequences 1 and group - 1: the first"


# ------------------------------------------------------------------ 3. model level
def _forward_text_logits(kind, model, tokens, z):
    """The text positions' logits [N, T, V] of the model's own forward."""
    with torch.no_grad():
        if kind == "gpt":
            return model(tokens)[0]
        if kind == "cross":
            return model(tokens, z=z)[0]
        return model(z, tokens)[0][:, -tokens.shape[1]:]


@functools.lru_cache(maxsize=None)
def _model_run(kind):
    """Model, inputs, the forward's logits, score(select='all') in one chunk, score(select=
    'masked') in chunks of 16 rows, and the references on those logits: computed once per kind."""
    import gvl.score as sc
    cuda = torch.device("cuda:0")
    model = _tiny(kind)
    tokens, mask = S.model_inputs(TINY["vocab_size"])
    tokens, mask = tokens.to(cuda), mask.to(cuda)
    z = None if kind == "gpt" else _z(S.Z_SEED, S.MODEL_N, TINY["n_embd"], cuda)
    logits = _forward_text_logits(kind, model, tokens, z)
    kw = dict(z=z, group=S.MODEL_GROUP, return_tokens=True)
    s_all = sc.score(model, tokens, mask, select="all", **kw)
    s_masked = sc.score(model, tokens, mask, select="masked", chunk_rows=16, **kw)
    torch.cuda.synchronize()
    ref = S.model_reference(logits.cpu(), tokens.cpu().numpy(), mask.cpu().numpy())
    return dict(model=model, tokens=tokens, mask=mask, z=z, logits=logits, all=s_all,
                masked=s_masked, ref=ref)


@pytest.mark.parametrize("kind", S.MODEL_KINDS)
def test_score_all_matches_reference_on_the_models_logits(cuda, kind):
    """(a) one chunk: the lm_head GEMM of score() is the one behind model(...)[0], so per token
    the kernel tolerance of test 1 holds against the reference applied to those logits."""
    r = _model_run(kind)
    s, tok = r["all"], r["ref"]["tok"]
    got = dict(logp=s.logp.reshape(-1).cpu().numpy(), rank=s.rank.reshape(-1).cpu().numpy(),
               argmax=s.argmax.reshape(-1).cpu().numpy())
    slack = _slack()
    units = S.check_token_outputs(got, tok, slack, f"{kind} all")
    print(f"{kind}: select='all' logp measured {units['logp']:.3f} units (allowed {slack['logp']:.3f})")
    _record(f"score_all:{kind}", dict(kernel_units=units, allowed_units=slack))
    seq = r["ref"]["seq"]
    S.check_sequence_outputs(dict(sum=s.sum_nll.cpu().numpy(), count=s.count.cpu().numpy(),
                                  mean=s.mean_nll.cpu().numpy(),
                                  pred_norm=s.pred_norm.cpu().numpy(), pred=s.pred.cpu().numpy()),
                             S.sequence_ref64(s.logp.cpu(), r["ref"]["smask"], S.MODEL_GROUP),
                             S.MODEL_T - 1, S.MODEL_GROUP, f"{kind} all sequence")
    assert np.array_equal(s.count.cpu().numpy(), seq["count"])


@pytest.mark.parametrize("kind", S.MODEL_KINDS)
def test_score_masked_in_chunks_matches_all(cuda, kind):
    """(b) several chunks and a ragged last one: per token within ulp_bf16(x_t) + max_v
    ulp_bf16(x_v) of select='all', mean_nll within the mean of those bounds; positions that were
    not scored hold 0, -1, -1."""
    r = _model_run(kind)
    a, m, ref = r["all"], r["masked"], r["ref"]
    sm = ref["smask"]
    assert int(sm.sum()) > 16 and int(sm.sum()) % 16 != 0  # chunks: several, the last ragged
    d = np.abs(m.logp.cpu().numpy().astype(np.float64) - a.logp.cpu().numpy().astype(np.float64))
    print(f"{kind}: masked vs all: max |dlogp| {d[sm].max():.3e} (smallest bound "
          f"{ref['bound'][sm].min():.3e}); identical bits: {bool((d[sm] == 0).all())}")
    assert (d[sm] <= ref["bound"][sm]).all()
    assert (m.logp.cpu().numpy()[~sm] == 0).all()
    for k in ("rank", "argmax"):
        g = getattr(m, k).cpu().numpy()
        assert (g[~sm] == -1).all() and (g[sm] >= 0).all()
    dm = np.abs(m.mean_nll.cpu().numpy().astype(np.float64) - a.mean_nll.cpu().numpy())
    assert (dm <= ref["seq_bound"]).all(), (dm, ref["seq_bound"])
    assert torch.equal(m.count, a.count)


@pytest.mark.parametrize("kind", S.MODEL_KINDS)
def test_pred_norm_matches_get_most_likely_row(cuda, kind):
    """(c) on every example whose reference gap exceeds twice the (b) bound."""
    from gvl.data import get_most_likely_row
    r = _model_run(kind)
    G, decided = S.MODEL_GROUP, r["ref"]["decided"]
    n = 0
    for e in range(S.MODEL_N // G):
        sl = slice(e * G, (e + 1) * G)
        want = get_most_likely_row(r["tokens"][sl], r["mask"][sl], r["logits"][sl])
        if decided[e]:
            n += 1
            for s in (r["all"], r["masked"]):
                assert int(s.pred_norm[e]) == want == int(r["ref"]["seq"]["pred_norm"][e])
    print(f"{kind}: {n} of {len(decided)} examples compared")
    assert len(decided) - n <= len(decided) // 8


@pytest.mark.parametrize("kind", S.MODEL_KINDS)
def test_lm_head_sees_only_scored_rows(cuda, kind, monkeypatch):
    """(d) with chunk_rows=16 no lm_head GEMM has more than 16 rows, together they have exactly
    the scored rows, and none of a caption model's image rows reaches one."""
    import gvl.kernels as K
    import gvl.score as sc
    r = _model_run(kind)
    real, seen = K.linear, []
    head = (r["model"].gpt if kind in ("linear", "qformer") else r["model"]).lm_head.weight
    assert head.dtype == BF and head.shape[0] % 8 == 0  # used as it is: no cast, no padding

    def spy(x2, w, *a, **kw):
        if w.data_ptr() == head.data_ptr():
            seen.append(x2.clone())
        return real(x2, w, *a, **kw)

    monkeypatch.setattr(K, "linear", spy)
    sc.score(r["model"], r["tokens"], r["mask"], z=r["z"], group=S.MODEL_GROUP, chunk_rows=16)
    n_scored = int(r["ref"]["smask"].sum())
    assert seen and max(x.shape[0] for x in seen) <= 16
    assert sum(x.shape[0] for x in seen) == n_scored
    # the rows are the text rows with a nonzero shifted mask, in order: none of the image rows
    model, tokens, z = r["model"], r["tokens"], r["z"]
    with torch.no_grad():
        if kind in ("linear", "qformer"):
            x, M, T = model.hidden(z, tokens)
            assert M >= 32
            x = x[:, M:M + T]
        else:
            x = model.hidden(tokens) if kind == "gpt" else model.hidden(tokens, z)
    want = x[:, :-1][torch.from_numpy(r["ref"]["smask"]).to(cuda)]
    assert torch.equal(torch.cat(seen, 0), want)


@pytest.mark.parametrize("select", ["masked", "all"])
def test_caption_text_is_cut_at_block_size_as_in_forward(cuda, select):
    """33 bridge tokens + 40 text tokens > block_size 64: forward keeps 31 text tokens, and so
    does score (the mask with them)."""
    import gvl.score as sc
    model = _model_run("linear")["model"]
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, TINY["vocab_size"], (4, 40), generator=g).to(cuda)
    mask = (torch.rand(4, 40, generator=g) < 0.5).to(cuda)
    mask[:, 35] = True  # scored only if the cut were missed
    z = _z(S.Z_SEED, 4, TINY["n_embd"], cuda)
    kw = dict(z=z, group=2, select=select, return_tokens=True)
    long, cut = sc.score(model, tokens, mask, **kw), sc.score(model, tokens[:, :31], mask[:, :31], **kw)
    assert tuple(long.logp.shape) == (4, 30)
    for k in ("sum_nll", "count", "mean_nll", "pred_norm", "pred", "logp", "rank", "argmax"):
        assert torch.equal(getattr(long, k), getattr(cut, k)), k
    assert int(long.count.sum()) == int(mask[:, 1:31].sum())


def test_evaluate_hellaswag_counts(cuda):
    """(e) 8 synthetic examples (the 2 of the model inputs and 6 more from other seeds, with
    labels that make some right and some wrong) against the count made by hand."""
    import gvl.score as sc
    r = _model_run("gpt")
    model, G = r["model"], S.MODEL_GROUP
    examples, want_norm, want_sum = [], 0, 0
    for i in range(4):
        tokens, mask = S.model_inputs(TINY["vocab_size"], seed=S.MODEL_SEED + i)
        s = sc.score(model, tokens.to(cuda), mask.to(cuda), group=G)
        for e in range(2):
            pn, ps = int(s.pred_norm[e]), int(s.pred[e])
            label = pn if (2 * i + e) % 3 else (pn + 1) % G
            examples.append((tokens[e * G:(e + 1) * G], mask[e * G:(e + 1) * G], label))
            want_norm += int(pn == label)
            want_sum += int(ps == label)
    assert int(r["all"].pred_norm[0]) == int(sc.score(model, *[t.to(cuda) for t in examples[0][:2]],
                                                      group=G).pred_norm[0])
    got = sc.evaluate_hellaswag(model, iter(examples))
    print(f"evaluate_hellaswag: {got}, by hand {(want_norm, want_sum, 8)}")
    assert got == (want_norm, want_sum, 8) and 0 < want_norm < 8
    assert sc.most_likely_row(model, examples[0][0].to(cuda), examples[0][1].to(cuda)) == \
        int(r["all"].pred_norm[0])


@pytest.mark.parametrize("kind", S.MODEL_KINDS)
def test_existing_paths_keep_their_bits(cuda, kind):
    """(f) forward, generate(greedy=True) and get_most_likely_row before and after calling
    gvl.score (which also leaves the model's training mode as it found it)."""
    import gvl.score as sc
    from gvl.data import get_most_likely_row
    from gvl.decode import generate
    r = _model_run(kind)
    model, tokens, mask, z = r["model"], r["tokens"], r["mask"], r["z"]

    def run():
        logits = _forward_text_logits(kind, model, tokens, z)
        if kind == "gpt":
            gen = generate(model, tokens[:2, :5], 6, greedy=True)
        else:
            gen = generate(model, tokens[:2, :5], 6, z=z[:2], greedy=True)
        return logits, gen, get_most_likely_row(tokens[:4], mask[:4], logits[:4])

    before = run()
    model.train()
    s = sc.score(model, tokens, mask, z=z, group=S.MODEL_GROUP, chunk_rows=16)
    assert model.training
    model.eval()
    sc.score(model, tokens, mask, z=z, group=S.MODEL_GROUP, select="all")
    assert not model.training
    after = run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[0], r["logits"])
    assert torch.equal(before[1], after[1]) and before[2] == after[2]
    assert torch.equal(s.pred_norm, r["masked"].pred_norm)
