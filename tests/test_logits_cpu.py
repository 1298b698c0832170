"""Logits processors without a GPU: tests/logits_ref.py against an independent restatement
written the way Hugging Face writes its processors, and the host-side argument validation of
gvl_logits_process (include/gvl.h)."""
import numpy as np
import pytest
import torch

from tests.logits_ref import logits_ref


# ------------------------------------------------------------------ the independent restatement
def hf_process(scores, seq, *, repetition_penalty=1.0, no_repeat_ngram_size=0, eos=None,
               ban_eos=False, bad_tokens=None):
    """One row.  scores: float32 [V] torch tensor; seq: the row's ids (prompt + generated).
    -> the processed float32 row: RepetitionPenaltyLogitsProcessor (gather / where / scatter),
    NoRepeatNGramLogitsProcessor (a dict from each generated (n-1)-gram to the tokens that
    followed it), MinLength and NoBadWords by plain indexing."""
    V = scores.shape[0]
    scores = scores.clone().view(1, V)
    if repetition_penalty != 1.0:
        ids = torch.tensor([[v for v in seq if 0 <= v < V]], dtype=torch.int64)
        score = torch.gather(scores, 1, ids)
        pen = torch.full_like(score, repetition_penalty)  # fp32 tensor: a true fp32 division
        score = torch.where(score < 0, score * pen, score / pen)
        scores = scores.scatter(1, ids, score)
    n = no_repeat_ngram_size
    if n > 0 and len(seq) + 1 >= n:
        grams = {}
        for gram in zip(*[seq[i:] for i in range(n)]):
            grams.setdefault(tuple(gram[:-1]), []).append(gram[-1])
        start = len(seq) + 1 - n
        for v in grams.get(tuple(seq[start:]), []):
            if 0 <= v < V:
                scores[0, v] = -float("inf")
    if ban_eos and eos is not None and 0 <= eos < V:
        scores[0, eos] = -float("inf")
    for v in ([] if bad_tokens is None else bad_tokens):
        if 0 <= int(v) < V:
            scores[0, int(v)] = -float("inf")
    return scores.view(V)


def hf_process_rows(logits, seqs, **kw):
    """hf_process on every row of logits [R, V] (any float dtype): computed in fp32, rounded
    back to the logits dtype."""
    rows = [hf_process(logits[r].float().cpu(), seqs[r], **kw) for r in range(logits.shape[0])]
    return torch.stack(rows).to(logits.dtype)


# ------------------------------------------------------------------ reference == restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_prompt", [False, True])
def test_reference_matches_independent_restatement(dtype, with_prompt):
    rng = np.random.default_rng(3 + with_prompt)
    V, R, checked = 11, 3, 0
    for n_hist in range(13):
        for n in (1, 2, 3, 4):
            for p in (0.5, 1.3):
                logits = torch.from_numpy(rng.standard_normal((R, V)).astype(np.float32) * 3)
                logits = logits.to(dtype)
                hist = rng.integers(0, 4, (max(n_hist, 1), R))
                prompt = rng.integers(0, 4, (R, 3)) if with_prompt else None
                bad = [9, 2] if n_hist % 3 == 0 else None
                kw = dict(repetition_penalty=p, no_repeat_ngram_size=n, eos=10,
                          ban_eos=bool(n_hist % 2), bad_tokens=bad)
                got = logits_ref(logits, hist, n_hist, prompt=prompt, **kw)
                seqs = [([] if prompt is None else prompt[r].tolist()) + hist[:n_hist, r].tolist()
                        for r in range(R)]
                want = hf_process_rows(logits, seqs, **kw)
                assert got.dtype == dtype
                assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), \
                    (n_hist, n, p)
                checked += int((got != logits).any())
    assert checked > 90  # the controls really acted


def test_reference_src_flen_and_out_of_range_ids():
    """What the restatement above has no notion of: the beam table, finished rows, ids outside
    the vocabulary, the pad."""
    V, ld, R = 8, 12, 4
    logits = torch.arange(R * ld, dtype=torch.float32).view(R, ld) - 20.0
    hist = np.array([[1, 2, 3, 4], [5, -1, 8, 2], [1, 2, 3, 4]])  # step-major
    src = np.array([[0, 9, 1, 2, 0], [0, 9, 0, -2, 1], [0, 9, 2, 1 + 5, 2], [0, 9, 3, 3, 3]])
    flen = np.array([0, 0, 3, 0])
    got = logits_ref(logits, hist, 3, src=src, t0=2, no_repeat_ngram_size=1, flen=flen, V=V,
                     bad_tokens=[-1, V, 0])
    # row 0: hist[0,1], hist[1,2], hist[2,0] = 2, 8, 1; row 1: hist[0,0], hist[1,0], hist[2,1]
    # = 1, 5, 2; row 2 finished; row 3: 4, hist[1,3] = 2, 4
    want = logits.clone()
    for r, toks in ((0, (2, 1, 0)), (1, (1, 5, 2, 0)), (3, (4, 2, 0))):
        for v in toks:
            want[r, v] = -float("inf")
    assert torch.equal(got, want)


# ------------------------------------------------------------------ host validation
def _call(lib, **over):
    """gvl_logits_process with valid host-only arguments (fake non-null device pointers, never
    dereferenced: validation fails, or every control is off) and `over` on top."""
    a = dict(logits=16, ld=16, f32=0, R=4, V=16, hist=16, hist_ld=4, n_hist=2, src=None, src_ld=0,
             t0=0, prompt=16, prompt_ld=3, P=3, rpi=2, pen=1.0, ngram=0, eos=-1, ban_eos=0,
             bad=None, n_bad=0, flen=None)
    a.update(over)
    return lib.gvl_logits_process(a["logits"], a["ld"], a["f32"], a["R"], a["V"], a["hist"],
                                  a["hist_ld"], a["n_hist"], a["src"], a["src_ld"], a["t0"],
                                  a["prompt"], a["prompt_ld"], a["P"], a["rpi"], a["pen"],
                                  a["ngram"], a["eos"], a["ban_eos"], a["bad"], a["n_bad"],
                                  a["flen"], None)


REJECTED = [
    (dict(V=0), b"V="), (dict(V=65537, ld=65537), b"V="),
    (dict(ld=15), b"ld="),
    (dict(P=4000, n_hist=97, prompt_ld=4000), b"L ="),
    (dict(ngram=-1), b"ngram="), (dict(ngram=17), b"ngram="),
    (dict(pen=0.0), b"rep_penalty"), (dict(pen=-1.5), b"rep_penalty"),
    (dict(pen=float("nan")), b"rep_penalty"), (dict(pen=float("inf")), b"rep_penalty"),
    (dict(rpi=0), b"rows_per_item"), (dict(rpi=3), b"rows_per_item"),
    (dict(hist_ld=3), b"hist_ld="),
    (dict(src=16, src_ld=6, t0=5), b"src_ld="),
    (dict(n_hist=-1), b"n_hist="), (dict(P=-1), b"P="), (dict(n_bad=-1), b"n_bad="),
    (dict(logits=None), b"null logits"), (dict(hist=None), b"null hist"),
    (dict(prompt=None), b"null prompt"), (dict(bad=None, n_bad=2), b"null bad"),
]


@pytest.mark.parametrize("over,word", REJECTED, ids=[",".join(f"{k}={v}" for k, v in o.items())
                                                     for o, _ in REJECTED])
def test_rejects_bad_arguments_without_gpu(over, word):
    from gvl import _lib
    lib = _lib.load()
    # the controls are on, so a call that passed validation would launch: it must not pass
    rc = _call(lib, **{"ngram": 2, **over})
    err = lib.gvl_last_error()
    assert rc == -1 and err.startswith(b"gvl_logits_process") and word in err, err


def test_all_controls_off_is_a_no_op_without_gpu():
    from gvl import _lib
    lib = _lib.load()
    assert _call(lib) == 0                      # p == 1, ngram == 0, no bans: no launch
    assert _call(lib, R=0, rpi=1, ngram=3, pen=1.3, ban_eos=1) == 0  # no rows: no launch
