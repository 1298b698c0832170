"""Prompts of different lengths in one batch, the parts that need no GPU: the length check of
gvl.decode.check_prompt_lens, the left-padded prompt the logits processors are given
(ragged_prompt_for_controls) through tests/logits_ref.py against each row's unpadded prompt run
alone, and the host-side argument validation of gvl_attn_decode_ragged / gvl_embedding_fwd_pos."""
import numpy as np
import pytest
import torch

from tests.logits_ref import logits_ref


# ------------------------------------------------------------------ check_prompt_lens
def _prompt(B=3, P=8):
    return torch.zeros(B, P, dtype=torch.int64)


@pytest.mark.parametrize("make", [list, torch.tensor, lambda v: torch.tensor(v, dtype=torch.int32),
                                  lambda v: np.array(v)], ids=["list", "int64", "int32", "numpy"])
def test_check_prompt_lens_accepts(make):
    from gvl.decode import check_prompt_lens
    got = check_prompt_lens(_prompt(), make([1, 5, 8]), 6, 64)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == [1, 5, 8]


def test_check_prompt_lens_block_size_edge():
    from gvl.decode import check_prompt_lens
    # max(len) + n_new - 1 == block_size is the last that fits
    assert check_prompt_lens(_prompt(), [1, 5, 8], 6, 13).tolist() == [1, 5, 8]
    with pytest.raises(ValueError, match="block_size"):
        check_prompt_lens(_prompt(), [1, 5, 8], 6, 12)
    with pytest.raises(ValueError, match="block_size"):
        check_prompt_lens(_prompt(), [1, 5, 8], 7, 13)


@pytest.mark.parametrize("lens,word", [
    ([1, 5], "entries"), ([1, 5, 8, 8], "entries"), ([[1, 5, 8], [1, 5, 8]], "entries"),
    ([1.0, 5.0, 8.0], "integers"), (torch.tensor([1.0, 5.0, 8.0]), "integers"),
    (torch.tensor([True, True, True]), "integers"),
    ([0, 5, 8], "1..P"), ([-1, 5, 8], "1..P"), ([1, 5, 9], "1..P")])
def test_check_prompt_lens_rejects(lens, word):
    from gvl.decode import check_prompt_lens
    with pytest.raises(ValueError, match=word):
        check_prompt_lens(_prompt(), lens, 6, 64)


# ------------------------------------------------------------------ ragged_prompt_for_controls
def test_ragged_prompt_layout():
    from gvl.decode import ragged_prompt_for_controls
    prompt = torch.arange(1, 13).view(3, 4)
    got = ragged_prompt_for_controls(prompt, torch.tensor([1, 3, 4]))
    assert got.dtype == torch.int64 and got.is_contiguous()
    assert got.tolist() == [[-1, -1, -1, 1], [-1, 5, 6, 7], [9, 10, 11, 12]]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("n_hist", [0, 4])
def test_ragged_prompt_through_logits_ref_equals_row_alone(dtype, n, n_hist):
    """Every row of the padded batch, processed with the left-padded prompt, has the bits of the
    same row processed alone with its unpadded prompt.  Ids from a vocabulary of 4 (logits of 11
    columns) so that n-grams repeat; lengths include 1 and P; the pad ids are random valid ones
    and a second run with other pads must not change a bit."""
    from gvl.decode import ragged_prompt_for_controls
    rng = np.random.default_rng(17 * n + n_hist)
    V, P = 11, 6
    lens = [1, 2, 3, 5, 6, 1, 6, 4]
    R = len(lens)
    acted = 0
    for trial in range(8):
        logits = torch.from_numpy(rng.standard_normal((R, V)).astype(np.float32) * 3).to(dtype)
        prompt = torch.from_numpy(rng.integers(0, 4, (R, P)))
        hist = rng.integers(0, 4, (max(n_hist, 1), R))
        kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=n)
        got = logits_ref(logits, hist, n_hist,
                         prompt=ragged_prompt_for_controls(prompt, torch.tensor(lens)), **kw)
        other = prompt.clone()
        for r, L in enumerate(lens):
            other[r, L:] = torch.from_numpy(rng.integers(0, V, P - L))
        again = logits_ref(logits, hist, n_hist,
                           prompt=ragged_prompt_for_controls(other, torch.tensor(lens)), **kw)
        bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert torch.equal(got.view(bits), again.view(bits))
        for r, L in enumerate(lens):
            alone = logits_ref(logits[r:r + 1], hist[:, r:r + 1], n_hist,
                               prompt=prompt[r:r + 1, :L], **kw)
            assert torch.equal(got[r:r + 1].view(bits), alone.view(bits)), (trial, r, L)
        assert (got != logits).any()  # the penalty acted
        acted += int(torch.isinf(got).any())
    assert acted > 0  # and so did the n-gram rule


# ------------------------------------------------------------------ host validation
def _lib():
    from gvl import _lib
    return _lib.load()


def test_attn_decode_ragged_rejects_bad_arguments_without_gpu():
    lib = _lib()

    def call(Tk=8, src=None, src_ld=0, gap_lo=0x6000, gap_hi=4, q=0x1000):
        return lib.gvl_attn_decode_ragged(q, 128, 0x2000, 4096, 384, 0x3000, 4096, 384, 0x5000,
                                          128, 2, 2, Tk, 0.125, src, src_ld, gap_lo, gap_hi, None)

    assert call(gap_lo=None) == -1 and b"gap_lo" in lib.gvl_last_error()
    assert call(gap_hi=-1) == -1 and b"gap_hi=-1" in lib.gvl_last_error()
    assert call(gap_hi=9) == -1 and b"gap_hi=9" in lib.gvl_last_error()
    assert call(Tk=4097, gap_hi=0) == -1 and b"Tk=4097" in lib.gvl_last_error()
    assert call(Tk=0, gap_hi=0) == -1 and b"Tk=0" in lib.gvl_last_error()
    assert call(src=0x4000, src_ld=4) == -1 and b"src_ld=4" in lib.gvl_last_error()
    assert call(q=None) == -1 and b"null buffer" in lib.gvl_last_error()


def test_embedding_fwd_pos_rejects_bad_arguments_without_gpu():
    lib = _lib()

    def call(C=128, vocab=512, n_pos=64, n=3, pos=0x2000):
        return lib.gvl_embedding_fwd_pos(0x1000, pos, 0x3000, 0x4000, 0x5000, n, C, vocab, n_pos,
                                         None)

    assert call(C=12) == -1 and b"C=12" in lib.gvl_last_error()
    assert call(n_pos=0) == -1 and b"n_pos" in lib.gvl_last_error()
    assert call(n=-1) == -1 and b"n_tokens=-1" in lib.gvl_last_error()
    assert call(pos=None) == -1 and b"null buffer" in lib.gvl_last_error()
    assert call(n=0, pos=None) == 0  # nothing to do: nothing is checked or launched


def test_binding_has_ragged_entry_points_at_abi_14():
    from gvl import _lib
    assert {"gvl_attn_decode_ragged", "gvl_embedding_fwd_pos"} <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 14 and _lib.load().gvl_abi_version() == 14
