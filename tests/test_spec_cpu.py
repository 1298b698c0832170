"""The speculative-decoding references themselves (tests/spec_ref.py) on cases worked out by
hand, and the host-side argument checks of the three entry points (no GPU needed)."""
import ctypes
import math

import pytest

from tests import spec_ref as R


def test_ngram_draft_longest_suffix_wins_and_takes_the_latest_match():
    #    0  1  2  3  4  5  6  7  8
    s = [1, 2, 3, 9, 1, 2, 3, 7, 2, 3]
    # suffix (2, 3): matches at i = 1 and i = 5; the latest is 5 -> continuation s[7:] = 7, 2, 3
    assert R.ngram_draft(s[:4], s[4:], 2, 4, 99) == [7, 2, 3, -1]
    # ngram 3: suffix (7, 2, 3) has no earlier match, falls back to g = 2
    assert R.ngram_draft(s[:4], s[4:], 3, 4, 99) == [7, 2, 3, -1]
    # the split between prompt and emitted tokens does not matter
    assert R.ngram_draft(s[:9], s[9:], 2, 4, 99) == R.ngram_draft(s[:1], s[1:], 2, 4, 99)


def test_ngram_draft_match_only_at_g1_none_and_run_into_the_end():
    assert R.ngram_draft([5, 6, 7, 8], [6], 3, 3, 99) == [7, 8, 6]   # only g = 1 matches (i = 1)
    assert R.ngram_draft([1, 2, 3], [4], 3, 3, 99) == [-1, -1, -1]   # no match at all
    assert R.ngram_draft([4, 4], [], 3, 3, 99) == [4, -1, -1]        # i = 0, g = 1: s[1], then the end
    assert R.ngram_draft([4], [], 3, 3, 99) == [-1, -1, -1]          # L = 1: no i with i + g <= 0
    # the match may not be the suffix itself: i + g <= L - 1
    assert R.ngram_draft([1, 2], [], 2, 2, 99) == [-1, -1]


def test_ngram_draft_given_overrides_and_done_rows_guess_nothing():
    given = [-1, 30, -1, 50, 60, -1]
    # n = 1: slot j guesses new token 1 + j -> given[1 + j] where >= 0, else the lookup's
    assert R.ngram_draft([5, 6, 7, 8], [6], 3, 3, 6, given) == [30, 8, 50]
    # slots whose token would lie past n_new are not overridden (given has no such entry)
    assert R.ngram_draft([9], [1, 2, 3, 4, 5], 1, 3, 6, given) == [-1, -1, -1]
    assert R.ngram_draft([5, 5], [5] * 6, 1, 3, 6, given) == [-1, -1, -1]  # done


def _state(B, n_new, n):
    return dict(n=list(n), kv_len=[10] * B, pos=[4] * B, lengths=[n_new] * B, last=[0] * B,
                drafted=[0] * B, accepted=[0] * B, out=[[-9] * n_new for _ in range(B)])


def test_spec_accept_counts_clipping_eos_and_finished_rows():
    n_new = 8
    st = _state(6, n_new, [2, 2, 2, 6, 2, 8])
    x = [[7, 8, 9, 4], [7, 8, 9, 4], [7, 8, 9, 4], [7, 8, 9, 4], [7, 3, 9, 4], [7, 8, 9, 4]]
    d = [[1, 8, 9], [7, 8, 1], [7, 8, 9], [7, 8, 9], [7, 3, 9], [7, 8, 9]]
    R.spec_accept(x, d, st, n_new, eos=3)
    # row 0: nothing accepted, the correction alone; row 1: partial; row 2: full; row 3: clipped
    # at n_new; row 4: eos in the middle of an accepted run; row 5: finished, untouched
    assert st["n"] == [3, 5, 6, 8, 8, 8]
    assert st["accepted"] == [0, 2, 3, 1, 1, 0]
    assert st["drafted"] == [3, 3, 3, 3, 3, 0]
    assert st["kv_len"] == [11, 13, 14, 12, 12, 10] and st["pos"] == [5, 7, 8, 6, 6, 4]
    assert st["last"] == [7, 9, 4, 8, 3, 0]
    assert st["lengths"] == [8, 8, 8, 8, 4, 8]
    assert st["out"][0] == [-9, -9, 7, -9, -9, -9, -9, -9]
    assert st["out"][2] == [-9, -9, 7, 8, 9, 4, -9, -9]
    assert st["out"][3] == [-9] * 6 + [7, 8]
    assert st["out"][4] == [-9, -9, 7, 3, 3, 3, 3, 3]
    assert st["out"][5] == [-9] * 8
    # a -1 guess is counted as not drafted and stops the run
    st = _state(1, n_new, [0])
    R.spec_accept([[7, 8, 9, 4]], [[7, -1, 9]], st, n_new)
    assert st["n"] == [2] and st["drafted"] == [2] and st["accepted"] == [1]


@pytest.mark.parametrize("n_new,D", [(24, 4), (128, 4), (6, 7), (1, 3), (2, 1)])
def test_simulate_perfect_draft_takes_the_fewest_rounds(n_new, D):
    true = [[(3 * i + b) % 11 for i in range(n_new)] for b in range(2)]
    r = R.simulate(true, true, D)
    assert r["out"] == true
    assert r["steps"] == math.ceil((n_new - 1) / (D + 1)) + 1
    # every token but the first of each round was a confirmed guess
    assert r["accepted"] == [n_new - r["steps"]] * 2 and r["lengths"] == [n_new] * 2


def test_simulate_corruption_pattern():
    n_new, D = 12, 3
    true = [[10 + i for i in range(n_new)]]
    given = [list(true[0])]
    given[0][2] = 99   # wrong
    given[0][7] = -1   # no guess
    # round 0: token 0.  pass 1 (n = 1): guesses 1, 2x, 3 -> accepts 1, corrects 2: n = 3
    # pass 2 (n = 3): 3, 4, 5 all right -> n = 7.  pass 3 (n = 7): -1 -> token 7 alone: n = 8
    # pass 4 (n = 8): 8, 9, 10 -> n = 12
    r = R.simulate(true, given, D)
    assert r["out"] == true and r["steps"] == 5
    assert r["accepted"] == [1 + 3 + 0 + 3] and r["drafted"] == [3 + 3 + 2 + 3]
    # with the lookup on (a prompt without repeats: it never matches) the same figures
    r2 = R.simulate(true, given, D, prompts=[[1, 2, 3]], ngram=3)
    assert (r2["steps"], r2["accepted"], r2["drafted"]) == (5, r["accepted"], r["drafted"])
    # eos in the middle of an accepted run ends the row there
    r3 = R.simulate(true, true, D, eos=15)
    assert r3["lengths"] == [6] and r3["out"][0] == [10, 11, 12, 13, 14, 15] + [15] * 6
    assert r3["steps"] == 3


def test_bad_arguments_are_named_without_a_gpu():
    from gvl import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    multi = lambda Q, kv: lib.gvl_attn_decode_multi(a, a, 8 * 384, 8, kv, a, 128, 1, 2, Q, 0.125,
                                                    None)
    assert multi(0, a) == -1 and b"Q=0" in lib.gvl_last_error()
    assert multi(9, a) == -1 and b"Q=9" in lib.gvl_last_error()
    assert multi(2, None) == -1 and b"kv_len" in lib.gvl_last_error()
    draft = lambda ngram, D, P=4, n_new=4: lib.gvl_ngram_draft(a, P, P, a, a, n_new, a, n_new,
                                                               None, 0, 1, ngram, D, a, None)
    assert draft(5, 3) == -1 and b"ngram=5" in lib.gvl_last_error()
    assert draft(3, 8) == -1 and b"D=8" in lib.gvl_last_error()
    assert draft(3, 3, P=4000, n_new=100) == -1 and b"4100" in lib.gvl_last_error()
    acc = lambda Q, d: lib.gvl_spec_accept(a, d, 1, Q, a, a, a, a, a, a, 4, 4, -1, None, None,
                                           None)
    assert acc(9, a) == -1 and b"Q=9" in lib.gvl_last_error()
    assert acc(3, None) == -1 and b"draft" in lib.gvl_last_error()


def test_public_names_and_argument_errors_need_no_gpu():
    import torch

    import gvl
    from gvl import decode
    assert gvl.speculative_generate is decode.speculative_generate
    assert hasattr(decode.KVDecoder, "step_multi")
    ids = torch.zeros(2, 4, dtype=torch.int64)
    for kw in (dict(draft_len=0), dict(draft_len=8), dict(ngram=0), dict(ngram=5),
               dict(draft_ids=torch.zeros(2, 5, dtype=torch.int64)),
               dict(draft_ids=torch.zeros(2, 6))):
        with pytest.raises(ValueError):
            decode.speculative_generate(None, ids, 6, **kw)
