"""Beam search without a GPU: the fp64 step reference (tests/beam_ref.py) on a hand-worked
example, and the host-side argument validation of gvl_beam_step / gvl_attn_decode_beam."""
import ctypes
import math

import numpy as np

from tests.beam_ref import beam_step_ref


def _hand_case(length_penalty):
    """B = 2, K = 2, V = 4, eos = 3, step 2 (candidates have 3 tokens), t0 = 2.
    item 0: slot 0 live (raw -1, p = [1/8, 1/8, 1/4, 1/2]), slot 1 finished after 1 token (raw -1.2)
    item 1: slot 0 live (raw -0.5, p = [.4, .4, .1, .1]), slot 1 live (raw -0.7, same p)."""
    logits = np.log(np.array([[.125, .125, .25, .5], [.25, .25, .25, .25],
                              [.4, .4, .1, .1], [.4, .4, .1, .1]]))
    score = np.array([-1.0, -1.2, -0.5, -0.7])
    flen = np.array([0, 1, 0, 0])
    len_norm = np.array([1.0] + [float(n) ** -length_penalty for n in range(1, 5)])
    src = np.array([[0, 0, 1, 0, -1, -1], [0, 0, 1, 1, -1, -1],
                    [2, 2, 3, 2, -1, -1], [2, 2, 2, 3, -1, -1]], dtype=np.int32)
    return beam_step_ref(logits, score, flen, len_norm, 2, 3, 2, src, 2)


def test_reference_hand_worked_without_length_penalty():
    r = _hand_case(0.0)
    # item 0: the carried finished beam (-1.2) beats the finishing candidate (0, eos) at
    # -1 + ln(1/2) = -1.693; item 1: (0, 0) and (0, 1) tie at -0.5 + ln 0.4 and go in token
    # order, ahead of slot 1's -0.7 + ln 0.4
    assert r["tok"].tolist() == [3, 3, 0, 1]
    assert r["parent"].tolist() == [1, 0, 0, 0]
    assert r["flen"].tolist() == [1, 3, 0, 0]
    want = [-1.2, -1.0 + math.log(.5), -0.5 + math.log(.4), -0.5 + math.log(.4)]
    assert np.allclose(r["score"], want, atol=1e-6)
    assert r["src"].tolist() == [[0, 0, 1, 1, 0, -1], [0, 0, 1, 0, 1, -1],
                                 [2, 2, 3, 2, 2, -1], [2, 2, 3, 2, 3, -1]]
    # the tie (same row, equal logits) is not a gap; the smallest real one is item 1's
    # (0, 1) -> (1, 0): 0.2
    assert abs(r["gap"] - 0.2) < 1e-12


def test_reference_hand_worked_with_length_penalty():
    r = _hand_case(1.0)
    # keys divide by the length: the 3-token finishing candidate -1.693 / 3 = -0.564 now beats
    # the 1-token finished beam -1.2 / 1; raw scores are reported unchanged
    assert r["tok"].tolist() == [3, 2, 0, 1]
    assert r["parent"].tolist() == [0, 0, 0, 0]
    assert r["flen"].tolist() == [3, 0, 0, 0]
    assert np.allclose(r["score"][:2], [-1.0 + math.log(.5), -1.0 + math.log(.25)], atol=1e-6)


def test_reference_empty_slots_and_first_step():
    # first step: slot 0 at 0, the others empty; V = 2 < 3 = K candidates short by one
    logits = np.log(np.array([[.75, .25]] * 3))
    r = beam_step_ref(logits, np.array([0.0, -np.inf, -np.inf]), np.zeros(3, int), np.ones(3), 0,
                      None, 1, np.zeros((3, 2), np.int32), 3)
    assert r["tok"].tolist() == [0, 1, 0] and r["parent"].tolist() == [0, 0, 2]
    assert r["score"][2] == -np.inf and r["flen"].tolist() == [0, 0, 0]
    assert r["src"].tolist() == [[0, 0], [0, 1], [0, 2]]


def _lib():
    from gvl import _lib
    return _lib.load()


def _beam_step(lib, *, K=2, V=16, B=1, null=None, ld=None, step=0, t0=1, src_ld=4):
    p = {n: 0x1000 + 0x100 * i for i, n in enumerate(
        ["logits", "score", "flen", "len_norm", "src_in", "tok", "parent", "score_out", "flen_out",
         "src_out", "ws"])}
    if null:
        p[null] = None
    return lib.gvl_beam_step(p["logits"], V if ld is None else ld, 0, B, K, V, p["score"], p["flen"],
                             p["len_norm"], step, -1, t0, p["src_in"], src_ld, p["tok"],
                             p["parent"], p["score_out"], p["flen_out"], p["src_out"], p["ws"], None)


def test_beam_step_rejects_bad_arguments_without_gpu():
    """Validation runs on the host before any launch (no device needed; pointers never read)."""
    lib = _lib()
    for K in (0, 9):
        assert _beam_step(lib, K=K) == -1
        assert b"K=%d out of range" % K in lib.gvl_last_error()
    assert _beam_step(lib, V=65537) == -1 and b"V=65537" in lib.gvl_last_error()
    assert _beam_step(lib, K=4, V=3) == -1 and b"V=3" in lib.gvl_last_error()
    for name in ("logits", "len_norm", "src_out", "ws"):
        assert _beam_step(lib, null=name) == -1 and b"null buffer" in lib.gvl_last_error()
    assert _beam_step(lib, step=3, t0=1, src_ld=4) == -1 and b"src table" in lib.gvl_last_error()
    assert _beam_step(lib, ld=8) == -1 and b"ld=8" in lib.gvl_last_error()
    assert lib.gvl_beam_step_workspace_size(3, 4) >= 3 * 4 * 4 * 12


def test_attn_decode_beam_rejects_bad_arguments_without_gpu():
    lib = _lib()

    def call(Tk=8, src=0x4000, src_ld=16):
        return lib.gvl_attn_decode_beam(0x1000, 128, 0x2000, 4096, 384, 0x3000, 4096, 384, 0x5000,
                                        128, 2, 2, Tk, 0.125, src, src_ld, None)

    assert call(src=None) == -1 and b"null src" in lib.gvl_last_error()
    assert call(Tk=4097, src_ld=8192) == -1 and b"Tk=4097" in lib.gvl_last_error()
    assert call(Tk=0) == -1 and b"Tk=0" in lib.gvl_last_error()
    assert call(Tk=8, src_ld=4) == -1 and b"src_ld=4" in lib.gvl_last_error()


def test_binding_has_beam_entry_points_at_abi_14():
    from gvl import _lib
    assert {"gvl_beam_step", "gvl_beam_step_workspace_size", "gvl_attn_decode_beam"} <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 14 and _lib.load().gvl_abi_version() == 14
