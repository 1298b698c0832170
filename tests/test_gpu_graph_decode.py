"""Graph-replayed decoding on the MI355X (gvl_attn_decode_step, gvl_logits_process_dev,
gvl_beam_step_dev, gvl.decode.GraphedGenerate / GraphedBeamSearch, generate / beam_search with
graph=True).  Everything here is an exact comparison:

  1-3. each device-stepped kernel has the bits of its host-stepped instance at the same step, for
       one set of host arguments and only the device int32 changing; what it must not load is
       NaN; a step outside its range writes nothing;
  4-9. a graphed call returns what the eager call returns on the same inputs (torch.equal on
       ids, logits, lengths, scores), whatever poll_every, and a session replays one capture for
       later calls.
"""
import numpy as np
import pytest
import torch

from tests.helpers import TINY
from tests.logits_ref import logits_ref
from tests.test_gpu_logits import _inputs as _logits_inputs
from tests.test_gpu_spec import (B, KB, KC, KH, KINDS, KTMAX, LENS, N_NEW, P, SEEDS, _greedy_case,
                                 _prompt, _tiny, _zin)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------ 1. gvl_attn_decode_step
# the edges of the 32-row value sweep and of the 256-thread key loop
T_EDGES = (0, 1, 31, 32, 255, 256, 257)
FORMS = {"plain": (False, False), "src": (True, False), "gap": (False, True),
         "src_gap": (True, True)}


# The skipped range [gap_lo[r], GAP_HI): row 0 skips everything below GAP_HI (at t < GAP_HI it
# has no key left and writes zeros), the last rows have an empty gap, one of them by the clamp.
# With a table every row has the same gap: a physical column is shared, so it can be poisoned
# only if nobody reads it.
GAP_HI = 16
GAP_LO = {False: (0, 5, 16, 21), True: (5, 5, 5, 5)}


@pytest.mark.parametrize("form", list(FORMS))
def test_attn_decode_step_bits_nan_append_and_nothing_baked_in(cuda, form):
    import gvl.kernels as Kn
    ind, gap = FORMS[form]
    g = torch.Generator(device="cuda").manual_seed(5)
    qkv = torch.randn(KB, 3 * KC, device=DEV, generator=g).to(BF)
    clean = torch.randn(KB, KTMAX, 3 * KC, device=DEV, generator=g).to(BF)
    src = torch.randint(0, KB, (KB, KTMAX), device=DEV, generator=g).to(torch.int32)
    own = torch.arange(KB, device=DEV, dtype=torch.int32)
    # one set of host arguments for every launch: the same buffers, only their contents change
    cache, o = torch.empty_like(clean), torch.empty(KB, KC, dtype=BF, device=DEV)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    gap_lo = torch.tensor(GAP_LO[ind], dtype=torch.int32, device=DEV)
    for t in T_EDGES:
        before = clean.clone()
        before[:, :, :KC] = NAN   # the q third
        before[:, t:] = NAN       # this column (the new k / v come from qkv) and all above
        if gap:
            for r, lo in enumerate(GAP_LO[ind]):
                before[(slice(None) if ind else r), lo:GAP_HI] = NAN
        cache.copy_(before)
        o.fill_(NAN)
        t_dev.fill_(t)
        ret = Kn.attn_decode_step(qkv, cache, t_dev, KH, src=src if ind else None,
                                  gap_lo=gap_lo if gap else None, gap_hi=GAP_HI if gap else 0,
                                  out=o)
        assert ret is o and torch.isfinite(o).all(), (form, t)
        # the host-stepped instance at Tk = t + 1 on a cache whose column t holds the new k / v
        want_cache = before.clone()
        want_cache[:, t, KC:] = qkv[:, KC:]
        Tk = t + 1
        k, v = want_cache[:, :Tk, KC:2 * KC], want_cache[:, :Tk, 2 * KC:]
        tab = None
        if ind:
            tab = src.clone()
            tab[:, t] = own
        if gap:
            # (the host-stepped instance takes gap_hi <= Tk: while Tk < GAP_HI the gap clamped to
            # Tk skips the same positions below Tk)
            want = Kn.attn_decode_ragged(qkv[:, :KC], k, v, KH, gap_lo.clamp(max=min(GAP_HI, Tk)),
                                         min(GAP_HI, Tk), src=tab)
        elif ind:
            want = Kn.attn_decode_beam(qkv[:, :KC], k, v, KH, tab)
        else:
            want = Kn.attn_decode(qkv[:, :KC], k, v, KH)
        assert torch.equal(_bits(o), _bits(want)), (form, t)
        # the append, and every other cache element keeps its (NaN or random) bits
        assert torch.equal(_bits(cache), _bits(want_cache)), (form, t)


def test_attn_decode_step_outside_the_cache_writes_nothing(cuda):
    import gvl.kernels as Kn
    qkv = torch.randn(KB, 3 * KC, device=DEV).to(BF)
    big = torch.full((KB, KTMAX + 4, 3 * KC), 7.0, dtype=BF, device=DEV)
    cache = big[:, :KTMAX]  # Tmax = KTMAX: column KTMAX exists in memory and must stay
    o = torch.full((KB, KC), 7.0, dtype=BF, device=DEV)
    for t in (KTMAX, -1, 2 ** 31 - 1, -2 ** 31):
        t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
        Kn.attn_decode_step(qkv, cache, t_dev, KH, out=o)
        assert (o == 7.0).all() and (big == 7.0).all(), t
    t_dev = torch.tensor([KTMAX - 1], dtype=torch.int32, device=DEV)  # the last column does run
    cache[:, :KTMAX - 1] = torch.randn(KB, KTMAX - 1, 3 * KC, device=DEV).to(BF)
    Kn.attn_decode_step(qkv, cache, t_dev, KH, out=o)
    assert torch.equal(cache[:, KTMAX - 1, KC:], qkv[:, KC:]) and (big[:, KTMAX:] == 7.0).all()
    assert torch.isfinite(o).all() and not (o == 7.0).all()


# ------------------------------------------------------------------ 2. gvl_logits_process_dev
HIST_CAP, MIN_NEW = 12, 5
LP_STEPS = (0, 1, 7, HIST_CAP, HIST_CAP + 3)


@pytest.mark.parametrize("full", [False, True], ids=["own_column", "src_flen_prompt"])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_logits_process_dev_equals_host_stepped_and_reference(cuda, dtype, full):
    import gvl.kernels as Kn
    R, rpi, V, ld = 6, 3, 1000, 1008
    c = _logits_inputs(R, rpi if full else 1, V, ld, 10 if full else 0, HIST_CAP, full,
                       (1, 3, 5, 6), seed=11)
    dev = lambda a, dt: None if a is None else torch.as_tensor(a).to(dt).to(cuda)
    flen = np.array([0, 2, 0, 0, 1, 0], dtype=np.int32) if full else None
    before = torch.from_numpy(c["logits"]).to(dtype)
    hist, src, prompt = dev(c["hist"], torch.int64), dev(c["src"], torch.int32), dev(c["prompt"], torch.int64)
    ctl = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, eos=6)
    kw = dict(src=src, t0=c["t0"], prompt=prompt, rows_per_item=c["rpi"], flen=dev(flen, torch.int32),
              bad_tokens=dev([3, 999], torch.int32), **ctl)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    buf = torch.empty(R, ld, dtype=dtype, device=cuda)  # the same arguments for every step
    for s in LP_STEPS:
        n, ban = min(s, HIST_CAP), s < MIN_NEW
        buf.copy_(before)
        step.fill_(s)
        Kn.logits_process_dev(buf[:, :V], hist, step, HIST_CAP, min_new=MIN_NEW, **kw)
        host = before.clone().to(cuda)
        Kn.logits_process(host[:, :V], hist, n, ban_eos=ban, **kw)
        assert torch.equal(_bits(buf), _bits(host)), s
        want = logits_ref(before, c["hist"], n, src=c["src"], t0=c["t0"], prompt=c["prompt"],
                          rows_per_item=c["rpi"], flen=flen, bad_tokens=[3, 999], V=V, ban_eos=ban,
                          **ctl)
        assert torch.equal(_bits(buf.cpu()), _bits(want)), s
        assert torch.isinf(buf[0, 3]).item()  # it ran


# ------------------------------------------------------------------ 3. gvl_beam_step_dev
def test_beam_step_dev_equals_host_stepped_bitwise(cuda):
    import gvl.kernels as Kn
    Bb, Kb, V, t0, MAXS = 2, 3, 50, 4, 6
    R = Bb * Kb
    g = torch.Generator(device="cuda").manual_seed(3)
    logits = (torch.randn(R, V, device=cuda, generator=g) * 3).to(BF)
    len_norm = torch.arange(MAXS + 2, dtype=torch.float32).clamp_(min=1.0).pow_(-0.7).to(cuda)
    item = torch.arange(R, device=cuda) // Kb * Kb
    src = (item[:, None] + torch.randint(0, Kb, (R, t0 + MAXS + 1), device=cuda, generator=g)).int()
    ws = torch.empty(Kn._L().gvl_beam_step_workspace_size(Bb, Kb) // 4, device=cuda)
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    fresh = lambda: (torch.full((R,), -9, dtype=torch.int64, device=cuda),
                     torch.full((R,), -9, dtype=torch.int32, device=cuda),
                     torch.full((R,), 7.0, device=cuda),
                     torch.full((R,), -9, dtype=torch.int32, device=cuda),
                     torch.full_like(src, -9))
    got = fresh()  # the same arguments for every step
    score, flen = torch.empty(R, device=cuda), torch.empty(R, dtype=torch.int32, device=cuda)
    for s in (0, 1, 5, MAXS, -1):
        if s == 0:  # the first step: slot 0 of every item at 0, the others empty
            sc = torch.full((R,), float("-inf"), device=cuda)
            sc[::Kb] = 0.0
            fl = torch.zeros(R, dtype=torch.int32, device=cuda)
        else:       # running scores; at the later steps one finished and one empty slot
            sc = -torch.rand(R, device=cuda, generator=g) * 5
            fl = torch.zeros(R, dtype=torch.int32, device=cuda)
            if s != 1:
                fl[1], sc[5] = 2, float("-inf")
        score.copy_(sc)
        flen.copy_(fl)
        for a, b in zip(got, fresh()):
            a.copy_(b)
        step.fill_(s)
        Kn.beam_step_dev(logits, score, flen, len_norm, src, Kb, step, MAXS, 7, t0, got, ws)
        if not 0 <= s < MAXS:  # outside [0, max_steps): nothing is written
            for a, b in zip(got, fresh()):
                assert torch.equal(a, b), s
            continue
        want = fresh()
        Kn.beam_step(logits, score, flen, len_norm, src, Kb, s, 7, t0, out=want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), (s, i)
        assert (got[0] >= 0).all() and (got[4][:, t0 + s] == torch.arange(R, device=cuda)).all()


# ------------------------------------------------------------------ 4-8. generate(graph=True)
def _inputs(kind, ragged, seed=None):
    prompt = _prompt(SEEDS[kind] if seed is None else seed)
    return prompt, _zin(kind), (list(LENS) if ragged else None)


def _same(got, want):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (i, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(_bits(a) if a.is_floating_point() else a,
                           _bits(b) if b.is_floating_point() else b), f"output {i} differs"


@pytest.mark.parametrize("ragged", [False, True], ids=["unpadded", "prompt_lens"])
@pytest.mark.parametrize("kind", KINDS)
def test_generate_graph_greedy_equals_eager(cuda, kind, ragged):
    from gvl.decode import generate
    prompt, z, lens = _inputs(kind, ragged)
    kw = dict(z=z, greedy=True, return_logits=True, return_lengths=True, prompt_lens=lens)
    want = generate(_tiny(kind), prompt, N_NEW, **kw)
    got = generate(_tiny(kind), prompt, N_NEW, graph=True, **kw)
    assert want[1].shape == (B, N_NEW, TINY["vocab_size"])
    _same(got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_generate_graph_sampling_with_generators_seeded_alike(cuda, kind):
    from gvl.decode import generate
    prompt, z, lens = _inputs(kind, True)
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)
    kw = dict(z=z, temperature=0.8, top_p=0.9, prompt_lens=lens)
    want = generate(_tiny(kind), prompt, N_NEW, generator=gen(), **kw)
    ga = gen()
    got = generate(_tiny(kind), prompt, N_NEW, generator=ga, graph=True, **kw)
    _same(got, want)
    assert len(set(want[0].tolist())) > 2  # it sampled, not one token over and over
    # the generator ends n_new draws on, as the eager call without eos leaves it
    gb = gen()
    for _ in range(N_NEW):
        torch.rand(B, generator=gb, device=cuda)
    assert torch.equal(torch.rand(4, generator=ga, device=cuda), torch.rand(4, generator=gb, device=cuda))


def _eos_of(kind):
    """The end token of test_gpu_spec.test_eos_mid_sequence: the first token some row emits for the
    first time at index 4 or later.  -> (eos, row, index)."""
    _, _, ids, _ = _greedy_case(kind)
    rows = ids.tolist()
    r0, i0 = next((r, i) for r in range(B) for i in range(4, 20) if rows[r][i] not in rows[r][:i])
    return rows[r0][i0], r0, i0


@pytest.mark.parametrize("kind", KINDS)
def test_generate_graph_eos_mid_sequence_and_poll_every(cuda, kind):
    from gvl.decode import GraphedGenerate, generate
    prompt, z, lens = _inputs(kind, True)
    eos, r0, i0 = _eos_of(kind)
    kw = dict(z=z, prompt_lens=lens, return_lengths=True)
    want = generate(_tiny(kind), prompt, N_NEW, greedy=True, eos=eos, **kw)
    assert int(want[1][r0]) == i0 + 1
    ended = want[1] < N_NEW
    all_done = int(want[1].max()) if bool(((want[0] == eos).any(1)).all()) else N_NEW
    for poll in (1, 8, 100):
        with GraphedGenerate(_tiny(kind), P, N_NEW, greedy=True, eos=eos, poll_every=poll) as ses:
            got = ses(prompt, **kw)
            _same(got, want)
            assert ses.stats["captures"] == 1 and ses.stats["replays"] <= all_done + poll
        for r in range(B):
            assert (got[0][r, int(got[1][r]):] == eos).all()
    assert ended.any()
    # one row alone: every row is done at i0 + 1, and a poll after every replay stops there
    one = dict(z=None if z is None else z[r0:r0 + 1], prompt_lens=[LENS[r0]], return_lengths=True)
    want1 = generate(_tiny(kind), prompt[r0:r0 + 1], N_NEW, greedy=True, eos=eos, **one)
    stop = int(want1[1][0])
    assert stop < N_NEW - 1
    for poll in (1, 8, 100):
        with GraphedGenerate(_tiny(kind), P, N_NEW, greedy=True, eos=eos, poll_every=poll) as ses:
            _same(ses(prompt[r0:r0 + 1], **one), want1)
            assert ses.stats["replays"] <= stop + poll
            if poll == 1:
                assert ses.stats["replays"] == stop - 1  # the first token came from the prefill


@pytest.mark.parametrize("penalize_prompt", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_generate_graph_controls_equal_eager(cuda, kind, penalize_prompt):
    from gvl.decode import generate
    prompt, z, lens = _inputs(kind, True)
    _, _, ids, _ = _greedy_case(kind)
    eos = int(ids[0, 0])  # what row 0 would emit first: banned for five steps
    kw = dict(z=z, greedy=True, prompt_lens=lens, return_logits=True, return_lengths=True, eos=eos,
              repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=5,
              bad_tokens=[int(ids[1, 0]), int(ids[2, 1])], penalize_prompt=penalize_prompt)
    want = generate(_tiny(kind), prompt, N_NEW, **kw)
    got = generate(_tiny(kind), prompt, N_NEW, graph=True, **kw)
    _same(got, want)
    assert not torch.equal(want[0], ids)  # the controls changed the output
    assert (want[0][:, :5] != eos).all() and (want[2] > 5).all()


def test_generate_session_reuse_and_refusals(cuda):
    from gvl.decode import GraphedGenerate, generate
    kind = "cross"
    model = _tiny(kind)
    pa, za, _ = _inputs(kind, False)
    pb, zb = _prompt(5), _zin(kind).flip(0) * 0.5
    kw = dict(greedy=True, return_logits=True)
    ses = GraphedGenerate(model, P, N_NEW, **kw)
    call = dict(return_lengths=True)
    one = ses(pa, z=za, **call)
    two = ses(pb, 7, z=zb, prompt_lens=list(LENS), **call)
    three = ses(pa, z=za, **call)
    short = ses(pb[:, :8], 9, z=zb, **call)  # a shorter prompt on the same graph
    assert ses.stats["captures"] == 1 and ses.stats["replays"] == 2 * (N_NEW - 1) + 6 + 8
    _same(one, generate(model, pa, N_NEW, z=za, **kw, **call))
    _same(two, generate(model, pb, 7, z=zb, prompt_lens=list(LENS), **kw, **call))
    _same(three, one)
    _same(short, generate(model, pb[:, :8], 9, z=zb, **kw, **call))
    assert two[0].shape == (B, 7) and two[1].shape == (B, 7, TINY["vocab_size"])
    # prompt_lens under a shorter prompt moves the gap end: its own capture, the same buffers
    lens8 = [3, 8, 6]
    _same(ses(pb[:, :8], 9, z=zb, prompt_lens=lens8, **call),
          generate(model, pb[:, :8], 9, z=zb, prompt_lens=lens8, **kw, **call))
    assert ses.stats["captures"] == 2
    _same(ses(pa, z=za, **call), one)
    before = dict(ses.stats)
    long = torch.cat([pa, pa[:, :1]], 1)
    with pytest.raises(ValueError, match="max_prompt"):
        ses(long, z=za)
    with pytest.raises(ValueError, match="max_new"):
        ses(pa, N_NEW + 1, z=za)
    with pytest.raises(ValueError, match="batch"):
        ses(pa[:2], z=za[:2])
    with pytest.raises(ValueError, match="image-token shape"):
        ses(pa, z=None)
    with pytest.raises(ValueError, match="prompt_lens"):
        ses(pa, z=za, prompt_lens=[1, 2])
    assert ses.stats == before  # refused before any launch
    ses.close()
    assert ses.closed
    with pytest.raises(RuntimeError, match="after close"):
        ses(pa, z=za)
    ses.close()  # idempotent


# ------------------------------------------------------------------ 9. beam_search(graph=True)
KBEAM = 3


@pytest.mark.parametrize("ragged", [False, True], ids=["unpadded", "prompt_lens"])
@pytest.mark.parametrize("kind", KINDS)
def test_beam_search_graph_equals_eager(cuda, kind, ragged):
    """All K hypotheses in rank order, with an end token that row r0 emits mid-sequence and every
    control on; then eos=None with the defaults (no control kernel, never finished)."""
    from gvl.decode import beam_search
    prompt, z, lens = _inputs(kind, ragged)
    _, _, ids, _ = _greedy_case(kind)
    eos, _, _ = _eos_of(kind)
    base = dict(z=z, num_beams=KBEAM, prompt_lens=lens)
    cases = [dict(eos=eos, return_all=True, length_penalty=0.7),
             dict(eos=eos, return_all=True, repetition_penalty=1.3, no_repeat_ngram_size=2,
                  min_new_tokens=5, bad_tokens=[int(ids[1, 0]), int(ids[2, 1])]),
             dict(eos=None), dict(eos=eos)]
    for kw in cases:
        want = beam_search(_tiny(kind), prompt, N_NEW, **base, **kw)
        got = beam_search(_tiny(kind), prompt, N_NEW, graph=True, **base, **kw)
        _same(got, want)
    assert want[0].shape == (B, N_NEW) and want[1].dtype == torch.int32


def test_beam_search_graph_early_end_and_poll_every(cuda):
    """An end token every hypothesis reaches early: the search stops there, and a late poll
    (extra steps that only carry finished hypotheses over) changes no output."""
    from gvl.decode import GraphedBeamSearch, beam_search
    kind = "gpt"
    prompt, z, lens = _inputs(kind, True)
    _, _, ids, _ = _greedy_case(kind)
    model = _tiny(kind)
    # tokens 10 and 11 once each (no token twice, all others banned, the end token 9 banned for
    # two steps), then only the end token is left: every hypothesis ends at length 3
    bad = [t for t in range(TINY["vocab_size"]) if t not in (9, 10, 11)]
    kw = dict(z=z, prompt_lens=lens, return_all=True)
    ctl = dict(num_beams=KBEAM, eos=9, bad_tokens=bad, min_new_tokens=2, no_repeat_ngram_size=1,
               penalize_prompt=False)
    want = beam_search(model, prompt, N_NEW, **ctl, **kw)
    steps = int(want[1].max())
    assert steps == 3
    for poll in (1, 8, 100):
        with GraphedBeamSearch(model, P, N_NEW, poll_every=poll, **ctl) as ses:
            _same(ses(prompt, **kw), want)
            assert ses.stats["replays"] <= steps + poll
            if poll == 1:
                assert ses.stats["replays"] < N_NEW - 1


def test_beam_session_reuse_and_refusals(cuda):
    from gvl.decode import GraphedBeamSearch, beam_search
    kind = "linear"
    model = _tiny(kind)
    pa, za, _ = _inputs(kind, False)
    pb, zb = _prompt(5), _zin(kind).flip(0) * 0.5
    eos, _, _ = _eos_of(kind)
    ctl = dict(num_beams=KBEAM, eos=eos, no_repeat_ngram_size=3)
    ses = GraphedBeamSearch(model, P, N_NEW, **ctl)
    one = ses(pa, z=za, return_all=True)
    two = ses(pb, 7, z=zb, prompt_lens=list(LENS))
    three = ses(pa, z=za, return_all=True)
    assert ses.stats["captures"] == 1
    _same(one, beam_search(model, pa, N_NEW, z=za, return_all=True, **ctl))
    _same(two, beam_search(model, pb, 7, z=zb, prompt_lens=list(LENS), **ctl))
    _same(three, one)
    # another P moves the table's t0: its own capture over the same buffers
    _same(ses(pb[:, :8], 9, z=zb), beam_search(model, pb[:, :8], 9, z=zb, **ctl))
    assert ses.stats["captures"] == 2
    _same(ses(pa, z=za, return_all=True), one)
    with pytest.raises(ValueError, match="max_prompt"):
        ses(torch.cat([pa, pa[:, :1]], 1), z=za)
    with pytest.raises(ValueError, match="max_new"):
        ses(pa, N_NEW + 1, z=za)
    with pytest.raises(ValueError, match="batch"):
        ses(pa[:2], z=za[:2])
    ses.close()
    with pytest.raises(RuntimeError, match="after close"):
        ses(pa, z=za)
