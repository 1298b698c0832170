"""Logits processors on the MI355X (gvl_logits_process, gvl.kernels.logits_process, and the
repetition / n-gram / length controls of gvl.decode generate and beam_search):

  1. the kernel against tests/logits_ref.py: the whole [R, ld] buffer bitwise, pad columns and
     untouched entries included;
  2. generate against a decoder driven by hand with the independent Hugging-Face-style
     restatement of tests/test_logits_cpu.py applied to every step's logits: same ids and lengths
     (the decoder logits are the same bits on both sides and the edits are exact: no tolerance);
  3. beam_search against a search driven by hand the same way: ids, lengths and raw scores of
     every beam bitwise;
  4. the new arguments at their defaults change nothing.
"""
import numpy as np
import pytest
import torch

from tests.helpers import TINY
from tests.logits_ref import logits_ref
from tests.test_gpu_beam import KINDS, _tiny, _tiny_inputs
from tests.test_logits_cpu import hf_process, hf_process_rows

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = 16384.0
DTYPES = [BF, torch.float32]
DT_IDS = ["bf16", "fp32"]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------ 1. the kernel
def _beam_table(rng, R, K, t0, n_hist, width):
    """A src table as a beam search leaves it: every step each row takes over the history of a
    random row of its item (rows permute and share parents) and appends itself."""
    rows = np.arange(R)
    src = np.zeros((R, width), dtype=np.int32)
    src[:, :t0] = (rows // K * K)[:, None]
    for s in range(n_hist):
        prow = rows // K * K + rng.integers(0, K, R)
        T = t0 + s
        src[:, :T] = src[prow, :T]
        src[:, T] = rows
    return src


def _inputs(R, rpi, V, ld, P, n_hist, use_src, symbols, seed=0, t0=3):
    rng = np.random.default_rng(seed)
    logits = np.full((R, ld), SENTINEL, dtype=np.float32)
    logits[:, :V] = rng.standard_normal((R, V)) * 3.0
    sym = np.asarray(symbols, dtype=np.int64)
    hist = sym[rng.integers(0, len(sym), (n_hist + 2, R + 1))]  # rows / columns to spare
    prompt = sym[rng.integers(0, len(sym), (R // rpi, P))] if P else None
    src = _beam_table(rng, R, rpi, t0, n_hist, t0 + n_hist + 2) if use_src else None
    return dict(logits=logits, hist=hist, n_hist=n_hist, prompt=prompt, src=src,
                t0=t0 if use_src else 0, rpi=rpi, V=V)


def _run(cuda, dtype, c, flen=None, **controls):
    """The kernel on buf[:, :V] (a strided view when ld > V) against the reference; -> the
    edited buffer and the input buffer on the CPU."""
    import gvl.kernels as Kn
    dev = lambda a, dt: None if a is None else torch.as_tensor(a).to(dt).to(cuda)
    before = torch.from_numpy(c["logits"]).to(dtype)
    buf = before.clone().to(cuda)
    view = buf[:, :c["V"]]
    bad = controls.pop("bad_tokens", None)
    args = dict(src=dev(c["src"], torch.int32), t0=c["t0"], prompt=dev(c["prompt"], torch.int64),
                rows_per_item=c["rpi"], flen=dev(flen, torch.int32),
                bad_tokens=dev(bad, torch.int32), **controls)
    ret = Kn.logits_process(view, dev(c["hist"], torch.int64), c["n_hist"], **args)
    torch.cuda.synchronize()
    assert ret is view
    want = logits_ref(before, c["hist"], c["n_hist"], src=c["src"], t0=c["t0"], prompt=c["prompt"],
                      rows_per_item=c["rpi"], flen=flen, bad_tokens=bad, V=c["V"], **controls)
    got = buf.cpu()
    diff = (_bits(got) != _bits(want)).nonzero().tolist()
    assert not diff, f"{len(diff)} entries differ from the reference, first (row, col): {diff[:4]}"
    return got, before


VOCABS = {8: (8, 12, (1, 3, 5, 6)), 50257: (50257, 50304, (0, 50256, 7, 300)),
          65536: (65536, 65536, (0, 65535, 7, 300))}
ROWS = {"one": (1, 1, False), "beams": (6, 3, True), "beams_nosrc": (6, 3, False)}
NGRAM = 3
LENGTHS = {0: (0, 0), NGRAM - 2: (1, 0), NGRAM - 1: (1, 1), NGRAM: (1, 2), 40: (10, 30),
           4096: (1000, 3096)}
ALL = dict(repetition_penalty=1.3, no_repeat_ngram_size=NGRAM, ban_eos=True)


@pytest.mark.parametrize("L", list(LENGTHS))
@pytest.mark.parametrize("V", list(VOCABS))
@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_kernel_matches_reference_bitwise(cuda, dtype, rows, V, L):
    R, rpi, use_src = ROWS[rows]
    V, ld, symbols = VOCABS[V]
    P, n_hist = LENGTHS[L]
    c = _inputs(R, rpi, V, ld, P, n_hist, use_src, symbols, seed=L + R)
    got, before = _run(cuda, dtype, c, eos=symbols[3], bad_tokens=[symbols[1], 2, V - 2], **ALL)
    assert torch.isinf(got[:, 2]).all() and torch.isinf(got[:, V - 2]).all()  # it did run
    assert torch.equal(_bits(got[:, V:]), _bits(before[:, V:]))  # the pad keeps the sentinel


CONTROLS = {"penalty": dict(repetition_penalty=1.3), "penalty_below_one": dict(repetition_penalty=0.5),
            "ngram1": dict(no_repeat_ngram_size=1), "ngram2": dict(no_repeat_ngram_size=2),
            "ngram3": dict(no_repeat_ngram_size=3), "ngram16": dict(no_repeat_ngram_size=16),
            "eos": dict(eos=5, ban_eos=True), "eos_not_banned": dict(eos=5, ban_eos=False,
                                                                     no_repeat_ngram_size=16),
            "bad": dict(bad_tokens=[0, 999, 5, 5]),
            "all": dict(eos=6, bad_tokens=[999, 17], **ALL)}


@pytest.mark.parametrize("name", list(CONTROLS))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_each_control_alone_and_all_together(cuda, dtype, name):
    c = _inputs(6, 3, 1000, 1008, 10, 30, True, (1, 3, 5, 6), seed=7)
    if name == "ngram16":  # every row generates one period-7 pattern: its last 15 tokens recur
        c["hist"][:] = np.array([1, 3, 5, 6, 1, 5, 3] * 5)[:c["hist"].shape[0], None]
    got, before = _run(cuda, dtype, c, **CONTROLS[name])
    changed = (_bits(got) != _bits(before)).any(1)
    if name == "ngram16":  # 30 tokens, so the next would be the pattern's third; nothing else
        assert (torch.isinf(got) != torch.isinf(before)).nonzero().tolist() == [[r, 5] for r in range(6)]
    # (random 16-grams of 4 symbols in 40 tokens: no match, so nothing is written at all)
    assert changed.any().item() == (name != "eos_not_banned")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_penalty_is_applied_once_per_distinct_token(cuda, dtype):
    """Token 5 three times in every row's history; its logit positive, negative and exactly 0."""
    c = _inputs(3, 1, 8, 12, 0, 5, False, (1, 3, 6))
    c["hist"][:5, :3] = np.array([[5, 1, 5, 3, 5]]).T
    c["logits"][:3, 5] = (2.5, -2.5, 0.0)
    got, _ = _run(cuda, dtype, c, repetition_penalty=1.3)
    cast = lambda x: torch.tensor(x, dtype=torch.float32).to(dtype).float().item()
    p = np.float32(1.3)
    assert got[0, 5].item() == cast(float(np.float32(2.5) / p))
    assert got[1, 5].item() == cast(float(np.float32(-2.5) * p))
    assert got[2, 5].item() == 0.0
    assert got[0, 5].item() != cast(float(np.float32(2.5) / p / p))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ngram_overlapping_matches_and_match_at_the_last_position(cuda, dtype):
    a, b = 3, 6
    c = _inputs(1, 1, 8, 8, 2, 3, False, (1,))
    c["prompt"][0] = (a, b)
    c["hist"][:3, 0] = (a, b, a)  # a b a b a, n = 3: the tail b a was followed by b, once
    got, _ = _run(cuda, dtype, c, no_repeat_ngram_size=3)
    assert torch.isinf(got[0]).nonzero().view(-1).tolist() == [b]
    c = _inputs(1, 1, 8, 8, 0, 4, False, (1,))
    c["hist"][:4, 0] = (1, 2, 3, 3)  # n = 2: the only earlier 3 is the one right before the end
    got, _ = _run(cuda, dtype, c, no_repeat_ngram_size=2)
    assert torch.isinf(got[0]).nonzero().view(-1).tolist() == [3]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_out_of_range_ids_and_table_entries(cuda, dtype):
    """Ids -1 and V in hist, prompt and bad; src entries R + 5 and -2 (clamped into [0, R)):
    nothing outside the rows' own V columns is written."""
    R, V = 6, 8
    c = _inputs(R, 3, V, 12, 4, 12, True, (-1, V, 2, 4), seed=5)
    c["src"][1, c["t0"] + 2] = R + 5
    c["src"][4, c["t0"] + 7] = -2
    c["src"][0, c["t0"] + 11] = R + 5
    got, before = _run(cuda, dtype, c, eos=V, bad_tokens=[-1, V, 7], **dict(ALL, no_repeat_ngram_size=2))
    assert torch.isinf(got[:, 7]).all()
    assert torch.equal(_bits(got[:, V:]), _bits(before[:, V:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_finished_rows_stay_untouched(cuda, dtype):
    c = _inputs(6, 3, 50257, 50304, 10, 30, True, (0, 50256, 7, 300), seed=9)
    flen = np.array([0, 4, 0, 0, 0, 17], dtype=np.int32)
    got, before = _run(cuda, dtype, c, flen=flen, eos=300, bad_tokens=[11], **ALL)
    for r in range(6):
        same = torch.equal(_bits(got[r]), _bits(before[r]))
        assert same == bool(flen[r] > 0), r


def test_wrapper_checks_its_arguments(cuda):
    import gvl.kernels as Kn
    lg = torch.zeros(2, 16, dtype=BF, device=cuda)
    hist = torch.zeros(3, 2, dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        Kn.logits_process(lg.cpu(), hist, 1, no_repeat_ngram_size=1)
    with pytest.raises(ValueError):
        Kn.logits_process(lg.half(), hist, 1, no_repeat_ngram_size=1)
    with pytest.raises(ValueError):
        Kn.logits_process(lg, hist.int(), 1, no_repeat_ngram_size=1)
    with pytest.raises(ValueError):
        Kn.logits_process(lg, hist, 4, no_repeat_ngram_size=1)  # more steps than hist holds
    with pytest.raises(ValueError):
        Kn.logits_process(lg, hist, 1, src=torch.zeros(2, 4, device=cuda), no_repeat_ngram_size=1)
    with pytest.raises(ValueError):
        Kn.logits_process(lg, hist, 1, prompt=hist[:1], rows_per_item=1, no_repeat_ngram_size=1)
    with pytest.raises(Exception, match="ngram"):
        Kn.logits_process(lg, hist, 1, no_repeat_ngram_size=17)
    assert not lg.any()


# ------------------------------------------------------------------ 2. generate
def _first_argmax(rows):
    return torch.from_numpy(rows.float().cpu().numpy().argmax(-1))  # numpy: the first maximum


def _generate_by_hand(model, prompt, z, n_new, eos=None, min_new_tokens=0, **kw):
    """Greedy decode with the restated processors applied on the host to every step's logits.
    -> ids [B, n_new] and lengths [B] on the CPU."""
    from gvl.decode import KVDecoder
    B = prompt.shape[0]
    dec = KVDecoder(model, B, n_new)
    logits = dec.start(prompt, z)
    seqs = [prompt[b].tolist() for b in range(B)]
    ids = torch.full((B, n_new), -1 if eos is None else eos, dtype=torch.int64)
    lengths, done = [n_new] * B, [False] * B
    for i in range(n_new):
        proc = hf_process_rows(logits, seqs, eos=eos, ban_eos=i < min_new_tokens, **kw)
        nxt = _first_argmax(proc)
        for b in range(B):
            if done[b]:
                nxt[b] = eos
            elif eos is not None and int(nxt[b]) == eos:
                done[b], lengths[b] = True, i + 1
            seqs[b].append(int(nxt[b]))
        ids[:, i] = nxt
        if all(done):
            break
        if i + 1 < n_new:
            logits = dec.step(nxt.to(prompt.device))
    return ids, torch.tensor(lengths, dtype=torch.int32)


def _repeated_ngrams(seq, n):
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(grams) - len(set(grams))


@pytest.mark.parametrize("kind", KINDS)
def test_generate_matches_hand_driven_decode(cuda, kind):
    from gvl.decode import generate
    B, P, n_new = 2, 5, 8
    model = _tiny(kind)
    prompt, z = _tiny_inputs(kind, B, cuda, P=P)
    pl = prompt.cpu().tolist()

    # no repeated token at all: the third token as the end token ends row 0 after exactly 3
    base = generate(model, prompt, n_new, z=z, greedy=True, repetition_penalty=1.3,
                    no_repeat_ngram_size=1).cpu()
    for b in range(B):
        assert len(set(pl[b] + base[b].tolist())) == len(set(pl[b])) + n_new
    eos = int(base[0, 2])
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=1)
    ids, lengths = generate(model, prompt, n_new, z=z, greedy=True, eos=eos, return_lengths=True, **kw)
    want_ids, want_len = _generate_by_hand(model, prompt, z, n_new, eos=eos, **kw)
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(lengths.cpu(), want_len)
    assert int(lengths[0]) == 3 and ids[0, :3].tolist() == base[0, :3].tolist()
    assert (ids[0, 3:] == eos).all()

    # the same end token under a minimum length: not among the first 5 tokens
    ids, lengths = generate(model, prompt, n_new, z=z, greedy=True, eos=eos, min_new_tokens=5,
                            return_lengths=True, **kw)
    want_ids, want_len = _generate_by_hand(model, prompt, z, n_new, eos=eos, min_new_tokens=5, **kw)
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(lengths.cpu(), want_len)
    assert not (ids[:, :5] == eos).any() and (lengths > 5).all()

    # penalty + 2-gram rule + minimum length + end token together
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    path = generate(model, prompt, n_new, z=z, greedy=True, **kw).cpu()
    eos = int(path[0, 3])
    ids, lengths = generate(model, prompt, n_new, z=z, greedy=True, eos=eos, min_new_tokens=2,
                            return_lengths=True, **kw)
    want_ids, want_len = _generate_by_hand(model, prompt, z, n_new, eos=eos, min_new_tokens=2, **kw)
    print(f"{kind}: ids {ids.tolist()} lengths {lengths.tolist()} eos {eos}")
    assert torch.equal(ids.cpu(), want_ids) and torch.equal(lengths.cpu(), want_len)
    ids, lengths = ids.cpu(), lengths.cpu()
    for b in range(B):
        n, row = int(lengths[b]), ids[b].tolist()
        assert _repeated_ngrams(pl[b] + row[:n], 2) == 0
        assert eos not in row[:2]
        first = row.index(eos) + 1 if eos in row else n_new
        assert n == first and all(t == eos for t in row[n:])


def test_generate_returns_logits_of_the_steps_that_ran(cuda):
    from gvl.decode import generate
    model = _tiny("gpt")
    prompt, _ = _tiny_inputs("gpt", 1, cuda)
    kw = dict(greedy=True, repetition_penalty=1.3, no_repeat_ngram_size=1)
    base = generate(model, prompt, 8, **kw)  # no token twice: its second token first comes second
    eos = int(base[0, 1])
    ids, lg, lengths = generate(model, prompt, 8, eos=eos, return_logits=True,
                                return_lengths=True, **kw)
    assert lengths.tolist() == [2] and lg.shape == (1, 2, TINY["vocab_size"])
    assert ids[0].tolist() == base[0, :2].tolist() + [eos] * 6


def test_generate_sampled_with_unigram_ban_draws_distinct_tokens(cuda):
    from gvl.decode import generate
    model = _tiny("gpt")
    prompt, _ = _tiny_inputs("gpt", 2, cuda)
    g = torch.Generator(device="cuda").manual_seed(4)
    ids = generate(model, prompt, 8, greedy=False, top_k=5, generator=g, no_repeat_ngram_size=1)
    for b in range(2):
        seq = prompt[b].tolist() + ids[b].tolist()
        assert len(set(seq)) == len(set(prompt[b].tolist())) + 8, seq


# ------------------------------------------------------------------ 3. beam search
def _beam_search_by_hand(model, prompt, z, n_new, Kb, eos, length_penalty=1.0, min_new_tokens=0,
                         penalize_prompt=True, **kw):
    """gvl.decode.beam_search step for step, with every hypothesis' history rebuilt on the host
    from the parents and the restated processors applied there.  -> ids [B, K, n_new], lengths,
    raw scores."""
    import gvl.kernels as Kn
    from gvl.decode import BeamDecoder
    B = prompt.shape[0]
    R = B * Kb
    dec = BeamDecoder(model, B, Kb, n_new)
    first = dec.start(prompt, z)
    dev, V, t0 = first.device, first.shape[1], dec.t
    logits = torch.zeros(R, V, dtype=first.dtype, device=dev)
    logits.view(B, Kb, V)[:, 0] = first
    len_norm = torch.arange(n_new + 2, dtype=torch.float32).clamp_(min=1.0).pow_(
        -float(length_penalty)).to(dev)
    score = torch.full((B, Kb), float("-inf"), dtype=torch.float32, device=dev)
    score[:, 0] = 0.0
    score, flen, src = score.view(R), torch.zeros(R, dtype=torch.int32, device=dev), dec.initial_src(dev)
    pl = prompt.cpu().tolist() if penalize_prompt else [[] for _ in range(B)]
    seqs = [[] for _ in range(R)]
    S = 0
    for s in range(n_new):
        lg, fl = logits.cpu(), flen.cpu()
        rows = [lg[r] if fl[r] > 0 else
                hf_process(lg[r].float(), pl[r // Kb] + seqs[r], eos=eos, ban_eos=s < min_new_tokens,
                           **kw).to(lg.dtype) for r in range(R)]
        tok, parent, score, flen, src = Kn.beam_step(torch.stack(rows).to(dev), score, flen,
                                                     len_norm, src, Kb, s, eos, t0)
        par, tk = parent.cpu().tolist(), tok.cpu().tolist()
        seqs = [seqs[r // Kb * Kb + par[r]] + [tk[r]] for r in range(R)]
        S = s + 1
        if S == n_new:
            break
        if bool(((flen > 0) | (score == float("-inf"))).all()):
            break
        logits = dec.step(tok, src)
    ids = torch.tensor([q + [eos] * (n_new - S) for q in seqs], dtype=torch.int64)
    sc, fl = score.cpu(), flen.cpu()
    live = torch.where(sc == float("-inf"), 0, S).to(torch.int32)
    lengths = torch.where(fl > 0, fl, live)
    return ids.view(B, Kb, n_new), lengths.view(B, Kb), sc.view(B, Kb)


@pytest.mark.parametrize("kind", ["gpt", "qformer"])
def test_beam_search_matches_hand_driven_search(cuda, kind):
    from gvl.decode import beam_search
    B, Kb, n_new = 2, 3, 6
    model = _tiny(kind)
    prompt, z = _tiny_inputs(kind, B, cuda)
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=2)
    # the end token: the third token of item 0's best hypothesis in a search without one, so that
    # hypothesis finishes right after the minimum length and competes on as a finished beam
    free = beam_search(model, prompt, n_new, z=z, num_beams=Kb, eos=None, return_all=True, **kw)
    eos = int(free[0][0, 0, 2])
    ids, lengths, scores = beam_search(model, prompt, n_new, z=z, num_beams=Kb, eos=eos,
                                       return_all=True, **kw)
    want = _beam_search_by_hand(model, prompt, z, n_new, Kb, eos, **kw)
    print(f"{kind}: eos {eos} lengths {lengths.tolist()} scores {scores.tolist()}")
    assert torch.equal(ids.cpu(), want[0])
    assert torch.equal(lengths.cpu(), want[1])
    assert torch.equal(_bits(scores.cpu()), _bits(want[2]))
    assert torch.isfinite(scores).all()
    assert (lengths < n_new).any(), "pick another end token: no hypothesis finished"
    pl = prompt.cpu().tolist()
    for b in range(B):
        for j in range(Kb):
            n, row = int(lengths[b, j]), ids[b, j].tolist()
            assert n >= 2 and eos not in row[:2]
            assert _repeated_ngrams(pl[b] + row[:n], 2) == 0, (b, j, row)
    best = beam_search(model, prompt, n_new, z=z, num_beams=Kb, eos=eos, **kw)
    assert torch.equal(best[0], ids[:, 0]) and torch.equal(best[2], scores[:, 0])


def test_beam_search_penalize_prompt_acts(cuda):
    """A prompt that repeats one token t which the model, after it, gives a real probability
    (asserted): with the prompt counted, t is penalised and `t t` may not be followed by t.
    Banning a token of probability q moves that step's log-normaliser by about q; at q >= 1e-3
    that is hundreds of fp32 spacings of a score below 64 (2**-18), so the scores must move."""
    from gvl.decode import KVDecoder, beam_search
    model = _tiny("gpt")
    cand = torch.arange(0, TINY["vocab_size"], 4, device=cuda)
    first = KVDecoder(model, cand.numel(), 1).start(cand.view(-1, 1).repeat(1, 5))
    p_self = torch.softmax(first.float(), -1).gather(1, cand.view(-1, 1)).view(-1)
    top = p_self.topk(2)
    print(f"p(t | t t t t t) of the two prompts' tokens {cand[top.indices].tolist()}: {top.values.tolist()}")
    assert (top.values >= 1e-3).all(),"pick other candidates: no token is likely after itself"
    prompt = cand[top.indices].view(2, 1).repeat(1, 5)
    kw = dict(num_beams=3, eos=None, return_all=True, repetition_penalty=1.2, no_repeat_ngram_size=2)
    with_p = beam_search(model, prompt, 6, penalize_prompt=True, **kw)
    without = beam_search(model, prompt, 6, penalize_prompt=False, **kw)
    want = _beam_search_by_hand(model, prompt, None, 6, 3, None, penalize_prompt=False,
                                repetition_penalty=1.2, no_repeat_ngram_size=2)
    assert torch.equal(without[0].cpu(), want[0]) and torch.equal(_bits(without[2].cpu()), _bits(want[2]))
    assert not (with_p[0][:, :, 0] == prompt[:, :1]).any()  # t banned at the first step
    assert not torch.equal(with_p[2], without[2]) or not torch.equal(with_p[0], without[0])


# ------------------------------------------------------------------ 4. neutral values
@pytest.mark.parametrize("kind", ["gpt", "cross"])
def test_default_arguments_change_nothing(cuda, kind):
    from gvl.decode import beam_search, generate
    model = _tiny(kind)
    prompt, z = _tiny_inputs(kind, 2, cuda)
    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, bad_tokens=None,
               penalize_prompt=True)
    a = generate(model, prompt, 8, z=z, greedy=True, return_logits=True)
    b = generate(model, prompt, 8, z=z, greedy=True, return_logits=True, eos=None,
                 return_lengths=False, **off)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].is_contiguous()
    gens = [torch.Generator(device="cuda").manual_seed(6) for _ in range(2)]
    a = generate(model, prompt, 8, z=z, temperature=0.9, top_k=20, top_p=0.9, generator=gens[0])
    b = generate(model, prompt, 8, z=z, temperature=0.9, top_k=20, top_p=0.9, generator=gens[1], **off)
    assert torch.equal(a, b)
    a = beam_search(model, prompt, 6, z=z, num_beams=3, eos=7, return_all=True)
    b = beam_search(model, prompt, 6, z=z, num_beams=3, eos=7, return_all=True, **off)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # min_new_tokens without an end token, and an empty bad-token list, are off too
    c = beam_search(model, prompt, 6, z=z, num_beams=3, eos=None, return_all=True)
    d = beam_search(model, prompt, 6, z=z, num_beams=3, eos=None, return_all=True,
                    min_new_tokens=3, bad_tokens=[])
    for x, y in zip(c, d):
        assert torch.equal(x, y)
