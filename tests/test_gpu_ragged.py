"""Prompts of different lengths in one batch on the MI355X (gvl_attn_decode_ragged,
gvl_embedding_fwd_pos, prompt_lens of gvl.decode KVDecoder / BeamDecoder / generate / beam_search):

  1. the gap kernel against fp32 torch with the same mask, plain and through a src table;
  2. an empty gap has the bits of gvl_attn_decode / gvl_attn_decode_beam;
  3. everything the kernel must not load filled with NaN / +inf changes no bit;
  4. a sequence with every key in the gap writes zeros;
  5. gvl_embedding_fwd_pos has the bits of per-row gvl_embedding_fwd calls;
  6. no output bit depends on the pad ids (decoder, generate, beam_search);
  7. prompt_lens = [P] * B has the bits of the call without it;
  8. every row's logits are those of the row run alone (and not those of the two wrong readings);
  9. scripted beam parents == a plain ragged decoder with physically reordered cache rows;
 10. beam scores == the gvl.score of each hypothesis after its unpadded prompt;
 11. the logits processors see each row's real sequence.
"""
import functools

import pytest
import torch

from tests.helpers import TINY, margins_out
from tests.logits_ref import banned_by_ngram, logits_ref
from tests.test_gpu_parity_full import _build_tiny, _recipe, _z

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KINDS = ("gpt", "linear", "qformer", "cross")
DEV = "cuda:0"


# ------------------------------------------------------------------ kernel level
KB, KH, KC, KTMAX = 3, 2, 128, 300

# name -> (gap_lo per row, gap_hi) per Tk.  "empty": gap_lo >= gap_hi (entries past gap_hi are
# clamped by the kernel); "head": [lo, hi) with only the tail valid (row 0 keeps one key);
# "to_end": the gap's last key is Tk - 1; "s256": straddles key 256 (the second sweep of the
# 256 score threads); "m32": straddles a multiple of 32 (the value sweep).
GAPS = {
    1: dict(empty=((0, 0, 0), 0), empty_hi=((1, 1, 7), 1)),
    37: dict(empty=((18, 19, 1000), 18), head=((0, 1, 2), 36), to_end=((36, 18, 1), 37),
             m32=((30, 31, 25), 35)),
    300: dict(empty=((150, 151, 1000), 150), head=((0, 1, 2), 299), to_end=((299, 150, 1), 300),
              s256=((250, 251, 255), 262), m32=((60, 63, 33), 70)),
}
GAP_CASES = [(Tk, name) for Tk, d in GAPS.items() for name in d]
GAP_CASES_NONEMPTY = [(Tk, name) for Tk, name in GAP_CASES if not name.startswith("empty")]


@functools.lru_cache(maxsize=None)
def _kernel_inputs():
    g = torch.Generator(device="cuda").manual_seed(0)
    cache = torch.randn(KB, KTMAX, 3 * KC, device=DEV, generator=g).to(BF)
    src = torch.randint(0, KB, (KB, KTMAX), device=DEV, generator=g).to(torch.int32)
    return cache, src


def _valid(Tk, lo, hi):
    """bool [B, Tk]: key t of sequence r is attended."""
    t = torch.arange(Tk, device=DEV)[None, :]
    lo = torch.tensor(lo, device=DEV).clamp(0, hi)[:, None]
    return ~((t >= lo) & (t < hi))


def _ragged(cache, Tk, lo, hi, src):
    import gvl.kernels as Kn
    q = cache[:, Tk - 1, :KC]
    gap_lo = torch.tensor(lo, dtype=torch.int32, device=DEV)
    return Kn.attn_decode_ragged(q, cache[:, :Tk, KC:2 * KC], cache[:, :Tk, 2 * KC:], KH, gap_lo,
                                 hi, src=src)


def _gathered(cache, src):
    if src is None:
        return cache
    return cache[src.long(), torch.arange(KTMAX, device=DEV)[None, :]].contiguous()


def _reference(cache, Tk, lo, hi, src):
    gath = _gathered(cache, src)
    qf = cache[:, Tk - 1, :KC].float().view(KB, KH, 64)
    kf = gath[:, :Tk, KC:2 * KC].float().view(KB, Tk, KH, 64).transpose(1, 2)
    vf = gath[:, :Tk, 2 * KC:].float().view(KB, Tk, KH, 64).transpose(1, 2)
    s = torch.einsum("bhd,bhtd->bht", qf, kf) / 8.0
    s = s.masked_fill(~_valid(Tk, lo, hi)[:, None, :], float("-inf"))
    return torch.einsum("bht,bhtd->bhd", s.softmax(-1), vf).reshape(KB, KC)


@pytest.mark.parametrize("use_src", [False, True], ids=["plain", "src"])
@pytest.mark.parametrize("Tk,name", GAP_CASES)
def test_attn_decode_ragged_matches_reference(cuda, Tk, name, use_src):
    cache, src = _kernel_inputs()
    src = src if use_src else None
    lo, hi = GAPS[Tk][name]
    o = _ragged(cache, Tk, lo, hi, src)
    want = _reference(cache, Tk, lo, hi, src)
    err = (o.float() - want).abs().max().item() / want.abs().max().item()
    print(f"Tk={Tk} {name} src={use_src}: rel err {err:.2e}")
    assert err < 1e-2


@pytest.mark.parametrize("Tk,name", [c for c in GAP_CASES if c[1].startswith("empty")])
def test_empty_gap_is_the_plain_kernel_bitwise(cuda, Tk, name):
    import gvl.kernels as Kn
    cache, src = _kernel_inputs()
    lo, hi = GAPS[Tk][name]
    q, k, v = cache[:, Tk - 1, :KC], cache[:, :Tk, KC:2 * KC], cache[:, :Tk, 2 * KC:]
    assert torch.equal(_ragged(cache, Tk, lo, hi, None), Kn.attn_decode(q, k, v, KH))
    assert torch.equal(_ragged(cache, Tk, lo, hi, src), Kn.attn_decode_beam(q, k, v, KH, src))


def _unused(Tk, lo, hi, src):
    """bool [B, Tmax]: cache entries (row, t) that no sequence may load: every key of a row's gap
    (through src: unless another sequence attends that entry) and everything from Tk on."""
    valid = _valid(Tk, lo, hi)
    used = torch.zeros(KB, KTMAX, dtype=torch.bool, device=DEV)
    rows = torch.arange(KB, device=DEV)[:, None].expand(KB, Tk) if src is None else src[:, :Tk].long()
    t = torch.arange(Tk, device=DEV)[None, :].expand(KB, Tk)
    used[rows[valid], t[valid]] = True
    return ~used


@pytest.mark.parametrize("use_src", [False, True], ids=["plain", "src"])
@pytest.mark.parametrize("Tk,name", GAP_CASES_NONEMPTY)
def test_gap_is_never_loaded(cuda, Tk, name, use_src):
    cache, src = _kernel_inputs()
    src = src if use_src else None
    lo, hi = GAPS[Tk][name]
    unused = _unused(Tk, lo, hi, src)
    assert unused[:, :Tk].any()
    outs = []
    for fill in (0.0, float("nan"), float("inf")):
        c = cache.clone()
        kv = c[:, :, KC:]  # q (cache[:, Tk - 1, :C]) stays
        kv[unused] = fill
        outs.append(_ragged(c, Tk, lo, hi, src))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[1], outs[0]), "a NaN in the gap reached the output"
    assert torch.equal(outs[2], outs[0]), "an infinity in the gap reached the output"
    assert torch.equal(outs[0], _ragged(cache, Tk, lo, hi, src))


@pytest.mark.parametrize("use_src", [False, True], ids=["plain", "src"])
@pytest.mark.parametrize("Tk", [1, 37])
def test_all_masked_sequence_writes_zeros(cuda, Tk, use_src):
    cache, src = _kernel_inputs()
    src = src if use_src else None
    lo, hi = (0, -3, Tk), Tk  # rows 0 and 1: every key in the gap; row 2: none
    c = cache.clone()
    c[:, :, KC:][_unused(Tk, lo, hi, src)] = float("nan")
    for cc in (cache, c):
        o = _ragged(cc, Tk, lo, hi, src)
        assert (o[:2] == 0).all()
        want = _reference(cache, Tk, (Tk, Tk, Tk), hi, src)[2]
        assert (o[2].float() - want).abs().max().item() / want.abs().max().item() < 1e-2


@pytest.mark.parametrize("C", [128, 768])
def test_embedding_fwd_pos_is_per_row_embedding_fwd(cuda, C):
    import gvl.kernels as Kn
    g = torch.Generator(device="cuda").manual_seed(1)
    V, T = TINY["vocab_size"], TINY["block_size"]
    wte = torch.randn(V, C, device=cuda, generator=g).to(BF)
    wpe = torch.randn(T, C, device=cuda, generator=g).to(BF)
    idx = torch.tensor([0, V - 1, 5, 5, 17, 300, 2], device=cuda)
    pos = torch.tensor([0, T - 1, T - 1, 0, 31, 32, 1], dtype=torch.int32, device=cuda)
    got = Kn.embedding_fwd_pos(idx, pos, wte, wpe)
    want = torch.empty_like(got)
    for r in range(idx.numel()):
        p = int(pos[r])
        Kn.embedding_fwd(idx[r:r + 1].view(1, 1), wte, wpe[p:p + 1], want[r:r + 1], 1, 1, 0)
    assert torch.equal(got, want)
    assert torch.equal(got.float(), (wte[idx].float() + wpe[pos.long()].float()).to(BF).float())
    # an id or a position outside its table reads row 0, as an id does in gvl_embedding_fwd
    bad = Kn.embedding_fwd_pos(torch.tensor([V + 3, 4, -1], device=cuda),
                               torch.tensor([3, T, -1], dtype=torch.int32, device=cuda), wte, wpe)
    rows = ((0, 3), (4, 0), (0, 0))
    want = torch.stack([(wte[i].float() + wpe[p].float()).to(BF) for i, p in rows])
    assert torch.equal(bad.float(), want.float())


# ------------------------------------------------------------------ decoder level
B, P, LENS, STEPS = 3, 8, (1, 5, 8), 6


@functools.lru_cache(maxsize=None)
def _tiny(kind):
    model, _ = _recipe(_build_tiny(kind), torch.device(DEV))
    return model.eval()


def _inputs(kind, pads="zero", seed=11):
    """(prompt [B, P] whose entries past LENS are 0 / random valid ids, z)."""
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(0, TINY["vocab_size"], (B, P), generator=g)
    fill = torch.randint(0, TINY["vocab_size"], (B, P), generator=g)
    for r, L in enumerate(LENS):
        prompt[r, L:] = 0 if pads == "zero" else fill[r, L:]
    z = None if kind == "gpt" else _z(3, B, TINY["n_embd"], torch.device(DEV))
    return prompt.to(DEV), z


def _script(rows, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, TINY["vocab_size"], (STEPS, rows), generator=g).to(DEV)


def _kv_logits(model, prompt, z, lens, toks):
    """[rows, STEPS + 1, V]: the first logits and those after each scripted token."""
    from gvl.decode import KVDecoder
    dec = KVDecoder(model, prompt.shape[0], toks.shape[0])
    out = [dec.start(prompt, z, lens)]
    for s in range(toks.shape[0]):
        out.append(dec.step(toks[s]))
    return torch.stack(out, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_pad_ids_change_no_bit(cuda, kind):
    from gvl.decode import beam_search, generate
    model = _tiny(kind)
    (p0, z), (p1, _) = _inputs(kind, "zero"), _inputs(kind, "rand")
    assert not torch.equal(p0, p1)
    toks = _script(B)
    a, b = (_kv_logits(model, p, z, LENS, toks) for p in (p0, p1))
    assert torch.isfinite(a).all() and torch.equal(a, b)
    ga, gb = (generate(model, p, STEPS, z=z, greedy=True, return_logits=True,
                       prompt_lens=torch.tensor(LENS, device=cuda)) for p in (p0, p1))
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    ba, bb = (beam_search(model, p, STEPS, z=z, num_beams=3, eos=None, return_all=True,
                          prompt_lens=list(LENS)) for p in (p0, p1))
    for x, y in zip(ba, bb):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", KINDS)
def test_equal_lengths_are_the_old_path_bitwise(cuda, kind):
    from gvl.decode import beam_search, generate
    model = _tiny(kind)
    prompt, z = _inputs(kind, "rand")
    full = [P] * B
    for kw in (dict(greedy=True), dict(top_k=50, temperature=0.8)):
        outs = []
        for lens in (None, full):
            gen = torch.Generator(device="cuda").manual_seed(42)
            outs.append(generate(model, prompt, STEPS, z=z, generator=gen, return_logits=True,
                                 prompt_lens=lens, **kw))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), kw
    ba, bb = (beam_search(model, prompt, STEPS, z=z, num_beams=3, eos=None, return_all=True,
                          prompt_lens=lens) for lens in (None, full))
    for x, y in zip(ba, bb):
        assert torch.equal(x, y)


def test_block_size_limit_follows_the_longest_prompt(cuda):
    """generate refuses up front what would run past the position table; a decoder stepped by
    hand is stopped at the step whose longest row has no position left."""
    from gvl.decode import KVDecoder, generate
    model = _tiny("gpt")
    prompt, _ = _inputs("gpt")
    T = TINY["block_size"]
    n_fit = T - P + 1  # 8 + n_new - 1 == block_size
    with pytest.raises(ValueError, match="block_size"):
        generate(model, prompt, n_fit + 1, greedy=True, prompt_lens=list(LENS))
    ids = generate(model, prompt, n_fit, greedy=True, prompt_lens=list(LENS))
    assert ids.shape == (B, n_fit)
    dec = KVDecoder(model, B, n_fit)
    dec.start(prompt, None, LENS)
    for s in range(n_fit - 1):  # positions 8 .. block_size - 1 of the longest row
        dec.step(ids[:, s])
    assert int(dec.pos.max()) == T
    with pytest.raises(ValueError, match="block_size"):
        dec.step(ids[:, n_fit - 1])


def _full(model, kind, seq, z):
    with torch.no_grad():
        return (model(seq)[0] if kind == "gpt" else model(seq, z=z)[0] if kind == "cross"
                else model(z, seq)[0]).float()


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


BOUND = 3e-2  # tests/test_gpu_decode.py test_kv_cached_greedy_vs_reference


@pytest.mark.parametrize("kind", KINDS)
def test_each_row_equals_the_row_alone(cuda, kind):
    """Row r's first logits and those after each of STEPS scripted tokens against the full
    forward of cat(prompt[r, :len_r], tokens), every step of every row.  The two wrong readings
    of a padded batch must be told apart: positions counted from the padded length (the full
    forward of the same unpadded sequence with wpe rows [P, P + STEPS) moved to
    [len_r, len_r + STEPS)), and pads attended (the full forward of the padded row)."""
    model, _ = _recipe(_build_tiny(kind), cuda)  # this test's own model: it edits wpe
    model.eval()
    prompt, z = _inputs(kind, "rand")
    toks = _script(B)
    got = _kv_logits(model, prompt, z, LENS, toks).float()
    wpe = (model if kind in ("gpt", "cross") else model.gpt).transformer.wpe.weight.data
    far_pos, far_pad = 0.0, 0.0
    for r, L in enumerate(LENS):
        zr = None if z is None else z[r:r + 1]
        seq = torch.cat([prompt[r, :L], toks[:, r]])[None]
        full = _full(model, kind, seq, zr)
        M = full.shape[1] - seq.shape[1]  # caption logits lead with M image rows
        right = full[0, M + L - 1:M + L + STEPS]
        err = _rel(got[r], right)
        print(f"{kind} row {r} (len {L}): logits rel {err:.2e} over {right.shape[0]} steps")
        assert right.shape[0] == STEPS + 1 and err < BOUND
        if L == P:
            continue
        padded = _full(model, kind, torch.cat([prompt[r], toks[:, r]])[None], zr)
        d_pad = _rel(padded[0, M + P - 1:M + P + STEPS], right)
        keep, moved = wpe[L:L + STEPS].clone(), wpe[P:P + STEPS].clone()
        try:
            wpe[L:L + STEPS] = moved
            shifted = _full(model, kind, seq, zr)
        finally:
            wpe[L:L + STEPS] = keep
        d_pos = _rel(shifted[0, M + L - 1:M + L + STEPS], right)
        print(f"{kind} row {r}: wrong positions are {d_pos:.2e} away, attended pads {d_pad:.2e}")
        far_pos, far_pad = max(far_pos, d_pos), max(far_pad, d_pad)
    assert far_pos > 3 * BOUND and far_pad > 3 * BOUND, "the comparison could not tell them apart"


def _plain_from_item_prefill(model, prompt, z, lens, K, max_new):
    """A plain ragged KVDecoder at batch R = B*K whose prefix is the batch-B prefill repeated K
    times (a prefill at batch R sends GEMMs of another M, which may take another kernel).
    Returns (decoder, its first logits [R, V])."""
    from gvl.decode import KVDecoder
    rep = lambda t: None if t is None else t.repeat_interleave(K, 0)
    item = KVDecoder(model, prompt.shape[0], 1)
    first = item.start(prompt, z, lens)
    plain = KVDecoder(model, prompt.shape[0] * K, max_new)
    plain.start(rep(prompt), rep(z), rep(torch.tensor(lens)))
    for l in range(len(plain.cache)):
        plain.cache[l][:, :item.t] = rep(item.cache[l][:, :item.t])
        if plain.kvz is not None:
            plain.kvz[l] = rep(item.kvz[l])
    return plain, rep(first)


@pytest.mark.parametrize("kind", KINDS)
def test_beam_decoder_scripted_parents_ragged_bitwise(cuda, kind):
    from gvl.decode import BeamDecoder
    K = 3
    R = B * K
    model = _tiny(kind)
    prompt, z = _inputs(kind, "rand")
    bd = BeamDecoder(model, B, K, STEPS)
    first = bd.start(prompt, z, LENS)
    plain, first_p = _plain_from_item_prefill(model, prompt, z, LENS, K, STEPS)
    assert bd.prefill_batch == B and torch.equal(first.repeat_interleave(K, 0), first_p)
    assert bd.gap_lo.tolist() == [bd.txt0 + L for L in LENS for _ in range(K)]
    t0 = bd.t
    src = bd.initial_src(cuda)
    g = torch.Generator().manual_seed(5)
    rows = torch.arange(R, device=cuda)
    for s in range(STEPS):
        tok = torch.randint(0, TINY["vocab_size"], (R,), generator=g).to(cuda)
        parent = torch.randint(0, K, (R,), generator=g).to(cuda)
        prow = rows // K * K + parent
        T = t0 + s
        new = src.clone()
        new[:, :T] = src[prow, :T]
        new[:, T] = rows.to(torch.int32)
        src = new
        got = bd.step(tok, src)
        for c in plain.cache:
            c[:, :T] = c[prow, :T]
        want = plain.step(tok)
        assert torch.equal(got, want), f"{kind}: step {s} logits differ from the reordered plain cache"


# |beam raw score + gvl.score sum_nll| per hypothesis of 6 tokens.  SCORE_TOL of
# tests/test_gpu_beam.py covers the fp32 log-sum-exp only; here the two sides also take their bf16 logits from GEMMs of another M and
# from another attention kernel.  Measured on one MI355X for the uniform path (prompt_lens=None,
# same models and seeds, the code path as it was before prompt_lens existed): gpt 1.163e-02,
# linear 1.951e-02, qformer 3.944e-03, cross 1.921e-02; the largest is BEAM_SCORE_UNIFORM and
# the bound is twice that (the margin allows for the different accumulation grouping of the gap
# kernel).  The ragged path measured in the same run: gpt 1.567e-02, linear 4.166e-03, qformer
# 3.944e-03, cross 7.961e-03; the largest is BEAM_SCORE_RAGGED (recorded, not asserted on).
BEAM_SCORE_UNIFORM = 1.951e-2
BEAM_SCORE_RAGGED = 1.567e-2


def _beam_score_diff(model, kind, prompt, z, lens):
    from gvl.decode import beam_search
    from gvl.score import score
    ids, lengths, scores = beam_search(model, prompt, STEPS, z=z, num_beams=3, eos=None,
                                       return_all=True, prompt_lens=lens)
    assert (lengths == STEPS).all() and torch.isfinite(scores).all()
    worst = 0.0
    for r in range(B):
        L = P if lens is None else lens[r]
        seq = torch.cat([prompt[r, :L].expand(3, L), ids[r]], 1)
        mask = torch.zeros_like(seq)
        mask[:, L:] = 1
        zr = None if z is None else z[r:r + 1].expand(3, *z.shape[1:]).contiguous()
        s = score(model, seq, mask, z=zr)
        assert (s.count == STEPS).all()
        worst = max(worst, (scores[r] + s.sum_nll).abs().max().item())
    return worst


@pytest.mark.parametrize("kind", KINDS)
def test_beam_scores_are_the_scores_of_the_unpadded_sequences(cuda, kind):
    model = _tiny(kind)
    prompt, z = _inputs(kind, "rand")
    uniform = _beam_score_diff(model, kind, prompt, z, None)
    ragged = _beam_score_diff(model, kind, prompt, z, list(LENS))
    print(f"{kind}: |beam score + sum_nll| uniform {uniform:.3e}, ragged {ragged:.3e}")
    margins_out(f"ragged_beam_score_{kind}", dict(uniform=uniform, ragged=ragged,
                                                  bound=2 * BEAM_SCORE_UNIFORM))
    assert ragged <= 2 * BEAM_SCORE_UNIFORM


def _control_prompt(pads):
    """Rows over a three-token alphabet so that the n-gram rule has something to ban from the
    first step: row 1 (a b a c a) bans b and c, row 2 (a b c a b c a b) bans c.  The pads repeat
    the same tokens: read as part of the prompt they would ban other tokens."""
    a, b, c = 7, 40, 300
    rows = [[a] + [b, a, c, a, b, c, a], [a, b, a, c, a] + [b, a, c], [a, b, c, a, b, c, a, b]]
    prompt = torch.tensor(rows)
    if pads == "zero":
        for r, L in enumerate(LENS):
            prompt[r, L:] = 0
    return prompt.to(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_controls_see_the_real_sequence(cuda, kind):
    from gvl.decode import generate
    model = _tiny(kind)
    _, z = _inputs(kind)
    kw = dict(z=z, greedy=True, repetition_penalty=1.3, no_repeat_ngram_size=2,
              return_logits=True, prompt_lens=list(LENS))
    prompt = _control_prompt("rand")
    ids, lg = generate(model, prompt, STEPS, **kw)
    ids0, lg0 = generate(model, _control_prompt("zero"), STEPS, **kw)
    assert torch.equal(ids, ids0) and torch.equal(lg, lg0)
    banned_steps = 0
    for r, L in enumerate(LENS):
        for i in range(STEPS):
            seq = prompt[r, :L].tolist() + ids[r, :i].tolist()
            hist = ids[r:r + 1, :max(i, 1)].t().cpu()  # step-major [n_hist, 1]
            want = logits_ref(lg[r:r + 1, i].to(BF).cpu(), hist, i, prompt=prompt[r:r + 1, :L].cpu(),
                              repetition_penalty=1.3, no_repeat_ngram_size=2)
            bans = {v for v in banned_by_ngram(seq, 2) if 0 <= v < lg.shape[-1]}
            banned_steps += bool(bans)
            tok = int(ids[r, i])
            assert tok not in bans and not torch.isinf(want[0, tok]), (kind, r, i, tok, sorted(bans))
            assert tok == int(want.float().argmax()), (kind, r, i)
    print(f"{kind}: {banned_steps} of {B * STEPS} steps had a banned token")
    assert banned_steps >= 2  # rows 1 and 2 at their first step, at the least
