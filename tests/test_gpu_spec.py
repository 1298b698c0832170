"""Speculative decoding on the MI355X (gvl_attn_decode_multi, gvl_ngram_draft, gvl_spec_accept,
KVDecoder.step_multi, gvl.decode.speculative_generate):

  1. every query of gvl_attn_decode_multi has the bits of gvl_attn_decode on the gathered cache;
     what it must not load is NaN; the append writes the new k / v and nothing else;
  2. the draft and accept kernels equal the plain-Python references (tests/spec_ref.py);
  3. step_multi with one token per row has the bits of step();
  4. speculative_generate against generate: greedy with a perfect, a corrupted and a looked-up
     draft, sampling with a shared seed, eos, bad arguments.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import spec_ref as R
from tests.helpers import TINY, margins_out
from tests.sampler_ref import cdf64, draw_ok
from tests.test_gpu_parity_full import GREEDY_BOUND, _build_tiny, _recipe, _z

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"
NAN = float("nan")

# ------------------------------------------------------------------ gvl_attn_decode_multi
KB, KH, KC, KTMAX = 4, 2, 128, 272
# the edges of the 32-row value sweep and of the 256-thread key loop
KV_LENS = {"low": (0, 1, 31, 32), "high": (33, 255, 256, 257)}


@functools.lru_cache(maxsize=None)
def _multi_inputs(Q, which):
    """(qkv [B, Q, 3C], cache [B, Tmax, 3C], kv_len).  In the cache, the q columns and every
    column from kv_len[b] on are NaN: the launch may load neither."""
    g = torch.Generator(device="cuda").manual_seed(10 * Q + len(which))
    qkv = torch.randn(KB, Q, 3 * KC, device=DEV, generator=g).to(BF)
    cache = torch.randn(KB, KTMAX, 3 * KC, device=DEV, generator=g).to(BF)
    kv_len = torch.tensor(KV_LENS[which], dtype=torch.int32, device=DEV)
    cache[:, :, :KC] = NAN
    t = torch.arange(KTMAX, device=DEV)[None, :]
    cache[(t >= kv_len[:, None].long())] = NAN
    return qkv, cache, kv_len


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("which", list(KV_LENS))
@pytest.mark.parametrize("Q", [1, 2, 5])
def test_attn_decode_multi_bits_nan_and_append(cuda, Q, which):
    import gvl.kernels as Kn
    qkv, cache0, kv_len = _multi_inputs(Q, which)
    cache = cache0.clone()
    out = Kn.attn_decode_multi(qkv, cache, kv_len, KH)
    assert out.shape == (KB * Q, KC) and torch.isfinite(out).all()
    # the cache a one-query decode would see: the old columns, then this step's rows
    gath = torch.zeros(KB, KTMAX, 3 * KC, dtype=BF, device=DEV)
    want_cache = cache0.clone()
    for b, L in enumerate(KV_LENS[which]):
        gath[b, :L] = cache0[b, :L]
        gath[b, L:L + Q] = qkv[b]
        want_cache[b, L:L + Q, KC:] = qkv[b, :, KC:]
    gath[:, :, :KC] = 0
    for b, L in enumerate(KV_LENS[which]):
        for j in range(Q):
            Tk = L + j + 1
            one = Kn.attn_decode(qkv[b:b + 1, j, :KC], gath[b:b + 1, :Tk, KC:2 * KC],
                                 gath[b:b + 1, :Tk, 2 * KC:], KH)
            assert torch.equal(out[b * Q + j], one[0]), (b, L, j)
    # the append, and every other cache element keeps its (NaN or random) bits
    assert torch.equal(_bits(cache), _bits(want_cache))
    # finite values where the NaNs were change no output bit
    clean = torch.nan_to_num(cache0, nan=1.5)
    assert torch.equal(Kn.attn_decode_multi(qkv, clean, kv_len, KH), out)
    # query j loads no qkv row of a later query
    if Q > 2:
        q2 = qkv.clone()
        q2[:, 2:] = NAN
        o2 = Kn.attn_decode_multi(q2, cache0.clone(), kv_len, KH).view(KB, Q, KC)
        assert torch.equal(o2[:, :2], out.view(KB, Q, KC)[:, :2])


def test_attn_decode_multi_clamps_a_bad_table(cuda):
    """kv_len outside [0, Tmax - Q] is clamped, so a bad table writes inside the cache."""
    import gvl.kernels as Kn
    Q = 3
    qkv, _, _ = _multi_inputs(Q, "low")
    big = torch.randn(KB, 20, 3 * KC, device=DEV).to(BF)  # the cache is its first 16 columns
    orig, guard = big.clone(), big.clone()
    kv_len = torch.tensor([-5, 13, 14, 10 ** 6], dtype=torch.int32, device=DEV)
    out = Kn.attn_decode_multi(qkv, big[:, :16], kv_len, KH)
    good = torch.tensor([0, 13, 13, 13], dtype=torch.int32, device=DEV)
    assert torch.equal(out, Kn.attn_decode_multi(qkv, guard[:, :16], good, KH))
    assert torch.equal(_bits(big), _bits(guard))
    assert torch.equal(_bits(big[:, 16:]), _bits(orig[:, 16:]))  # nothing past Tmax is written


def test_multi_bad_arguments(cuda):
    import gvl.kernels as Kn
    from gvl._lib import GvlError
    lib = Kn._L()
    cache = torch.zeros(1, 16, 3 * KC, dtype=BF, device=DEV)
    kv = torch.zeros(1, dtype=torch.int32, device=DEV)
    o = torch.zeros(16, KC, dtype=BF, device=DEV)
    call = lambda Q, kvp: lib.gvl_attn_decode_multi(cache.data_ptr(), cache.data_ptr(),
                                                    cache.stride(0), 16, kvp, o.data_ptr(), KC, 1,
                                                    KH, Q, 0.125, None)
    assert call(0, kv.data_ptr()) == -1 and b"Q=0" in lib.gvl_last_error()
    assert call(9, kv.data_ptr()) == -1 and b"Q=9" in lib.gvl_last_error()
    assert call(2, None) == -1 and b"kv_len" in lib.gvl_last_error()
    with pytest.raises(GvlError, match="Q=9"):
        Kn.attn_decode_multi(torch.zeros(1, 9, 3 * KC, dtype=BF, device=DEV), cache, kv, KH)


# ------------------------------------------------------------------ draft and accept
V5 = 5


def _draft_gpu(prompt, plen, emitted, n, ngram, D, given):
    import gvl.kernels as Kn
    dv = lambda x, dt: torch.tensor(x, dtype=dt, device=DEV)
    return Kn.ngram_draft(dv(prompt, torch.int64), dv(plen, torch.int32),
                          dv(emitted, torch.int64), dv(n, torch.int32), ngram, D,
                          given=None if given is None else dv(given, torch.int64)).tolist()


@pytest.mark.parametrize("ngram,D", [(1, 1), (2, 4), (3, 4), (4, 7)])
def test_ngram_draft_equals_reference_on_random_rows(cuda, ngram, D):
    rng = np.random.default_rng(100 * ngram + D)
    B, P, n_new = 96, 12, 10
    prompt = rng.integers(0, V5, (B, P)).tolist()
    emitted = rng.integers(0, V5, (B, n_new)).tolist()
    plen = rng.integers(1, P + 1, B).tolist()
    n = rng.integers(0, n_new + 1, B).tolist()  # n == n_new: a finished row
    given = np.where(rng.random((B, n_new)) < 0.3, rng.integers(0, V5, (B, n_new)), -1).tolist()
    for gv in (None, given):
        got = _draft_gpu(prompt, plen, emitted, n, ngram, D, gv)
        want = [R.ngram_draft(prompt[b][:plen[b]], emitted[b][:n[b]], ngram, D, n_new,
                              None if gv is None else gv[b]) for b in range(B)]
        assert got == want
        flat = [d for row in want for d in row]
        assert -1 in flat and any(d >= 0 for d in flat)  # both kinds of entry occur


def test_ngram_draft_named_cases(cuda):
    P, n_new = 700, 6
    far = list(range(1000, 1000 + P))  # only match: the very start, two key sweeps away
    rows = [  # (prompt, plen, emitted, what)
        ([5, 6, 7, 8], 4, [6], "a match only at g = 1"),
        ([1, 2, 3, 9], 3, [4], "no match at all (the pad 9 is not part of the row)"),
        ([4, 4], 2, [], "the continuation runs into the end"),
        ([4], 1, [], "a single token"),
        (far, P, [1000, 1001], "the latest match is the first position"),
        ([3, 3, 3, 3, 3, 3], 6, [3, 3, 3, 3, 3, 3], "finished"),
    ]
    prompt = [r[0] + [0] * (P - len(r[0])) for r in rows]
    emitted = [r[2] + [0] * (n_new - len(r[2])) for r in rows]
    plen, n = [r[1] for r in rows], [len(r[2]) for r in rows]
    got = _draft_gpu(prompt, plen, emitted, n, 3, 3, None)
    want = [R.ngram_draft(r[0][:r[1]], r[2], 3, 3, n_new) for r in rows]
    assert want == [[7, 8, 6], [-1] * 3, [4, -1, -1], [-1] * 3, [1002, 1003, 1004], [-1] * 3]
    assert got == want
    given = [[-1, 30, -1, 50, 60, -1]] * len(rows)
    got = _draft_gpu(prompt, plen, emitted, n, 3, 3, given)
    assert got == [R.ngram_draft(r[0][:r[1]], r[2], 3, 3, n_new, given[0]) for r in rows]
    assert got[0] == [30, 8, 50] and got[5] == [-1] * 3


STATE = ("n", "kv_len", "pos", "lengths", "drafted", "accepted")


def _accept_gpu(x, draft, st, n_new, eos):
    import gvl.kernels as Kn
    t = {k: torch.tensor(st[k], dtype=torch.int32, device=DEV) for k in STATE}
    last = torch.tensor(st["last"], dtype=torch.int64, device=DEV)
    out = torch.tensor(st["out"], dtype=torch.int64, device=DEV)
    xd = torch.tensor(x, dtype=torch.int64, device=DEV)
    dd = torch.tensor(draft, dtype=torch.int64, device=DEV) if len(x[0]) > 1 else None
    Kn.spec_accept(xd, dd, t["n"], t["kv_len"], t["pos"], t["lengths"], last, out,
                   None if eos < 0 else eos, t["drafted"], t["accepted"])
    got = {k: t[k].tolist() for k in STATE}
    got.update(last=last.tolist(), out=out.tolist())
    return got


ACCEPT_B, ACCEPT_N_NEW = 256, 12


def _accept_case(Q, eos):
    """Random rows over five tokens: (x, draft, state before, state after by the reference)."""
    rng = np.random.default_rng(10 * Q + eos + 1)
    B, n_new = ACCEPT_B, ACCEPT_N_NEW
    x = rng.integers(0, V5, (B, Q))
    draft = np.where(rng.random((B, Q - 1)) < 0.85, x[:, :Q - 1], rng.integers(-1, V5, (B, Q - 1)))
    x, draft = x.tolist(), draft.tolist()
    st = dict(n=rng.integers(0, n_new + 1, B).tolist(), kv_len=rng.integers(0, 50, B).tolist(),
              pos=rng.integers(0, 50, B).tolist(), lengths=[n_new] * B,
              last=rng.integers(0, V5, B).tolist(), drafted=rng.integers(0, 9, B).tolist(),
              accepted=rng.integers(0, 9, B).tolist(), out=[[-9] * n_new for _ in range(B)])
    after = {k: [list(r) for r in v] if k == "out" else list(v) for k, v in st.items()}
    R.spec_accept(x, draft, after, n_new, eos)
    return x, draft, st, after


def _accept_coverage(Q, eos, x, draft, before, after):
    """The random rows hold what the kernel has to get right: finished rows; for Q > 2 accept
    counts 0, partial and full and a row clipped at n_new; with eos, a row ended after at least
    one accepted token."""
    B, n_new = ACCEPT_B, ACCEPT_N_NEW
    assert any(before["n"][b] == n_new for b in range(B))
    if Q > 2:
        gain = [after["accepted"][b] - before["accepted"][b] for b in range(B)]
        live = [b for b in range(B) if before["n"][b] < n_new]
        assert any(gain[b] == 0 for b in live) and Q - 1 in gain
        assert any(0 < a < Q - 1 for a in gain)
        lead = lambda b: next((j for j in range(Q - 1) if draft[b][j] != x[b][j]), Q - 1)
        assert any(lead(b) + 1 > n_new - before["n"][b] and after["lengths"][b] == n_new
                   for b in live)  # more confirmed than n_new leaves room for
        if eos >= 0:
            assert any(after["lengths"][b] - before["n"][b] >= 2 for b in live
                       if after["lengths"][b] < n_new)


@pytest.mark.parametrize("eos", [-1, 3])
@pytest.mark.parametrize("Q", [1, 2, 5, 8])
def test_spec_accept_equals_reference_on_random_rows(cuda, Q, eos):
    x, draft, st, want = _accept_case(Q, eos)
    _accept_coverage(Q, eos, x, draft, st, want)
    got = _accept_gpu(x, draft, st, ACCEPT_N_NEW, eos)
    assert got == want
    for b in range(ACCEPT_B):  # finished rows untouched
        if st["n"][b] == ACCEPT_N_NEW:
            assert all(got[k][b] == st[k][b] for k in st), b


# ------------------------------------------------------------------ decoder and generate
KINDS = ("gpt", "linear", "cross")
B, P, LENS, N_NEW, DL = 3, 12, (5, 9, 12), 24, 4
# Prompt seeds for which generate() alone keeps every top-1/top-2 margin of all three rows at or
# above GREEDY_BOUND over the 24 tokens (measured on one MI355X: the smallest margins are 0.035
# (gpt), 0.035 (linear), 0.035 (cross), profiles/spec_margins.json; every run records them again
# through margins_out as spec_generate_margins_<kind>).
SEEDS = {"gpt": 83, "linear": 11, "cross": 44}


@functools.lru_cache(maxsize=None)
def _tiny(kind):
    model, _ = _recipe(_build_tiny(kind), torch.device(DEV))
    return model.eval()


def _prompt(seed):
    """Right-padded prompts [B, P]: row r is a block of four tokens over and over, cut at
    LENS[r]; the pads are other valid ids."""
    g = torch.Generator().manual_seed(1000 + seed)
    V = TINY["vocab_size"]
    block = torch.randint(0, V, (B, 4), generator=g)
    prompt = block.repeat(1, P // 4)
    fill = torch.randint(0, V, (B, P), generator=g)
    for r, L in enumerate(LENS):
        prompt[r, L:] = fill[r, L:]
    return prompt.to(DEV)


def _zin(kind):
    return None if kind == "gpt" else _z(3, B, TINY["n_embd"], torch.device(DEV))


def _margins(lg):
    top2 = lg.float().topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _greedy_case(kind, seed=None):
    """(prompt, z, generate's greedy ids [B, N_NEW], per-row count of leading tokens whose margin
    is at least GREEDY_BOUND)."""
    from gvl.decode import generate
    seed = SEEDS[kind] if seed is None else seed
    prompt, z = _prompt(seed), _zin(kind)
    ids, lg = generate(_tiny(kind), prompt, N_NEW, z=z, greedy=True, return_logits=True,
                       prompt_lens=list(LENS))
    marg = _margins(lg)
    safe = [int(np.argmax(m < GREEDY_BOUND)) if (m < GREEDY_BOUND).any() else N_NEW for m in marg]
    margins_out(f"spec_generate_margins_{kind}", dict(seed=seed, min_margin=marg.min(1).tolist(),
                                                      compared=safe, bound=GREEDY_BOUND))
    return prompt, z, ids, safe


def _same_up_to_low_margin(kind, got, want, safe, what):
    """Row r equals generate's up to its first position whose margin is below GREEDY_BOUND, and
    at least 2 of the 3 rows compare over all N_NEW tokens."""
    assert sum(s == N_NEW for s in safe) >= 2, f"{kind}: generate's own margins {safe}"
    for r, s in enumerate(safe):
        assert torch.equal(got[r, :s], want[r, :s]), (kind, what, r, got[r].tolist(),
                                                      want[r].tolist())


def _spec(kind, prompt, z, **kw):
    from gvl.decode import speculative_generate
    return speculative_generate(_tiny(kind), prompt, N_NEW, z=z, draft_len=DL,
                                prompt_lens=list(LENS), return_stats=True, **kw)


def _predict(prompt, out, given, eos=-1):
    """spec_ref's rounds for rows that emit `out` whatever is drafted."""
    prompts = [prompt[r, :L].tolist() for r, L in enumerate(LENS)]
    return R.simulate(out.tolist(), None if given is None else given.tolist(), DL, eos=eos,
                      prompts=prompts, ngram=3)


@pytest.mark.parametrize("kind", ["gpt", "cross"])
def test_step_multi_of_one_token_is_step_bitwise(cuda, kind):
    from gvl.decode import KVDecoder
    model = _tiny(kind)
    prompt, z = _prompt(7), _zin(kind)
    toks = torch.randint(0, TINY["vocab_size"], (3, B), generator=torch.Generator().manual_seed(3))
    toks = toks.to(cuda)
    a, b = KVDecoder(model, B, 3), KVDecoder(model, B, 3)
    b.slack = 1
    first = a.start(prompt, z)
    assert torch.equal(first, b.start(prompt, z))
    kv_len = torch.full((B,), P, dtype=torch.int32, device=cuda)
    pos = kv_len.clone()
    for s in range(3):
        want = a.step(toks[s])
        got = b.step_multi(toks[s].view(B, 1), kv_len, pos)
        assert torch.equal(got, want), s
        for l in range(len(a.cache)):
            assert torch.equal(a.cache[l][:, P + s, 128:], b.cache[l][:, P + s, 128:])
        kv_len += 1
        pos += 1


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_perfect_draft(cuda, kind):
    prompt, z, ids, safe = _greedy_case(kind)
    got, st = _spec(kind, prompt, z, greedy=True, draft_ids=ids)
    print(f"{kind}: steps {st['steps']}, accepted {st['accepted'].tolist()} of "
          f"{st['drafted'].tolist()}, rows compared over {safe}")
    _same_up_to_low_margin(kind, got, ids, safe, "perfect")
    assert st["steps"] == math.ceil((N_NEW - 1) / (DL + 1)) + 1
    want = _predict(prompt, got, ids)
    assert st["accepted"].tolist() == want["accepted"] and st["drafted"].tolist() == want["drafted"]


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_corrupted_draft(cuda, kind):
    prompt, z, ids, safe = _greedy_case(kind)
    V = TINY["vocab_size"]
    given = ids.clone()
    for r, wrong, none in ((0, (3, 4, 17), (9,)), (1, (1,), (2, 3, 20)), (2, (23,), ())):
        for i in wrong:
            given[r, i] = (given[r, i] + 1 + r) % V  # a different valid id
        for i in none:
            given[r, i] = -1
    got, st = _spec(kind, prompt, z, greedy=True, draft_ids=given)
    _same_up_to_low_margin(kind, got, ids, safe, "corrupted")
    want = _predict(prompt, got, given)
    print(f"{kind}: steps {st['steps']}, accepted {st['accepted'].tolist()} of "
          f"{st['drafted'].tolist()}; predicted {want['accepted']} in {want['steps']} steps")
    assert st["accepted"].tolist() == want["accepted"]
    assert st["drafted"].tolist() == want["drafted"] and st["steps"] == want["steps"]
    assert st["steps"] > math.ceil((N_NEW - 1) / (DL + 1)) + 1  # the corruption costs passes


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_lookup(cuda, kind):
    prompt, z, ids, safe = _greedy_case(kind)
    got, st = _spec(kind, prompt, z, greedy=True, ngram=3)
    _same_up_to_low_margin(kind, got, ids, safe, "lookup")
    acc, dr = int(st["accepted"].sum()), int(st["drafted"].sum())
    print(f"{kind}: lookup accepted {acc} of {dr} guesses ({acc / max(dr, 1):.2f}) in "
          f"{st['steps']} steps for {B * N_NEW} tokens")
    want = _predict(prompt, got, None)
    assert st["accepted"].tolist() == want["accepted"] and st["steps"] == want["steps"]


@pytest.mark.parametrize("kind", KINDS)
def test_sampling_with_a_shared_seed(cuda, kind):
    from gvl.decode import generate
    prompt, z = _prompt(SEEDS[kind]), _zin(kind)
    kw = dict(temperature=0.8, top_p=0.9)
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)
    ids, lg = generate(_tiny(kind), prompt, N_NEW, z=z, generator=gen(), return_logits=True,
                       prompt_lens=list(LENS), **kw)
    g = gen()
    u = torch.stack([torch.rand(B, generator=g, device=cuda) for _ in range(N_NEW)], 1).cpu()
    got, st = _spec(kind, prompt, z, generator=gen(), draft_ids=ids, **kw)
    same = []
    for r in range(B):
        diff = (got[r] != ids[r]).nonzero()
        i = int(diff[0]) if diff.numel() else N_NEW
        same.append(i)
        if i < N_NEW:  # the rounding allowance of the sampler tests, at the first difference
            dist = O.sampling_distribution(lg[r, i].double().cpu().numpy(), 0.8, 0, 0.9)
            tok, ui = got[r, i:i + 1].cpu().numpy(), u[r, i:i + 1].numpy()
            assert draw_ok(dist, cdf64(dist), tok, ui)[0], (kind, r, i, int(tok[0]), float(ui[0]))
    print(f"{kind}: sampled rows equal generate's over {same} of {N_NEW} tokens; steps "
          f"{st['steps']}")


@pytest.mark.parametrize("kind", KINDS)
def test_eos_mid_sequence(cuda, kind):
    from gvl.decode import generate
    prompt, z, ids, safe = _greedy_case(kind)
    rows = ids.tolist()
    # the first token some row emits for the first time at index 4 or later: mid-sequence, and
    # with a perfect draft in the middle of an accepted run
    r0, i0 = next((r, i) for r in range(B) for i in range(4, 20) if rows[r][i] not in rows[r][:i])
    eos = rows[r0][i0]
    want, wlen = generate(_tiny(kind), prompt, N_NEW, z=z, greedy=True, eos=eos,
                          return_lengths=True, prompt_lens=list(LENS))
    assert int(wlen[r0]) == i0 + 1
    from gvl.decode import speculative_generate
    for draft in (ids, None):
        got, glen, st = speculative_generate(_tiny(kind), prompt, N_NEW, z=z, draft_len=DL,
                                             greedy=True, eos=eos, draft_ids=draft,
                                             prompt_lens=list(LENS), return_lengths=True,
                                             return_stats=True)
        assert glen.dtype == torch.int32
        assert sum(s == N_NEW for s in safe) >= 2
        for r, s in enumerate(safe):
            if int(wlen[r]) <= s or s == N_NEW:  # ended before any low margin: the whole row
                assert torch.equal(got[r], want[r]) and int(glen[r]) == int(wlen[r]), (kind, r)
                assert (got[r, int(glen[r]):] == eos).all()
            else:
                assert torch.equal(got[r, :s], want[r, :s]), (kind, r)
        print(f"{kind}: eos {eos}: lengths {glen.tolist()} in {st['steps']} steps")


def test_arguments(cuda):
    import gvl
    from gvl import decode
    assert gvl.speculative_generate is decode.speculative_generate
    model = _tiny("gpt")
    prompt = _prompt(0)
    for kw in (dict(draft_len=0), dict(draft_len=8),
               dict(draft_ids=torch.zeros(B, N_NEW + 1, dtype=torch.int64, device=cuda)),
               dict(draft_ids=torch.zeros(B + 1, N_NEW, dtype=torch.int64, device=cuda))):
        with pytest.raises(ValueError):
            decode.speculative_generate(model, prompt, N_NEW, greedy=True, **kw)
    with pytest.raises(ValueError, match="block_size"):
        decode.speculative_generate(model, prompt, TINY["block_size"], greedy=True)
    # without prompt_lens, without stats: the ids alone, equal to the uniform-length generate
    # and one row alone (a [1, n] tensor may report any row stride), its own output as the draft
    for rows in (B, 1):
        ids, lg = decode.generate(model, prompt[:rows], 8, greedy=True, return_logits=True)
        got = decode.speculative_generate(model, prompt[:rows], 8, greedy=True, draft_len=7,
                                          draft_ids=ids if rows == 1 else None)
        safe = _margins(lg) >= GREEDY_BOUND
        for r in range(rows):
            s = 8 if safe[r].all() else int(np.argmin(safe[r]))
            assert torch.equal(got[r, :s], ids[r, :s])
