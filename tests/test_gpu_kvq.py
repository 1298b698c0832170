"""The int8 KV cache on the MI355X (include/gvl.h gvl_kv_quantize_i8, gvl_attn_decode_q8;
kv_cache="int8" in gvl/decode.py) against tests/kvq_ref.py.

  quantiser   bit for bit the CPU quantiser, on strided rows, at a column offset, nothing else
              written;
  attention   every element of o against the float64 reference attention(q, fp64(kq) * ks,
              fp64(vq) * vs) under test_attn_decode_per_element's bound: 2 units of 2**-8 E (one
              bf16 rounding on the way to o, so one in hand) + 4 x the fp32 baseline; the appended
              column equals the bulk quantiser's bytes; nothing else is written;
  policies    src, gap and t_dev against the plain instance, bit for bit;
  decoders    cache contents, eager = graph, ragged, caption / cross-att, with int8 weights;
  accuracy    the logits against an fp32 restatement that fake-quantises k and v, held to twice
              the bf16 cache's own error against the restatement without it.
The measured figures go to profiles/kvq_margins.json through helpers.margins_out."""
import functools

import pytest
import torch

from tests import attn_ref as A
from tests import kvq_ref as R
from tests.helpers import TINY, assert_attn_close, margins_out
from tests.test_gpu_parity_full import _build_tiny, _recipe, _z

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
H, C, B = 3, 192, 2
SENT8 = 0x55

_MARGINS = {}


def _record(key, rec):
    _MARGINS[key] = rec
    margins_out("kvq_margins", _MARGINS)


def _k():
    from gvl import kernels as K
    return K


class _Buf:
    """A tensor of any dtype at a 64-byte offset inside a byte buffer of 0xA5 sentinels on the
    device; check() compares every byte outside the owned elements with what it was."""

    def __init__(self, init, cuda):
        self.init = init.contiguous()
        raw = self.init.view(-1).view(torch.uint8)
        n = raw.numel()
        big = torch.full((n + 128,), 0xA5, dtype=torch.uint8)
        big[64:64 + n] = raw
        self.big, self.n = big.to(cuda), n
        self.t = self.big[64:64 + n].view(init.dtype).view(init.shape)

    def _bytes(self, t):
        return t.contiguous().view(-1).view(torch.uint8)

    def check(self, owned=None, name="buffer"):
        """owned: bool tensor of init's shape, the elements the kernel may have written."""
        big = self.big.cpu()
        assert (big[:64] == 0xA5).all() and (big[64 + self.n:] == 0xA5).all(), \
            f"a store outside the {name}"
        keep = torch.ones(self.n, dtype=torch.bool)
        if owned is not None:
            assert owned.shape == self.init.shape
            keep = ~owned.reshape(-1, 1).expand(-1, self.init.element_size()).reshape(-1)
        assert torch.equal(big[64:64 + self.n][keep], self._bytes(self.init)[keep]), \
            f"a store next to the owned part of the {name}"


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(-1).view(torch.uint8),
                                              b.view(-1).view(torch.uint8))


# ------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("col0", [0, 3])
@pytest.mark.parametrize("S", [1, 5])
def test_kv_quantize_equals_the_reference(cuda, S, col0):
    """B = 2, H = 3, the sequences a [:, 0] view of [B, 2, ...] (qkv, kv8 and kvs alike); head
    vectors scaled over 12 binades, one of them zero.  The q third is NaN: never read."""
    Tmax = col0 + S + 2
    g = torch.Generator().manual_seed(100 * S + col0)
    qkv = torch.randn(B, 2, S, 3 * C, generator=g)
    scale = torch.exp2(torch.randint(-6, 7, (B, 2, S, 3 * H), generator=g).float())
    qkv = (qkv.view(B, 2, S, 3 * H, 64) * scale[..., None]).view(B, 2, S, 3 * C)
    qkv[1, 0, S - 1, C + 64:C + 128] = 0
    qkv[..., :C] = NAN
    qkv = qkv.to(BF)
    kv8 = _Buf(torch.full((B, 2, Tmax, 2 * C), SENT8, dtype=torch.int8), cuda)
    kvs = _Buf(torch.full((B, 2, Tmax, 2 * H), NAN), cuda)
    _k().kv_quantize_i8(qkv.to(cuda)[:, 0], kv8.t[:, 0], kvs.t[:, 0], H, col0=col0)
    torch.cuda.synchronize()
    want8, wants = R.quantize_kv(qkv[:, 0], H)
    assert float(wants[1, S - 1, 1]) == 0.0
    assert torch.equal(kv8.t[:, 0, col0:col0 + S].cpu(), want8)
    assert _same_bits(kvs.t[:, 0, col0:col0 + S], wants)
    own = torch.zeros(B, 2, Tmax, 1, dtype=torch.bool)
    own[:, 0, col0:col0 + S] = True
    kv8.check(own.expand(-1, -1, -1, 2 * C), "kv8")
    kvs.check(own.expand(-1, -1, -1, 2 * H), "kvs")


# ------------------------------------------------------------------------------ attention
class _Step:
    """Device buffers of one step of kvq_ref.case(Tk) at column tc = Tk - 1: the cached columns
    hold the CPU quantiser's bytes, every other column sentinels (kv8) and NaN (kvs), o is a NaN
    slice of a wider buffer."""

    def __init__(self, cuda, Tk, Tmax=None):
        self.c = c = R.case(Tk)
        self.Tk, self.tc = Tk, Tk - 1
        self.Tmax = Tmax = min(Tk + 2, 4096) if Tmax is None else Tmax
        k8 = torch.full((B, Tmax, 2 * C), SENT8, dtype=torch.int8)
        ks = torch.full((B, Tmax, 2 * H), NAN)
        k8[:, :Tk - 1], ks[:, :Tk - 1] = c["kv8"], c["kvs"]
        self.kv8, self.kvs = _Buf(k8, cuda), _Buf(ks, cuda)
        self.qkv = _Buf(c["qkv"], cuda)
        self.o = _Buf(torch.full((B, C + 128), NAN, dtype=BF), cuda)

    def run(self, t=None, **kw):
        out = self.o.t[:, 64:64 + C]
        _k().attn_decode_q8(self.qkv.t, self.kv8.t, self.kvs.t, self.tc if t is None else t, H,
                            out=out, **kw)
        torch.cuda.synchronize()
        return out.cpu()

    def check_rest(self, wrote=True):
        """Only column tc of the cache and the o slice were written (wrote=False: nothing)."""
        col = torch.zeros(B, self.Tmax, 1, dtype=torch.bool)
        col[:, self.tc] = wrote
        self.kv8.check(col.expand(-1, -1, 2 * C), "kv8")
        self.kvs.check(col.expand(-1, -1, 2 * H), "kvs")
        self.qkv.check(None, "qkv")
        own = torch.zeros(B, C + 128, dtype=torch.bool)
        own[:, 64:64 + C] = wrote
        self.o.check(own, "o")


@functools.lru_cache(maxsize=None)
def _ref(Tk):
    return R.case_ref(R.case(Tk), H)


@pytest.mark.parametrize("Tk", [1, 31, 32, 33, 255, 256, 257, 4096])
def test_attn_decode_q8_per_element(cuda, Tk):
    st = _Step(cuda, Tk)
    got = st.run()
    st.check_rest()
    o, E = _ref(Tk)
    r = assert_attn_close(got.reshape(B, H, 1, 64), o, E, A.HARD_UNITS["o"],
                          name=f"decode_q8 Tk={Tk}", slack=4 * A.baseline()["o"])
    _record(f"decode_q8 Tk={Tk}", dict(kernel=dict(o=r), bound=dict(o=A.HARD_UNITS["o"])))
    # the appended column: the CPU quantiser's and the bulk quantiser's bytes
    c = st.c
    assert torch.equal(st.kv8.t[:, st.tc].cpu(), c["all8"][:, st.tc])
    assert _same_bits(st.kvs.t[:, st.tc], c["alls"][:, st.tc])
    b8 = torch.full((B, 1, 2 * C), SENT8, dtype=torch.int8, device=cuda)
    bs = torch.full((B, 1, 2 * H), NAN, device=cuda)
    _k().kv_quantize_i8(st.qkv.t.view(B, 1, 3 * C), b8, bs, H)
    assert torch.equal(b8[:, 0], st.kv8.t[:, st.tc]) and _same_bits(bs[:, 0], st.kvs.t[:, st.tc])


# ------------------------------------------------------------------------------- policies
@pytest.mark.parametrize("Tk", [1, 37, 257])
def test_identity_src_and_empty_gap_are_the_plain_instance(cuda, Tk):
    want = _Step(cuda, Tk).run()
    ident = torch.arange(B, dtype=torch.int32, device=cuda).view(B, 1).expand(B, Tk + 2).contiguous()
    empty = torch.full((B,), Tk // 2, dtype=torch.int32, device=cuda)
    for kw in (dict(src=ident), dict(gap_lo=empty, gap_hi=Tk // 2),
               dict(src=ident, gap_lo=empty, gap_hi=Tk // 2)):
        st = _Step(cuda, Tk)
        assert _same_bits(st.run(**kw), want), sorted(kw)
        st.check_rest()


@pytest.mark.parametrize("Tk", [9, 257])
def test_permuted_src_is_the_gathered_cache(cuda, Tk):
    g = torch.Generator().manual_seed(Tk)
    src = torch.randint(0, B, (B, Tk + 2), generator=g, dtype=torch.int32)
    src[:, Tk - 1] = torch.arange(B)
    assert not torch.equal(src[:, :Tk - 1], torch.arange(B).view(B, 1).expand(B, Tk - 1).int())
    st = _Step(cuda, Tk)
    got = st.run(src=src.to(cuda))
    st.check_rest()
    gat = _Step(cuda, Tk)
    idx = src[:, :Tk - 1].long().to(cuda)
    for buf in (gat.kv8, gat.kvs):
        w = buf.t.shape[2]
        buf.t[:, :Tk - 1] = torch.gather(buf.t[:, :Tk - 1].clone(), 0,
                                         idx[:, :, None].expand(-1, -1, w))
    assert _same_bits(gat.run(), got)
    o, E = R.case_ref(st.c, H, src=src[:, :Tk])
    assert_attn_close(got.reshape(B, H, 1, 64), o, E, A.HARD_UNITS["o"], name=f"src Tk={Tk}",
                      slack=4 * A.baseline()["o"])
    assert not _same_bits(got, _Step(cuda, Tk).run())


@pytest.mark.parametrize("use_src", [False, True], ids=["plain", "src"])
@pytest.mark.parametrize("Tk", [37, 300])
def test_gap_columns_are_never_loaded(cuda, Tk, use_src):
    """Gap columns hold arbitrary bytes in kv8 and NaN in kvs: the output has the bits of the
    same gap over clean columns, and meets the reference that leaves the gap out."""
    lo = torch.tensor([3, Tk - 5], dtype=torch.int32)
    hi = Tk - 2
    kw = dict(gap_lo=lo.to(cuda), gap_hi=hi)
    if use_src:  # (the rows of a two-row cache swapped at every odd position)
        src = torch.arange(B).view(B, 1).expand(B, Tk + 2).clone().int()
        src[:, 1:Tk - 1:2] = 1 - src[:, 1:Tk - 1:2]
        kw["src"] = src.to(cuda)
    clean = _Step(cuda, Tk)
    want = clean.run(**kw)
    dirty = _Step(cuda, Tk)
    skip = torch.zeros(B, Tk, dtype=torch.bool)
    for b in range(B):
        skip[b, int(lo[b]):hi] = True
    # dirty every cached cell (row, column) that no sequence reads
    rows = kw["src"].cpu().long() if use_src else torch.arange(B).view(B, 1).expand(B, Tk + 2)
    read = torch.zeros(B, Tk - 1, dtype=torch.bool)
    for b in range(B):
        cols = (~skip[b, :Tk - 1]).nonzero().view(-1)
        read[rows[b, cols], cols] = True
    assert (~read).sum() >= 3
    unread = (~read).to(cuda)
    dirty.kv8.t[:, :Tk - 1][unread] = 0x7B
    dirty.kvs.t[:, :Tk - 1][unread] = NAN
    dirty.kv8.init, dirty.kvs.init = dirty.kv8.t.cpu().clone(), dirty.kvs.t.cpu().clone()
    got = dirty.run(**kw)
    dirty.check_rest()
    assert _same_bits(got, want) and torch.isfinite(got.float()).all()
    o, E = R.case_ref(clean.c, H, skip=skip, src=kw["src"].cpu()[:, :Tk] if use_src else None)
    assert_attn_close(got.reshape(B, H, 1, 64), o, E, A.HARD_UNITS["o"], name=f"gap Tk={Tk}",
                      slack=4 * A.baseline()["o"])


@pytest.mark.parametrize("Tk", [1, 37])
def test_all_skipped_row_writes_zeros(cuda, Tk):
    st = _Step(cuda, Tk)
    lo = torch.tensor([0, Tk], dtype=torch.int32, device=cuda)  # row 0: everything, row 1: nothing
    got = st.run(gap_lo=lo, gap_hi=Tk)
    st.check_rest()
    assert not got[0].float().any() and (got[0].view(torch.int16) == 0).all()
    assert _same_bits(got[1], _Step(cuda, Tk).run()[1])


@pytest.mark.parametrize("Tk", [1, 37, 257])
def test_t_dev_gives_the_bits_of_t(cuda, Tk):
    want_st = _Step(cuda, Tk)
    want = want_st.run()
    st = _Step(cuda, Tk)
    got = st.run(t=torch.tensor([Tk - 1], dtype=torch.int32, device=cuda))
    st.check_rest()
    assert _same_bits(got, want)
    assert torch.equal(st.kv8.t.cpu(), want_st.kv8.t.cpu()) and _same_bits(st.kvs.t, want_st.kvs.t)


@pytest.mark.parametrize("tc", ["Tmax", -1])
def test_a_column_outside_the_cache_writes_nothing(cuda, tc):
    st = _Step(cuda, 37)
    t = st.Tmax if tc == "Tmax" else tc
    st.run(t=torch.tensor([t], dtype=torch.int32, device=cuda))
    st.check_rest(wrote=False)
    st.run(t=t)  # and the same column from the host
    st.check_rest(wrote=False)


def test_attn_decode_q8_refuses_a_long_cache(cuda):
    from gvl._lib import GvlError
    st = _Step(cuda, 5, Tmax=4097)
    with pytest.raises(GvlError, match="4097"):
        st.run()
    st.check_rest(wrote=False)


# ------------------------------------------------------------------ decoder level
TINY256 = dict(block_size=64, vocab_size=256, n_layer=2, n_head=2, n_embd=128)
DB, DP, STEPS = 3, 8, 6
LENS = (3, 8, 5)


@functools.lru_cache(maxsize=None)
def _gpt():
    import gvl.gpt2 as g2
    model, _ = _recipe(g2.GPT(g2.GPTConfig(**TINY256)), torch.device("cuda:0"))
    return model.eval()


@functools.lru_cache(maxsize=None)
def _tiny(kind):
    model, _ = _recipe(_build_tiny(kind), torch.device("cuda:0"))
    return model.eval()


def _prompt(V, seed=11, rows=DB, cols=DP):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (rows, cols), generator=g).to("cuda:0")


def _script(V, rows=DB, steps=STEPS, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, V, (steps, rows), generator=g).to("cuda:0")


def _stepped(model, prompt, toks, z=None, lens=None, **kw):
    """(decoder, logits [rows, steps + 1, V]) after start + one step per row of toks."""
    from gvl.decode import KVDecoder
    dec = KVDecoder(model, prompt.shape[0], toks.shape[0], **kw)
    out = [dec.start(prompt, z, lens)]
    for s in range(toks.shape[0]):
        out.append(dec.step(toks[s]))
    return dec, torch.stack(out, 1)


def test_layer0_cache_is_the_quantised_bf16_cache(cuda):
    """Layer 0's k and v depend on nothing quantised: after start + 3 steps its kv8 / kvs are the
    CPU quantiser applied to the bf16 decoder's layer-0 cache, bit for bit."""
    model = _gpt()
    prompt, toks = _prompt(256), _script(256, steps=3)
    d16, _ = _stepped(model, prompt, toks)
    d8, _ = _stepped(model, prompt, toks, kv_cache="int8")
    t = DP + 3
    assert d8.t == t and d16.t == t
    kv8, kvs = d8.cache[0]
    assert kv8.dtype == torch.int8 and kvs.dtype == torch.float32
    assert kv8.shape == (DB, DP + 3, 256) and kvs.shape == (DB, DP + 3, 4)
    want8, wants = R.quantize_kv(d16.cache[0][:, :t].cpu(), 2)
    assert torch.equal(kv8[:, :t].cpu(), want8) and _same_bits(kvs[:, :t], wants)


@pytest.mark.parametrize("weights", [None, "int8"])
def test_generate_graph_equals_eager(cuda, weights):
    from gvl.decode import generate
    model = _gpt()
    prompt = _prompt(256)
    samp = dict(temperature=0.9, top_k=40, top_p=0.95)
    gen = lambda: torch.Generator(device="cuda").manual_seed(21)
    kw = dict(return_logits=True, return_lengths=True, eos=7, kv_cache="int8", weights=weights)
    for lens in (None, list(LENS)):
        want = generate(model, prompt, 10, prompt_lens=lens, generator=gen(), **samp, **kw)
        got = generate(model, prompt, 10, prompt_lens=lens, generator=gen(), graph=True, **samp,
                       **kw)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    plain = generate(model, prompt, 10, prompt_lens=lens, generator=gen(), return_logits=True,
                     eos=7, weights=weights, **samp)
    assert not torch.equal(plain[1][:, :2], want[1][:, :2]), "kv_cache='int8' changed nothing"


@pytest.mark.parametrize("weights", [None, "int8"])
def test_beam_search_graph_equals_eager(cuda, weights):
    from gvl.decode import beam_search
    model = _gpt()
    prompt = _prompt(256)
    for lens in (None, list(LENS)):
        kw = dict(num_beams=3, eos=None, prompt_lens=lens, return_all=True, kv_cache="int8",
                  weights=weights)
        want = beam_search(model, prompt, 8, **kw)
        got = beam_search(model, prompt, 8, graph=True, **kw)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert torch.isfinite(want[2]).all()


def test_beam_decoder_prefill_writes_only_the_items_rows(cuda):
    """cache_fill: kv8 takes the value cast to int8, kvs the value; the prefill writes rows b*K."""
    from gvl.decode import BeamDecoder
    model = _gpt()
    dec = BeamDecoder(model, DB, 3, 4, cache_fill=5.0, kv_cache="int8")
    dec.start(_prompt(256))
    kv8, kvs = dec.cache[0]
    assert kv8.shape == (DB * 3, DP + 4, 256) and kvs.shape == (DB * 3, DP + 4, 4)
    v8, vs = kv8.view(DB, 3, DP + 4, 256), kvs.view(DB, 3, DP + 4, 4)
    assert (v8[:, 1:] == 5).all() and (vs[:, 1:] == 5.0).all()
    assert (v8[:, 0, DP:] == 5).all() and (vs[:, 0, DP:] == 5.0).all()
    assert (v8[:, 0, :DP].abs().amax(-1) == 127).all() and (vs[:, 0, :DP] != 5.0).all()


def test_full_length_prompt_lens_are_the_plain_call(cuda):
    from gvl.decode import beam_search, generate
    model = _gpt()
    prompt = _prompt(256)
    a, b = (generate(model, prompt, STEPS, greedy=True, return_logits=True, prompt_lens=lens,
                     kv_cache="int8") for lens in (None, [DP] * DB))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = (beam_search(model, prompt, STEPS, num_beams=3, eos=None, return_all=True,
                        prompt_lens=lens, kv_cache="int8") for lens in (None, [DP] * DB))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


BOUND = 3e-2  # tests/test_gpu_ragged.py test_each_row_equals_the_row_alone


def test_unequal_lengths_match_the_rows_alone(cuda):
    """Row r of a right-padded batch against the same scripted decode of prompt[r, :len_r] alone
    (another GEMM row count, so another rounding: the relative bound of the bf16 ragged test),
    and no bit depends on the pad ids."""
    model = _gpt()
    prompt, toks = _prompt(256), _script(256)
    _, got = _stepped(model, prompt, toks, lens=LENS, kv_cache="int8")
    other = prompt.clone()
    for r, L in enumerate(LENS):
        other[r, L:] = _prompt(256, seed=99)[r, L:]
    assert not torch.equal(other, prompt)
    _, again = _stepped(model, other, toks, lens=LENS, kv_cache="int8")
    assert torch.equal(got, again) and torch.isfinite(got).all()
    worst = 0.0
    for r, L in enumerate(LENS):
        _, alone = _stepped(model, prompt[r:r + 1, :L].contiguous(), toks[:, r:r + 1].contiguous(),
                            kv_cache="int8")
        err = ((got[r].float() - alone[0].float()).abs().max() / alone.float().abs().max()).item()
        worst = max(worst, err)
        assert err < BOUND, (r, L, err)
    _record("ragged rows alone", dict(worst_rel=worst, bound=BOUND))


@pytest.mark.parametrize("kind", ["linear", "cross"])
def test_caption_and_cross_models_run_end_to_end(cuda, kind):
    from gvl.decode import beam_search, generate
    model = _tiny(kind)
    V = TINY["vocab_size"]
    prompt, toks = _prompt(V), _script(V)
    z = _z(11, DB, TINY["n_embd"], cuda)
    d8, l8 = _stepped(model, prompt, toks, z=z, kv_cache="int8")
    _, l16 = _stepped(model, prompt, toks, z=z)
    assert torch.isfinite(l8).all() and all(c[0].dtype == torch.int8 for c in d8.cache)
    if kind == "cross":
        assert d8.kvz is not None and all(k.dtype == BF for k in d8.kvz)
    assert torch.equal(l8[:, 0], l16[:, 0]) and not torch.equal(l8[:, 1:], l16[:, 1:])
    rel = ((l8.float() - l16.float()).abs().max() / l16.float().abs().max()).item()
    _record(f"{kind} int8 vs bf16 cache", dict(rel_logit_diff=rel))
    kw = dict(z=z, kv_cache="int8", prompt_lens=list(LENS))
    want = generate(model, prompt, 8, greedy=True, return_logits=True, **kw)
    got = generate(model, prompt, 8, greedy=True, return_logits=True, graph=True, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    want = beam_search(model, prompt, 6, num_beams=2, eos=None, return_all=True, **kw)
    got = beam_search(model, prompt, 6, num_beams=2, eos=None, return_all=True, graph=True, **kw)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_logits_against_the_fake_quantised_restatement(cuda):
    """e8 = max |int8-cache logits - fp32 restatement with quantise -> dequantise of every
    layer's k and v|, e16 = max |bf16-cache logits - the restatement without it| (the existing
    path's own error).  Both paths carry the same bf16 roundings on the way to the logits; the
    factor 2 allows for rint near-ties that the fp32 restatement and the kernel's bf16 k / v
    resolve differently.  Teacher-forced on scripted tokens."""
    model = _gpt()
    prompt, toks = _prompt(256), _script(256, steps=12)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    _, l16 = _stepped(model, prompt, toks)
    _, l8 = _stepped(model, prompt, toks, kv_cache="int8")
    r16 = R.decode_logits(sd, 2, prompt, toks, False)
    r8 = R.decode_logits(sd, 2, prompt, toks, True)
    e16 = (l16.float().cpu() - r16).abs().max().item()
    e8 = (l8.float().cpu() - r8).abs().max().item()
    moved = (r8 - r16).abs().max().item()
    # greedy agreement of the two caches over 32 tokens: recorded, not asserted
    from gvl.decode import generate
    a = generate(model, prompt, 32, greedy=True)
    b = generate(model, prompt, 32, greedy=True, kv_cache="int8")
    first = (a != b).any(0).nonzero()
    _record("logits", dict(e8=e8, e16=e16, ratio=e8 / e16, bound_ratio=2.0,
                           fake_quant_moves_the_reference_by=moved,
                           max_abs_logit=r16.abs().max().item(),
                           greedy_equal_tokens=int((a == b).sum()), of=int(a.numel()),
                           first_different_step=int(first[0]) if first.numel() else None))
    print(f"e8 {e8:.4g} e16 {e16:.4g} ratio {e8 / e16:.3f}; fake-quant moves the reference by "
          f"{moved:.4g}")
    assert e8 <= 2 * e16, (e8, e16)
