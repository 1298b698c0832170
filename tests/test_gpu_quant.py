"""Int8 weight-only decoding on the MI355X (include/gvl.h gvl_quantize_rows_i8,
gvl_dequantize_rows_i8, gvl_linear_w8; gvl/quant.py; weights="int8" in gvl/decode.py):

  * the quantiser and dequantiser equal their CPU restatement bit for bit (tests/quant_ref.py),
    strided inputs and the special rows included, inside NaN-filled arenas that stay NaN;
  * gvl_linear_w8 per element (assert_bf16_rounded; slack from the reference's own fp32
    emulations) over both weight types and the five epilogues, with ldc > N, a residual that
    aliases c, NaN rows of x past M, c in a NaN-filled arena; an element's bits do not depend on
    M, ldc or the call;
  * the decoders with weights="int8" against a bf16 copy of the model that holds the reference's
    dequantised matrices, and the decoders' guarantees (graph replay = eager, speculative =
    generate, a reused quantize_decoder result) bit for bit.
"""
import copy
import functools

import pytest
import torch

from tests import quant_ref as Q
from tests.test_gpu_parity_full import _build_tiny, _recipe, _z

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")


# ------------------------------------------------------------ quantiser / dequantiser
def _special_rows(w):
    """Rows the format singles out: zeros, the absmax negative / in the last column, ties on a
    power-of-two scale."""
    N, K = w.shape
    w[1] = 0
    w[2, K - 1] = -1024.0  # above anything the scaled random rows reach (64 * |N(0, 1)|)
    w[3, 0] = 1024.0
    w[4] = 0
    w[4, 0], w[4, 1], w[4, 2], w[4, 3] = 127.0 * 0.25, 2.5 * 0.25, 3.5 * 0.25, -2.5 * 0.25
    return w


@pytest.mark.parametrize("N,K", [(8, 64), (24, 192), (520, 1600)])
@pytest.mark.parametrize("strided", [False, True])
def test_quantiser_and_dequantiser_equal_the_reference(cuda, N, K, strided):
    import gvl.kernels as KN
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 7, (N, 1), generator=g))
    w = _special_rows(w.to(BF))
    ldw = K + 24 if strided else K
    wa = torch.full((N, ldw), NAN, dtype=BF, device=cuda)
    wa[:, :K] = w.to(cuda)
    # outputs as interior views of arenas: one guard row above and below, guard columns
    ldq = K + 16 if strided else K
    qa = torch.full((N + 2, ldq), 77, dtype=torch.int8, device=cuda)
    sa = torch.full((N + 8,), NAN, device=cuda)
    q, s = KN.quantize_rows_i8(wa[:, :K], q=qa[1:N + 1, :K], scale=sa[4:N + 4])
    qr, sr = Q.quantize(w)
    assert torch.equal(s.cpu(), sr) and torch.equal(q.cpu(), qr)
    assert (qa[0] == 77).all() and (qa[N + 1] == 77).all() and (qa[:, K:] == 77).all()
    assert sa[:4].isnan().all() and sa[N + 4:].isnan().all()
    assert s[1] == 0 and (q[1] == 0).all() and q[2, K - 1] == -127 and q[3, 0] == 127
    assert q[4, :4].tolist() == [127, 2, 4, -2]

    oa = torch.full((N + 2, K + 8), NAN, dtype=BF, device=cuda)
    out = KN.dequantize_rows_i8(q, s, out=oa[1:N + 1, :K])
    assert torch.equal(out.cpu(), Q.dequantize(qr, sr))
    assert oa[0].isnan().all() and oa[N + 1].isnan().all() and oa[:, K:].isnan().all()


def test_quantize_weight_refuses_a_non_finite_weight(cuda):
    from gvl import quant
    w = torch.randn(16, 64, device=cuda).to(BF)
    quant.quantize_weight(w)
    for bad in (float("nan"), float("inf"), float("-inf")):
        wb = w.clone()
        wb[5, 9] = bad
        with pytest.raises(ValueError, match="not finite"):
            quant.quantize_weight(wb)


# ---------------------------------------------------------------------- linear_w8
SHAPES = [(1, 8, 64), (3, 24, 128), (16, 136, 1600), (17, 520, 64), (64, 24, 1600),
          (65, 136, 128), (Q.CAP, 520, 1600), (1, 520, 1600), (65, 8, 1600), (Q.CAP, 8, 64),
          (16, 24, 64), (64, 520, 128), (17, 136, 128), (3, 8, 1600)]


def test_shapes_cover_the_issue_grid():
    assert {s[0] for s in SHAPES} == {1, 3, 16, 17, 64, 65, Q.CAP}
    assert {s[1] for s in SHAPES} == {8, 24, 136, 520} and {s[2] for s in SHAPES} == {64, 128, 1600}


@functools.lru_cache(maxsize=4)
def _ins(kind, M, N, K):
    return Q.inputs(kind, M, N, K)


def _launch(cuda, ins, wt, epi, M, N, ldc, alias):
    """One gvl_linear_w8 call inside NaN arenas -> (c view, arena).  x has 5 NaN rows past M;
    c is the interior [1 : M + 1, :N] of a NaN arena of row length ldc."""
    import gvl.kernels as KN
    K = ins["x"].shape[1]
    xa = torch.full((M + 5, K), NAN, dtype=BF, device=cuda)
    xa[:M] = ins["x"].to(cuda)
    arena = torch.full((M + 2, ldc), NAN, dtype=BF, device=cuda)
    c = arena[1:M + 1, :N]
    kw = {k: (v.to(cuda) if isinstance(v, torch.Tensor) else v)
          for k, v in Q.epi_operands(epi, ins).items()}
    if alias and "residual" in kw:
        c.copy_(kw["residual"])
        kw["residual"] = c
    if wt == "i8":
        KN.linear_w8(xa[:M], ins["q"].to(cuda), ins["scale"].to(cuda), out=c, **kw)
    else:
        KN.linear_w8(xa[:M], ins["w"].to(cuda), None, out=c, **kw)
    return c, arena


@pytest.mark.parametrize("kind", ["random", "scaled", "exact"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_w8_per_element(cuda, M, N, K, kind):
    ins = _ins(kind, M, N, K)
    worst = {}
    for wt in ("i8", "bf16"):
        P = Q.products(ins["x"], ins["q"] if wt == "i8" else ins["w"],
                       ins["scale"] if wt == "i8" else None)
        for epi in Q.EPIS:
            R = Q.reference(P, **Q.epi_operands(epi, ins))
            if kind == "exact" and epi in Q.LINEAR_EPIS:
                assert R["slack"] == 0  # bit for bit the correctly rounded reference
            c, arena = _launch(cuda, ins, wt, epi, M, N, N + 8, alias=epi == "bias_res")
            Q.check(c, R, f"{wt} {epi} {kind} M{M} N{N} K{K}")
            worst[f"{wt}/{epi}"] = R["emu"]
            assert arena[0].isnan().all() and arena[M + 1].isnan().all()
            assert arena[:, N:].isnan().all()
            assert not c.isnan().any()
    print(f"M{M} N{N} K{K} {kind}: the emulations' own error {max(worst.values()):.3f} units")


@pytest.mark.parametrize("wt", ["i8", "bf16"])
def test_linear_w8_bits_do_not_depend_on_rows_stride_or_call(cuda, wt):
    M, N, K = 65, 136, 1600
    ins = _ins("random", M, N, K)
    for epi in Q.EPIS:
        c, _ = _launch(cuda, ins, wt, epi, M, N, N + 8, alias=False)
        again, _ = _launch(cuda, ins, wt, epi, M, N, N + 8, alias=False)
        dense, _ = _launch(cuda, ins, wt, epi, M, N, N, alias=False)
        assert torch.equal(c, again) and torch.equal(c, dense), epi
        for r in (0, 15, 16, 63, 64):
            one = dict(ins, x=ins["x"][r:r + 1], residual=ins["residual"][r:r + 1])
            alone, _ = _launch(cuda, one, wt, epi, 1, N, N + 24, alias=False)
            assert torch.equal(alone[0], c[r]), (epi, r)
    # the rows of a capped call equal the same rows in 64-row calls (row passes)
    big = _ins("random", Q.CAP, 520, 1600)
    full, _ = _launch(cuda, big, wt, "bias_gelu", Q.CAP, 520, 528, alias=False)
    for r0 in (0, 64, 192):
        part = dict(big, x=big["x"][r0:r0 + 64], residual=big["residual"][r0:r0 + 64])
        got, _ = _launch(cuda, part, wt, "bias_gelu", 64, 520, 520, alias=False)
        assert torch.equal(got, full[r0:r0 + 64]), r0


def test_qweight_linear_above_the_cap_dequantises_into_the_callers_scratch(cuda):
    import gvl.kernels as KN
    from gvl import quant
    from gvl._lib import GvlError
    M, N, K = Q.CAP + 1, 136, 128
    ins = _ins("random", M, N, K)
    qw = quant.QWeight(ins["q"].to(cuda), ins["scale"].to(cuda))
    x, bias = ins["x"].to(cuda), ins["bias"].to(cuda)
    scr = torch.full((N * K + 8,), NAN, dtype=BF, device=cuda)
    got = qw.linear(x, bias, scratch=scr)
    w = Q.dequantize(ins["q"], ins["scale"])
    assert torch.equal(scr[:N * K].view(N, K).cpu(), w) and scr[N * K:].isnan().all()
    assert torch.equal(got, KN.linear(x, w.to(cuda), bias))
    with pytest.raises(GvlError, match="outside 1..256 rows"):  # the library itself refuses
        KN.linear_w8(x, qw.q, qw.scale, bias)
    # at the cap the skinny kernel runs and leaves the scratch alone
    scr.fill_(NAN)
    at_cap = qw.linear(x[:Q.CAP], bias, scratch=scr)
    assert scr.isnan().all()
    assert torch.equal(at_cap, KN.linear_w8(x[:Q.CAP], qw.q, qw.scale, bias))


# ------------------------------------------------------------------ decoder level
KINDS = ("gpt", "linear", "qformer", "cross")


def _model(kind, cuda):
    model, _ = _recipe(_build_tiny(kind), cuda)
    return model.eval()


def _zfor(kind, B, cuda):
    from tests.helpers import TINY
    return None if kind == "gpt" else _z(11, B, TINY["n_embd"], cuda)


def _dequantised_copy(model, kind, cuda):
    """A bf16 copy of the model whose quantised matrices hold the reference's dequantised values;
    its lm_head is untied from wte, which keeps the original."""
    ref = copy.deepcopy(model)
    dec = ref.gpt if kind in ("linear", "qformer") else ref
    dq = lambda p: Q.dequantize(*Q.quantize(p.detach())).to(cuda)
    with torch.no_grad():
        for b in dec.transformer.h:
            mats = [b.attn.c_attn, b.attn.c_proj, b.mlp.c_fc, b.mlp.c_proj]
            if kind == "cross":
                mats += [b.xattn.q_proj, b.xattn.c_proj]
            for lin in mats:
                lin.weight.copy_(dq(lin.weight))
        dec.lm_head.weight = torch.nn.Parameter(dq(dec.lm_head.weight), requires_grad=False)
    assert dec.lm_head.weight is not dec.transformer.wte.weight
    assert torch.equal(dec.transformer.wte.weight, (model.gpt if dec is not ref else model)
                       .transformer.wte.weight)
    return ref


@pytest.mark.parametrize("kind", KINDS)
def test_int8_generate_matches_the_dequantised_model(cuda, kind):
    from gvl import quant
    from gvl.decode import KVDecoder, generate
    model = _model(kind, cuda)
    prompt = torch.randint(0, 512, (1, 6), device=cuda,
                           generator=torch.Generator(device="cuda").manual_seed(5))
    z = _zfor(kind, 1, cuda)
    toks, lg = generate(model, prompt, 16, z=z, greedy=True, return_logits=True, weights="int8")
    dec = KVDecoder(model, 1, 4, weights="int8")
    stored = [P[k][0] for P in dec.blocks for k in ("attn", "aproj", "fc", "mproj")]
    if kind == "cross":
        stored += [P[k][0] for P in dec.cross for k in ("q", "c")]
    stored.append(dec.qdec.head)
    assert all(isinstance(w, quant.QWeight) and w.q.dtype == torch.int8 and
               w.scale.dtype == torch.float32 for w in stored)
    # teacher-forced on the int8 run's tokens through the full forward of the dequantised copy
    ref = _dequantised_copy(model, kind, cuda)
    with torch.no_grad():
        seq = torch.cat([prompt, toks[:, :-1]], 1)
        full = (ref(seq)[0] if kind == "gpt" else ref(seq, z=z)[0] if kind == "cross"
                else ref(z, seq)[0]).float()
    P = prompt.shape[1] + full.shape[1] - seq.shape[1]
    ref_lg = full[0, P - 1:P - 1 + 16]
    err = (lg[0] - ref_lg).abs().max().item() / ref_lg.abs().max().item()
    same = int((ref_lg.argmax(-1) == toks[0]).sum())
    print(f"{kind}: int8 decode vs dequantised model: logits rel {err:.2e}, {same}/16 argmax equal")
    assert err < 3e-2


def _ragged(cuda, B=3, Pn=7):
    g = torch.Generator(device="cuda").manual_seed(9)
    return torch.randint(0, 512, (B, Pn), device=cuda, generator=g), [7, 4, 5]


@pytest.mark.parametrize("kind", ["gpt", "cross"])
def test_int8_graph_replay_equals_eager(cuda, kind):
    from gvl.decode import GraphedGenerate, generate
    model = _model(kind, cuda)
    prompt, lens = _ragged(cuda)
    z = _zfor(kind, 3, cuda)
    samp = dict(temperature=0.9, top_k=40, top_p=0.95)
    gen = lambda: torch.Generator(device="cuda").manual_seed(21)
    want = generate(model, prompt, 10, z=z, prompt_lens=lens, generator=gen(), return_logits=True,
                    weights="int8", **samp)
    got = generate(model, prompt, 10, z=z, prompt_lens=lens, generator=gen(), return_logits=True,
                   weights="int8", graph=True, **samp)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with GraphedGenerate(model, 7, 10, return_logits=True, weights="int8", **samp) as ses:
        for _ in range(2):
            again = ses(prompt, 10, z=z, prompt_lens=lens, generator=gen())
            assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
        assert ses.stats["captures"] == 1
    # and the quantised call is not the bf16 one under another name
    plain = generate(model, prompt, 10, z=z, prompt_lens=lens, generator=gen(), return_logits=True,
                     **samp)
    assert not torch.equal(plain[1], want[1])


@pytest.mark.parametrize("kind", ["gpt", "cross"])
def test_int8_beam_search_graph_equals_eager(cuda, kind):
    from gvl.decode import beam_search
    model = _model(kind, cuda)
    prompt, lens = _ragged(cuda)
    z = _zfor(kind, 3, cuda)
    kw = dict(z=z, num_beams=3, eos=None, prompt_lens=lens, return_all=True, weights="int8")
    want = beam_search(model, prompt, 8, **kw)
    got = beam_search(model, prompt, 8, graph=True, **kw)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["gpt", "cross"])
def test_int8_speculative_tokens_equal_generate(cuda, kind):
    from gvl.decode import generate, speculative_generate
    model = _model(kind, cuda)
    g = torch.Generator(device="cuda").manual_seed(13)
    prompt = torch.randint(0, 512, (2, 6), device=cuda, generator=g)
    z = _zfor(kind, 2, cuda)
    want = generate(model, prompt, 14, z=z, greedy=True, weights="int8")
    got = speculative_generate(model, prompt, 14, z=z, greedy=True, draft_len=4, weights="int8")
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["gpt", "cross"])
def test_a_quantize_decoder_result_gives_the_bits_of_int8(cuda, kind):
    from gvl import quant
    from gvl.decode import generate
    model = _model(kind, cuda)
    prompt, lens = _ragged(cuda)
    z = _zfor(kind, 3, cuda)
    want = generate(model, prompt, 8, z=z, greedy=True, return_logits=True, weights="int8")
    qd = quant.quantize_decoder(model)
    for _ in range(2):
        got = generate(model, prompt, 8, z=z, greedy=True, return_logits=True, weights=qd)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    other = _model("gpt" if kind == "cross" else "cross", cuda)
    with pytest.raises(ValueError, match="another model"):
        generate(other, prompt, 4, z=_zfor("cross" if kind == "gpt" else "gpt", 3, cuda),
                 weights=qd)
