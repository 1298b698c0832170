"""The int8 KV cache without a GPU: the format and the reference of tests/kvq_ref.py, the bound
tests/test_gpu_kvq.py holds the kernel to, gvl.decode.kv_cache_bytes, and the arguments that are
refused before any launch."""
import numpy as np
import pytest
import torch

from tests import attn_ref as A
from tests import kvq_ref as R
from tests.helpers import assert_attn_close

BF = torch.bfloat16
TINY = dict(block_size=64, vocab_size=256, n_layer=2, n_head=2, n_embd=128)


def _vectors():
    """bf16 [40, 64]: normals scaled over 12 binades, a zero vector, a one-hot, a constant."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(40, 64, generator=g) * torch.exp2(torch.randint(-6, 7, (40, 1), generator=g))
    x[7] = 0
    x[8] = 0
    x[8, 13] = -3.0
    x[9] = 0.4375
    return x.to(BF)


def test_format_round_trip_zero_vector_and_full_range():
    x = _vectors()
    q, s = R.quantize_heads(x)
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    assert q.shape == x.shape and s.shape == x.shape[:-1]
    err = (R.dequantize_heads(q, s, torch.float64) - x.double()).abs()
    # |x / s - rint(x / s)| <= 1/2, and the fp32 division moves x / s by at most 2**-24 of it
    assert (err <= s.double()[:, None] * (0.5 + 127 * 2.0 ** -23)).all()
    assert float(s[7]) == 0.0 and not q[7].any()
    nz = s != 0
    assert int(nz.sum()) == 39 and (q[nz].abs().amax(1) == 127).all()
    assert (q.abs() <= 127).all() and (q == -128).sum() == 0
    assert int(q[8, 13]) == -127 and int(q[8].abs().sum()) == 127
    assert torch.equal(s, x.float().abs().amax(1) / torch.full((40,), 127.0))


def test_quantize_kv_takes_the_k_and_v_thirds_head_by_head():
    H, C = 3, 192
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(2, 5, 3 * C, generator=g).to(BF)
    kv8, kvs = R.quantize_kv(qkv, H)
    assert kv8.shape == (2, 5, 2 * C) and kvs.shape == (2, 5, 2 * H)
    for j in (0, 2, 3, 5):
        q, s = R.quantize_heads(qkv[..., C + 64 * j:C + 64 * (j + 1)])
        assert torch.equal(kv8[..., 64 * j:64 * (j + 1)], q) and torch.equal(kvs[..., j], s)
    kq, ks, vq, vs = R.heads(kv8, kvs, H)
    assert torch.equal(kq[1, 2], kv8[1, :, 128:192]) and torch.equal(vs[0, 1], kvs[0, :, H + 1])
    assert torch.equal(vq[1, 0], kv8[1, :, C:C + 64])


@pytest.mark.parametrize("Tk", [1, 33, 257])
def test_reference_gap_and_fp32_emulation(Tk):
    """An empty gap changes no bit of the reference; a skipped position may hold anything; an
    all-skipped row is zeros; and the kernel's arithmetic in fp32 torch, rounded once to bf16,
    sits inside the bound test_gpu_kvq.py uses (2 units of 2**-8 E + 4 x the fp32 baseline)."""
    H = 3
    c = R.case(Tk)
    o, E = R.case_ref(c, H)
    none = torch.zeros(2, Tk, dtype=torch.bool)
    o2, E2 = R.case_ref(c, H, skip=none)
    assert np.array_equal(o, o2) and np.array_equal(E, E2)
    kq, ks, vq, vs = R.heads(c["all8"], c["alls"], H)
    emu = R.attention_f32(c["q"], kq, ks, vq, vs, 0.125)
    r = assert_attn_close(emu, o, E, A.HARD_UNITS["o"], name=f"emu Tk={Tk}",
                          slack=4 * A.baseline()["o"])
    assert r <= 1.0, r  # one rounding to bf16 and fp32 arithmetic: under one unit of the two
    if Tk > 2:
        skip = none.clone()
        skip[0, 1:Tk - 1] = True
        skip[1, :] = True
        junk8, junks = c["all8"].clone(), c["alls"].clone()
        junk8[0, 1:Tk - 1] = 77
        junks[0, 1:Tk - 1] = float("nan")
        a = R.attention_ref(c["q"], kq, ks, vq, vs, 0.125, skip)
        b = R.attention_ref(c["q"], *R.heads(junk8, junks, H), 0.125, skip)
        assert np.array_equal(a[0], b[0]) and np.isfinite(a[0]).all()
        assert not a[0][1].any() and not a[1][1].any()
        assert not np.array_equal(a[0][0], o[0])
        e = R.attention_f32(c["q"], *R.heads(junk8, junks, H), 0.125, skip)
        assert_attn_close(e, a[0], a[1], A.HARD_UNITS["o"], name="emu gap",
                          slack=4 * A.baseline()["o"])


def test_reference_follows_the_beam_table():
    H, Tk = 3, 9
    c = R.case(Tk)
    src = torch.tensor([[1, 0, 1, 1, 0, 0, 1, 0, 0], [1, 1, 0, 0, 1, 0, 1, 0, 1]])
    o, _ = R.case_ref(c, H, src=src)
    g8 = torch.stack([c["all8"][src[b], torch.arange(Tk)] for b in range(2)])
    gs = torch.stack([c["alls"][src[b], torch.arange(Tk)] for b in range(2)])
    o2, _ = R.attention_ref(c["q"], *R.heads(g8, gs, H), 0.125)
    assert np.array_equal(o, o2)
    assert not np.array_equal(o, R.case_ref(c, H)[0])


def test_decode_restatement_steps_equal_the_full_forward_without_quantisation():
    """Without fake quantisation the restated decode is the full causal forward of the whole
    sequence (up to fp32 order); with it the logits move, by about the quantisation step."""
    import gvl.gpt2 as g2
    torch.manual_seed(0)
    model = g2.GPT(g2.GPTConfig(**TINY)).eval()
    sd = model.state_dict()
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, 256, (3, 6), generator=g)
    toks = torch.randint(0, 256, (4, 3), generator=g)
    a = R.decode_logits(sd, 2, prompt, toks, False)
    assert a.shape == (3, 5, 256)
    whole = torch.cat([prompt, toks.t()], 1)
    b = R.decode_logits(sd, 2, whole, toks[:0], False)
    assert torch.allclose(a[:, -1], b[:, 0], atol=1e-5, rtol=1e-5)
    q = R.decode_logits(sd, 2, prompt, toks, True)
    d = float((q - a).abs().max())
    assert torch.equal(q[:, 0], a[:, 0])  # the prefill attends its unquantised k / v
    assert 0 < d < 0.1 * float(a.abs().max())


def test_kv_cache_bytes_ratio_is_exact():
    import gvl.gpt2 as g2
    from gvl.decode import kv_cache_bytes
    for size in ("gpt2", "gpt2-xl"):
        cfg = g2.GPTConfig.for_size(size)
        for rows, Tmax in ((1, 1024), (64, 512), (7, 33)):
            b16 = kv_cache_bytes(cfg, rows, Tmax)
            i8 = kv_cache_bytes(cfg, rows, Tmax, kv_cache="int8")
            assert b16 == cfg.n_layer * rows * Tmax * 6 * cfg.n_embd
            assert i8 * 6000 == b16 * 2125  # int8 / bf16 == 2.125 / 6
            assert kv_cache_bytes(cfg, rows, Tmax, kv_cache=None) == b16
    xl = g2.GPTConfig.for_size("gpt2-xl")
    assert kv_cache_bytes(xl, 1, 1) == 460800  # the 460 KB per cached position per row
    with pytest.raises(ValueError, match="kv_cache"):
        kv_cache_bytes(xl, 1, 1, kv_cache="fp8")


def test_bad_kv_cache_arguments_are_refused_before_any_launch():
    import gvl.gpt2 as g2
    from gvl import decode
    model = g2.GPT(g2.GPTConfig(**TINY)).eval()
    prompt = torch.zeros(2, 4, dtype=torch.int64)
    for bad in ("int4", "bf16", "INT8", ""):
        with pytest.raises(ValueError, match="kv_cache"):
            decode.KVDecoder(model, 2, 4, kv_cache=bad)
        with pytest.raises(ValueError, match="kv_cache"):
            decode.BeamDecoder(model, 2, 3, 4, kv_cache=bad)
        with pytest.raises(ValueError, match="kv_cache"):
            decode.generate(model, prompt, 4, kv_cache=bad)
        with pytest.raises(ValueError, match="kv_cache"):
            decode.beam_search(model, prompt, 4, kv_cache=bad)
        with pytest.raises(ValueError, match="kv_cache"):
            decode.speculative_generate(model, prompt, 4, kv_cache=bad)
        with pytest.raises(ValueError, match="kv_cache"):
            decode.GraphedGenerate(model, 4, 4, kv_cache=bad)
        with pytest.raises(ValueError, match="kv_cache"):
            decode.GraphedBeamSearch(model, 4, 4, kv_cache=bad)
    with pytest.raises(ValueError, match="kv_cache"):
        decode.speculative_generate(model, prompt, 4, kv_cache="int8")
    dec = decode.KVDecoder(model, 2, 4, kv_cache="int8")
    with pytest.raises(ValueError, match="kv_cache"):
        dec.step_multi(torch.zeros(2, 2, dtype=torch.int64), None, None)
    assert decode.KVDecoder(model, 2, 4).kv8 is False and dec.kv8 is True
