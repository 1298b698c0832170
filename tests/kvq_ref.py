"""CPU restatement of the int8 KV cache (include/gvl.h gvl_kv_quantize_i8, gvl_attn_decode_q8;
csrc/attn_decode_q8.hip; kv_cache="int8" in gvl/decode.py).

Format: tests/quant_ref.py's quantiser with one "row" being one head's 64-wide key or value
vector at one position.  A layer's cache: kv8 int8 [rows, T, 2C] (k heads, then v heads), kvs
fp32 [rows, T, 2H] (k scales, then v scales).

Semantics: the attention of a step sees, for every position including the step's own,
fp32(q8) * scale; nothing else changes.  attention_ref is that in float64 with the per-element
scale E of tests/attn_ref.py (the same products with every term replaced by its absolute value);
attention_f32 the kernel's arithmetic in fp32 torch.  decode_logits restates a GPT's prefill and
decode steps in fp32 torch, with or without quantise -> dequantise of every layer's cached k and v.
Nothing here reads a kernel's output."""
import math

import numpy as np
import torch

from tests import quant_ref as Q

BF = torch.bfloat16
F64 = torch.float64


# ------------------------------------------------------------------------------ format
def quantize_heads(x):
    """x [..., 64] (bf16 or fp32, CPU) -> (q int8 [..., 64], scale fp32 [...])."""
    assert x.shape[-1] == 64
    q, s = Q.quantize(x.reshape(-1, 64))
    return q.view(x.shape), s.view(x.shape[:-1])


def dequantize_heads(q, scale, dtype=torch.float32):
    """dtype(q) * dtype(scale)[..., None]: exact in float64, one rounding in fp32."""
    return q.to(dtype) * scale.to(dtype)[..., None]


def quantize_kv(qkv, H):
    """The k and v thirds of qkv [..., 3C] (C = H*64) -> (kv8 int8 [..., 2C], kvs fp32 [..., 2H]):
    what gvl_kv_quantize_i8 and the fused append write for those rows."""
    C = H * 64
    assert qkv.shape[-1] == 3 * C
    kv = qkv[..., C:].reshape(*qkv.shape[:-1], 2 * H, 64)
    q, s = quantize_heads(kv)
    return q.reshape(*qkv.shape[:-1], 2 * C), s


def heads(kv8, kvs, H):
    """kv8 [B, T, 2C], kvs [B, T, 2H] -> (kq, ks, vq, vs) as [B, H, T, 64] / [B, H, T]."""
    B, T, _ = kv8.shape
    x = kv8.view(B, T, 2, H, 64).permute(2, 0, 3, 1, 4)
    s = kvs.view(B, T, 2, H).permute(2, 0, 3, 1)
    return x[0], s[0], x[1], s[1]


# --------------------------------------------------------------------------- attention
def _attend(q, k, v, scale, skip, dt):
    """softmax(scale q.k) v over the positions not skipped, in dtype dt; q [B, H, 1, 64], k, v
    [B, H, T, 64] (already dequantised), skip bool [B, T] or None.  A row with every position
    skipped gives zeros.  -> (o [B, H, 1, 64], P [B, H, 1, T])"""
    s = (q.to(dt) @ k.to(dt).transpose(-1, -2)) * scale
    if skip is not None:
        s = s.masked_fill(skip[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))
    return P @ v.to(dt), P


def attention_ref(q, kq, ks, vq, vs, scale, skip=None):
    """The float64 reference of a step: attention(q, fp64(kq) * ks, fp64(vq) * vs).
    q bf16 [B, H, 1, 64]; kq, vq int8 [B, H, T, 64]; ks, vs fp32 [B, H, T]; skip bool [B, T].
    -> (o, E) float64 numpy [B, H, 1, 64], E = P @ |v|."""
    scale = float(np.float32(scale))
    k, v = dequantize_heads(kq, ks, F64), dequantize_heads(vq, vs, F64)
    if skip is not None:  # a skipped position is never loaded: whatever it holds
        dead = skip[:, None, :, None]
        k, v = k.masked_fill(dead, 0.0), v.masked_fill(dead, 0.0)
    o, P = _attend(q, k, v, scale, skip, F64)
    return o.numpy(), (P @ v.abs()).numpy()


def attention_f32(q, kq, ks, vq, vs, scale, skip=None):
    """The kernel's arithmetic in fp32 torch, rounded once to bf16: the score is ks * (q . kq)
    with the scale applied after the sum, the value weight p * vs.  -> bf16 [B, H, 1, 64]"""
    f = torch.float32
    s = ((q.to(f) * np.float32(scale)) @ kq.to(f).transpose(-1, -2)) * ks.to(f)[:, :, None, :]
    if skip is not None:
        s = s.masked_fill(skip[:, None, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    w = e * vs.to(f)[:, :, None, :]
    if skip is not None:
        w = w.masked_fill(skip[:, None, None, :], 0.0)
        vq = vq.masked_fill(skip[:, None, :, None], 0)
    o = w @ vq.to(f)
    o = torch.where(l > 0, o / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(o))
    return o.to(BF)


def case(Tk, B=2, H=3, seed=5):
    """One step at column tc = Tk - 1: qkv bf16 [B, 3C] (the new row), the Tk - 1 cached positions
    quantised on the CPU (kv8 [B, Tk - 1, 2C], kvs [B, Tk - 1, 2H]) from i.i.d. normal k / v whose
    head vectors are scaled by powers of two (k: 2**-2 .. 1, so that the softmax stays spread
    over many keys; v: 2**-6 .. 2**6, 12 binades), and the same with the new row appended
    (`all8`, `alls`: [B, Tk, .]) for the reference."""
    C = H * 64
    g = torch.Generator().manual_seed(9100 + 100 * seed + Tk)
    rows = torch.randn(B, Tk, 3 * C, generator=g)
    binade = torch.cat([torch.randint(-2, 1, (B, Tk, H), generator=g),
                        torch.randint(-6, 7, (B, Tk, H), generator=g)], 2).float()
    rows[..., C:] = (rows[..., C:].view(B, Tk, 2 * H, 64) *
                     torch.exp2(binade)[..., None]).view(B, Tk, 2 * C)
    rows = rows.to(BF)
    all8, alls = quantize_kv(rows, H)
    return dict(qkv=rows[:, Tk - 1].contiguous(), kv8=all8[:, :Tk - 1].contiguous(),
                kvs=alls[:, :Tk - 1].contiguous(), all8=all8, alls=alls,
                q=rows[:, Tk - 1, :C].view(B, H, 1, 64).contiguous())


def case_ref(c, H, scale=0.125, skip=None, src=None):
    """(o, E) of case `c` (attention_ref over all Tk positions).  src int [B, Tk]: the cache row
    of every position (the beam table; column Tk - 1 names the row itself)."""
    all8, alls = c["all8"], c["alls"]
    if src is not None:
        idx = src.long()
        all8 = torch.gather(all8, 0, idx[:, :, None].expand(-1, -1, all8.shape[2]))
        alls = torch.gather(alls, 0, idx[:, :, None].expand(-1, -1, alls.shape[2]))
    return attention_ref(c["q"], *heads(all8, alls, H), scale, skip)


# ------------------------------------------------------------------ the decoder, restated
def _fake(x, H, on):
    """Quantise -> dequantise (fp32) every head vector of x [B, H, T, 64] when `on`."""
    if not on:
        return x
    assert x.shape[1] == H
    return dequantize_heads(*quantize_heads(x.contiguous()))


def _ln(x, w, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def decode_logits(sd, H, prompt, toks, fake_quant):
    """A GPT's decode in fp32 torch on the CPU from its state dict (any float dtype): prefill of
    prompt [B, P] with full causal attention over the unquantised k / v, then one step per row of
    toks [S, B], each attending the cache and its own position.  fake_quant: every layer's cached
    k and v, the step's own included, are quantised and dequantised per head vector; the prefill's
    own attention stays unquantised, as in KVDecoder.prefill.  -> logits fp32 [B, S + 1, V]"""
    f = lambda k: sd[k].detach().to("cpu", torch.float32)
    n_layer = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.h."))
    wte, wpe = f("transformer.wte.weight"), f("transformer.wpe.weight")
    B, P = prompt.shape
    C = wte.shape[1]
    prompt, toks = prompt.cpu(), toks.cpu()

    def split(qkv):  # [B, T, 3C] -> q, k, v as [B, H, T, 64]
        T = qkv.shape[1]
        return (qkv[..., i * C:(i + 1) * C].reshape(B, T, H, 64).transpose(1, 2) for i in range(3))

    def block(l, x, cache):
        p = f"transformer.h.{l}."
        qkv = _ln(x, f(p + "ln_1.weight"), f(p + "ln_1.bias")) @ f(p + "attn.c_attn.weight").t() \
            + f(p + "attn.c_attn.bias")
        T = x.shape[1]
        q, k, v = split(qkv)
        new = (_fake(k, H, fake_quant), _fake(v, H, fake_quant))
        if cache[l] is None:  # prefill: causal, on the unquantised k / v
            cache[l] = new
            s = (q @ k.transpose(-1, -2)) / math.sqrt(64)
            s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
        else:
            cache[l] = tuple(torch.cat([a, b], 2) for a, b in zip(cache[l], new))
            k, v = cache[l]
            s = (q @ k.transpose(-1, -2)) / math.sqrt(64)
        y = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)
        x = x + y @ f(p + "attn.c_proj.weight").t() + f(p + "attn.c_proj.bias")
        h = _ln(x, f(p + "ln_2.weight"), f(p + "ln_2.bias")) @ f(p + "mlp.c_fc.weight").t() \
            + f(p + "mlp.c_fc.bias")
        h = torch.nn.functional.gelu(h, approximate="tanh")
        return x + h @ f(p + "mlp.c_proj.weight").t() + f(p + "mlp.c_proj.bias")

    def run(x, cache):
        for l in range(n_layer):
            x = block(l, x, cache)
        x = _ln(x[:, -1], f("transformer.ln_f.weight"), f("transformer.ln_f.bias"))
        return x @ f("lm_head.weight").t()

    cache = [None] * n_layer
    out = [run(wte[prompt] + wpe[:P], cache)]
    for s in range(toks.shape[0]):
        out.append(run(wte[toks[s]][:, None] + wpe[P + s], cache))
    return torch.stack(out, 1)
