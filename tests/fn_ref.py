"""float64 autograd references, a bf16-rounding emulation, per-line bounds and the shared case
list for the fused autograd Functions of gvl/functional.py (plus _SelfAttnFn of gvl/gpt2.py and
_CrossSDPAFn of gvl/cross_att.py).  CPU only: nothing here reads a kernel's output.

Every unit's forward is written once in plain torch ops over a `Mode`:
  REF  float64, no rounding: the reference.  Its gradients are torch.autograd.grad of that
       forward against a fixed bf16 `dout` (LMHeadLossFn: dloss = DLOSS), so they do not depend
       on the hand-written backward formulas of functional.py.
  EMU  float64 with a straight-through bf16 rounding at every tensor the Function materialises in
       bf16: `m.f` rounds a forward value (identity backward), `m.b` is the identity whose
       backward rounds the gradient, `m.fb` both.  The rounding points are listed per unit.
  ALT  the same graph in fp32 arithmetic throughout, with attn_ref's P / dS roundings inside
       attention as well: a second evaluation whose roundings fall differently.

Bound (per tensor t, per line i; a line is a row of a 2-D / 3-D activation or weight gradient, a
1-D bias / LayerNorm gradient or the query-token gradient is one whole line, the gate one
element): s_i = rms of the reference line, U_t = max_i max_j |emu - ref| / s_i, and
  |got - ref| <= ulp_bf16(ref) + MARGIN * U_t * s_i        (MARGIN = misc_ref.MARGIN = 4)
per element; where s_i == 0 the result must be exactly zero.  For a gradient accumulated into a
sink the target is g0 + ref and the ulp that of the sum.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import attn_ref, gemm_ref
from tests.helpers import f64, margins_out, ulp_bf16
from tests.misc_ref import MARGIN

BF = torch.bfloat16
F64 = torch.float64
F32 = torch.float32

C, H = 128, 2
B, T = 3, 33
S_CLIP, Q, L = 33, 32, 2
DROP_P = 0.1
SEED = 0x1234ABCD5
SEED_OFFSETS = (0, 977)
DLOSS = 0.75
LN_EPS = 1e-5
ATT_SCALE = 0.125
ATTN_XOR = 0x5A5A5A5A  # MHAFn: the attention-probability site hashes with seed ^ this


# ------------------------------------------------------------------------------ rounding
def _r(x):
    return x.to(F32).to(BF).to(x.dtype)


class _RoundF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _r(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _r(g)


class Mode:
    def __init__(self, name, dt, rnd, attn):
        self.name, self.dt, self.rnd, self.attn = name, dt, rnd, attn

    def f(self, x):
        return _RoundF.apply(x) if self.rnd else x

    def b(self, x):
        return _RoundB.apply(x) if self.rnd else x

    def fb(self, x):
        return self.f(self.b(x))


REF = Mode("ref", F64, False, False)
EMU = Mode("emu", F64, True, False)
ALT = Mode("alt", F32, True, True)
MODES = dict(ref=REF, emu=EMU, alt=ALT)


# ---------------------------------------------------------------------------- primitives
def layer_norm(x, w, b, eps=LN_EPS):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    return d * torch.rsqrt(var + eps) * w + b


def linear(x, w, b=None):
    y = x @ w.transpose(-1, -2)
    return y if b is None else y + b


def gelu(m, x, act):
    """act 1: tanh form, 2: erf form.  EMU / ALT: the backward multiplies by the bf16 gelu'(x)
    the forward epilogue stored (GEMM act 3 / 4 -> pre_out, dact 3)."""
    approx = "tanh" if act == 1 else "none"
    y = F.gelu(x, approximate=approx)
    if not m.rnd:
        return y
    with torch.enable_grad():
        xd = x.detach().requires_grad_()
        (d,) = torch.autograd.grad(F.gelu(xd, approximate=approx).sum(), xd)
    return y.detach() + (x - x.detach()) * _r(d)


def heads(t, n_head):
    Bq, Tq, Cq = t.shape
    return t.view(Bq, Tq, n_head, Cq // n_head).transpose(1, 2)


def attention(m, q, k, v, n_head, causal, kd=None):
    """softmax(q k^T / 8) v per 64-wide head over [B, T, C] tensors; kd: keep / (1 - p) as a
    constant [B, H, Tq, Tk] multiplier of the probabilities, or None."""
    qh, kh, vh = heads(q, n_head), heads(k, n_head), heads(v, n_head)
    s = qh @ kh.transpose(-1, -2)
    if m.attn:
        s = m.b(s)  # dS rounded before dS K / dS^T Q (the scale 1/8 is a power of two)
    s = s * ATT_SCALE
    if causal:
        s = s.masked_fill(~attn_ref.visible(q.shape[1], k.shape[1], True), float("-inf"))
    P = torch.softmax(s, dim=-1)
    if kd is not None:
        P = P * kd.to(P.dtype)
    if m.attn:
        P = m.f(P)
    o = P @ vh
    return o.transpose(1, 2).reshape(q.shape)


def gated(m, res, br, gate):
    """res + tanh(gate) * br.  EMU / ALT: the gate gradient is formed from the stored bf16 branch
    (pre_out), the output from the unrounded one."""
    t = torch.tanh(gate)
    if not m.rnd:
        return res + t * br
    return res + t.detach() * br + (t - t.detach()) * _r(br).detach()


def keep_rows(seed, off, rows, cols, p):
    """keep / (1 - p) of a GEMM-epilogue dropout or dropout_mask_apply over [rows, cols]."""
    k = gemm_ref.keep_mask(attn_ref.seed_eff(seed, off), rows, cols, p)
    return torch.from_numpy(k).to(F64) * attn_ref.drop_scale(p)


def keep_attn(seed, off, nb, nh, tq, tk, p):
    k = attn_ref.keep_mask(attn_ref.seed_eff(seed, off), nb, nh, tq, tk, p)
    return torch.from_numpy(k).to(F64) * attn_ref.drop_scale(p)


class _CESum(torch.autograd.Function):
    """Sum of the row losses whose backward hands back the ROUNDED softmax - onehot times the
    incoming scalar: the CE kernel stores dlogits in bf16 before the GEMMs scale it."""

    @staticmethod
    def forward(ctx, x, tgt, valid):
        lse = torch.logsumexp(x, dim=-1)
        tc = torch.where(valid, tgt, torch.zeros_like(tgt))
        loss = torch.where(valid, lse - x.gather(-1, tc[:, None])[:, 0], torch.zeros_like(lse))
        p = torch.softmax(x, dim=-1)
        p = p - F.one_hot(tc, x.shape[-1]).to(p.dtype)
        ctx.save_for_backward(_r(torch.where(valid[:, None], p, torch.zeros_like(p))))
        return loss.sum()

    @staticmethod
    def backward(ctx, g):
        return ctx.saved_tensors[0] * g, None, None


def ce_loss(m, rows, tgt, mask, mask_mode):
    """Mean cross-entropy over the counted rows as K.cross_entropy defines it: a row counts in
    the sum when its target is not -100 and its mask (if any) is set; the divisor is the number
    of such rows, or with mask_mode the number of set mask entries (clamped to >= 1)."""
    valid = tgt != -100
    if mask is not None:
        mask = mask.reshape(-1)
        valid = valid & mask.bool()
    n = float(mask.bool().sum().clamp(min=1)) if mask_mode else float(valid.sum())
    if m.rnd:
        total = _CESum.apply(rows, tgt, valid)
    else:
        tc = torch.where(valid, tgt, torch.zeros_like(tgt))
        total = (F.cross_entropy(rows, tc, reduction="none") * valid.to(rows.dtype)).sum()
    return total / n


# --------------------------------------------------------------------------------- units
def _probe(c, name, x):
    """Registers an intermediate whose gradient evaluate_with(probe=True) returns as p_<name>."""
    if "probe" in c:
        c["probe"][name] = x
    return x


def u_linear(m, t, c):
    """LinearFn.  Rounding points (functional.py LinearFn): forward `y` (K.linear's store);
    `ybr` (pre_out) enters only the gate gradient.  Backward: `dbr` = gate_bwd's store, then
    dropout_mask_apply's store; dx, dw, db, dgate."""
    x = t["x"]
    h = m.b(linear(x, t["w"], t.get("b")))
    if c.get("drop"):
        h = m.b(h * c["kd"].view(h.shape).to(h.dtype))
    res = t["res"] if "res" in t else 0.0
    if "gate" in t:
        return dict(out=m.f(gated(m, res, h, t["gate"])))
    return dict(out=m.f(res + h))


def u_layernorm(m, t, c):
    """LayerNormFn: forward `y`; backward dx, dw, db."""
    return dict(out=m.f(layer_norm(t["x"], t["w"], t["b"])))


def u_mlp(m, t, c):
    """MLPFn.  Forward: `hpre` (gelu' in bf16, used by the backward only), `h`, `y`.  Backward:
    `d2` after dropout_mask_apply, `dpre` (the dX epilogue x hpre), dx and the four parameter
    gradients."""
    pre = m.b(linear(t["x"], t["w1"], t["b1"]))
    h = m.f(gelu(m, pre, c["act"]))
    y = m.b(linear(h, t["w2"], t["b2"]))
    if c.get("drop"):
        y = y * c["kd"].view(y.shape).to(y.dtype)
    return dict(out=m.f((t["res"] if "res" in t else 0.0) + y))


def u_mha(m, t, c):
    """MHAFn.  Forward: `qkv` (self) or `qp`, `kvp` (cross), `o`, `out`.  Backward: `dbr` after
    dropout_mask_apply, `do`, `dqkv` / `dqp`, `dkvp`, dq_in, dkv_in and the packed in_proj
    gradients; dres = dout."""
    x = t["q_in"]
    if c["self_attn"]:
        qkv = m.fb(linear(x, t["in_w"], t["in_b"]))
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    else:
        q = m.fb(linear(x, t["in_w"][:C], t["in_b"][:C]))
        kv = _probe(c, "kvp", m.fb(linear(t["kv_in"], t["in_w"][C:], t["in_b"][C:])))
        k, v = kv[..., :C], kv[..., C:]
    o = m.fb(attention(m, q, k, v, H, False, c.get("kd_attn")))
    y = m.b(linear(o, t["out_w"], t["out_b"]))
    if c.get("kd_out") is not None:
        yd = y * c["kd_out"].view(y.shape).to(y.dtype)
        if c.get("kd_out_bwd") is not None:  # (doctored: another mask in the backward)
            yb = y * c["kd_out_bwd"].view(y.shape).to(y.dtype)
            yd = yd.detach() + yb - yb.detach()
        y = yd
    return dict(out=m.f(t["res"] + y))


def u_gpt_block(m, t, c):
    """GPTBlockFn.  Forward: xn1, qkv, y, xm, xn2, hpre, h, out.  Backward: dpre, dxn2, dxm
    (= dout + LN_2 backward in one store), dy, dqkv, dxn1, dx (= dxm + LN_1 backward)."""
    return dict(out=_gpt_block(m, t["x"], t))


def _gpt_block(m, x, t, sfx=""):
    g = lambda n: t[n + sfx]
    x = m.b(x)
    xn1 = m.fb(layer_norm(x, g("ln1_w"), g("ln1_b")))
    qkv = m.fb(linear(xn1, g("attn_w"), g("attn_b")))
    y = m.fb(attention(m, qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], H, True))
    xm = m.fb(x + linear(y, g("aproj_w"), g("aproj_b")))
    xn2 = m.fb(layer_norm(xm, g("ln2_w"), g("ln2_b")))
    pre = m.b(linear(xn2, g("fc_w"), g("fc_b")))
    h = m.f(gelu(m, pre, 1))
    return m.f(xm + linear(h, g("mproj_w"), g("mproj_b")))


def u_gpt_stack(m, t, c):
    """Two GPTBlockFn in a row (the in-place flush per block under set_overlap_blocks(1))."""
    x = t["x"]
    for l in range(L):
        x = _gpt_block(m, x, t, str(l))
    return dict(out=x)


def u_kv_only(m, t, c):
    """CrossKVFn alone: the packed [B, S, L*2C] projection; one shape group of L weight
    gradients over column slices of one dkv."""
    return dict(out=torch.cat([m.f(linear(t["z"], t[f"kv_w{l}"], t[f"kv_b{l}"])) for l in range(L)], -1))


def u_lin_lmhead(m, t, c):
    """LinearFn -> lm_head_loss: the device-scaled lm_head entry next to a plain one in one flush."""
    h = m.fb(linear(t["x"], t["pw"], t["pb"]))
    logits, loss = _lm(m, h, t["w"], c)
    return dict(out=loss, logits=logits)


def _xattn(m, x, k, v, t, sfx=""):
    """_xattn_fwd / _xattn_bwd: xn, qp, o, ybr (gate gradient only), out; dbr, do, dqp, dxn, dx."""
    g = lambda n: t[n + sfx]
    x = m.b(x)
    xn = m.fb(layer_norm(x, g("ln_w"), g("ln_b")))
    qp = m.fb(linear(xn, g("q_w"), g("q_b")))
    o = m.fb(attention(m, qp, k, v, H, False))
    br = m.b(linear(o, g("c_w"), g("c_b")))
    return m.f(gated(m, x, br, g("gate")))


def u_cross_attn(m, t, c):
    """CrossAttnFn: kvp forward, dkvp and dz backward, plus everything of _xattn."""
    kvp = m.fb(linear(t["z"], t["kv_w"], t["kv_b"]))
    return dict(out=_xattn(m, t["x"], kvp[..., :C], kvp[..., C:], t))


def u_cross_kv(m, t, c):
    """CrossKVFn + L CrossAttnKVFn over one KVGradSlab: two gated cross-attention blocks in a
    row, each with a kv_proj of its own over the same z.  The packed `kv` forward; the slab's
    columns and dz (ONE GEMM over K = L*2C: one rounding of the layers' sum) backward."""
    x = t["x"]
    for l in range(L):
        kvp = _probe(c, f"kvp{l}", m.fb(linear(t["z"], t[f"kv_w{l}"], t[f"kv_b{l}"])))
        x = _xattn(m, x, kvp[..., :C], kvp[..., C:], t, str(l))
    return dict(out=x)


def u_embed(m, t, c):
    """EmbedFn: out = wte[idx] + wpe[arange(T)] (one store) behind the prefix rows; backward:
    per-id / per-position sums, dprefix = the prefix rows of dout."""
    idx = c["idx"]
    wte = t["wte"].detach() if c.get("detach_embed") else t["wte"]  # (doctored: lm_head part only)
    x = m.f(wte[idx] + t["wpe"][: idx.shape[1]])
    if "prefix" in t:
        x = torch.cat([t["prefix"], x], dim=1)
    return dict(out=x)


def _lm(m, x, w, c):
    V = c["V"]
    logits = m.f(linear(x, w))
    off, Tt = c["off"], c["tgt"].shape[1]
    rows = logits[:, off:off + Tt].reshape(-1, V)
    loss = ce_loss(m, rows, c["tgt"].reshape(-1), c.get("mask"), c.get("mask_mode", False))
    return logits, loss


def u_lmhead(m, t, c):
    """lm_head_loss (LMHeadLossFn + pad_vocab): `logits`; `dl` = softmax - onehot in bf16 before
    the device scale; dx (text rows at `off`, zero elsewhere) and dw."""
    logits, loss = _lm(m, t["x"], t["w"], c)
    return dict(out=loss, logits=logits)


def u_tied(m, t, c):
    """EmbedFn -> LayerNormFn -> lm_head_loss over one tied wte: its gradient is the sum of the
    embedding rows' and the lm_head's contributions in one buffer."""
    x = u_embed(m, t, c)["out"]
    xn = m.fb(layer_norm(m.b(x), t["ln_w"], t["ln_b"]))
    logits, loss = _lm(m, xn, t["wte"], c)
    return dict(out=loss, logits=logits)


def u_query_expand(m, t, c):
    """QueryExpandFn: a copy; backward the batch sum in one store."""
    return dict(out=t["q"].unsqueeze(0).expand(c["B"], -1, -1) * 1.0)


def u_self_attn(m, t, c):
    """_SelfAttnFn: causal attention over packed qkv; y forward, dqkv backward."""
    qkv = t["qkv"]
    return dict(out=m.f(attention(m, qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], H, True)))


def u_cross_sdpa(m, t, c):
    """_CrossSDPAFn: q over packed kv, not causal."""
    return dict(out=m.f(attention(m, t["q"], t["kv"][..., :C], t["kv"][..., C:], H, False)))


def u_qformer(m, t, c):
    """One QFormerLayer-shaped chain in train mode: q -> q + f(LN(q)) three times (MHAFn self,
    MHAFn cross over LN(v), MLPFn act 2), each unit with the detached stream as its residual,
    ResTapFn + ResTape handing the residual gradient to LayerNormFn: dq of each stage is
    residual path + LN path in ONE store (gvl_layernorm_bwd_res)."""
    q = m.b(t["q"])
    q2 = m.fb(layer_norm(q, t["ln1_w"], t["ln1_b"]))
    q = m.b(u_mha(m, dict(q_in=q2, in_w=t["sa_in_w"], in_b=t["sa_in_b"], out_w=t["sa_out_w"],
                          out_b=t["sa_out_b"], res=q),
                  dict(self_attn=True, kd_attn=c["kd_attn0"], kd_out=c["kd_out0"]))["out"])
    q2 = m.fb(layer_norm(q, t["ln2q_w"], t["ln2q_b"]))
    v2 = m.fb(layer_norm(t["v"], t["ln2v_w"], t["ln2v_b"]))
    q = m.b(u_mha(m, dict(q_in=q2, kv_in=v2, in_w=t["ca_in_w"], in_b=t["ca_in_b"],
                          out_w=t["ca_out_w"], out_b=t["ca_out_b"], res=q),
                  dict(self_attn=False, kd_attn=c["kd_attn1"], kd_out=c["kd_out1"]))["out"])
    q2 = m.fb(layer_norm(q, t["ln3_w"], t["ln3_b"]))
    return u_mlp(m, dict(x=q2, w1=t["w1"], b1=t["b1"], w2=t["w2"], b2=t["b2"], res=q),
                 dict(act=2, drop=True, kd=c["kd_mlp"]))


UNITS = dict(linear=u_linear, layernorm=u_layernorm, mlp=u_mlp, mha=u_mha, gpt_block=u_gpt_block,
             cross_attn=u_cross_attn, cross_kv=u_cross_kv, embed=u_embed, lmhead=u_lmhead,
             tied=u_tied, query_expand=u_query_expand, self_attn=u_self_attn,
             cross_sdpa=u_cross_sdpa, qformer=u_qformer, gpt_stack=u_gpt_stack, kv_only=u_kv_only,
             lin_lmhead=u_lin_lmhead)

# ------------------------------------------------------------------------------- cases
# name -> (unit, settings).  Shapes: the smallest at which the wiring can go wrong (C = 128 = 2
# heads of 64; 99 LayerNorm rows = 13 backward blocks, the last partial; T = 33 crosses 32).
CASES = {
    "linear": ("linear", dict()),
    "linear_nobias": ("linear", dict(bias=False, N=517)),  # lm_logits, the pad_vocab path
    "linear_res": ("linear", dict(res=True)),
    "linear_drop": ("linear", dict(drop=True)),
    "linear_res_gate": ("linear", dict(res=True, gate=0.3)),
    "linear_res_gate_neg": ("linear", dict(res=True, gate=-4.0)),
    "linear_res_gate_drop": ("linear", dict(res=True, gate=0.3, drop=True)),
    "layernorm": ("layernorm", dict()),
    "mlp_tanh": ("mlp", dict(act=1)),
    "mlp_erf_res_drop": ("mlp", dict(act=2, res=True, drop=True)),
    "mha_self": ("mha", dict(self_attn=True, p_attn=0.0, p_out=0.0)),
    "mha_self_drop": ("mha", dict(self_attn=True, p_attn=DROP_P, p_out=DROP_P)),
    "mha_cross": ("mha", dict(self_attn=False, p_attn=0.0, p_out=0.0)),
    "mha_cross_drop": ("mha", dict(self_attn=False, p_attn=DROP_P, p_out=DROP_P)),
    "gpt_block": ("gpt_block", dict()),
    "cross_attn": ("cross_attn", dict(gate=0.3)),
    "cross_attn_neg": ("cross_attn", dict(gate=-4.0)),
    "cross_kv": ("cross_kv", dict(gates=(0.3, -4.0))),
    "embed": ("embed", dict(V=520)),
    "embed_prefix": ("embed", dict(V=517, prefix=32, Tt=15)),
    "lmhead_520": ("lmhead", dict(V=520, off=0, S=33, Tt=33)),
    "lmhead_517_prefix": ("lmhead", dict(V=517, off=32, S=47, Tt=15)),
    "lmhead_mask": ("lmhead", dict(V=520, off=32, S=47, Tt=15, mask=True, mask_mode=False)),
    "lmhead_mask_mode": ("lmhead", dict(V=517, off=0, S=33, Tt=33, mask=True, mask_mode=True)),
    "tied": ("tied", dict(V=520, off=0, Tt=33)),
    "tied_prefix": ("tied", dict(V=517, off=32, prefix=32, Tt=15)),
    "query_expand": ("query_expand", dict()),
    "self_attn": ("self_attn", dict()),
    "cross_sdpa": ("cross_sdpa", dict()),
    "qformer": ("qformer", dict()),
    # flush routes: 64 rows, since the batched / grouped launches need K % 32 == 0, K >= 64
    "mlp_k64": ("mlp", dict(act=1, BT=(2, 32))),
    "gpt_stack": ("gpt_stack", dict(BT=(2, 32))),
    "kv_only": ("kv_only", dict(BT=(2, 32))),
    "kv_only_99": ("kv_only", dict(BT=(B, S_CLIP))),
    "lin_lmhead": ("lin_lmhead", dict(V=520, off=0, BT=(2, 32))),
}
# gradients that form one whole-vector line although they are 2-D
WHOLE = ("q",)


def _gen(name):
    return torch.Generator().manual_seed(9000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))


def _ids(g, shape, V):
    """Token ids with repeats, id 0 and id V - 1 present; most of the table absent."""
    idx = torch.randint(0, 40, shape, generator=g)
    flat = idx.view(-1)
    flat[0], flat[1], flat[2], flat[-1] = 0, V - 1, 7, 7
    return idx


def _targets(g, shape, V):
    tg = torch.randint(0, V, shape, generator=g)
    flat = tg.view(-1)
    flat[1], flat[5], flat[-1] = -100, -100, -100
    flat[2], flat[3] = 0, V - 1
    return tg


@functools.lru_cache(maxsize=None)
def inputs(name, offset=0):
    """(tensors: name -> bf16 CPU tensor, the differentiable inputs in the order of use, `dout`
    among them under its own name; settings: ints, index tensors and the keep / (1 - p)
    multipliers for seed offset `offset`)."""
    unit, cfg = CASES[name]
    g = _gen(name)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF)
    wgt = lambda n, k: rn(n, k, scale=1.0 / math.sqrt(k))
    bias = lambda n: rn(n, scale=0.1)
    lnw = lambda: (1 + 0.1 * torch.randn(C, generator=g)).to(BF)
    t, c = {}, dict(cfg)
    Bc, Tc = cfg.get("BT", (B, T))  # (the flush-route cases: 64 rows, a multiple of the K-step)
    dshape = (Bc, Tc, C)
    if unit == "linear":
        N = cfg.get("N", C)
        t["x"], t["w"] = rn(B, T, C), wgt(N, C)
        if cfg.get("bias", True):
            t["b"] = bias(N)
        if cfg.get("res"):
            t["res"] = rn(B, T, N)
        if "gate" in cfg:
            t["gate"] = torch.tensor(cfg["gate"]).to(BF)
        if cfg.get("drop"):
            c["kd"] = keep_rows(SEED, offset, B * T, N, DROP_P)
        dshape = (B, T, N)
    elif unit == "layernorm":
        t["x"], t["w"], t["b"] = rn(B, T, C, scale=2.0), lnw(), bias(C)
    elif unit == "mlp":
        t["x"], t["w1"], t["b1"] = rn(Bc, Tc, C), wgt(4 * C, C), bias(4 * C)
        t["w2"], t["b2"] = wgt(C, 4 * C), bias(C)
        if cfg.get("res"):
            t["res"] = rn(Bc, Tc, C)
        if cfg.get("drop"):
            c["kd"] = keep_rows(SEED, offset, Bc * Tc, C, DROP_P)
    elif unit == "mha":
        Tq = Q if not cfg["self_attn"] else T
        t["q_in"] = rn(B, Tq, C)
        if not cfg["self_attn"]:
            t["kv_in"] = rn(B, S_CLIP, C)
        t["in_w"], t["in_b"] = wgt(3 * C, C), bias(3 * C)
        t["out_w"], t["out_b"], t["res"] = wgt(C, C), bias(C), rn(B, Tq, C)
        Tk = Tq if cfg["self_attn"] else S_CLIP
        c["kd_attn"] = c["kd_out"] = None
        if cfg["p_attn"] > 0:
            c["kd_attn"] = keep_attn(SEED ^ ATTN_XOR, offset, B, H, Tq, Tk, cfg["p_attn"])
        if cfg["p_out"] > 0:
            c["kd_out"] = keep_rows(SEED, offset, B * Tq, C, cfg["p_out"])
        dshape = (B, Tq, C)
    elif unit in ("gpt_block", "gpt_stack"):
        t["x"] = rn(Bc, Tc, C)
        for s in ([""] if unit == "gpt_block" else [str(l) for l in range(L)]):
            t["ln1_w" + s], t["ln1_b" + s] = lnw(), bias(C)
            t["attn_w" + s], t["attn_b" + s] = wgt(3 * C, C), bias(3 * C)
            t["aproj_w" + s], t["aproj_b" + s] = wgt(C, C), bias(C)
            t["ln2_w" + s], t["ln2_b" + s] = lnw(), bias(C)
            t["fc_w" + s], t["fc_b" + s] = wgt(4 * C, C), bias(4 * C)
            t["mproj_w" + s], t["mproj_b" + s] = wgt(C, 4 * C), bias(C)
    elif unit == "kv_only":
        t["z"] = rn(Bc, Tc, C)
        for l in range(L):
            t[f"kv_w{l}"], t[f"kv_b{l}"] = wgt(2 * C, C), bias(2 * C)
        dshape = (Bc, Tc, L * 2 * C)
    elif unit == "lin_lmhead":
        t["x"], t["pw"], t["pb"] = rn(Bc, Tc, C), wgt(C, C), bias(C)
        t["w"] = rn(cfg["V"], C, scale=0.04)
        c["tgt"] = _targets(g, (Bc, Tc), cfg["V"])
        dshape = ()
    elif unit in ("cross_attn", "cross_kv"):
        t["x"], t["z"] = rn(B, T, C), rn(B, S_CLIP, C)
        sfxs = [""] if unit == "cross_attn" else [str(l) for l in range(L)]
        gates = [cfg["gate"]] if unit == "cross_attn" else cfg["gates"]
        for s, gv in zip(sfxs, gates):
            t["ln_w" + s], t["ln_b" + s] = lnw(), bias(C)
            t["q_w" + s], t["q_b" + s] = wgt(C, C), bias(C)
            t["kv_w" + s], t["kv_b" + s] = wgt(2 * C, C), bias(2 * C)
            t["c_w" + s], t["c_b" + s] = wgt(C, C), bias(C)
            t["gate" + s] = torch.tensor(gv).to(BF)
    elif unit in ("embed", "tied"):
        V, M, Tt = cfg["V"], cfg.get("prefix", 0), cfg.get("Tt", T)
        c["idx"] = _ids(g, (B, Tt), V)
        # wte at GPT-2's scale: logits of order 0.5, so that their bf16 rounding does not
        # dominate the softmax (at logits of order 6 it moves a probability by 3 %)
        t["wte"], t["wpe"] = rn(V, C, scale=0.04), rn(64, C, scale=0.04)
        if M:
            t["prefix"] = rn(B, M, C)
        dshape = (B, M + Tt, C)
        if unit == "tied":
            t["ln_w"], t["ln_b"] = lnw(), bias(C)
            c["tgt"] = _targets(g, (B, Tt), V)
            dshape = ()
    elif unit == "lmhead":
        V, S, Tt = cfg["V"], cfg["S"], cfg["Tt"]
        t["x"], t["w"] = rn(B, S, C), rn(V, C, scale=0.04)  # logits of order 0.5, see above
        c["tgt"] = _targets(g, (B, Tt), V)
        if cfg.get("mask"):
            mk = torch.rand(B, Tt, generator=g) < 0.7
            mk.view(-1)[1] = True   # a set mask entry over an ignored target
            mk.view(-1)[2] = False
            c["mask"] = mk
        dshape = ()
    elif unit == "query_expand":
        t["q"] = rn(Q, C)
        c["B"] = B
        dshape = (B, Q, C)
    elif unit == "self_attn":
        t["qkv"] = rn(B, T, 3 * C)
    elif unit == "cross_sdpa":
        t["q"], t["kv"] = rn(B, T, C), rn(B, S_CLIP, 2 * C)
    elif unit == "qformer":
        t["q"], t["v"] = rn(B, Q, C), rn(B, S_CLIP, C)
        for ln in ("ln1", "ln2q", "ln2v", "ln3"):
            t[ln + "_w"], t[ln + "_b"] = lnw(), bias(C)
        for a in ("sa", "ca"):
            t[a + "_in_w"], t[a + "_in_b"] = wgt(3 * C, C), bias(3 * C)
            t[a + "_out_w"], t[a + "_out_b"] = wgt(C, C), bias(C)
        t["w1"], t["b1"], t["w2"], t["b2"] = wgt(4 * C, C), bias(4 * C), wgt(C, 4 * C), bias(C)
        c["seeds"] = (SEED, SEED + 11, SEED + 23)
        c["kd_attn0"] = keep_attn(c["seeds"][0] ^ ATTN_XOR, offset, B, H, Q, Q, DROP_P)
        c["kd_out0"] = keep_rows(c["seeds"][0], offset, B * Q, C, DROP_P)
        c["kd_attn1"] = keep_attn(c["seeds"][1] ^ ATTN_XOR, offset, B, H, Q, S_CLIP, DROP_P)
        c["kd_out1"] = keep_rows(c["seeds"][1], offset, B * Q, C, DROP_P)
        c["kd_mlp"] = keep_rows(c["seeds"][2], offset, B * Q, C, DROP_P)
        dshape = (B, Q, C)
    else:
        raise KeyError(unit)
    dout = torch.tensor(DLOSS) if dshape == () else torch.randn(*dshape, generator=g).to(BF)
    return t, c, dout


def evaluate_with(name, mode, offset=0, settings=None, probe=False):
    """One evaluation of case `name` in `mode` -> dict of float64 numpy arrays: `out` (the loss for
    the loss units), `logits` where there are any, and `d_<input>` for every input tensor.
    `settings` overrides entries of the case settings (the doctored-mask tests)."""
    unit, _ = CASES[name]
    t, c, dout = inputs(name, offset)
    c = dict(c, **(settings or {}))
    if probe:
        c["probe"] = {}
    leaves = {k: v.to(mode.dt).requires_grad_() for k, v in t.items()}
    outs = UNITS[unit](mode, leaves, c)
    out = outs["out"]
    probes = c.get("probe", {})
    grads = torch.autograd.grad(out, list(leaves.values()) + list(probes.values()),
                                dout.to(mode.dt).expand_as(out), allow_unused=True)
    res = dict(out=f64(out if (not mode.rnd or out.dim() == 0) else _r(out)))
    if "logits" in outs:
        res["logits"] = f64(outs["logits"])
    for k, g in zip(leaves, grads):
        g = torch.zeros_like(leaves[k]) if g is None else g
        res["d_" + k] = f64(_r(g) if mode.rnd else g)
    for k, g in zip(probes, grads[len(leaves):]):
        res["p_" + k] = f64(g)
    return res


@functools.lru_cache(maxsize=None)
def evaluate(name, mode_name, offset=0):
    return evaluate_with(name, MODES[mode_name], offset)


# ----------------------------------------------------------------------------- the loss
def loss_of_logits(name, logits):
    """The fp32 loss is one step from the bf16 logits the Function itself stored (which are held
    to the line bound): -> (float64 loss of those logits over the case's targets / mask, scale =
    the mean over the counted rows of |lse| + |x_target|, slack = MARGIN x the error of the same
    formula in fp32 torch in units of 2**-24 * scale, floored at one unit), as the row-wise tests
    take theirs."""
    c = inputs(name)[1]
    V, off, Tt = c["V"], c.get("off", 0), c["tgt"].shape[1]
    x = torch.as_tensor(f64(logits))[:, off:off + Tt, :V].reshape(-1, V)
    tgt = c["tgt"].reshape(-1)
    mask, mm = c.get("mask"), c.get("mask_mode", False)
    ref = float(ce_loss(REF, x, tgt, mask, mm))
    valid = tgt != -100
    if mask is not None:
        valid = valid & mask.reshape(-1).bool()
    n = float(mask.sum().clamp(min=1)) if mm else float(valid.sum())
    terms = torch.logsumexp(x, -1).abs() + x.gather(-1, tgt.clamp(min=0)[:, None])[:, 0].abs()
    scale = float((terms * valid).sum() / n)
    l32 = float(ce_loss(REF, x.to(F32), tgt, mask, mm))
    base = abs(l32 - ref) / (2.0 ** -24 * scale)
    return ref, scale, MARGIN * max(base, 1.0)


# ------------------------------------------------------------------------------- bounds
def line_scale(key, ref):
    """s_i broadcast to ref's shape: the rms of each row; one whole line for 1-D tensors, the
    query-token gradient and scalars."""
    ref = f64(ref)
    if ref.ndim <= 1 or key in tuple("d_" + w for w in WHOLE):
        return np.full(ref.shape, math.sqrt(float((ref * ref).mean())) if ref.size else 0.0)
    return np.broadcast_to(np.sqrt((ref * ref).mean(axis=-1, keepdims=True)), ref.shape)


def u_of(key, ref, emu):
    """U_t = max over lines of max_j |emu - ref| / s_i (from the reference and emulation alone)."""
    s = line_scale(key, ref)
    err = np.abs(f64(emu) - f64(ref))
    assert (err[s == 0] == 0).all(), f"{key}: the emulation is off where the reference line is zero"
    return float((err[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0


def tolerance(key, ref, emu, g0=None):
    """(target, tol, s, U): tol = ulp_bf16(target) + MARGIN * U_t * s_i per element, exactly zero
    where s_i == 0 and nothing is accumulated."""
    ref = f64(ref)
    s, U = line_scale(key, ref), u_of(key, ref, emu)
    target = ref if g0 is None else ref + f64(g0)
    tol = ulp_bf16(target) + MARGIN * U * s
    if g0 is None:
        tol = np.where(s == 0, 0.0, tol)
    return target, tol, s, U


def violations(key, got, ref, emu, g0=None):
    """(number of elements out of bound, ratio, units): ratio = max |got - target| / tol (<= 1
    passes), units = the worst line error / (U_t * s_i) where that is defined."""
    target, tol, s, U = tolerance(key, ref, emu, g0)
    got = f64(got)
    assert got.shape == target.shape, f"{key}: shape {got.shape} vs {target.shape}"
    err = np.abs(got - target)
    err = np.where(np.isnan(err), np.inf, err)
    bad = err > tol
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
        den = U * s
        units = np.where(den > 0, err / den, 0.0)
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0, \
        float(units.max()) if units.size else 0.0, bad


RATIOS = {}


def assert_line_close(case, key, got, ref, emu, g0=None, path="plain"):
    """Holds `got` to the bound and records the measured ratio (profiles/fn_margins.json)."""
    n, ratio, units, bad = violations(key, got, ref, emu, g0)
    RATIOS.setdefault(case, {})[f"{path}:{key}"] = dict(ratio=ratio, units=units)
    margins_out("fn_margins", RATIOS)
    if n:
        i = tuple(int(k) for k in np.unravel_index(int(np.argmax(bad)), bad.shape)) if bad.ndim else ()
        target = f64(ref) if g0 is None else f64(ref) + f64(g0)
        raise AssertionError(
            f"{case} {path} {key}: {n} of {bad.size} elements out of bound (worst ratio {ratio:.3g}, "
            f"{units:.3g} x U s); first at {i}: got {float(f64(got)[i])!r} want {float(target[i])!r}")
    return ratio


# ----------------------------------------------------------------------- old criteria
def old_tensor_ok(got, ref):
    """test_backward_grads' criterion: within 1.2e-1 of the tensor's largest element."""
    ref = f64(ref)
    return float(np.abs(f64(got) - ref).max()) < 1.2e-1 * max(float(np.abs(ref).max()), 1e-30)


def old_arena_ok(gots, refs):
    """test_fused_grad_accumulation's: one max-norm over all gradients concatenated, 1e-2."""
    a = np.concatenate([f64(g).reshape(-1) for g in gots])
    b = np.concatenate([f64(r).reshape(-1) for r in refs])
    return float(np.abs(a - b).max()) < 1e-2 * float(np.abs(b).max())
