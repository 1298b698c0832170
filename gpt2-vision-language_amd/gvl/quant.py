"""Int8 weight-only decoding: the quantised weight format and the quantised copy of a decoder.

A decode step at small batch reads every block matrix and the lm_head once per token, so its
device time is the weight stream.  Here an nn.Linear weight [N, K] is stored as int8 with one
fp32 scale per output row (symmetric, no zero point; include/gvl.h has the arithmetic) and
multiplied by gvl_linear_w8, a kernel for a few rows of x that streams it once.

Quantised: per block c_attn, attn.c_proj, c_fc, mlp.c_proj; the cross-att model's q_proj and
xattn.c_proj; the lm_head (padded to a multiple of 8 rows once).  Kept in bf16: wte / wpe for
the embedding (tied to the lm_head or not), the LayerNorm parameters, and kv_proj, vis_proj and
the caption bridges, which run once per call at many rows.

The reference has no counterpart: it decodes in the weights' own precision
(train_gpt2.py:440-449, gpt2_linear/data.py:111-127).  The mode is opt-in (weights="int8" on
the gvl.decode entry points); nothing changes without it.
"""
from __future__ import annotations

import torch

from . import functional as Fn
from . import kernels as K
from .functional import bf

BF16 = torch.bfloat16
ACCEPTED = 'None, "int8" or a gvl.quant.quantize_decoder(model) result'


class QWeight:
    """One quantised nn.Linear weight: q int8 [Np, K], scale fp32 [Np], rows = the true row count
    N <= Np (Np > N where the rows were padded to a multiple of 8: outputs then have Np columns,
    the pad columns zero, and the caller slices)."""

    __slots__ = ("q", "scale", "rows")

    def __init__(self, q, scale, rows=None):
        self.q, self.scale = q, scale
        self.rows = q.shape[0] if rows is None else int(rows)

    @property
    def shape(self):
        return self.q.shape

    def linear(self, x2, bias=None, *, scratch=None, dequant=False, **epi):
        """epi(x2 @ W.T): gvl_linear_w8 up to its row cap; above it (or with dequant=True: the
        prefill) the weight is dequantised into `scratch` (bf16, at least Np * K elements, owned
        by the caller; allocated here when None) and goes through K.linear."""
        if not dequant and x2.shape[0] <= K.LINEAR_W8_MAX_ROWS:
            return K.linear_w8(x2, self.q, self.scale, bias, **epi)
        return K.linear(x2, dequantize(self, scratch), bias, **epi)


def quantize_weight(w):
    """QWeight of a bf16 [N, K] weight (N padded with zero rows to a multiple of 8).  One host
    read: raises ValueError if a weight is not finite (its row's scale is then not finite)."""
    w = bf(w)
    if w.dim() != 2:
        raise ValueError(f"quantize_weight: a 2-D weight is needed (got {tuple(w.shape)})")
    wp, N = Fn.pad_vocab(w)
    q, scale = K.quantize_rows_i8(wp.contiguous())
    if not bool(torch.isfinite(scale).all()):
        raise ValueError("quantize_weight: the weight holds a value that is not finite")
    return QWeight(q, scale, N)


def dequantize(qw, out=None):
    """bf16 [Np, K] = bf16(fp32(q) * scale[n]).  out: a bf16 buffer of at least Np * K elements
    (any shape) to write into."""
    Np, Kd = qw.q.shape
    if out is not None:
        if out.dtype != BF16 or out.numel() < Np * Kd or not out.is_contiguous():
            raise ValueError("dequantize: out must be a contiguous bf16 buffer of >= N * K elements")
        out = out.view(-1)[:Np * Kd].view(Np, Kd)
    return K.dequantize_rows_i8(qw.q, qw.scale, out)


class QuantizedDecoder:
    """The quantised matrices of one model, as the decoders of gvl.decode take them: blocks[l] =
    dict(attn, aproj, fc, mproj), cross[l] = dict(q, c) for the cross-att model (else None), head.

    A snapshot: it holds the weights as they were when quantize_decoder ran and does not follow
    later training of the model (quantise again after an optimizer step)."""

    def __init__(self, blocks, cross, head, n_embd):
        self.blocks, self.cross, self.head, self.n_embd = blocks, cross, head, n_embd

    def scratch_elems(self):
        """Elements of the largest block matrix (4 C^2): the prefill's dequantisation buffer."""
        return max(w.q.numel() for b in self.blocks for w in b.values())


@torch.no_grad()
def quantize_decoder(model):
    """QuantizedDecoder of a gvl.gpt2.GPT, gvl.caption.GPT_Caption (its decoder) or
    gvl.cross_att.GPT on the GPU.  Pass it as `weights=` to the gvl.decode entry points so that
    repeated calls do not quantise again.  A snapshot: it does not follow later training."""
    from . import caption, cross_att
    dec = model.gpt if isinstance(model, caption.GPT_Caption) else model
    tr = dec.transformer
    blocks = [dict(attn=quantize_weight(b.attn.c_attn.weight),
                   aproj=quantize_weight(b.attn.c_proj.weight),
                   fc=quantize_weight(b.mlp.c_fc.weight),
                   mproj=quantize_weight(b.mlp.c_proj.weight)) for b in tr.h]
    cross = None
    if isinstance(model, cross_att.GPT):
        cross = [dict(q=quantize_weight(b.xattn.q_proj.weight),
                      c=quantize_weight(b.xattn.c_proj.weight)) for b in tr.h]
    return QuantizedDecoder(blocks, cross, quantize_weight(dec.lm_head.weight),
                            tr.wte.weight.shape[1])


def check_weights(weights):
    """ValueError unless `weights` is an accepted value (no device is touched)."""
    if weights is None or isinstance(weights, QuantizedDecoder):
        return
    if isinstance(weights, str) and weights == "int8":
        return
    raise ValueError(f"weights={weights!r}: accepted values are {ACCEPTED}")


def resolve_weights(model, weights):
    """None (bf16) or the QuantizedDecoder for `weights` (quantising `model` for "int8")."""
    check_weights(weights)
    if isinstance(weights, str):
        return quantize_decoder(model)
    return weights
