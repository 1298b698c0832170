"""float64 reference, per-element error scales and a bf16-rounding emulation of the fused
attention kernels (csrc/attention.hip, csrc/decode.hip), the restated dropout hash, the route
table of gvl_attn_fwd / gvl_attn_bwd and the case lists.  Shared by test_attn_ref_cpu.py, which
proves that the per-element assertions reject doctored outputs the max-norm comparison accepts,
and test_gpu_attention.py, which holds the HIP kernels to them.  Everything here runs on the
CPU and reads the same bf16 values the kernels read; nothing reads a kernel's output."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests.helpers import err_units, f64

BF = torch.bfloat16
F64 = torch.float64
OUTS = ("o", "dq", "dk", "dv")
HARD_UNITS = dict(o=2, dv=2, dq=3, dk=3)  # roundings per output, see test_gpu_attention.py

# ------------------------------------------------------------------------- dropout hash
_M64 = (1 << 64) - 1


def mix64(z):
    """common.h seed_eff's mixing of the device-side step offset (include/gvl.h: seed_eff =
    seed ^ mix64(*seed_ptr))."""
    z = ((z + 0x632BE59BD9B4E019) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def seed_eff(seed, offset=None):
    """The seed the kernels hash with: `seed` when there is no seed_ptr or it points at zero."""
    seed &= _M64
    if offset is None or offset == 0:
        return seed
    return seed ^ mix64(offset & _M64)


def keep_mask(seed, B, H, Tq, Tk, p, row_len=None):
    """bool [B, H, Tq, Tk]: common.h rng_keep on element index ((b*H + h)*Tq + q)*Tk + k
    (test_gpu_kernels.keep_mask restated for that index).  row_len: a wrong row length, for the
    doctored-output tests."""
    rl = Tk if row_len is None else row_len
    rows = np.arange(B * H * Tq, dtype=np.uint64).reshape(B, H, Tq, 1)
    idx = rows * np.uint64(rl) + np.arange(Tk, dtype=np.uint64)
    G, M1, M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) + (idx + np.uint64(1)) * G
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        z = z ^ (z >> np.uint64(31))
    thresh = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    return (z >> np.uint64(32)) >= thresh


def drop_scale(p):
    """attention.hip fill(): 1.f / (1.f - drop_p) in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


# ---------------------------------------------------------------------------- formulas
def visible(Tq, Tk, causal):
    """bool [Tq, Tk]: key k is visible to query q.  Causal is the top-left mask k <= q for any
    Tq, Tk (attention.hip `kk > ql`, oracle.ops.attention)."""
    if not causal:
        return torch.ones(Tq, Tk, dtype=torch.bool)
    return torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None]


def _formulas(q, k, v, dO, vis, scale, kd, dt):
    """Forward and closed-form backward in dtype dt; kd = keep * drop_scale or None."""
    q, k, v, dO = (t.to(dt) for t in (q, k, v, dO))
    kd = None if kd is None else kd.to(dt)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    Pd = P if kd is None else P * kd
    o = Pd @ v
    dP = dO @ v.transpose(-1, -2)
    if kd is not None:
        dP = dP * kd
    D = (dO * o).sum(-1, keepdim=True)
    dS = P * (dP - D)
    out = dict(o=o, lse=(m + torch.log(l)).squeeze(-1), dq=scale * (dS @ k),
               dk=scale * (dS.transpose(-1, -2) @ q), dv=Pd.transpose(-1, -2) @ dO)
    return out, dict(m=m, e=e, l=l, P=P, Pd=Pd, dP=dP, s=s)


def _bf(t):
    """Round to bf16 (through fp32, as the kernels' v_cvt_pk_bf16_f32 does), back to float64."""
    return t.to(torch.float32).to(BF).to(F64)


def attention_ref(q, k, v, dO, causal, scale, drop_p=0.0, keep=None):
    """q, dO [B, H, Tq, 64], k, v [B, H, Tk, 64] bf16; keep: bool [B, H, Tq, Tk] or None.
    Returns (ref, E, emu), dicts of float64 numpy arrays:
    ref: o, lse (the natural-log row logsumexp of scale*q.k over the visible keys, dropout or
         not, include/gvl.h), dq, dk, dv in closed form: P from lse, dP = dO V^T (masked,
         /(1-p)), D = rowsum(dO o), dS = P (dP - D), dq = scale dS K, dk = scale dS^T Q,
         dv = P_drop^T dO.
    E:   per-element error scales, the same products with every term replaced by its absolute
         value; lse: |lse| + scale * max over the visible keys of sum_d |q_d k_d|.
    emu: the same formulas rounded to bf16 only where the kernels round:
         - the un-normalised P before P.V (attention.hip pack_frag in attn_fwd_kernel /
           attn_fwd_dma_kernel; with dropout after the 1/(1-p) factor), the no-dropout
           denominator of o being the sum of those rounded values (the ones-fragment MFMA,
           o[g][4]); the emulation exponentiates against the row's final maximum where the
           kernels use the running maximum of the deferred rescale;
         - P_drop before P^T dO and dS before dS K and dS^T Q (pack_frag in the dQ, dK/dV
           and short kernels);
         - the stored o that D = rowsum(dO o) is formed from;
         - the four outputs.
         lse is not rounded: it comes from the fp32 sum of the unrounded exponentials."""
    scale = float(np.float32(scale))
    Tq, Tk = q.shape[2], k.shape[2]
    vis = visible(Tq, Tk, causal)
    kd = None
    if keep is not None:
        kd = torch.as_tensor(keep).to(F64) * drop_scale(drop_p)
    q, k, v, dO = (t.to(F64) for t in (q, k, v, dO))
    ref, x = _formulas(q, k, v, dO, vis, scale, kd, F64)
    # error scales
    aq, ak, av, ad = q.abs(), k.abs(), v.abs(), dO.abs()
    E = dict(o=x["Pd"] @ av, dv=x["Pd"].transpose(-1, -2) @ ad)
    A = ad @ av.transpose(-1, -2)
    if kd is not None:
        A = A * kd
    S_abs = x["P"] * (A + (ad * E["o"]).sum(-1, keepdim=True))
    E["dq"] = scale * (S_abs @ ak)
    E["dk"] = scale * (S_abs.transpose(-1, -2) @ aq)
    sa = (aq @ ak.transpose(-1, -2)).masked_fill(~vis, 0.0).amax(-1)
    E["lse"] = ref["lse"].abs() + scale * sa
    # emulation
    if kd is None:
        pb = _bf(x["e"])
        o_e = _bf((pb @ v) / pb.sum(-1, keepdim=True))
    else:
        o_e = _bf((_bf(x["e"] * kd) @ v) / x["l"])
    Pd_e = _bf(x["Pd"])
    dS_e = _bf(x["P"] * (x["dP"] - (dO * o_e).sum(-1, keepdim=True)))
    emu = dict(o=o_e, lse=ref["lse"], dq=_bf(scale * (dS_e @ k)),
               dk=_bf(scale * (dS_e.transpose(-1, -2) @ q)), dv=_bf(Pd_e.transpose(-1, -2) @ dO))
    n = lambda d: {a: b.numpy() for a, b in d.items()}
    return n(ref), n(E), n(emu)


def attention_f32(q, k, v, dO, causal, scale, drop_p=0.0, keep=None):
    """The same formulas in fp32 torch on the CPU (the baseline of the fp32 `slack`)."""
    scale = float(np.float32(scale))
    vis = visible(q.shape[2], k.shape[2], causal)
    kd = None if keep is None else torch.as_tensor(keep).to(F64) * drop_scale(drop_p)
    out, _ = _formulas(q, k, v, dO, vis, scale, kd, torch.float32)
    return {a: f64(b) for a, b in out.items()}


# ------------------------------------------------------------------------------ inputs
def inputs(B, H, Tq, Tk, seed=0):
    """i.i.d. normal bf16 q, k, v, dO as [B, H, T, 64]."""
    g = torch.Generator().manual_seed(7000 + 1000 * seed + 31 * Tq + Tk)
    r = lambda T: torch.randn(B, H, T, 64, generator=g).to(BF)
    return r(Tq), r(Tk), r(Tk), r(Tq)


STRUCTURED = ("rising", "span60", "low", "same", "dO0")


def structured_inputs(kind, B, H, Tq, Tk, scale):
    """Inputs that i.i.d. normals never give (u is the unit vector of 64 entries 1/8):
    rising: k_j carries 1.5 j / 64 / scale along u and q two u, so every row's score rises by
            about 3 per 64-key tile and the running maximum moves in every tile;
    span60: q, k scaled for a score deviation of 20, so scores span about +-60: rows are nearly
            one-hot and most exponentials underflow;
    low:    q + a u, k - a u with scale a^2 = 200: every visible score is below -100;
    same:   all keys identical: o is the exact mean of the visible v, lse = s + ln(n);
    dO0:    dO = 0: the three gradients are exactly zero."""
    q, k, v, dO = (t.float() for t in inputs(B, H, Tq, Tk, seed=3))
    u = torch.full((64,), 0.125)
    if kind == "rising":
        q = 0.25 * q + 2.0 * u
        k = 0.25 * k + (1.5 / 64.0 / scale) * torch.arange(Tk, dtype=torch.float32)[:, None] * u
    elif kind == "span60":
        f = math.sqrt(20.0 / (8.0 * scale))
        q, k = q * f, k * f
    elif kind == "low":
        a = math.sqrt(200.0 / scale)
        q, k = 0.5 * q + a * u, 0.5 * k - a * u
    elif kind == "same":
        k = k[:, :, :1].expand(-1, -1, Tk, -1).contiguous()
    elif kind == "dO0":
        dO = torch.zeros_like(dO)
    else:
        raise ValueError(kind)
    return q.to(BF), k.to(BF), v.to(BF), dO.to(BF)


# ------------------------------------------------------------------------------ routes
FWD_CLASSES = ("dma<2>", "dma<1>", "fwd<2>", "fwd<1,one,32>", "fwd<1,one,32,64>", "fwd<1,one>", "fwd<1>")
BWD_CLASSES = ("short<32>", "short<32,64>", "short<64>", "dq<2>+dkdv", "dq<1>+dkdv")


def routes(Tq, Tk, drop):
    """(forward kernel, backward path) of gvl_attn_fwd / gvl_attn_bwd, restated branch for branch
    from attention.hip (pick_groups: two query groups when Tq > 64; the LDS-DMA forward needs no
    dropout and more than one 64-key tile)."""
    G = 2 if Tq > 64 else 1
    if not drop and Tk > 64:
        fwd = f"dma<{G}>"
    elif G == 2:
        fwd = "fwd<2>"
    elif Tq <= 32 and Tk <= 32:
        fwd = "fwd<1,one,32>"
    elif Tq <= 32 and Tk <= 64:
        fwd = "fwd<1,one,32,64>"
    elif Tk <= 64:
        fwd = "fwd<1,one>"
    else:
        fwd = "fwd<1>"
    if Tq <= 64 and Tk <= 64:
        bwd = "short<32>" if Tq <= 32 and Tk <= 32 else ("short<32,64>" if Tq <= 32 else "short<64>")
    else:
        bwd = f"dq<{G}>+dkdv"
    return fwd, bwd


# the smallest shapes on each side of each threshold of the dispatch (32 and 64 rows on either
# side, the 128-row query tile of two groups, a second and third 64-key tile)
SHAPES = ((1, 1), (17, 29), (32, 32),
          (31, 33), (32, 64),
          (33, 9), (64, 64), (63, 63),
          (40, 130), (64, 65), (1, 129),
          (65, 64), (100, 33), (129, 9),
          (65, 65), (130, 257), (200, 192), (300, 300), (257, 130))
LONG = (1024, 1024)
DROP_P = 0.1
SEED = 4242
# one shape per backward path (layouts, seed_ptr, determinism)
PATH_SHAPES = {"short<32>": (17, 29), "short<32,64>": (31, 33), "short<64>": (63, 63),
               "dq<1>+dkdv": (40, 130), "dq<2>+dkdv": (130, 257)}
STRUCT_SHAPES = ((40, 130), (130, 257))
STRUCT_SCALES = (0.2, 1.0)


def bh(Tq, Tk):
    """B = 2, H = 3 catches batch- and head-stride slips; only the long case is B = 1, H = 2."""
    return (1, 2) if (Tq, Tk) == LONG else (2, 3)


def cases():
    """(Tq, Tk, causal, drop_p) of the shape sweep."""
    out = [(tq, tk, c, p) for (tq, tk) in SHAPES for c in (False, True) for p in (0.0, DROP_P)]
    return out + [LONG + (True, p) for p in (0.0, DROP_P)]


def case_data(Tq, Tk, causal, drop_p, scale=0.125, seed=SEED, seed_offset=None):
    """(inputs, keep, ref, E, emu) of one sweep case."""
    B, H = bh(Tq, Tk)
    x = inputs(B, H, Tq, Tk)
    keep = keep_mask(seed_eff(seed, seed_offset), B, H, Tq, Tk, drop_p) if drop_p > 0 else None
    return (x, keep) + attention_ref(*x, causal, scale, drop_p, keep)


@functools.lru_cache(maxsize=None)
def baseline():
    """The fp32 `slack` baseline per output: the worst error of attention_f32 against the float64
    reference, in units of 2**-24 * E, over a handful of sweep cases."""
    worst = dict.fromkeys(OUTS + ("lse",), 0.0)
    for (tq, tk) in ((17, 29), (64, 64), (130, 257), (300, 300)):
        for causal in (False, True):
            for p in (0.0, DROP_P):
                x, keep, ref, E, _ = case_data(tq, tk, causal, p)
                got = attention_f32(*x, causal, 0.125, p, keep)
                for n in worst:
                    worst[n] = max(worst[n], err_units(got[n], ref[n], E[n]))
    return worst
