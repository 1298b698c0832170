"""float64 references (and the same formulas in fp32 torch, the CPU baseline) of the row-wise
kernels: AdamW, cross-entropy, LayerNorm.  Shared by test_helpers_cpu.py, which proves that
the per-element assertions reject doctored outputs, and test_gpu_rowwise.py, which holds the
HIP kernels to them.  Every reference reads the same bf16 / fp32 values the kernel reads."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests.helpers import err_units, f64, ulp_bf16

BF = torch.bfloat16
F32 = torch.float32

# ------------------------------------------------------------------------------ AdamW
ADAM = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, gscale=0.37)
ADAM_STEPS = (1, 7, 1000)
ADAM_BIG = 8 * 256 * 3 + 5  # vector body over three blocks + a 5-element tail
ADAM_SIZES = (5, 8, ADAM_BIG)


def adam_decays(n):
    """n_decay cases: none, a boundary inside the first 8-wide vector, one inside the last
    vector / the tail, all."""
    return (0, 3, n - 3, n)


def adam_inputs(n, seed=0):
    """(p fp32, g bf16, m fp32, v fp32); the bf16 entry points read p, m, v rounded to bf16."""
    gen = torch.Generator().manual_seed(1000 + seed)
    p = 0.02 * torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen).to(BF)
    m = 0.1 * torch.randn(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen) + 1e-6
    return p, g, m, v


def adam_scaled_grad(g, gscale=ADAM["gscale"]):
    """bf16(g * scale) with the product in fp32, as the kernel forms it (clip_grad_norm_
    scales the bf16 gradient in place)."""
    return (g.float() * torch.tensor(gscale, dtype=F32)).to(BF)


def _hp():
    # the fp32 values the kernel receives
    return {k: float(np.float32(x)) for k, x in ADAM.items()}


def adamw_ref64(p, gs, m, v, n_decay, step, bias_step=None):
    """One AdamW step in float64.  p, m, v: the stored values; gs: adam_scaled_grad.  Returns
    the new p, m, v and, for p and m, the sum of the absolute values of the terms added to
    form them (helpers.assert_bf16_close's `scale`); v has no cancellation (scale = v)."""
    h = _hp()
    p, gs, m, v = f64(p), f64(gs), f64(m), f64(v)
    t = step if bias_step is None else bias_step
    pd = np.where(np.arange(p.size) < n_decay, p * (1.0 - h["lr"] * h["wd"]), p)
    t1, t2 = h["b1"] * m, (1.0 - h["b1"]) * gs
    m2 = t1 + t2
    v2 = h["b2"] * v + (1.0 - h["b2"]) * gs * gs
    c = h["lr"] / (1.0 - h["b1"] ** t)
    den = np.sqrt(v2) / math.sqrt(1.0 - h["b2"] ** t) + h["eps"]
    sm = np.abs(t1) + np.abs(t2)
    return dict(p=pd - c * m2 / den, m=m2, v=v2, scale_p=np.abs(pd) + c * sm / den, scale_m=sm,
                scale_v=v2)


def adamw_f32(p, gs, m, v, n_decay, step, dev=False):
    """The kernel's formula (optim.hip adam_elem) in fp32 torch on the CPU; dev: the bias
    corrections from fp32 pow, as the device-hyper entry points form them."""
    h = {k: torch.tensor(x, dtype=F32) for k, x in ADAM.items()}
    one = torch.tensor(1.0, dtype=F32)
    p, gs, m, v = p.float(), gs.float(), m.float(), v.float()
    pd = torch.where(torch.arange(p.numel()) < n_decay, p * (one - h["lr"] * h["wd"]), p)
    m2 = h["b1"] * m + (one - h["b1"]) * gs
    v2 = h["b2"] * v + (one - h["b2"]) * gs * gs
    if dev:
        st = torch.tensor(float(step), dtype=F32)
        bc1 = one - torch.pow(h["b1"], st)
        bc2s = torch.sqrt(one - torch.pow(h["b2"], st))
    else:
        bc1 = torch.tensor(1.0 - float(h["b1"]) ** step, dtype=F32)
        bc2s = torch.tensor(math.sqrt(1.0 - float(h["b2"]) ** step), dtype=F32)
    den = torch.sqrt(v2) / bc2s + h["eps"]
    return dict(p=pd - (h["lr"] / bc1) * m2 / den, m=m2, v=v2)


_ADAM_BASE = {}


def adam_baseline():
    """Worst error of adamw_f32 against adamw_ref64 over every (step, n_decay) case at
    n = ADAM_BIG, fp32 state, in units of 2**-24 * scale: the CPU baseline the kernels get
    four times of (the device's powf, sqrtf and division need not round like the host's)."""
    if not _ADAM_BASE:
        base = dict(p=0.0, m=0.0, v=0.0)
        p, g, m, v = adam_inputs(ADAM_BIG)
        gs = adam_scaled_grad(g)
        for step in ADAM_STEPS:
            for nd in adam_decays(ADAM_BIG):
                ref = adamw_ref64(p, gs, m, v, nd, step)
                for dev in (False, True):
                    got = adamw_f32(p, gs, m, v, nd, step, dev=dev)
                    for k in base:
                        base[k] = max(base[k], err_units(got[k], ref[k], ref["scale_" + k]))
        _ADAM_BASE.update(base)
    return dict(_ADAM_BASE)


def moved_fraction(before, after64):
    """Fraction of elements the reference moves by at least one bf16 ulp (of the old value)."""
    b = f64(before)
    return float((np.abs(f64(after64) - b) >= ulp_bf16(b)).mean())


# ---------------------------------------------------------------------- cross entropy
def ce_ref64(logits, targets, mask=None):
    """logits [rows, V] (bf16 values), targets [rows] (-100: ignored) -> (row losses, dlogits)
    in float64; an ignored / masked row has loss 0 and a zero gradient row."""
    x = f64(logits)
    t = np.asarray(targets, dtype=np.int64)
    valid = t != -100
    if mask is not None:
        valid &= np.asarray(mask).astype(bool)
    mx = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - mx)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    r = np.arange(x.shape[0])
    tc = np.where(valid, t, 0)
    loss = np.where(valid, (mx + np.log(s))[:, 0] - x[r, tc], 0.0)
    p[r[valid], tc[valid]] -= 1.0
    p[~valid] = 0.0
    return loss, p


def ce_f32(logits, targets):
    """softmax - onehot in fp32 torch, rounded to bf16 (valid targets only)."""
    p = torch.softmax(logits.float(), dim=-1)
    p[torch.arange(p.shape[0]), targets] -= 1.0
    return p.to(BF)


# -------------------------------------------------------------------------- LayerNorm
LN_EPS = 1e-5
LN_WIDTHS = (8, 128, 768, 776, 1024)  # 776: the first width of the IT = 4 instantiation
LN_ROWS = (1, 7, 9, 37)               # 8 rows per forward block, 4 waves per backward block


def ln_inputs(rows, C, seed=0, scaled=True):
    """x with row i scaled by 2**((5 * i) % 13 - 6) (2**-6 .. 2**6), w, b, dy, prev: bf16."""
    gen = torch.Generator().manual_seed(2000 + seed + 7 * rows + C)
    x = torch.randn(rows, C, generator=gen) * 2 + 0.5
    if scaled:
        x = x * torch.exp2(((5 * torch.arange(rows)) % 13 - 6).float())[:, None]
    w = 1 + 0.1 * torch.randn(C, generator=gen)
    b = 0.1 * torch.randn(C, generator=gen)
    dy = torch.randn(rows, C, generator=gen)
    prev = torch.randn(rows, C, generator=gen)
    return tuple(t.to(BF) for t in (x, w, b, dy, prev))


def ln_special_rows(C):
    """Row 0 constant (zero variance), row 1 offset x = 256 + {0, 2, 4} (exact in bf16; a
    one-pass variance E[x^2] - mean^2 loses rstd accuracy on it), row 2 the same at -256."""
    pat = (2.0 * (torch.arange(C) % 3))
    x = torch.stack([torch.full((C,), 3.25), 256.0 + pat, -256.0 - pat])
    xb = x.to(BF)
    assert torch.equal(xb.float(), x)
    return xb


def ln_ref64(x, w, b, eps=LN_EPS):
    """-> dict(mean, rstd, y) in float64 plus the scales of the added terms: scale_mean =
    mean|x|, scale_rstd = rstd (the two-pass variance has no cancellation), scale_y =
    (|x| + mean|x|) * rstd * |w| + |b|."""
    x, w, b = f64(x), f64(w), f64(b)
    eps = float(np.float32(eps))
    mean = x.mean(axis=1)
    d = x - mean[:, None]
    rstd = 1.0 / np.sqrt((d * d).mean(axis=1) + eps)
    am = np.abs(x).mean(axis=1)
    y = d * rstd[:, None] * w + b
    sy = (np.abs(x) + am[:, None]) * rstd[:, None] * np.abs(w) + np.abs(b)
    return dict(mean=mean, rstd=rstd, y=y, scale_mean=am, scale_rstd=rstd, scale_y=sy)


def ln_bwd_dx_ref64(dy, x, w, mean, rstd, prev=None):
    """-> (dx (+ prev) in float64 from the given statistics, the scale of the added terms:
    rstd * (|g| + mean|g| + |xh| * mean|g * xh|) + |prev|, with g = dy * w)."""
    dy, x, w = f64(dy), f64(x), f64(w)
    mean, rstd = f64(mean)[:, None], f64(rstd)[:, None]
    xh = (x - mean) * rstd
    g = dy * w
    dx = rstd * (g - g.mean(axis=1, keepdims=True) - xh * (g * xh).mean(axis=1, keepdims=True))
    scale = np.abs(rstd) * (np.abs(g) + np.abs(g).mean(axis=1, keepdims=True)
                            + np.abs(xh) * np.abs(g * xh).mean(axis=1, keepdims=True))
    if prev is not None:
        dx, scale = dx + f64(prev), scale + np.abs(f64(prev))
    return dx, scale


def ln_bwd_ref64(dy, x, w, mean, rstd, prev=None):
    """dx (+ prev) in float64 from the given statistics."""
    return ln_bwd_dx_ref64(dy, x, w, mean, rstd, prev)[0]


def ln_bwd_wb_ref64(dy, x, mean, rstd, dw_prev=None, db_prev=None):
    """-> dict(dw = sum_r dy * xh, db = sum_r dy (each + its previous value when accumulating),
    scale_dw = sum_r |dy * xh| (+ |prev|), scale_db = sum_r |dy| (+ |prev|)) in float64."""
    dy, x = f64(dy), f64(x)
    xh = (x - f64(mean)[:, None]) * f64(rstd)[:, None]
    out = dict(dw=(dy * xh).sum(axis=0), db=dy.sum(axis=0),
               scale_dw=np.abs(dy * xh).sum(axis=0), scale_db=np.abs(dy).sum(axis=0))
    for k, p in (("dw", dw_prev), ("db", db_prev)):
        if p is not None:
            out[k], out["scale_" + k] = out[k] + f64(p), out["scale_" + k] + np.abs(f64(p))
    return out


def ln_bwd_f32(dy, x, w, mean, rstd, prev=None, dw_prev=None, db_prev=None):
    """The kernel's formulas (layernorm.hip ln_bwd_kernel) in fp32 torch on the CPU -> dict(dx,
    dw, db): the two row means are fp32 sums divided by C, dw and db are accumulated row by row
    in fp32; a previous value is added last, in fp32."""
    dy, x, w = dy.float(), x.float(), w.float()
    C = x.shape[1]
    mean, rstd = mean.float().cpu()[:, None], rstd.float().cpu()[:, None]
    xh = (x - mean) * rstd
    g = dy * w
    m1 = g.sum(dim=1, keepdim=True) / C
    m2 = (g * xh).sum(dim=1, keepdim=True) / C
    dx = rstd * (g - m1 - xh * m2)
    t = dy * xh
    dw, db = torch.zeros(C, dtype=F32), torch.zeros(C, dtype=F32)
    for r in range(x.shape[0]):
        dw += t[r]
        db += dy[r]
    if prev is not None:
        dx = dx + prev.float()
    if dw_prev is not None:
        dw = dw + dw_prev.float()
    if db_prev is not None:
        db = db + db_prev.float()
    return dict(dx=dx, dw=dw, db=db)


def ln_f32(x, eps=LN_EPS, one_pass=False):
    """mean, rstd in fp32 torch on the CPU: two passes as the kernel, or E[x^2] - mean^2."""
    x = x.float()
    C = x.shape[1]
    mean = x.sum(dim=1) / C
    if one_pass:
        var = (x * x).sum(dim=1) / C - mean * mean
    else:
        d = x - mean[:, None]
        var = (d * d).sum(dim=1) / C
    return mean, torch.rsqrt(var + torch.tensor(eps, dtype=F32))


_LN_BASE = {}


def ln_baseline():
    """Worst error of ln_f32 (two-pass) against ln_ref64 over every test shape and the special
    rows, in units of 2**-24 * scale: the CPU baseline the kernel gets four times of."""
    if not _LN_BASE:
        base = dict(mean=0.0, rstd=0.0)
        for C in LN_WIDTHS:
            xs = [ln_inputs(rows, C)[0] for rows in LN_ROWS] + [ln_special_rows(C)]
            for x in xs:
                ref = ln_ref64(x, torch.ones(C), torch.zeros(C))
                mean, rstd = ln_f32(x)
                base["mean"] = max(base["mean"], err_units(mean, ref["mean"], ref["scale_mean"]))
                base["rstd"] = max(base["rstd"], err_units(rstd, ref["rstd"], ref["scale_rstd"]))
        _LN_BASE.update(base)
    return dict(_LN_BASE)


# ----------------------------------------------------------------- LayerNorm backward
# Lane l of the backward wave holds columns 4 * (l + 64 * it): 256 fills it = 0 exactly, 264 and
# 520 end inside it = 1 and it = 2.  Rows: 4 waves per block (1 .. 9), more than one block (37),
# the finalize's 16 partial groups (129 rows = 17 blocks, 136 = 17 full ones).
LN_BWD_WIDTHS = LN_WIDTHS + (256, 264, 520)
LN_BWD_ROWS = (1, 3, 4, 5, 8, 9, 37, 129, 136)
# the block cap (512 blocks of 4 rows): 4088 rows = 511 blocks, 4096 = 512 with two passes per
# wave, 4099 = three passes for three of the waves
LN_BWD_TALL_ROWS = (4088, 4096, 4099)
LN_BWD_TALL_WIDTHS = (8, 128, 776)
LN_BWD_SHAPES = tuple((r, c) for c in LN_BWD_WIDTHS for r in LN_BWD_ROWS) + tuple(
    (r, c) for c in LN_BWD_TALL_WIDTHS for r in LN_BWD_TALL_ROWS)
LN_COUNT_SHAPES = ((4099, 128), (4099, 776), (137, 264))
LN_FWD_TALL = tuple((r, c) for c in (8, 776) for r in (8192, 8193, 8203))  # 8192 rows per pass


def ln_wb_prev(C, seed=0):
    """Previous dw, db (bf16) to accumulate over."""
    gen = torch.Generator().manual_seed(2500 + seed + C)
    return (4 * torch.randn(C, generator=gen)).to(BF), (4 * torch.randn(C, generator=gen)).to(BF)


def ln_count_inputs(rows, C):
    """ln_inputs with dy[r, c] = 1 where c == r % C, 0 elsewhere, and db_prev[c] = c % 5: db[c]
    is the number of rows congruent to c (+ db_prev[c]), an integer below 256."""
    x, w, b, _, prev = ln_inputs(rows, C, seed=3)
    dy = torch.zeros(rows, C)
    dy[torch.arange(rows), torch.arange(rows) % C] = 1.0
    db_prev = (torch.arange(C) % 5).float()
    counts = torch.bincount(torch.arange(rows) % C, minlength=C).float()
    assert float((counts + db_prev).max()) < 256
    return x, w, b, dy.to(BF), prev, db_prev.to(BF), counts


def ln_bwd_cases():
    """[(key, (x, w, dy, prev))]: every input set the backward tests run."""
    out = []
    for rows, C in LN_BWD_SHAPES:
        x, w, _, dy, prev = ln_inputs(rows, C)
        out.append((f"{rows}x{C}", (x, w, dy, prev)))
    for rows, C in LN_COUNT_SHAPES:
        x, w, _, dy, prev, _, _ = ln_count_inputs(rows, C)
        out.append((f"count:{rows}x{C}", (x, w, dy, prev)))
    for C in LN_WIDTHS:  # test_layernorm_per_row's dx at the one row count not among the above
        x, w, _, dy, prev = ln_inputs(7, C)
        out.append((f"7x{C}", (x, w, dy, prev)))
    return out


def ln_bwd_units(x, w, dy, prev, mean, rstd, got=None):
    """Errors of `got` (default: ln_bwd_f32, from the fp32 statistics mean, rstd taken as exact
    inputs) against float64 in units of 2**-24 * scale, storing and accumulating over prev /
    ln_wb_prev: dict(dx, dw, db)."""
    C = x.shape[1]
    f = got or ln_bwd_f32(dy, x, w, mean, rstd)
    dwp, dbp = ln_wb_prev(C)
    units = {}
    dx, sdx = ln_bwd_dx_ref64(dy, x, w, mean, rstd)
    units["dx"] = max(err_units(f["dx"], dx, sdx),
                      err_units(f["dx"] + prev.float(), dx + f64(prev), sdx + np.abs(f64(prev))))
    r = ln_bwd_wb_ref64(dy, x, mean, rstd)
    for k, p in (("dw", dwp), ("db", dbp)):
        units[k] = max(err_units(f[k], r[k], r["scale_" + k]),
                       err_units(f[k] + p.float(), r[k] + f64(p), r["scale_" + k] + np.abs(f64(p))))
    return units


_LN_BWD_BASE = {}


def ln_bwd_baseline():
    """Worst error of ln_bwd_f32 against float64 over every backward test shape (ln_bwd_cases),
    in units of 2**-24 * scale, for dx, dw and db, plus the same per case under "cases": the
    CPU baseline the kernel gets 4 x max(baseline, 1) of (ln_bwd_slack)."""
    if not _LN_BWD_BASE:
        base, cases = dict(dx=0.0, dw=0.0, db=0.0), {}
        for key, (x, w, dy, prev) in ln_bwd_cases():
            mean, rstd = ln_f32(x)
            cases[key] = ln_bwd_units(x, w, dy, prev, mean, rstd)
            for k in base:
                base[k] = max(base[k], cases[key][k])
        _LN_BWD_BASE.update(base, cases=cases)
    return {k: (dict(v) if k == "cases" else v) for k, v in _LN_BWD_BASE.items()}


def ln_bwd_slack():
    """dict(dx, dw, db): 4 x max(baseline, 1) fp32 roundings (misc_ref.slack_of's rule)."""
    base = ln_bwd_baseline()
    return {k: 4 * max(base[k], 1.0) for k in ("dx", "dw", "db")}


_LN_TALL_BASE = {}


def ln_fwd_tall_baseline():
    """ln_baseline's figure over LN_FWD_TALL, the shapes of the persistent forward's second
    pass (their own baseline: ln_baseline and the bounds that hang on it stay as they are)."""
    if not _LN_TALL_BASE:
        base = dict(mean=0.0, rstd=0.0)
        for rows, C in LN_FWD_TALL:
            x = ln_inputs(rows, C)[0]
            ref = ln_ref64(x, torch.ones(C), torch.zeros(C))
            mean, rstd = ln_f32(x)
            base["mean"] = max(base["mean"], err_units(mean, ref["mean"], ref["scale_mean"]))
            base["rstd"] = max(base["rstd"], err_units(rstd, ref["rstd"], ref["scale_rstd"]))
        _LN_TALL_BASE.update(base)
    return dict(_LN_TALL_BASE)


# ---------------------------------------------------------- LayerNorm backward finalize
LN_FIN_NBLK = (0, 1, 15, 16, 17, 511, 512)  # 16 partial groups: k = g + 16 j; 512 is the cap
LN_FIN_WIDTHS = (8, 72, 776, 1024)          # 2 * 72 = 144 leaves a 16-column last block
LN_FIN_COUNTS = (1, 64, 65)                 # 64 items per launch: 65 needs a second one
LN_FIN_POOL = 1024

_LN_FIN_POOLS = {}


def ln_fin_pool(C):
    """fp32 [1024, 2C] partials, as misc_ref.colsum_input: column c scaled by 2**(c % 9 - 4),
    every seventh (c % 7 == 3) +-3 alternating by row plus noise of 2**-6, so that its sum is
    far below its sum of absolute values.  An item's workspace is a run of its rows."""
    if C not in _LN_FIN_POOLS:
        g = torch.Generator().manual_seed(2600 + C)
        p = torch.randn(LN_FIN_POOL, 2 * C, generator=g)
        sign = torch.where(torch.arange(LN_FIN_POOL) % 2 == 0, 3.0, -3.0)[:, None]
        cancel = (torch.arange(2 * C) % 7 == 3)[None, :]
        p = torch.where(cancel, sign + p * 2.0 ** -6, p)
        colscale = torch.exp2((torch.arange(2 * C) % 9 - 4).float())[None, :]
        _LN_FIN_POOLS[C] = (p * colscale).contiguous()
    return _LN_FIN_POOLS[C]


def ln_fin_items(nblk, C, count):
    """[(first pool row, blocks, has dw, has db, dw_prev, db_prev)]: item 0 has `nblk` blocks,
    the next ones walk LN_FIN_NBLK from there; every fourth item lacks dw, every fourth db;
    item i's previous values are scaled by 2**(i % 7 - 3)."""
    k0 = LN_FIN_NBLK.index(nblk)
    gen = torch.Generator().manual_seed(2700 + 13 * nblk + C + count)
    items = []
    for i in range(count):
        n = LN_FIN_NBLK[(k0 + i) % len(LN_FIN_NBLK)]
        start = (8 * i) % (LN_FIN_POOL - n + 1)
        prev = (torch.randn(2, C, generator=gen) * 2.0 ** (i % 7 - 3)).to(BF)
        items.append((start, n, i % 4 != 1, i % 4 != 3, prev[0], prev[1]))
    return items


def ln_fin_ref(part, prev=None, first=None):
    """part fp32 [nblk, 2C] (+ prev [2C]) -> (float64 column sums, sum of |terms|, the error of
    a running fp32 sum over the rows in units of 2**-24 * that).  first: sum only that many
    rows (a doctored finalize)."""
    p64 = f64(part)[:first]
    add = np.zeros(p64.shape[1]) if prev is None else f64(prev)
    ref = p64.sum(axis=0) + add
    E = np.abs(p64).sum(axis=0) + np.abs(add)
    s32 = np.zeros(p64.shape[1], dtype=np.float32)
    if p64.shape[0]:
        s32 = np.cumsum(p64.astype(np.float32), axis=0, dtype=np.float32)[-1]
    s32 = s32 + add.astype(np.float32)
    return ref, E, err_units(s32, ref, E)
