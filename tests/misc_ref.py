"""float64 references, error scales, fp32 baselines and input builders for the last kernels that
were held by a max-norm only: column sums, the dropout mask, the tanh-gate backward
(csrc/optim.hip), CLIP pooling and the atomic embedding backward (csrc/embed_pool.hip).  CPU
only; every input is a bf16 or fp32 value, exact in float64, so a reference reads what the
kernel read.  A bound taken from "the same formula in fp32 on the CPU" is that baseline's error
in units of 2**-24 * (sum of |terms|), floored at one unit (one fp32 rounding of the result: the
least any order of evaluation costs) and applied times four, the margin of the row-wise tests.
tests/test_misc_ref_cpu.py checks all of this; tests/test_gpu_misc.py and
tests/test_gpu_sampler.py hold the kernels to it and record what they measure through
`record` (profiles/misc_margins.json)."""
import math

import numpy as np
import torch

from oracle import ops as O
from tests.gemm_ref import keep_mask
from tests.attn_ref import seed_eff
from tests.helpers import err_units, f64, margins_out

BF = torch.bfloat16
F32 = torch.float32
MARGIN = 4

MARGINS = {}


def record(key, rec):
    """One entry of profiles/misc_margins.json (shared by the sampler and the misc GPU tests)."""
    MARGINS[key] = rec
    margins_out("misc_margins", MARGINS)


def slack_of(baseline_units):
    return MARGIN * max(float(baseline_units), 1.0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------- column sums
COLSUM_ROWS = (1, 15, 16, 17, 63, 64, 65, 113, 128, 129)
COLSUM_COLS = (8, 120, 128, 136, 264)
COLSUM_TALL = (8200, 8)  # the 128-split cap, chunk = 65: not a multiple of 16


def colsum_input(rows, cols, seed=0, shift=0):
    """bf16 [rows, cols]: column c scaled by 2**(c mod 9 - 4 + shift); every seventh column
    (c mod 7 == 3) cancels: +-3 alternating by row plus noise of 2**-6, so that its sum is far
    below its sum of absolute values."""
    g = torch.Generator().manual_seed(7000 + 131 * rows + cols + seed)
    x = torch.randn(rows, cols, generator=g)
    sign = torch.where(torch.arange(rows) % 2 == 0, 3.0, -3.0)[:, None]
    cancel = (torch.arange(cols) % 7 == 3)[None, :]
    x = torch.where(cancel, sign + x * 2.0 ** -6, x)
    x = x * torch.exp2((torch.arange(cols) % 9 - 4 + shift).float())[None, :]
    return x.to(BF)


def colsum_ref(x, prev=None):
    """-> (float64 column sums (+ prev), sum of |terms|, fp32 baseline in units)."""
    x64 = f64(x)
    add = np.zeros(x64.shape[1]) if prev is None else f64(prev)
    ref = x64.sum(axis=0) + add
    E = np.abs(x64).sum(axis=0) + np.abs(add)
    s32 = np.zeros(x64.shape[1], dtype=np.float32)
    x32 = x64.astype(np.float32)
    for r in range(x32.shape[0]):  # a plain fp32 loop over the rows
        s32 = s32 + x32[r]
    s32 = s32 + add.astype(np.float32)
    return ref, E, err_units(s32, ref, E)


# ----------------------------------------------------------------------------- dropout
def dropout_ref(x, p, seed, offset=None):
    """bf16_rne(fl32(x) * fl32(1 / (1 - p))) where rng_keep(seed_eff, r * cols + c) holds, +0
    elsewhere (bit for bit): x a logical bf16 [rows, cols]."""
    rows, cols = x.shape
    keep = torch.from_numpy(keep_mask(seed_eff(seed, offset), rows, cols, p))
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    y = (x.float() * torch.tensor(float(scale), dtype=F32)).to(BF)
    return torch.where(keep, y, torch.zeros_like(y)), keep


# -------------------------------------------------------------------------------- gate
GATES = (0.0, 0.3, -4.0, 9.0)
GATE_SIZES = (1, 7, 8, 9, 2048, 2049)
GATE_STRIDE_SCALAR = 262145 + 300       # > RED_MAXB * RED_NT elements
GATE_STRIDE_VEC = 2097152 + 2048        # > 8 * RED_MAXB * RED_NT elements


def gate_inputs(n, seed=0, cancel=False):
    """bf16 dx, y [n]; cancel: neighbours (2k, 2k + 1) share dx and have opposite y up to 2**-7
    relative noise, so that sum(dx * y) is far below sum(|dx * y|)."""
    g = torch.Generator().manual_seed(7100 + n + seed)
    dx = torch.randn(n, generator=g)
    y = torch.randn(n, generator=g)
    if cancel and n > 1:
        m = n // 2 * 2
        dx[1:m:2] = dx[0:m:2]
        y[1:m:2] = -y[0:m:2] * (1 + 2.0 ** -7 * torch.randn(m // 2, generator=g))
    return dx.to(BF), y.to(BF)


def gate_ref(dx, y, gate):
    """gate: a bf16 scalar tensor -> dict(dy, dg, E (= sum |dx y| (1 - t^2)), base (fp32
    baseline of dg in units of 2**-24 * E))."""
    t = math.tanh(float(gate.double()))
    d, yy = f64(dx), f64(y)
    dy = t * d
    sech2 = 1.0 / math.cosh(float(gate.double())) ** 2  # 1 - t^2 without its cancellation
    dg = float((d * yy).sum() * sech2)
    E = float(np.abs(d * yy).sum() * sech2)
    t32 = np.tanh(np.float32(float(gate.float())))
    prod = d.astype(np.float32) * yy.astype(np.float32)
    s32 = np.cumsum(prod, dtype=np.float32)[-1]  # (a running fp32 sum, element by element)
    dg32 = np.float32(s32 * np.float32(np.float32(1) - t32 * t32))
    base = abs(float(dg32) - dg) / (2.0 ** -24 * E) if E > 0 else (0.0 if dg32 == 0 else np.inf)
    return dict(dy=dy, dg=dg, E=E, base=base, t=t)


def bf16_add_two_roundings(g0, dg32):
    """bf16(g0 + bf16(dg)): autograd's two roundings, from the fp32 gradient dg32."""
    d = torch.tensor(float(dg32), dtype=F32).to(BF).float()
    return (g0.float() + d).to(BF)


# -------------------------------------------------------------------------------- pool
POOL_SIDES = (1, 2, 3, 7, 14, 16, 24)
POOL_DS = (4, 6, 260, 768, 1024)


def pool_windows(side):
    """[(r0, r1, c0, c1)] of the 32 adaptive-average windows (oracle/ops.py pool_clip)."""
    w = []
    for i in range(4):
        r0, r1 = (i * side) // 4, -(-((i + 1) * side) // 4)
        for j in range(8):
            c0, c1 = (j * side) // 8, -(-((j + 1) * side) // 8)
            w.append((r0, r1, c0, c1))
    return w


def pool_route(side, D, in_fp32, aligned=True):
    """The kernel instance gvl_pool_clip_ex launches (csrc/embed_pool.hip), as a test id."""
    mw = max((r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in pool_windows(side))
    if in_fp32 and D % 4 == 0 and aligned and mw <= 8:
        return "pool4<8>"
    if in_fp32 and D % 4 == 0 and aligned and mw <= 16:
        return "pool4<16>"
    return ("pool<float>" if in_fp32 else "pool<bf16>") + ("-unrolled" if mw <= 8 else "-loop")


def pool_input(B, side, D, dtype, seed=0, zero_grid=False):
    """[B, 1 + side^2, D]: the CLS row scaled by 2**10, the tokens of window 5 by 2**-10."""
    g = torch.Generator().manual_seed(7200 + 97 * side + D + seed)
    t = torch.randn(B, 1 + side * side, D, generator=g)
    t[:, 0] *= 2.0 ** 10
    r0, r1, c0, c1 = pool_windows(side)[5]
    grid = t[:, 1:].view(B, side, side, D)
    grid[:, r0:r1, c0:c1] *= 2.0 ** -10
    if zero_grid:
        t[:, 1:] = 0.0
    return t.to(dtype)


def _pool(t, normalize, dt):
    B, L, D = t.shape
    side = int(round((L - 1) ** 0.5))
    t = t.to(dt)
    grid = t[:, 1:].view(B, side, side, D)
    outs, mabs = [t[:, 0]], [t[:, 0].abs()]
    for r0, r1, c0, c1 in pool_windows(side):
        outs.append(grid[:, r0:r1, c0:c1].mean(dim=(1, 2)))
        mabs.append(grid[:, r0:r1, c0:c1].abs().mean(dim=(1, 2)))
    z, e = torch.stack(outs, dim=1), torch.stack(mabs, dim=1)
    if normalize:
        n = z.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        z, e = z / n, e / n
    return z, e


def pool_ref(tokens, normalize):
    """-> (float64 [B, 33, D], scale: the window mean of |x| (/ the norm), fp32 baseline units)."""
    z, e = _pool(tokens, normalize, torch.float64)
    z32, _ = _pool(tokens, normalize, F32)
    return z.numpy(), e.numpy(), err_units(z32, z.numpy(), e.numpy())


# ------------------------------------------------------------------ embedding backward
EMB_HOT, EMB_HOT_COPIES = 7, 500


def emb_case(C):
    """-> (idx [61, 23] int64, dout [61 * 26, C] bf16, T, S, off, V, n_tokens): 1,402 tokens (no
    multiple of 4) at out_offset 3 of 26-row groups; id 7 is hot, 500 copies whose rows share a
    common direction (so the hot row's sum grows like the count: one dropped token is 1 / 500
    of it); one id above V and one negative; ids V - 40 .. V - 1 never occur."""
    V, G, T, S, off = 300, 61, 23, 26, 3
    n = G * T - 1
    gen = torch.Generator().manual_seed(7300 + C)
    idx = torch.randint(0, V - 40, (G, T), generator=gen)
    flat, perm = idx.view(-1), torch.randperm(n, generator=gen)
    flat[perm[:EMB_HOT_COPIES]] = EMB_HOT
    flat[perm[EMB_HOT_COPIES]], flat[perm[EMB_HOT_COPIES + 1]] = V + 3, -1
    dout = torch.randn(G * S, C, generator=gen)
    r = perm[:EMB_HOT_COPIES]
    rows = (r // T) * S + off + r % T
    dout[rows] = torch.randn(C, generator=gen)[None, :] + 0.25 * dout[rows]
    return idx, dout.to(BF), T, S, off, V, n


def emb_bwd_ref(idx, dout, T, S, off, C, V, n_tokens, dwte0, dwpe0):
    """The atomic path: token r (< n_tokens, row-major over idx) reads row
    (r // T) * S + off + r % T of dout [*, C]; an id outside [0, V) adds nothing to dwte and
    still adds to dwpe.  -> dict(dwte, dwpe: float64 results from the initial accumulators,
    E_*: sum of |terms|, S_*: terms per element + 1), None for a null accumulator."""
    ids = idx.reshape(-1).numpy()[:n_tokens]
    r = np.arange(n_tokens)
    rows = f64(dout).reshape(-1, C)[(r // T) * S + off + r % T]
    out = {}
    for name, init, key, ok in (("dwte", dwte0, ids, (ids >= 0) & (ids < V)),
                                ("dwpe", dwpe0, r % T, np.ones(n_tokens, dtype=bool))):
        if init is None:
            out[name] = None
            continue
        acc, E = f64(init).copy(), np.abs(f64(init))
        cnt = np.ones(acc.shape[0])
        np.add.at(acc, key[ok], rows[ok])
        np.add.at(E, key[ok], np.abs(rows[ok]))
        np.add.at(cnt, key[ok], 1.0)
        out[name], out["E_" + name], out["S_" + name] = acc, E, cnt[:, None] + 1.0
        out["touched_" + name] = np.unique(key[ok])
    return out
