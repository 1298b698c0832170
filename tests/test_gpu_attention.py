"""Per-element parity of the attention kernels on the MI355X, every route of gvl_attn_fwd and
gvl_attn_bwd (tests/attn_ref.routes) and gvl_attn_decode.

test_gpu_kernels.py's attention tests divide one max-norm error by the tensor's largest element,
which leaves the last key tile's dK / dV rows, lse and single rows of o unverified.  Here every
element of o, dq, dk, dv is compared with a float64 reference that reads the same bf16 inputs,
against the per-element scale E of tests/attn_ref.py (the same products with every term replaced
by its absolute value):

  hard bound   |got - ref| <= units * 2**-8 * E + 4 * baseline * 2**-24 * E, one unit per bf16
               rounding on the way to the element, each at most 2**-8 of what it rounds:
               o, dv: 2 (P, the output); dq, dk: 3 (dS, the output, the bf16 o inside D, whose
               terms S_abs carries); `baseline` is the error of the same formulas in fp32 torch
               on the CPU in units of 2**-24 * E (attn_ref.baseline);
  tight bound  dq, dk also within 4 x the worst error of attn_ref's bf16-rounding emulation for
               that case (+ the same fp32 term), computed from the reference alone;
  lse          helpers.assert_f32_close, 4 x baseline units of 2**-24 * (|lse| + scale * max_k
               sum_d |q_d k_d|).

tests/test_attn_ref_cpu.py shows that the emulation passes these bounds and that doctored
outputs the max-norm comparison accepts do not.  The measured ratios go to
profiles/attn_margins.json through helpers.margins_out."""
import functools

import pytest
import torch

from tests import attn_ref as A
from tests.helpers import (assert_attn_close, assert_attn_tight, assert_bf16_close,
                           assert_f32_close, margins_out)
from tests.test_gpu_rowwise import _arena, _bits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")

_MARGINS = {}


def _record(key, rec):
    _MARGINS[key] = rec
    margins_out("attn_margins", _MARGINS)


def _k():
    from gvl import kernels as K
    return K


@functools.lru_cache(maxsize=24)
def _data(Tq, Tk, causal, drop_p, seed_offset=None):
    """One sweep case's inputs, mask, reference, scales and emulation, computed once and shared
    by the tests that use the shape (nothing modifies them)."""
    return A.case_data(Tq, Tk, causal, drop_p, seed_offset=seed_offset)


# ------------------------------------------------------------------------------ running
def _btc(t):
    """[B, H, T, 64] -> the kernels' [B, T, H*64]."""
    B, H, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * 64).contiguous()


def _bhtd(t, H):
    B, T, _ = t.shape
    return t.reshape(B, T, H, 64).permute(0, 2, 1, 3).cpu()


class _Out:
    """A NaN-filled output buffer inside a sentinel arena, and the views of it a kernel owns."""

    def __init__(self, cuda, shape, **views):
        self.init = torch.full(shape, NAN, dtype=BF)
        flat, self.untouched = _arena(self.init.reshape(-1), cuda)
        self.outer = flat.view(shape)
        self.views = views

    def __getitem__(self, name):
        return self.views[name](self.outer)

    def check_rest(self):
        """Every element outside the owned views, the arena's sentinels included, kept its bits."""
        assert self.untouched(), f"a store outside the {'/'.join(self.views)} buffer"
        own = torch.zeros(self.init.shape, dtype=torch.bool)
        for v in self.views.values():
            v(own)[...] = True
        got = self.outer.cpu()
        assert torch.equal(_bits(got)[~own], _bits(self.init)[~own]), \
            f"a store next to the {'/'.join(self.views)} view"


LAYOUTS = ("packed", "kv", "bstride", "oslice")


def _place(cuda, layout, q, k, v, dO):
    """Device inputs and NaN-filled outputs of one layout; q, k, v, dO are [B, T, C] on the CPU.
    plain:   separate contiguous tensors;
    packed:  q, k, v column slices of one [B, T, 3C] buffer, the gradients likewise;
    kv:      k, v slices of one [B, Tk, 2C] buffer (dk, dv likewise), q separate;
    bstride: every tensor the first T rows of a [B, T + 3, C] buffer;
    oslice:  o (written through out=) and dO column slices of [B, Tq, C + 128] buffers."""
    B, Tq, C = q.shape
    Tk = k.shape[1]
    full = lambda t: t
    if layout == "packed":
        buf = torch.cat([q, k, v], dim=2).to(cuda)
        ins = [buf[:, :, :C], buf[:, :, C:2 * C], buf[:, :, 2 * C:], dO.to(cuda)]
        g = _Out(cuda, (B, Tq, 3 * C), dq=lambda t: t[:, :, :C], dk=lambda t: t[:, :, C:2 * C],
                 dv=lambda t: t[:, :, 2 * C:])
        return ins, _Out(cuda, (B, Tq, C), o=full), [g]
    if layout == "kv":
        buf = torch.cat([k, v], dim=2).to(cuda)
        ins = [q.to(cuda), buf[:, :, :C], buf[:, :, C:], dO.to(cuda)]
        g = _Out(cuda, (B, Tk, 2 * C), dk=lambda t: t[:, :, :C], dv=lambda t: t[:, :, C:])
        return ins, _Out(cuda, (B, Tq, C), o=full), [_Out(cuda, (B, Tq, C), dq=full), g]
    if layout == "bstride":
        def pad(t):
            big = torch.full((B, t.shape[1] + 3, C), NAN, dtype=BF)
            big[:, :t.shape[1]] = t
            return big.to(cuda)[:, :t.shape[1]]
        ins = [pad(t) for t in (q, k, v, dO)]
        fq, fk = (lambda t: t[:, :Tq]), (lambda t: t[:, :Tk])
        return ins, _Out(cuda, (B, Tq + 3, C), o=fq), [_Out(cuda, (B, Tq + 3, C), dq=fq),
                                                       _Out(cuda, (B, Tk + 3, C), dk=fk),
                                                       _Out(cuda, (B, Tk + 3, C), dv=fk)]
    ins = [t.to(cuda) for t in (q, k, v, dO)]
    o = _Out(cuda, (B, Tq, C), o=full)
    if layout == "oslice":
        sl = lambda t: t[:, :, 64:64 + C]
        wide = torch.full((B, Tq, C + 128), NAN, dtype=BF)
        sl(wide)[...] = dO
        ins[3] = sl(wide.to(cuda))
        o = _Out(cuda, (B, Tq, C + 128), o=sl)
    else:
        assert layout == "plain", layout
    return ins, o, [_Out(cuda, (B, Tq, C), dq=full), _Out(cuda, (B, Tk, C), dk=full),
                    _Out(cuda, (B, Tk, C), dv=full)]


def _run(cuda, x, causal, scale, drop_p=0.0, seed=A.SEED, layout="plain", seed_ptr=None):
    """gvl_attn_fwd + gvl_attn_bwd on x = (q, k, v, dO) [B, H, T, 64]: the five results as
    [B, H, T, 64] / [B, H, Tq] CPU tensors, after checking that the inputs and everything
    around the outputs kept their bits."""
    K_ = _k()
    H = x[0].shape[1]
    cpu = [_btc(t) for t in x]
    ins, o, grads = _place(cuda, layout, *cpu)
    kw = dict(scale=scale, drop_p=drop_p, seed=seed, seed_ptr=seed_ptr)
    _, lse = K_.attn_fwd(ins[0], ins[1], ins[2], H, causal, out=o["o"], **kw)
    g = {n: b[n] for b in grads for n in b.views}
    K_.attn_bwd(ins[3], ins[0], ins[1], ins[2], o["o"], lse, H, causal, g["dq"], g["dk"], g["dv"], **kw)
    torch.cuda.synchronize()
    for b in [o] + grads:
        b.check_rest()
    for t, c, n in zip(ins, cpu, "q k v dO".split()):
        assert torch.equal(_bits(t), _bits(c)), f"input {n} was written"
    got = {n: _bhtd(t, H) for n, t in g.items()}
    got.update(o=_bhtd(o["o"], H), lse=lse.cpu())
    return got


def _assert_case(got, ref, E, emu, name):
    """The hard bound on o, dq, dk, dv, the tight bound on dq, dk and the fp32 bound on lse;
    returns the measured ratios (kernel and emulation, units of 2**-8 * E; lse in 2**-24 * E)."""
    base = A.baseline()
    rec = dict(kernel={}, emulation={}, bound=dict(A.HARD_UNITS))
    for n in A.OUTS:
        rec["kernel"][n] = assert_attn_close(got[n], ref[n], E[n], A.HARD_UNITS[n],
                                             name=f"{name} {n}", slack=4 * base[n])
    for n in ("dq", "dk"):
        _, rec["emulation"][n] = assert_attn_tight(got[n], ref[n], E[n], emu[n],
                                                   name=f"{name} {n} (tight)", slack=4 * base[n])
    for n in ("o", "dv"):
        rec["emulation"][n] = assert_attn_close(emu[n], ref[n], E[n], A.HARD_UNITS[n])
    rec["kernel"]["lse"] = assert_f32_close(got["lse"], ref["lse"], E["lse"], 4 * base["lse"],
                                            name=f"{name} lse")
    rec["bound"]["lse"] = 4 * base["lse"]
    rec["bound"]["tight"] = {n: 4 * rec["emulation"][n] for n in ("dq", "dk")}
    return rec


# -------------------------------------------------------------------------------- sweep
def _id(c):
    return f"{c[0]}x{c[1]}-{'causal' if c[2] else 'full'}-p{c[3]}"


@pytest.mark.parametrize("case", A.cases(), ids=_id)
def test_attention_per_element(cuda, case):
    """Every (Tq, Tk) on each side of each threshold of the dispatch (attn_ref.SHAPES), causal
    (the top-left mask when Tq != Tk) and not, drop_p 0 and 0.1 with the restated hash mask:
    o, lse, dq, dk, dv per element against the float64 reference.
    Measured on the MI355X, worst over the sweep (units of 2**-8 E; kernel / emulation / bound):
    o 1.57 / 1.57 / 2, dv 1.87 / 1.87 / 2, dq 1.10 / 1.10 / 3, dk 0.43 / 0.43 / 3 (the worst
    elements have one or two terms, where kernel and emulation round alike); against the tight
    bound dq is at most 1.29 x and dk 1.09 x its case's emulation, of the 4 x allowed; lse 1.31
    units of 2**-24 E of 2.95.  Before the forward kernels summed the unrounded exponentials for
    lse (they took the ones-MFMA sum of the bf16 P), every no-dropout case here missed the lse
    bound by three orders of magnitude: errors of 4e-4 to 1.4e-3, e.g. 17x29 causal row 1 of
    (0, 0) 0.95149 for 0.95046."""
    Tq, Tk, causal, p = case
    x, keep, ref, E, emu = _data(*case)
    got = _run(cuda, x, causal, 0.125, p)
    rec = _assert_case(got, ref, E, emu, _id(case))
    rec["routes"] = A.routes(Tq, Tk, p > 0)
    print(f"{_id(case)} {rec['routes']}: kernel {rec['kernel']} emulation {rec['emulation']}")
    _record(_id(case), rec)


# ------------------------------------------------------------------------------ layouts
def _layout_cases():
    sq = ((32, 32), (63, 63), (300, 300))  # q, k, v in one buffer need Tq = Tk: three paths have one
    out = [("packed",) + s for s in sq]
    out += [(lay,) + s for lay in LAYOUTS[1:] for s in A.PATH_SHAPES.values()]
    return out


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout,Tq,Tk", _layout_cases())
def test_attention_layouts_stay_inside_their_views(cuda, layout, Tq, Tk, causal):
    """One shape per backward path in each strided layout of _place, every output NaN-filled in
    a sentinel arena: each owned element finite and in bound, every other element (the
    neighbouring column slices, the rows behind a batch, the sentinels) bit-identical."""
    x, keep, ref, E, emu = _data(Tq, Tk, causal, 0.0)
    got = _run(cuda, x, causal, 0.125, layout=layout)
    _assert_case(got, ref, E, emu, f"{layout} {Tq}x{Tk} causal={causal}")


# --------------------------------------------------------------------------- structured
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("scale", A.STRUCT_SCALES)
@pytest.mark.parametrize("Tq,Tk", A.STRUCT_SHAPES)
@pytest.mark.parametrize("kind", A.STRUCTURED)
def test_attention_structured_inputs(cuda, kind, Tq, Tk, scale, causal):
    """Inputs i.i.d. normals never give (attn_ref.structured_inputs), at softmax scales 0.2 and
    1.0: a running maximum that moves in every key tile, one-hot rows with underflowing
    exponentials, every score below -100 (lse must follow: no absolute clamp, no finite initial
    maximum), identical keys (o the exact mean of v to one bf16 ulp) and dO = 0 (gradients
    exactly zero).  Measured: o 1.41, dv 1.84, dq 0.33, dk 0.57 units (dq, dk at most 1.28 x the
    emulation), lse 1.70 of 2.95."""
    B, H = A.bh(Tq, Tk)
    x = A.structured_inputs(kind, B, H, Tq, Tk, scale)
    ref, E, emu = A.attention_ref(*x, causal, scale)
    got = _run(cuda, x, causal, scale)
    name = f"{kind} {Tq}x{Tk} scale={scale} causal={causal}"
    rec = _assert_case(got, ref, E, emu, name)
    if kind == "low":  # a property of the inputs, on the reference
        assert ref["lse"].max() < -100, "the inputs do not push every score below -100"
    if kind == "same":
        vis = A.visible(Tq, Tk, causal).to(torch.float64)
        mean = (vis / vis.sum(-1, keepdim=True)) @ x[2].to(torch.float64)
        assert_bf16_close(got["o"], mean.numpy(), scale=E["o"], slack=4 * A.baseline()["o"],
                          name=f"{name} o = mean(v)")  # (the scale: a mean of v may cancel)
    if kind == "dO0":
        for n in ("dq", "dk", "dv"):
            assert not got[n].float().abs().max() > 0, f"{name}: {n} is not exactly zero"
    _record(name, rec)


# ------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("path", sorted(A.PATH_SHAPES))
def test_attention_dropout_seed_ptr(cuda, path):
    """seed_ptr at a non-zero device offset: forward and backward both use the mask of
    seed_eff = seed ^ mix64(offset); at a zero offset the bits are those of no seed_ptr."""
    Tq, Tk = A.PATH_SHAPES[path]
    off = 0x1234567
    x, keep, ref, E, emu = _data(Tq, Tk, False, A.DROP_P, off)
    ptr = torch.tensor([off], dtype=torch.int64, device=cuda)
    got = _run(cuda, x, False, 0.125, A.DROP_P, seed_ptr=ptr)
    _assert_case(got, ref, E, emu, f"seed_ptr {path}")
    plain = _run(cuda, x, False, 0.125, A.DROP_P)
    zero = _run(cuda, x, False, 0.125, A.DROP_P, seed_ptr=torch.zeros(1, dtype=torch.int64, device=cuda))
    for n in plain:
        assert torch.equal(_bits(plain[n]), _bits(zero[n])), f"{path} {n}: *seed_ptr = 0 changed the bits"
    assert not torch.equal(_bits(plain["o"]), _bits(got["o"])), "the offset did not re-key the mask"


# -------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("path", sorted(A.PATH_SHAPES))
def test_attention_is_deterministic(cuda, path):
    """"No atomics, deterministic": two runs over NaN-refilled free memory give the same bits."""
    Tq, Tk = A.PATH_SHAPES[path]
    x = _data(Tq, Tk, True, A.DROP_P)[0]
    runs = []
    for _ in range(2):
        junk = torch.full((32 << 20,), NAN, device=cuda)
        del junk
        runs.append(_run(cuda, x, True, 0.125, A.DROP_P))
    for n in runs[0]:
        assert torch.equal(_bits(runs[0][n]), _bits(runs[1][n])), f"{path} {n} differs between runs"


# ------------------------------------------------------------------------------- decode
def _decode_setup(cuda, Tk, B=2, H=3):
    """The new query of a [B, Tmax, 3C] packed cache (NaN wherever the kernel has no business)
    and a NaN-filled output slice of a wider buffer in a sentinel arena."""
    C = H * 64
    q, k, v, _ = A.inputs(B, H, 1, Tk, seed=5)
    cache = torch.full((B, Tk + 2, 3 * C), NAN, dtype=BF)
    cache[:, :Tk, C:2 * C], cache[:, :Tk, 2 * C:] = _btc(k), _btc(v)
    cache = cache.to(cuda)
    row = torch.full((B, 2 * C), NAN, dtype=BF)
    row[:, C:] = _btc(q)[:, 0]
    out = _Out(cuda, (B, C + 128), o=lambda t: t[:, 64:64 + C])
    return (q, k, v), row.to(cuda)[:, C:], cache[:, :Tk, C:2 * C], cache[:, :Tk, 2 * C:], out


@pytest.mark.parametrize("Tk", [1, 31, 32, 33, 255, 256, 257, 4096])
def test_attn_decode_per_element(cuda, Tk):
    """gvl_attn_decode on strided views of a packed cache: the last row of the causal problem,
    held to the o bound (its P is not rounded, so it has a rounding in hand).  Measured: at most
    0.72 units of the 2 (Tk = 33)."""
    (q, k, v), qd, kd, vd, out = _decode_setup(cuda, Tk)
    ref, E, _ = A.attention_ref(q, k, v, torch.zeros_like(q), False, 0.125)
    _k().attn_decode(qd, kd, vd, 3, out=out["o"])
    torch.cuda.synchronize()
    out.check_rest()
    got = out["o"].cpu().reshape(2, 3, 1, 64)
    r = assert_attn_close(got, ref["o"], E["o"], A.HARD_UNITS["o"], name=f"decode Tk={Tk}",
                          slack=4 * A.baseline()["o"])
    _record(f"decode Tk={Tk}", dict(kernel=dict(o=r), bound=dict(o=A.HARD_UNITS["o"])))


def test_attn_decode_refuses_long_cache(cuda):
    """Tk = 4097 is past the kernel's score buffer: an error, and nothing launched."""
    from gvl._lib import GvlError
    _, qd, kd, vd, out = _decode_setup(cuda, 4097)
    with pytest.raises(GvlError, match="4097"):
        _k().attn_decode(qd, kd, vd, 3, out=out["o"])
    torch.cuda.synchronize()
    out.check_rest()
    assert torch.equal(_bits(out.outer), _bits(out.init)), "the refused call wrote its output"
