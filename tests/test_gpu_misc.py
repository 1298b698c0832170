"""Per-element parity of the last kernels a max-norm held, on the MI355X: gvl_colsum /
gvl_colsum_batched, gvl_dropout_mask_apply, gvl_gate_bwd / gvl_gate_bwd_acc_bf16
(csrc/optim.hip), gvl_pool_clip_ex and gvl_embedding_bwd (csrc/embed_pool.hip).

Every element is compared with a float64 reference of tests/misc_ref.py that reads the same
bf16 / fp32 inputs: bf16 outputs to one bf16 ulp (+ a count of fp32 roundings of the sum of the
absolute values of the terms, which matters only where the operation cancels), fp32 outputs to
a count of fp32 roundings, the dropout mask and the bf16 gate gradient bit for bit.  The counts
come from the same formula in fp32 on the CPU, times four (misc_ref.slack_of), never from a
kernel's output.  Shapes are the smallest that reach each branch of each kernel, views sit in
sentinel- or NaN-filled buffers, and what is measured goes to profiles/misc_margins.json."""
import numpy as np
import pytest
import torch

from tests import misc_ref as M
from tests.helpers import assert_bf16_close, assert_bf16_rounded, assert_f32_close
from tests.misc_ref import bits as _bits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
SENT = 7.0


def _k():
    from gvl import kernels as K
    return K


def _arena(t, cuda, off=None, fill=SENT):
    """The 1-D or 2-D tensor t inside a `fill`-filled flat buffer on the device, `off` elements
    in (default 16 bytes: aligned) -> (the view, a check that nothing outside it changed).  A
    2-D t keeps a row stride of cols + 8."""
    off = 16 // t.element_size() if off is None else off
    if t.dim() == 1:
        n, ld = t.numel(), None
    else:
        ld = t.shape[1] + 8
        n = t.shape[0] * ld
    big = torch.full((n + 2 * off + 8,), fill, dtype=t.dtype)
    inner = big[off:off + n]
    view = inner if ld is None else inner.view(t.shape[0], ld)[:, :t.shape[1]]
    view.copy_(t)
    before = big.clone()
    dev = big.to(cuda)
    inner_d = dev[off:off + n]
    view_d = inner_d if ld is None else inner_d.view(t.shape[0], ld)[:, :t.shape[1]]

    def untouched():
        now = dev.cpu()
        mask = torch.ones(big.numel(), dtype=torch.bool)
        m = mask[off:off + n]
        (m if ld is None else m.view(t.shape[0], ld)[:, :t.shape[1]]).fill_(False)
        a, b = _bits(now)[mask], _bits(before)[mask]
        return bool(torch.equal(a, b))

    return view_d, untouched


# ------------------------------------------------------------------------- column sums
def _colsum_check(cuda, rows, cols, acc, strided, key):
    K_ = _k()
    x = M.colsum_input(rows, cols)
    prev = (torch.randn(cols, generator=torch.Generator().manual_seed(cols)) * 4).to(BF)
    ref, E, base = M.colsum_ref(x, prev if acc else None)
    if strided:
        xd, x_ok = _arena(x, cuda, fill=float("nan"))
    else:
        xd, x_ok = x.to(cuda), lambda: True
    od, o_ok = _arena(prev if acc else torch.full((cols,), float("nan"), dtype=BF), cuda)
    K_.colsum(xd, out=od, accumulate=acc)
    torch.cuda.synchronize()
    assert o_ok() and x_ok(), "a store outside the output"
    e = assert_bf16_close(od.cpu(), ref, scale=E, slack=M.slack_of(base),
                          name=f"colsum {rows}x{cols} acc={acc} strided={strided}")
    M.record(f"colsum:{key}", dict(worst_ulp=e, cpu_baseline_units=base, slack=M.slack_of(base)))


@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("cols", M.COLSUM_COLS)
@pytest.mark.parametrize("rows", M.COLSUM_ROWS)
def test_colsum_per_column(cuda, rows, cols, acc):
    """Every column against its own float64 sum and its own sum of |x| (columns differ by up to
    2**8 in scale and every seventh cancels), contiguous and as a strided view (ld = cols + 8)
    of a NaN-filled buffer, into an output surrounded by sentinels; with `accumulate` the
    result is bf16(sum + previous), one rounding.  Rows 1 .. 129 walk the 16 row groups, the
    unrolled 128-row trip and its tail; cols 8 .. 264 a partial 128-column block and a partial
    32-column block of the finish."""
    for strided in (False, True):
        _colsum_check(cuda, rows, cols, acc, strided, f"{rows}x{cols}:{'acc' if acc else 'store'}"
                      f":{'view' if strided else 'dense'}")


@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
def test_colsum_split_cap(cuda, acc):
    """8200 x 8: 128 row splits (the cap) of 65 rows, a chunk that is no multiple of 16."""
    rows, cols = M.COLSUM_TALL
    for strided in (False, True):
        _colsum_check(cuda, rows, cols, acc, strided, f"{rows}x{cols}:{'acc' if acc else 'store'}"
                      f":{'view' if strided else 'dense'}")


@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("rows,cols", [(65, 136), (129, 264)])
@pytest.mark.parametrize("count", [1, 3, 16])
def test_colsum_batched_per_column(cuda, count, rows, cols, acc):
    """gvl_colsum_batched: problem i scaled by 2**(i - 3), strided inputs in NaN-filled buffers,
    every output checked per column with sentinels around it."""
    K_ = _k()
    xs, outs, oks, refs = [], [], [], []
    for i in range(count):
        x = M.colsum_input(rows, cols, seed=i, shift=i % 7 - 3)
        prev = (torch.randn(cols, generator=torch.Generator().manual_seed(i)) * 2.0 ** (i % 7 - 3)).to(BF)
        xd, x_ok = _arena(x, cuda, fill=float("nan"))
        od, o_ok = _arena(prev if acc else torch.full((cols,), float("nan"), dtype=BF), cuda)
        xs.append(xd), outs.append(od), oks.extend([x_ok, o_ok])
        refs.append(M.colsum_ref(x, prev if acc else None))
    K_.colsum_batched(xs, outs, accumulate=acc)
    torch.cuda.synchronize()
    assert all(ok() for ok in oks), "a store outside an output"
    worst = 0.0
    for i, (ref, E, base) in enumerate(refs):
        worst = max(worst, assert_bf16_close(outs[i].cpu(), ref, scale=E, slack=M.slack_of(base),
                                             name=f"colsum_batched[{i}/{count}] {rows}x{cols}"))
    M.record(f"colsum_batched:{count}x{rows}x{cols}:{'acc' if acc else 'store'}",
             dict(worst_ulp=worst, cpu_baseline_units=max(r[2] for r in refs)))


# ----------------------------------------------------------------------------- dropout
def _dropout_run(cuda, x, p, seed, in_off, out_off, offset=None):
    """x through gvl_dropout_mask_apply between strided views `in_off` / `out_off` elements
    into sentinel-filled buffers -> the output on the CPU."""
    K_ = _k()
    xd, x_ok = _arena(x, cuda, off=in_off)
    od, o_ok = _arena(torch.full(x.shape, float("nan"), dtype=BF), cuda, off=out_off)
    sp = None if offset is None else torch.tensor([offset], dtype=torch.int64, device=cuda)
    K_.dropout_mask_apply(xd, p, seed, out=od, seed_ptr=sp)
    torch.cuda.synchronize()
    assert x_ok() and o_ok(), "a store outside the output view"
    return od.cpu()


@pytest.mark.parametrize("p", [0.0, 0.1, 0.999])
@pytest.mark.parametrize("route,rows,cols,in_off,out_off", [
    ("8-wide", 37, 48, 8, 8),
    ("scalar-cols45", 37, 45, 8, 8),
    ("scalar-misaligned-in", 37, 48, 9, 8),
    ("scalar-misaligned-out", 37, 48, 8, 9),
])
def test_dropout_mask_apply_exact(cuda, route, rows, cols, in_off, out_off, p):
    """Bit for bit bf16_rne(fl32(x) * fl32(1 / (1 - p))) where the keep mask of element
    r * cols + c holds and +0 elsewhere, on strided views (ld = cols + 8) inside sentinel-filled
    buffers, with `seed` and with `seed_ptr`; p = 0 is the identity.  48 columns at an aligned
    offset take the 8-wide kernel; 45 columns, or 48 one element off, the scalar one: both give
    the same bits for the same logical tensor."""
    g = torch.Generator().manual_seed(rows * cols)
    x = (torch.randn(rows, cols, generator=g) * 3).to(BF)
    for seed, offset in ((77, None), (0x1234567890ABCDEF, None), (77, 5)):
        want, keep = M.dropout_ref(x, p, seed, offset)
        got = _dropout_run(cuda, x, p, seed, in_off, out_off, offset)
        assert torch.equal(_bits(got), _bits(want)), \
            f"{route} p={p} seed={seed} offset={offset}: {int((_bits(got) != _bits(want)).sum())} differ"
        if p == 0.0:
            assert torch.equal(_bits(got), _bits(x)) and bool(keep.all())
        else:
            assert 0 < int(keep.sum()) < keep.numel()
    M.record(f"dropout:{route}:p{p}", dict(bitwise=True, elements=rows * cols))


@pytest.mark.parametrize("route,rows,cols,off", [("scalar", 23400, 45, 9), ("8-wide", 8200, 1032, 8)])
def test_dropout_mask_apply_grid_stride(cuda, route, rows, cols, off):
    """More elements than one trip of the 4096 x 256 grid covers (scalar: 23,400 x 45; 8-wide:
    8,200 x 1,032 in vectors of 8), bit for bit."""
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, cols, generator=g).to(BF)
    want, _ = M.dropout_ref(x, 0.1, 99)
    got = _dropout_run(cuda, x, 0.1, 99, off, off)
    assert torch.equal(_bits(got), _bits(want))


# -------------------------------------------------------------------------------- gate
def _gate_run(cuda, dx, y, gate, off, acc=None, grad_bf16=None):
    """gvl_gate_bwd (acc: fp32 [1] on the device) or gvl_gate_bwd_acc_bf16 through the C ABI on
    views `off` elements into sentinel-filled buffers -> dy on the CPU."""
    K_ = _k()
    n = dx.numel()
    dxd, a_ok = _arena(dx, cuda, off=off)
    yd, b_ok = _arena(y, cuda, off=off)
    dyd, c_ok = _arena(torch.full((n,), float("nan"), dtype=BF), cuda, off=off)
    gd = gate.to(cuda)
    ws = torch.empty(max(K_._L().gvl_gate_bwd_workspace_size(n), 4) // 4, dtype=F32, device=cuda)
    if grad_bf16 is not None:
        K_._lib.check(K_._L().gvl_gate_bwd_acc_bf16(dxd.data_ptr(), yd.data_ptr(), gd.data_ptr(),
                                                    dyd.data_ptr(), grad_bf16.data_ptr(), n,
                                                    ws.data_ptr(), K_._stream()), "gate_bwd_acc_bf16")
    else:
        K_._lib.check(K_._L().gvl_gate_bwd(dxd.data_ptr(), yd.data_ptr(), gd.data_ptr(),
                                           dyd.data_ptr(), acc.data_ptr(), n, ws.data_ptr(),
                                           K_._stream()), "gate_bwd")
    torch.cuda.synchronize()
    assert a_ok() and b_ok() and c_ok(), "a store outside dy"
    return dyd.cpu()


GATE_CASES = [(n, 8, False) for n in M.GATE_SIZES] + [
    (2048, 9, False),               # an 8-multiple on a misaligned view: the scalar kernel
    (2048, 8, True), (2049, 8, True),  # dx * y cancels
    (M.GATE_STRIDE_SCALAR, 8, False), (M.GATE_STRIDE_VEC, 8, False)]


@pytest.mark.parametrize("gate", M.GATES)
@pytest.mark.parametrize("n,off,cancel", GATE_CASES)
def test_gate_bwd_per_element(cuda, n, off, cancel, gate):
    """dy within one bf16 ulp of tanh(gate) * dx in float64, and correctly rounded up to two
    fp32 roundings (tanhf, the product), which truncation is not; the gate gradient within
    4 x the CPU fp32 baseline of 2**-24 * sum|dx y| (1 - t^2) of float64; a second call adds
    into the same non-zero accumulator; gvl_gate_bwd_acc_bf16 gives the same dy and
    bf16(g + bf16(dg)) from the fp32 entry point's own dg, bit for bit.  n = 1 .. 9 and 2049
    take the scalar kernel, 8 and 2048 the 8-wide one; the two largest sizes need a second trip
    of the grid-stride loops.  At gate 9 tanh saturates: 1 - t^2 = 6e-8."""
    dx, y = M.gate_inputs(n, cancel=cancel)
    g = torch.tensor(gate).to(BF)
    ref = M.gate_ref(dx, y, g)
    slack = M.slack_of(ref["base"])
    acc = torch.zeros(1, dtype=F32, device=cuda)
    dy = _gate_run(cuda, dx, y, g, off, acc=acc)
    name = f"gate_bwd n={n} off={off} gate={gate}"
    e = assert_bf16_close(dy, ref["dy"], name=name + " dy")
    assert_bf16_rounded(dy, ref["dy"], np.abs(ref["dy"]), 2, name=name + " dy rounding")
    dg32 = acc.cpu().clone()
    units = assert_f32_close(dg32, [ref["dg"]], [ref["E"]], slack, name=name + " dgate")
    # twice more into a non-zero accumulator
    acc2 = torch.tensor([1.5], dtype=F32, device=cuda)
    _gate_run(cuda, dx, y, g, off, acc=acc2)
    dy2 = _gate_run(cuda, dx, y, g, off, acc=acc2)
    assert torch.equal(_bits(dy2), _bits(dy))
    assert_f32_close(acc2.cpu(), [1.5 + 2 * ref["dg"]], [1.5 + 2 * ref["E"]], slack + 2,
                     name=name + " accumulated")
    # the bf16 accumulator: two roundings from the kernel's own fp32 gradient
    g0 = torch.tensor([0.75], dtype=BF)
    gb = g0.to(cuda)
    dy3 = _gate_run(cuda, dx, y, g, off, grad_bf16=gb)
    assert torch.equal(_bits(dy3), _bits(dy))
    assert torch.equal(_bits(gb), _bits(M.bf16_add_two_roundings(g0, float(dg32[0]))))
    M.record(f"gate_bwd:n{n}:off{off}:{'cancel' if cancel else 'plain'}:gate{gate}",
             dict(dy_worst_ulp=e, dgate_units=units, cpu_baseline_units=ref["base"], slack=slack))


@pytest.mark.parametrize("gate", M.GATES)
def test_gate_bwd_routes_agree(cuda, gate):
    """The 8-wide and the scalar kernel on the same 2048 elements: dy bit-identical."""
    dx, y = M.gate_inputs(2048, seed=1)
    g = torch.tensor(gate).to(BF)
    a = _gate_run(cuda, dx, y, g, 8, acc=torch.zeros(1, dtype=F32, device=cuda))
    b = _gate_run(cuda, dx, y, g, 9, acc=torch.zeros(1, dtype=F32, device=cuda))
    assert torch.equal(_bits(a), _bits(b))


# -------------------------------------------------------------------------------- pool
def _pool_run(cuda, tok, out_dtype, normalize, in_off):
    K_ = _k()
    B, L, D = tok.shape
    td, t_ok = _arena(tok.reshape(-1), cuda, off=in_off)
    od, o_ok = _arena(torch.full((B * 33 * D,), float("nan"), dtype=out_dtype), cuda)
    K_._lib.check(K_._L().gvl_pool_clip_ex(td.data_ptr(), int(tok.dtype == F32), od.data_ptr(),
                                           int(out_dtype == F32), B, L, D, int(normalize),
                                           K_._stream()), "gvl_pool_clip_ex")
    torch.cuda.synchronize()
    assert t_ok() and o_ok(), "a store outside the output"
    return od.cpu().view(B, 33, D)


def _pool_cases():
    c = []
    for side in M.POOL_SIDES:
        for D in M.POOL_DS:
            for dt in (F32, BF):
                c.append((side, D, dt, None))
    c.append((16, 768, F32, 5))  # one float off 16 bytes: pool_kernel<float>, unrolled
    c.append((14, 260, F32, 5))
    return c


def _pool_id(c):
    side, D, dt, off = c
    return (f"{M.pool_route(side, D, dt == F32, off is None)}-side{side}-D{D}-"
            f"{'fp32' if dt == F32 else 'bf16'}{'' if off is None else '-misaligned'}")


@pytest.mark.parametrize("case", _pool_cases(), ids=_pool_id)
def test_pool_clip_per_element(cuda, case):
    """CLS + the 32 adaptive-average windows (+ L2 normalise) against float64, each of the 33
    rows against its own scale (the window mean of |x|, over the norm when normalising; the CLS
    row, one window and the rest differ by 2**10): fp32 out within 4 x the CPU fp32 baseline of
    2**-24 * scale, bf16 out to one bf16 ulp on top, for B = 1 and 3, with and without
    normalising, sentinels around the output.  The test id names the kernel instance: pool4<8>
    (windows <= 8), pool4<16> (<= 16), pool<float> / pool<bf16> with the unrolled window
    (<= 8 patches) or the runtime loop, D % 4 != 0 and a misaligned input included; windows
    overlap below side 8."""
    side, D, dt, off = case
    in_off = (16 // (4 if dt == F32 else 2)) if off is None else off
    worst = {}
    for B in (1, 3):
        tok = M.pool_input(B, side, D, dt)
        for normalize in (0, 1):
            ref, scale, base = M.pool_ref(tok, normalize)
            slack = M.slack_of(base)
            for od in (F32, BF):
                got = _pool_run(cuda, tok, od, normalize, in_off)
                name = f"pool {_pool_id(case)} B={B} normalize={normalize} out={od}"
                if od == F32:
                    u = assert_f32_close(got, ref, scale, slack, name=name)
                    worst[f"norm{normalize}"] = dict(kernel_units=u, cpu_baseline_units=base)
                else:
                    assert_bf16_close(got, ref, scale=scale, slack=slack, name=name)
    M.record(f"pool:{_pool_id(case)}", worst)


@pytest.mark.parametrize("side,D,dt", [(16, 768, F32), (14, 768, F32), (16, 6, F32), (24, 260, F32),
                                       (16, 768, BF), (24, 260, BF)])
def test_pool_clip_zero_grid(cuda, side, D, dt):
    """An all-zero token grid pools to exact zeros (the 1e-12 clamp of the norm), not NaN; the
    CLS row is still normalised."""
    tok = M.pool_input(2, side, D, dt, zero_grid=True)
    ref, scale, base = M.pool_ref(tok, 1)
    for od in (F32, BF):
        got = _pool_run(cuda, tok, od, 1, 16 // tok.element_size())
        assert not torch.any(_bits(got[:, 1:]) != 0), "a zero window must pool to +0"
        if od == F32:
            assert_f32_close(got[:, 0], ref[:, 0], scale[:, 0], M.slack_of(base))
        else:
            assert_bf16_close(got[:, 0], ref[:, 0], scale=scale[:, 0], slack=M.slack_of(base))


# ------------------------------------------------------------------ embedding backward
@pytest.mark.parametrize("which", ["both", "dwte", "dwpe"])
@pytest.mark.parametrize("C", [2, 130, 768])
def test_embedding_bwd_atomic_per_element(cuda, C, which):
    """gvl_embedding_bwd (fp32 atomics, any order): every element of dwte / dwpe within
    (terms + 1) * 2**-24 * (sum of |terms|) of float64, from non-zero accumulators; id 7 is hot
    (500 copies), two ids are out of range (nothing for dwte, still counted in dwpe), the rows
    start at out_offset = 3 of 24-row groups, 1,402 tokens are no multiple of 4, either
    accumulator may be null, and the rows of untouched ids keep their bits."""
    K_ = _k()
    idx, dout, T, S, off, V, n = M.emb_case(C)
    gen = torch.Generator().manual_seed(C)
    w0 = torch.randn(V, C, generator=gen) if which != "dwpe" else None
    p0 = torch.randn(T + 2, C, generator=gen) if which != "dwte" else None
    ref = M.emb_bwd_ref(idx, dout, T, S, off, C, V, n, w0, p0)
    wd = pd = None
    oks = []
    if w0 is not None:
        wd, ok = _arena(w0.reshape(-1), cuda)
        oks.append(ok)
    if p0 is not None:
        pd, ok = _arena(p0.reshape(-1), cuda)
        oks.append(ok)
    idx_d, dout_d = idx.to(cuda), dout.to(cuda)
    K_._lib.check(K_._L().gvl_embedding_bwd(idx_d.data_ptr(), dout_d.data_ptr(),
                                            K_._p(wd), K_._p(pd), n, T, C, V, S, off,
                                            K_._stream()), "gvl_embedding_bwd")
    torch.cuda.synchronize()
    assert all(ok() for ok in oks), "a store outside the accumulators"
    rec = {}
    for name, dev, init in (("dwte", wd, w0), ("dwpe", pd, p0)):
        if init is None:
            continue
        got = dev.cpu().view(init.shape)
        rec[name] = assert_f32_close(got, ref[name], ref["E_" + name] * ref["S_" + name], 1,
                                     name=f"embedding_bwd C={C} {name}")
        same = np.ones(init.shape[0], dtype=bool)
        same[ref["touched_" + name]] = False
        assert same.any() and torch.equal(_bits(got[same]), _bits(init[same]))
        assert not torch.equal(_bits(got[~same]), _bits(init[~same]))
    if w0 is not None:
        assert int((idx.view(-1)[:n] == M.EMB_HOT).sum()) >= M.EMB_HOT_COPIES
    M.record(f"embedding_bwd:C{C}:{which}", dict(units_of_terms_plus_one=rec))
