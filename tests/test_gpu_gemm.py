"""Per-element parity of the GEMM family on the MI355X, one case per kernel instance.

tests/test_gpu_kernels.py judges a GEMM by rel_err < 8e-3: one number per tensor, divided by the
largest output.  Here every element of C and of the side output is compared with the float64
reference of tests/gemm_ref.py: a bf16 output within half a bf16 ulp plus slack * 2**-24 * E
(helpers.assert_bf16_rounded), an fp32 output within slack * 2**-24 * E, where E is the sum of
the absolute values of the terms added to form the element and slack is four times the error
of the same operation in fp32 on the CPU, never taken from the kernel.  On the *exact* inputs
(small integers: every partial sum exact in fp32) the linear epilogues must give the correctly
rounded result bit for bit, whatever the route.  C and pre_out live in NaN-filled arenas with
ld > N, so a store outside the M x N view shows; the inputs must come back unchanged; two calls
must agree bit for bit.  tests/test_gemm_ref_cpu.py shows that the bound rejects the doctored
outputs rel_err accepts.  The measured margins go to profiles/gemm_margins.json through
helpers.margins_out."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_ref as G
from tests.helpers import assert_bf16_rounded, assert_f32_close, f64, margins_out

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_MARGINS = {}


def _record(key, rec):
    _MARGINS[key] = rec
    margins_out("gemm_margins", _MARGINS)


def _k():
    from gvl import kernels as K
    return K


def _lib():
    from gvl import _lib as L
    return L


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Arena:
    """An [M, N] view with row stride ld > N at a 16-byte offset inside a NaN-filled buffer on
    the device; untouched(): nothing outside the view (gap columns included) has changed."""

    def __init__(self, M, N, ld, dtype, cuda, vals=None):
        self.off = 16 // torch.empty(0, dtype=dtype).element_size()
        self.M, self.N, self.ld = M, N, ld
        self.flat = torch.full((M * ld + 2 * self.off,), float("nan"), dtype=dtype, device=cuda)
        self.view = self.flat[self.off:self.off + M * ld].view(M, ld)[:, :N]
        if vals is not None:
            self.view.copy_(vals.to(cuda))
        self.before = _bits(self.flat).clone()

    def untouched(self):
        now = _bits(self.flat)
        same = now == self.before
        body = same[self.off:self.off + self.M * self.ld].view(self.M, self.ld)
        return bool(same[:self.off].all() and same[self.off + self.M * self.ld:].all()
                    and body[:, self.N:].all())

    def unchanged(self):
        return bool((_bits(self.flat) == self.before).all())


class Run:
    """The device operands of one case on one input set, and its launch."""

    def __init__(self, case, ins, cuda):
        K_ = _k()
        f = G.EPIS[case["epi"]]
        M, N = case["M"], case["N"]
        _, _, ldc, ld = G.lds_of(case)
        self.case, self.f, self.cuda = case, f, cuda
        A, B = ins["A"], ins["B"]
        self.A = (A.t().contiguous() if case["a_mn"] else A.contiguous()).to(cuda)
        self.B = (B.contiguous() if case["b_mn"] else B.t().contiguous()).to(cuda)
        self.bias = ins["bias"].to(cuda) if "bias" in ins else None
        self.gate = ins["gate"].to(cuda) if "gate" in ins else None
        self.inplace = f.get("residual") == "c"
        self.res0 = ins.get("residual")
        self.Cd = Arena(M, N, ldc, torch.float32 if f.get("c_fp32") else BF, cuda,
                        vals=self.res0 if self.inplace else None)
        self.aux = None  # residual or pre_in
        if "pre_in" in ins or (self.res0 is not None and not self.inplace):
            self.aux = Arena(M, N, ld, BF, cuda, vals=ins["pre_in"] if "pre_in" in ins else self.res0)
        self.pre = Arena(M, N, ld, BF, cuda) if f.get("pre_out") else None
        ad = case.get("alpha_dev")
        self.alpha_ptr = torch.tensor([ad], dtype=torch.float32, device=cuda) if ad is not None else None
        so = case.get("seed_off")
        self.seed_ptr = torch.tensor([so], dtype=torch.int64, device=cuda) if so is not None else None
        self.ws, self.tk = K_._gemm_workspace(cuda), K_._gemm_tickets(cuda)
        self.const = [t for t in (self.A, self.B, self.bias, self.gate) if t is not None]
        self.const0 = [_bits(t).clone() for t in self.const]

    def ptrs(self):
        z = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        return dict(a=z(self.A), b=z(self.B), c=self.Cd.view.data_ptr(),
                    aux=z(self.aux.view if self.aux else None), aux2=z(self.pre.view if self.pre else None),
                    bias=z(self.bias), gate=z(self.gate), alpha_ptr=z(self.alpha_ptr), seed_ptr=z(self.seed_ptr),
                    ws=self.ws.data_ptr(), tickets=self.tk.data_ptr())

    def name(self):
        return G.kernel_name(_lib().lib(), self.case, self.ptrs())

    def reset(self):
        if self.inplace:
            self.Cd.view.copy_(self.res0.to(self.cuda))

    def launch(self):
        """Under the case's tune: through gvl.kernels.gemm with workspace and tickets, or through
        the descriptor alone without them."""
        c, f, L = self.case, self.f, _lib()
        L.lib().gvl_gemm_tune(*c["tune"])
        try:
            if c["ws"]:
                res = self.Cd.view if self.inplace else (self.aux.view if f.get("residual") else None)
                _k().gemm(self.A, self.B, a_mn=bool(c["a_mn"]), b_mn=bool(c["b_mn"]), out=self.Cd.view,
                          alpha=c.get("alpha", 1.0), alpha_ptr=self.alpha_ptr, bias=self.bias,
                          act=f.get("act", 0), dact=f.get("dact", 0),
                          pre_out=self.pre.view if self.pre else None,
                          pre_in=self.aux.view if f.get("pre_in") else None, residual=res, gate=self.gate,
                          drop_p=c.get("drop_p", G.DROP_P) if f.get("drop") else 0.0, seed=G.SEED,
                          seed_ptr=self.seed_ptr, out_dtype=self.Cd.view.dtype)
            else:
                d = G.fill_desc(c, self.ptrs())
                L.check(L.lib().gvl_gemm(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                        "gvl_gemm")
            torch.cuda.synchronize()
        finally:
            L.lib().gvl_gemm_tune(3, -1)
        return self.Cd.view.detach().cpu().clone(), (self.pre.view.detach().cpu().clone() if self.pre else None)


def _beyond_rounding(got, ref64, E, fp32):
    """max over the elements of (|got - ref| - half a bf16 ulp of ref) in units of 2**-24 E: what
    the arithmetic in front of the final rounding added (an fp32 output has no such rounding)."""
    err = np.abs(f64(got) - f64(ref64)) - (0.0 if fp32 else 0.5 * G.ulp_bf16(ref64))
    unit = G.F32_UNIT * np.abs(f64(E))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err <= 0, 0.0, np.where(unit > 0, err / unit, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max())


def _check_case(case, kind, cuda):
    if kind == "exact" and G.EPIS[case["epi"]].get("drop"):
        case = dict(case, drop_p=0.5)  # drop_scale = 2: the kept elements stay exact
    ins = G.inputs(kind, case["M"], case["N"], case["K"], case["epi"], seed=case["i"])
    exact = kind == "exact" and G.bitwise(case)
    ref = G.reference(case, ins, seed_off=case.get("seed_off"), emulate=not exact)
    r = Run(case, ins, cuda)
    assert r.name() == case["name"], (case["id"], r.name())
    got, side = r.launch()
    tag = f"{case['id']}/{kind}"
    rec = dict(instance=case["name"])
    f = r.f
    # ---- buffers
    assert r.Cd.untouched(), f"{tag}: C written outside its M x N view"
    if r.pre:
        assert r.pre.untouched(), f"{tag}: pre_out written outside its M x N view"
    if r.aux:
        assert r.aux.unchanged(), f"{tag}: pre_in / residual changed"
    for t, b in zip(r.const, r.const0):
        assert bool((_bits(t) == b).all()), f"{tag}: an input operand changed"
    if case["ws"]:
        assert int(r.tk.abs().max()) == 0, f"{tag}: tickets not returned to zero"
    # ---- dropout: the zero pattern is the restated hash
    if f.get("drop"):
        keep = ref["kw"]["keep"]
        base, _ = G.epilogue64(f64(ins["A"]) @ f64(ins["B"]), **{**ref["kw"], "residual": None, "drop_p": 0.0,
                                                                   "keep": None})
        res = f64(ins["residual"])
        # a dropped element is the residual, bit for bit; a kept one differs from it wherever the
        # branch is large enough to survive the rounding of the sum (two ulps of the result)
        assert np.all(f64(got)[~keep] == res[~keep]), f"{tag}: a dropped element is not the residual"
        sure = np.abs(base) * G.drop_scale(ref["kw"]["drop_p"]) > 2 * G.ulp_bf16(ref["ref"])
        assert np.array_equal((f64(got) != res)[sure], keep[sure]), f"{tag}: dropout mask differs from the hash"
        if side is not None:  # the un-gated branch after the dropout: its zeros are the mask itself
            nz = ref["side"] != 0
            assert np.array_equal((f64(side) != 0)[nz | ~keep], keep[nz | ~keep]), f"{tag}: pre_out zeros differ from the hash"
    # ---- values
    if exact:
        want = np.asarray(ref["ref"], dtype=np.float32)
        if f.get("c_fp32"):
            assert np.array_equal(got.numpy(), want), f"{tag}: fp32 C differs from the exact result"
        else:
            assert torch.equal(_bits(got), _bits(G.round_bf16(ref["ref"]))), \
                f"{tag}: C is not the correctly rounded exact result " \
                f"({int((_bits(got) != _bits(G.round_bf16(ref['ref']))).sum())} elements differ)"
        rec.update(bitwise=True)
    else:
        # figures first (printed and recorded whether or not the assertions hold): the kernel's
        # error beyond the half ulp of its final rounding, the emulation's own error and the
        # bound, all in units of 2**-24 E
        fp32 = bool(f.get("c_fp32"))
        rec.update(kernel=_beyond_rounding(got, ref["ref"], ref["E"], fp32), emu=ref["emu"], bound=ref["slack"])
        if side is not None:
            rec.update(kernel_side=_beyond_rounding(side, ref["side"], ref["E_side"], False),
                       emu_side=ref["emu_side"], bound_side=ref["slack_side"])
        print(tag, {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items() if k != "instance"})
        _record(tag, rec)
        if fp32:
            assert_f32_close(got, ref["ref"], ref["E"], ref["slack"], tag + " C(fp32)")
        else:
            assert_bf16_rounded(got, ref["ref"], ref["E"], ref["slack"], tag + " C")
        if side is not None:
            assert_bf16_rounded(side, ref["side"], ref["E_side"], ref["slack_side"], tag + " pre_out")
    # ---- determinism
    r.reset()
    got2, side2 = r.launch()
    assert torch.equal(_bits(got), _bits(got2)), f"{tag}: two calls differ in C"
    if side is not None:
        assert torch.equal(_bits(side), _bits(side2)), f"{tag}: two calls differ in pre_out"
    _record(tag, rec)


def _family(c):
    return c["name"].split("<")[0]


def _ids(cs):
    return [c["id"] for c in cs]


_PP3 = [c for c in G.CASES if _family(c) == "gemm_pp3_kernel"]
_PP3_A = [c for c in _PP3 if not c["a_mn"]]
_PP3_B = [c for c in _PP3 if c["a_mn"]]
_W4 = [c for c in G.CASES if _family(c).startswith("gemm_w4")]
_REST = [c for c in G.CASES if _family(c) not in ("gemm_pp3_kernel",) and not _family(c).startswith("gemm_w4")]
assert len(_PP3_A) + len(_PP3_B) + len(_W4) + len(_REST) == len(G.CASES)


def _run(case, cuda):
    for kind in G.kinds_of(case):
        _check_case(case, kind, cuda)


@pytest.mark.parametrize("case", _PP3_A, ids=_ids(_PP3_A))
def test_gemm_pp3_k_contiguous_a(cuda, case):
    _run(case, cuda)


@pytest.mark.parametrize("case", _PP3_B, ids=_ids(_PP3_B))
def test_gemm_pp3_mn_contiguous_a(cuda, case):
    _run(case, cuda)


@pytest.mark.parametrize("case", _W4, ids=_ids(_W4))
def test_gemm_four_wave(cuda, case):
    _run(case, cuda)


@pytest.mark.parametrize("case", _REST, ids=_ids(_REST))
def test_gemm_ring_lds_regstage(cuda, case):
    _run(case, cuda)


@pytest.mark.parametrize("case", G.EXCLUDED_CASES, ids=_ids(G.EXCLUDED_CASES))
def test_gemm_excluded_instances_exact(cuda, case):
    """Instances whose planner forces a shape over the cost cap: the *exact* inputs only, an fp32
    reference (exact), bit for bit."""
    _check_case(case, "exact", cuda)


# ------------------------------------------------------------------- route agreement
@pytest.mark.parametrize("epi", ["bias_res", "plain"])
def test_routes_agree_on_exact_inputs(cuda, epi):
    """Every route that admits 304 x 136 x 192 gives the same bits on the *exact* inputs."""
    seen = {}
    for tune in G.AGREE_TUNES:
        for ws in (1, 0):
            case = G._case(900, ("?", tune, ws, 304, 136, 192, 0, 0, epi))
            ins = G.inputs("exact", 304, 136, 192, epi, seed=900)
            r = Run(case, ins, cuda)
            got, _ = r.launch()
            assert r.Cd.untouched()
            seen.setdefault(r.name(), got)
            want = G.round_bf16(G.reference(case, ins, emulate=False)["ref"])
            assert torch.equal(_bits(got), _bits(want)), (tune, ws, r.name())
    assert len(seen) >= 4, sorted(seen)


# ------------------------------------------------- batched, grouped and bias sums
def _sum_slack(x64, axis, add64, ref, E, a=1.0):
    """4 x the error of the same sum in fp32 on the CPU, pairwise (numpy) and term by term."""
    x32, add32 = np.asarray(x64, dtype=np.float32), np.asarray(add64, dtype=np.float32)
    seq = np.zeros(np.shape(ref), dtype=np.float32)
    for row in np.moveaxis(x32, axis, 0):
        seq += row
    return G.slack_of([np.float32(a) * x32.sum(axis=axis, dtype=np.float32) + add32, np.float32(a) * seq + add32],
                      ref, E)


def _dw_items(cuda, count, M, N, K, kind, seed, acc):
    """count weight-gradient problems dW (+)= dY^T X: dY [K, M], X [K, N] (both MN-contiguous)."""
    items, refs = [], []
    for i in range(count):
        ins = G.inputs(kind, M, N, K, "bias_res", seed=seed + i)
        A, B = ins["A"], ins["B"]  # [M, K], [K, N]
        out0 = ins["residual"] if acc else torch.zeros(M, N, dtype=BF)
        arena = Arena(M, N, N + 8, BF, cuda, vals=out0)
        items.append((A.t().contiguous().to(cuda), B.contiguous().to(cuda), arena.view, acc))
        h = f64(A) @ f64(B)
        E = np.abs(f64(A)) @ np.abs(f64(B))
        if acc:
            h, E = h + f64(out0), E + np.abs(f64(out0))
        emu = [G.matmul32_seq(f64(A), f64(B)) + (np.asarray(f64(out0), dtype=np.float32) if acc else 0),
               (A.float() @ B.float()).numpy() + (out0.float().numpy() if acc else 0)]
        db0 = ins["bias"][:M] if M <= N else torch.cat([ins["bias"]] * (M // N + 1))[:M]
        cs = f64(A).sum(axis=1) + f64(db0)
        Ecs = np.abs(f64(A)).sum(axis=1) + np.abs(f64(db0))
        refs.append(dict(arena=arena, ref=h, E=E, slack=G.slack_of(emu, h, E), db0=db0, cs=cs, Ecs=Ecs,
                         cs_slack=_sum_slack(f64(A), 1, f64(db0), cs, Ecs)))
    return items, refs


@pytest.mark.parametrize("kind", ["exact", "scaled"])
@pytest.mark.parametrize("acc,dbias", [(False, False), (True, False), (True, True)])  # dbias needs C += AB
@pytest.mark.parametrize("count,M,N,K", [
    (12, 776, 776, 64),   # 12 x 4 x 4 tiles of 256 x 256: one fused launch of whole-K tiles
    (4, 776, 776, 1024),  # 64 tiles: the two K-halves meet inside the launch; N % 16 == 8
], ids=["whole_k", "split_k"])
def test_gemm_batched_per_element(cuda, kind, acc, dbias, count, M, N, K):
    K_ = _k()
    items, refs = _dw_items(cuda, count, M, N, K, kind, 40, acc)
    dbs = [r["db0"].clone().to(cuda) for r in refs] if dbias else None
    ok = K_.gemm_batched(items, a_mn=True, b_mn=True, dbias=dbs)
    torch.cuda.synchronize()
    assert ok is not False
    name = K_._batched_name()
    assert name, "the batch ran problem by problem"
    worst = bound = 0.0
    for i, (it, r) in enumerate(zip(items, refs)):
        assert r["arena"].untouched()
        got = it[2].detach().cpu()
        if kind == "exact":
            assert torch.equal(_bits(got), _bits(G.round_bf16(r["ref"]))), f"problem {i}"
        else:
            worst = max(worst, _beyond_rounding(got, r["ref"], r["E"], False))
            bound = max(bound, r["slack"])
            assert_bf16_rounded(got, r["ref"], r["E"], r["slack"], f"batched[{i}]")
        if dbias:
            # the bias sums are MFMA sums of K terms, then added to the bf16 gradient in fp32
            gd = dbs[i].detach().cpu()
            if kind == "exact":
                assert torch.equal(_bits(gd), _bits(G.round_bf16(r["cs"]))), f"dbias {i}"
            else:
                assert_bf16_rounded(gd, r["cs"], r["Ecs"], r["cs_slack"], f"dbias[{i}]")
    assert int(K_._gemm_tickets(cuda).abs().max()) == 0, "tickets not returned to zero"
    _record(f"batched/{count}x{K}/{kind}/acc{int(acc)}/dbias{int(dbias)}", dict(instance=name, bitwise=True) if kind == "exact" else
            dict(instance=name, kernel=worst, emu=bound / 4, bound=bound))


@pytest.mark.parametrize("kind", ["exact", "scaled"])
def test_gemm_grouped_per_element(cuda, kind):
    K_ = _k()
    shapes = [(776, 264, 64), (264, 776, 96), (520, 520, 160)]
    items, refs, dbs = [], [], []
    alpha_dev = 0.5
    ap = torch.tensor([alpha_dev], dtype=torch.float32, device=cuda)
    for i, (M, N, K) in enumerate(shapes):
        ins = G.inputs(kind, M, N, K, "bias_res", seed=60 + i)
        A, B, out0 = ins["A"], ins["B"], ins["residual"]
        a = alpha_dev if i == 1 else 1.0
        arena = Arena(M, N, N + 8, BF, cuda, vals=out0)
        items.append((A.t().contiguous().to(cuda), B.contiguous().to(cuda), arena.view) + ((ap,) if i == 1 else ()))
        h = a * (f64(A) @ f64(B)) + f64(out0)
        E = a * (np.abs(f64(A)) @ np.abs(f64(B))) + np.abs(f64(out0))
        emu = [np.float32(a) * G.matmul32_seq(f64(A), f64(B)) + out0.float().numpy(),
               np.float32(a) * (A.float() @ B.float()).numpy() + out0.float().numpy()]
        db0 = torch.cat([ins["bias"]] * (M // N + 1))[:M]
        dbs.append(None if i == 2 else db0.clone().to(cuda))
        cs, Ecs = a * f64(A).sum(axis=1) + f64(db0), a * np.abs(f64(A)).sum(axis=1) + np.abs(f64(db0))
        refs.append(dict(arena=arena, ref=h, E=E, slack=G.slack_of(emu, h, E), cs=cs, Ecs=Ecs,
                         cs_slack=_sum_slack(f64(A), 1, f64(db0), cs, Ecs, a)))
    assert K_.gemm_grouped(items, dbias=dbs), "the grouped launch did not qualify"
    torch.cuda.synchronize()
    name = K_._batched_name()
    assert name
    worst = bound = 0.0
    for i, (it, r) in enumerate(zip(items, refs)):
        assert r["arena"].untouched()
        got = it[2].detach().cpu()
        if kind == "exact":
            assert torch.equal(_bits(got), _bits(G.round_bf16(r["ref"]))), f"problem {i}"
        else:
            worst = max(worst, _beyond_rounding(got, r["ref"], r["E"], False))
            bound = max(bound, r["slack"])
            assert_bf16_rounded(got, r["ref"], r["E"], r["slack"], f"grouped[{i}]")
        if dbs[i] is not None:
            gd = dbs[i].detach().cpu()
            if kind == "exact":
                assert torch.equal(_bits(gd), _bits(G.round_bf16(r["cs"]))), f"dbias {i}"
            else:
                assert_bf16_rounded(gd, r["cs"], r["Ecs"], r["cs_slack"], f"grouped dbias[{i}]")
    _record(f"grouped/{kind}", dict(instance=name, bitwise=True) if kind == "exact" else
            dict(instance=name, kernel=worst, emu=bound / 4, bound=bound))


@pytest.mark.parametrize("kind", ["exact", "scaled"])
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("batched", [False, True])
def test_colsum_per_element(cuda, kind, acc, batched):
    K_ = _k()
    rows, cols, n = 1000, 264, (3 if batched else 1)
    xs, outs, refs = [], [], []
    for i in range(n):
        ins = G.inputs(kind, rows, cols, 32, "bias", seed=80 + i)
        x = torch.cat([ins["A"]] * (cols // 32 + 1), dim=1)[:, :cols].contiguous()  # [rows, cols]
        x = (x.float() * ins["B"][0].float()[None, :]).to(BF) if kind == "scaled" else x
        o0 = ins["bias"]
        xa = Arena(rows, cols, cols + 8, BF, cuda, vals=x)
        xs.append(xa)
        outs.append(o0.clone().to(cuda) if acc else torch.full((cols,), float("nan"), dtype=BF, device=cuda))
        add = f64(o0) if acc else np.zeros(cols)
        ref, E = f64(x).sum(axis=0) + add, np.abs(f64(x)).sum(axis=0) + np.abs(add)
        refs.append((ref, E, _sum_slack(f64(x), 0, add, ref, E)))
    if batched:
        K_.colsum_batched([a.view for a in xs], outs, accumulate=acc)
    else:
        K_.colsum(xs[0].view, out=outs[0], accumulate=acc)
    torch.cuda.synchronize()
    for i in range(n):
        assert xs[i].unchanged()
        got = outs[i].detach().cpu()
        if kind == "exact":
            assert torch.equal(_bits(got), _bits(G.round_bf16(refs[i][0])))
        else:
            assert_bf16_rounded(got, refs[i][0], refs[i][1], refs[i][2], f"colsum[{i}]")
