"""The wide row kernels (1024 < cols <= 2048) and the named GPT-2 sizes, without a GPU: the three
gvl_layernorm_*_wide entry points refuse what they cannot run before any launch (tests/
test_capi.py's host-array and sentinel method), GPT2_SIZES / GPTConfig.for_size give the four
published shapes, the wide CPU baselines (tests/wide_ref.py) keep the references inside their
own 4 x rule, and the GEMM routes of the wide LM shapes match tests/data/gemm_routes_wide.json."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from tests import wide_ref as WR
from tests.conftest import ROOT
from tests.test_capi import SENT16, _host

sys.path.insert(0, os.path.join(ROOT, "tools"))


def _lib():
    from gvl import _lib as L
    return L.load()


def test_layernorm_fwd_wide_refuses_bad_arguments_before_any_launch():
    """cols = 1024 (the narrow entry's), 2056 (past the cap), 1036 (no multiple of 8), a leading
    dimension that is no multiple of 8, x / y / w / b off the 16-byte grid: -1 with the message,
    y and the statistics keep their sentinels."""
    lib = _lib()
    rows, ld = 2, 2064
    x = _host(rows * ld + 8, np.uint16, 0x3F80)
    w, b = _host(ld + 8, np.uint16, 0x3F80), _host(ld + 8, np.uint16, 0)
    y = _host(rows * ld + 8, np.uint16, SENT16)
    mean, rstd = _host(rows, np.float32, 7.0), _host(rows, np.float32, 7.0)
    P = lambda a, byte_off=0: a.ctypes.data + byte_off

    def fwd(cols=1032, ldx=1040, ldy=1040, xp=P(x), yp=P(y), wp=P(w), bp=P(b)):
        return lib.gvl_layernorm_fwd_wide(xp, ldx, wp, bp, yp, ldy, P(mean), P(rstd), rows, cols,
                                          1e-5, None)

    def refused(rc, cols):
        want = b"gvl_layernorm_fwd_wide: cols=%d unsupported" % cols
        assert rc == -1 and want in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (y == SENT16).all() and (mean == 7.0).all() and (rstd == 7.0).all()

    for cols in (1024, 2056, 1036, 0, 8):
        refused(fwd(cols=cols, ldx=2064, ldy=2064), cols)
    refused(fwd(ldx=1036), 1032)
    refused(fwd(ldy=1044), 1032)
    refused(fwd(xp=P(x, 8)), 1032)
    refused(fwd(yp=P(y, 8)), 1032)
    refused(fwd(yp=P(y, 2)), 1032)
    refused(fwd(wp=P(w, 8)), 1032)
    refused(fwd(bp=P(b, 8)), 1032)
    assert b"<= 2048" in lib.gvl_last_error()


def test_layernorm_bwd_wide_refuses_bad_arguments_before_any_launch():
    """Every GVL_REQUIRE of gvl_layernorm_bwd_wide: a width of 1024, 2056 or 1036, a leading
    dimension (dy, x, dx, residual) that is no multiple of 8, a dx or residual off the 16-byte
    grid, dw / db / deferral without a workspace.  -1 with the message, and dx, dw, db and the
    workspace keep their sentinels."""
    lib = _lib()
    rows, ld = 4, 2064
    dy, x, res = (_host(rows * ld, np.uint16, 0x3F80) for _ in range(3))
    w = _host(ld, np.uint16, 0x3F80)
    mean, rstd = _host(rows, np.float32, 0.0), _host(rows, np.float32, 1.0)
    dx = _host(rows * ld + 8, np.uint16, SENT16)
    dw, db = _host(ld, np.uint16, SENT16), _host(ld, np.uint16, SENT16)
    ws = _host(2 * ld, np.float32, 7.0)
    P = lambda a, byte_off=0: a.ctypes.data + byte_off

    def bwd(cols=1032, lddy=1040, ldx=1040, rp=None, ldr=0, dxp=None, lddx=1040, acc_dx=0, dwp=None,
            dbp=None, acc_wb=0, wsp=None):
        return lib.gvl_layernorm_bwd_wide(P(dy), lddy, P(x), ldx, P(w), P(mean), P(rstd), rp, ldr,
                                          P(dx) if dxp is None else dxp, lddx, acc_dx, dwp, dbp,
                                          acc_wb, wsp, rows, cols, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (dx == SENT16).all() and (dw == SENT16).all() and (db == SENT16).all()
        assert (ws == 7.0).all()

    shape = b"gvl_layernorm_bwd_wide: cols unsupported"
    for cols in (1024, 2056, 1036, 0):
        refused(bwd(cols=cols, lddy=2064, ldx=2064, lddx=2064, dwp=P(dw), dbp=P(db), wsp=P(ws)), shape)
    refused(bwd(lddy=1044), shape)
    refused(bwd(ldx=1044), shape)
    refused(bwd(lddx=1044), shape)
    refused(bwd(lddx=1036, acc_dx=1), shape)
    refused(bwd(dxp=P(dx, 8)), shape)   # 8-byte aligned only
    refused(bwd(dxp=P(dx, 2)), shape)
    refused(bwd(rp=P(res), ldr=1044, acc_dx=1), shape)
    refused(bwd(rp=P(res, 8), ldr=1040, acc_dx=1), shape)
    assert b"<= 2048" in lib.gvl_last_error()
    need = b"gvl_layernorm_bwd_wide: dw/db need a workspace"
    refused(bwd(dwp=P(dw)), need)
    refused(bwd(dbp=P(db)), need)
    refused(bwd(dwp=P(dw), dbp=P(db), acc_wb=1), need)
    refused(bwd(acc_wb=2), need)        # deferred partials with nowhere to leave them


def test_layernorm_finalize_batched_wide_refuses_bad_arguments_before_any_launch():
    """gvl_layernorm_bwd_finalize_batched_wide: 65 items, a width of 1024, 2056 or 0, a block
    count of 513, a null workspace item, null lists: -1 with the message, no output written."""
    lib = _lib()
    C_, n = 1032, 65
    ws = _host(2 * C_, np.float32, 1.0)
    outs = _host(2 * n * C_, np.uint16, SENT16)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32

    def call(count, cols=C_, nblk=None, null_ws=None, ws_list=True, nb_list=True):
        wsl = (vp * n)(*[None if i == null_ws else ws.ctypes.data for i in range(n)])
        nbl = (i32 * n)(*[(nblk or {}).get(i, 512) for i in range(n)])
        dwl = (vp * n)(*[outs.ctypes.data + 2 * C_ * (2 * i) for i in range(n)])
        dbl = (vp * n)(*[outs.ctypes.data + 2 * C_ * (2 * i + 1) for i in range(n)])
        return lib.gvl_layernorm_bwd_finalize_batched_wide(wsl if ws_list else None,
                                                           nbl if nb_list else None, count, cols,
                                                           dwl, dbl, 1, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (outs == SENT16).all() and (ws == 1.0).all()

    bad = b"gvl_layernorm_bwd_finalize_batched_wide: bad arguments"
    refused(call(65), bad)
    refused(call(-1), bad)
    refused(call(2, cols=1024), bad)
    refused(call(2, cols=2056), bad)
    refused(call(2, cols=0), bad)
    assert b"cols <= 2048" in lib.gvl_last_error()
    refused(call(2, ws_list=False), bad)
    refused(call(2, nb_list=False), bad)
    refused(call(3, nblk={2: 513}), b"item 2: null workspace or bad block count")
    refused(call(64, null_ws=63), b"item 63: null workspace or bad block count")
    assert call(0) == 0  # nothing to do: no launch either
    assert (outs == SENT16).all()


def test_narrow_entry_points_keep_refusing_wide_rows():
    """The wide path is additive: gvl_layernorm_fwd still refuses 1032 columns."""
    lib = _lib()
    rc = lib.gvl_layernorm_fwd(None, 1032, None, None, None, 1032, None, None, 1, 1032, 1e-5, None)
    assert rc == -1 and b"cols=1032 unsupported" in lib.gvl_last_error()


def test_embedding_bwd_det_width_cap():
    """gvl_embedding_bwd_det takes rows of up to 2048 columns and refuses 2056 before any launch
    (n_tokens = 0 passes the checks and launches nothing)."""
    lib = _lib()
    assert lib.gvl_embedding_bwd_det(None, None, None, None, 0, 4, 2048, 16, 4, 0, None, 0, None) == 0
    rc = lib.gvl_embedding_bwd_det(None, None, None, None, 0, 4, 2056, 16, 4, 0, None, 0, None)
    assert rc == -1 and b"C <= 2048" in lib.gvl_last_error()


# ------------------------------------------------------------------------------ sizes
SIZES = {"gpt2": (12, 12, 768), "gpt2-medium": (24, 16, 1024), "gpt2-large": (36, 20, 1280),
         "gpt2-xl": (48, 25, 1600)}


@pytest.mark.parametrize("mod", ["gvl.gpt2", "gvl.cross_att"])
def test_named_sizes(mod):
    import dataclasses
    import importlib

    import gvl.gpt2 as g2
    M = importlib.import_module(mod)
    assert g2.GPT2_SIZES == SIZES
    for name, (L, H, C) in SIZES.items():
        cfg = M.GPTConfig.for_size(name)
        assert isinstance(cfg, M.GPTConfig)
        assert (cfg.n_layer, cfg.n_head, cfg.n_embd) == (L, H, C)
        assert cfg.n_embd // cfg.n_head == 64 and cfg.n_embd % cfg.n_head == 0
        assert (cfg.block_size, cfg.vocab_size) == (1024, 50257)
    cfg = M.GPTConfig.for_size("gpt2-xl", n_layer=1, vocab_size=512, block_size=64)
    assert (cfg.n_layer, cfg.n_head, cfg.n_embd, cfg.vocab_size, cfg.block_size) == (1, 25, 1600, 512, 64)
    # the dataclass fields are what they were
    want = ["block_size", "vocab_size", "n_layer", "n_head", "n_embd"] + (
        ["img_embd"] if mod == "gvl.cross_att" else [])
    assert [f.name for f in dataclasses.fields(M.GPTConfig)] == want
    with pytest.raises(ValueError, match="gpt2-xxl"):
        M.GPTConfig.for_size("gpt2-xxl")
    with pytest.raises(ValueError, match="2048"):
        M.GPTConfig.for_size("gpt2-xl", n_embd=2112, n_head=33)


def test_width_above_the_cap_fails_at_construction():
    import gvl.gpt2 as g2
    with pytest.raises(ValueError, match="2048"):
        g2.GPT(g2.GPTConfig(block_size=8, vocab_size=16, n_layer=1, n_head=33, n_embd=2112))


def test_wide_models_construct_with_the_reference_layout():
    """gpt2-xl's width with one layer: the state_dict keys and shapes are those of the 768-wide
    model with the width replaced."""
    import gvl.gpt2 as g2
    small = g2.GPT(g2.GPTConfig(block_size=8, vocab_size=16, n_layer=1, n_head=2, n_embd=128))
    wide = g2.GPT(g2.GPTConfig.for_size("gpt2-xl", block_size=8, vocab_size=16, n_layer=1))
    a, b = small.state_dict(), wide.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert tuple(b[k].shape) == tuple(1600 * (d // 128) if d % 128 == 0 else d
                                          for d in a[k].shape), k


# -------------------------------------------------------------------------- baselines
def test_wide_baselines_are_finite_and_inside_the_4x_rule():
    """The fp32 CPU evaluation of the references at the wide shapes, against float64, in units
    of 2**-24 * scale: finite, and the reference itself passes the bound it sets for the kernel
    (4 x the baseline, resp. 4 x max(baseline, 1)).  Measured: forward mean 0.90, rstd 2.6;
    backward dx about 2, dw about 4, db 0.7."""
    fwd, tall, bwd = WR.wide_ln_baseline(), WR.wide_ln_tall_baseline(), WR.wide_bwd_baseline()
    print("wide baselines:", fwd, tall, {k: bwd[k] for k in ("dx", "dw", "db")})
    for base in (fwd, tall):
        for k in ("mean", "rstd"):
            assert np.isfinite(base[k]) and 0 < base[k] < 16, (k, base)
    slack = WR.wide_bwd_slack()
    for k in ("dx", "dw", "db"):
        assert np.isfinite(bwd[k]) and 0 < bwd[k] < 16, (k, bwd[k])
        assert bwd[k] <= slack[k] / 4 or slack[k] == 4.0
        assert all(c[k] <= slack[k] for c in bwd["cases"].values())
    assert set(bwd["cases"]) == {f"{r}x{c}" for r, c in WR.WIDE_BWD_SHAPES}
    assert set(WR.WIDE_WIDTHS) >= {1032, 1280, 1600, 2040, 2048}
    assert all(1024 < c <= 2048 and c % 8 == 0 for c in WR.WIDE_WIDTHS)


# ----------------------------------------------------------------------------- routes
WIDE_TABLE = os.path.join(ROOT, "tests", "data", "gemm_routes_wide.json")


def test_wide_gemm_routes_match_table():
    """A routing change at the GPT-2 large / XL shapes shows as a changed cell."""
    import gemm_routes as R
    import gemm_routes_wide as RW
    want = json.load(open(WIDE_TABLE))
    got = RW.table(_lib())
    assert got["settings"] == want["settings"]
    assert len(got["rows"]) == len(want["rows"]) >= 100
    have = R.cells(got)
    bad = [(k, n, have.get(k)) for k, n in R.cells(want).items() if have.get(k) != n]
    assert not bad, f"{len(bad)} cells differ, first: {bad[:5]}"
    shapes = {(r["n"], r["k"]) for r in want["rows"]} | {(r["m"], r["n"]) for r in want["rows"]}
    for C in (1280, 1600):
        assert {(3 * C, C), (C, C), (4 * C, C), (C, 4 * C)} <= shapes
    assert {r["m"] for r in want["rows"]} >= {16384, 64, 8}

