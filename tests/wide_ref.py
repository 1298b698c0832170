"""The shapes of the wide row kernels (1024 < cols <= 2048: GPT-2 large / XL) and their own CPU
baselines, from the references of tests/rowwise_ref.py (fp32 torch against float64, in units of
2**-24 * scale).  Shared by test_wide_cpu.py, which holds the baselines to the 4 x rule, and
test_gpu_wide.py, which holds the HIP kernels to them.  rowwise_ref's baselines, and the bounds
that hang on them, stay as they are."""
from __future__ import annotations

import torch

from tests import rowwise_ref as R
from tests.helpers import err_units

# 1032: the first width past the narrow kernels.  1280 / 1600: GPT-2 large / XL.  1536 is the last
# width of the IT = 3 instances and 1544 the first of IT = 4, forward and backward alike (forward:
# lane l of the row's wave holds 8-column chunks l + 64 it; backward: two waves of 256 IT columns
# each, lane l holding 4-column chunks l + 64 it of its half).  2040 ends inside the last chunk,
# 2048 fills it.
WIDE_WIDTHS = (1032, 1280, 1536, 1544, 1600, 2040, 2048)
# backward: 2 rows per block (1 .. 5 leave a pair idle or give the pairs unequal trip counts), more
# than one block (9, 37), the finalize's 16 partial groups (129 rows = 17 blocks)
WIDE_BWD_ROWS = (1, 3, 4, 5, 9, 37, 129)
WIDE_BWD_SHAPES = tuple((r, c) for c in WIDE_WIDTHS for r in WIDE_BWD_ROWS)
# 4099 rows: the 512-block cap, five passes for three of the pairs' rows; 137 = 18 blocks
WIDE_COUNT_SHAPES = ((4099, 1032), (137, 2040))
# the persistent forward holds 1024 blocks x 4 rows: one row more than a full pass
WIDE_FWD_TALL = ((4097, 1032), (4097, 2048))
WIDE_FIN_WIDTHS = (1032, 2048)
WIDE_FIN_NBLK = (0, 1, 17, 512)
WIDE_FIN_COUNTS = (1, 65)
WIDE_EMB_WIDTHS = (1032, 1280, 1600, 2048)

_BASE = {}


def _fwd_units(xs):
    base = dict(mean=0.0, rstd=0.0)
    for x in xs:
        C = x.shape[1]
        ref = R.ln_ref64(x, torch.ones(C), torch.zeros(C))
        mean, rstd = R.ln_f32(x)
        base["mean"] = max(base["mean"], err_units(mean, ref["mean"], ref["scale_mean"]))
        base["rstd"] = max(base["rstd"], err_units(rstd, ref["rstd"], ref["scale_rstd"]))
    return base


def wide_ln_baseline():
    """rowwise_ref.ln_baseline's figure over WIDE_WIDTHS x LN_ROWS and the special rows."""
    if "fwd" not in _BASE:
        _BASE["fwd"] = _fwd_units([R.ln_inputs(rows, C)[0] for C in WIDE_WIDTHS for rows in R.LN_ROWS]
                                  + [R.ln_special_rows(C) for C in WIDE_WIDTHS])
    return dict(_BASE["fwd"])


def wide_ln_tall_baseline():
    """The same over WIDE_FWD_TALL (their own baseline, as rowwise_ref.ln_fwd_tall_baseline)."""
    if "tall" not in _BASE:
        _BASE["tall"] = _fwd_units([R.ln_inputs(rows, C)[0] for rows, C in WIDE_FWD_TALL])
    return dict(_BASE["tall"])


def wide_bwd_baseline():
    """Worst error of rowwise_ref.ln_bwd_f32 against float64 over WIDE_BWD_SHAPES, for dx, dw and
    db, plus the same per shape under "cases"."""
    if "bwd" not in _BASE:
        base, cases = dict(dx=0.0, dw=0.0, db=0.0), {}
        for rows, C in WIDE_BWD_SHAPES:
            x, w, _, dy, prev = R.ln_inputs(rows, C)
            mean, rstd = R.ln_f32(x)
            cases[f"{rows}x{C}"] = R.ln_bwd_units(x, w, dy, prev, mean, rstd)
            for k in base:
                base[k] = max(base[k], cases[f"{rows}x{C}"][k])
        _BASE["bwd"] = dict(base, cases=cases)
    return {k: (dict(v) if k == "cases" else v) for k, v in _BASE["bwd"].items()}


def wide_bwd_slack():
    """dict(dx, dw, db): 4 x max(baseline, 1) fp32 roundings."""
    base = wide_bwd_baseline()
    return {k: 4 * max(base[k], 1.0) for k in ("dx", "dw", "db")}
