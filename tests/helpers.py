"""Shared test helpers: recipe weights, fixture comparison, model builders."""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from oracle import models as OM
from oracle import weights as W

TINY = dict(block_size=64, vocab_size=512, n_layer=2, n_head=2, n_embd=128)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILE_LIMIT = 1 << 20  # no committed file is larger than 1 MiB


def _golden_parts(name, root):
    return sorted(glob.glob(os.path.join(root, glob.escape(name) + ".part[0-9][0-9].npz")))


def load_golden(name, root=GOLDEN):
    """The arrays of fixture `name`: one NAME.npz, or NAME.part00.npz, NAME.part01.npz, ...
    holding consecutive runs of its arrays when one file would exceed the size limit."""
    whole = os.path.join(root, name + ".npz")
    paths = [whole] if os.path.exists(whole) else _golden_parts(name, root)
    if not paths:
        raise FileNotFoundError(f"no fixture {name} (.npz or .partNN.npz) in {root}")
    out = {}
    for p in paths:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


def save_golden(name, arrays, compressed=True, root=GOLDEN, limit=GOLDEN_FILE_LIMIT):
    """Write fixture `name` for load_golden: one file when it stays under `limit` bytes, else
    the fewest equal-count runs of its arrays (in order) whose files all do."""
    save = np.savez_compressed if compressed else np.savez
    keys = list(arrays)
    for old in [os.path.join(root, name + ".npz")] + _golden_parts(name, root):
        if os.path.exists(old):
            os.remove(old)
    for n in range(1, len(keys) + 1):
        per = -(-len(keys) // n)
        paths = []
        for i in range(0, len(keys), per):
            part = name + (".npz" if n == 1 else f".part{i // per:02d}.npz")
            paths.append(os.path.join(root, part))
            save(paths[-1], **{k: arrays[k] for k in keys[i:i + per]})
        if all(os.path.getsize(p) <= limit for p in paths):
            return paths
        for p in paths:
            os.remove(p)
    raise ValueError(f"fixture {name}: one array alone exceeds {limit} bytes")


def recipe_params(keys_shapes, dtype=torch.float32, device="cpu"):
    """Parameter dict from the deterministic recipe, tied wte/lm_head as ONE tensor."""
    ks = [(k, tuple(s)) for k, s in keys_shapes if not k.endswith(".attn.bias")]
    vals = W.make_state(ks)
    P = {k: torch.from_numpy(v.copy()).to(dtype).to(device) for k, v in vals.items()}
    for k in list(P):
        if k.endswith("lm_head.weight"):
            kb = k[: -len("lm_head.weight")] + "transformer.wte.weight"
            if kb in P:
                P[kb] = P[k]
    if "gpt.transformer.wte.weight" in P:  # caption aliases
        P["wte.weight"] = P["gpt.transformer.wte.weight"]
        P["wpe.weight"] = P["gpt.transformer.wpe.weight"]
    return P


def margins_out(name, rec):
    """Write a parity test's measured errors as JSON under $GVL_MARGINS_DIR (default
    gpurun_out/parity_margins; the GPU session copies them into profiles/)."""
    import json
    d = os.environ.get("GVL_MARGINS_DIR", os.path.join("gpurun_out", "parity_margins"))
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"{name}.json"), "w") as f:
            json.dump(rec, f, indent=1, default=float)
    except OSError:
        pass


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / den)


def f64(t):
    """A tensor or array as a float64 numpy array (exact for bf16 / fp32 values)."""
    if isinstance(t, torch.Tensor):
        return t.detach().to(torch.float64).cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def rel_err_rows(a, b):
    """rel_err per row: every row of the [..., cols] arrays is divided by its own max |b|; the
    worst row is returned, so a row of small scale is not hidden behind a large one."""
    a, b = f64(a), f64(b)
    a = a.reshape(-1, a.shape[-1])
    b = b.reshape(-1, b.shape[-1])
    den = np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float((np.abs(a - b).max(axis=1) / den).max())


def ulp_bf16(ref):
    """The bf16 unit in the last place at |ref| (8 significand bits): 2**(floor(log2|ref|) - 7),
    in float64, |ref| clamped below at 2**-126 (the smallest normal)."""
    a = np.maximum(np.abs(f64(ref)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(a)) - 7)


F32_UNIT = 2.0 ** -24  # half an fp32 ulp, relative: the most one fp32 rounding adds


def err_units(got, ref64, scale):
    """max |got - ref64| in units of 2**-24 * scale (the measured `slack` of assert_f32_close)."""
    err = np.abs(f64(got) - f64(ref64))
    unit = F32_UNIT * np.abs(f64(scale))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def _close(got, ref64, tol, ulp, name):
    got, ref = f64(got), f64(ref64)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs {ref.shape}"
    if got.size == 0:
        return 0.0
    fin = np.isfinite(ref)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))  # a non-finite reference: identical
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
        ok = np.where(fin, err <= tol, same)
        excess = np.where(ok, 0.0, np.where(fin & np.isfinite(err), (err - tol) / ulp, np.inf))
    if not ok.all():
        i = tuple(int(k) for k in np.unravel_index(int(np.argmax(excess)), excess.shape))
        raise AssertionError(
            f"{name}: {int((~ok).sum())} of {ok.size} elements out of tolerance; worst at {i}: "
            f"got {float(got[i])!r} want {float(ref[i])!r}, |diff| {err[i]:.6g} exceeds the bound "
            f"{np.broadcast_to(tol, ref.shape)[i]:.6g} by {excess[i]:.3g} ulp")
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(fin, err / ulp, 0.0).max())


def assert_bf16_close(got, ref64, *, scale=None, slack=0, name=""):
    """Every element of the bf16 result `got` within ulp_bf16(ref64) + slack * 2**-24 * scale of
    the float64 reference.  One ulp is derived, not tuned: half an ulp is the final
    round-to-nearest-even, the other half lets fp32 arithmetic in front of it flip a near-tie.
    `scale` (an array: the sum of the absolute values of the terms that were added to form the
    result) and `slack` (a count of fp32 roundings) matter only where the operation cancels.
    Returns the worst error in ulps; on failure reports the worst element."""
    ulp = ulp_bf16(ref64)
    tol = ulp if scale is None else ulp + slack * F32_UNIT * np.abs(f64(scale))
    return _close(got, ref64, tol, ulp, name or "bf16")


def assert_bf16_rounded(got, ref64, scale, slack, name=""):
    """Every element of the bf16 result `got` within ulp_bf16(ref64) / 2 + slack * 2**-24 * scale
    of the float64 reference: the correct rounding (to nearest) of a value that fp32 arithmetic
    may have moved by `slack` units of 2**-24 * scale before it was rounded.  Unlike
    assert_bf16_close there is no second half ulp for a flipped near-tie: `slack`, taken from an
    fp32 evaluation of the reference itself, is what may flip it, so truncation (up to one ulp)
    fails.  The ulp is that of the reference's binade, so just below a power of two, where the
    value may round up into the next binade, the bound is the tighter of the two.  Returns the
    worst error in ulps; on failure reports the worst element."""
    ulp = ulp_bf16(ref64)
    tol = 0.5 * ulp + slack * F32_UNIT * np.abs(f64(scale))
    return _close(got, ref64, tol, ulp, name or "bf16 rounded")


def assert_f32_close(got, ref64, scale, slack, name=""):
    """Every element of the fp32 result `got` within slack * 2**-24 * scale of the float64
    reference (no ulp term).  Returns the measured error in those units."""
    s = np.abs(f64(scale))
    _close(got, ref64, slack * F32_UNIT * s, np.maximum(F32_UNIT * s, 2.0 ** -149), name or "f32")
    return err_units(got, ref64, scale)


BF16_UNIT = 2.0 ** -8  # the largest relative error of one bf16 rounding
# Below the smallest normal (2**-126, bf16 and fp32 alike) a rounding is no longer relative and
# the GPU may flush a term to zero: an absolute 2**-126 per term, for the at most 2**10 terms of
# at most 2**4 that the attention tests sum.  Nothing above 1e-33 is affected.
ATTN_FLUSH = 2.0 ** -112


def attn_units(got, ref64, E):
    """max |got - ref64| in units of 2**-8 * E (E: the per-element sum of the absolute values of
    the terms added to form the result, tests/attn_ref.py)."""
    err = np.abs(f64(got) - f64(ref64))
    unit = BF16_UNIT * np.abs(f64(E))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r) | (err <= ATTN_FLUSH), np.where(np.isnan(err), np.inf, 0.0), r)
    return float(r.max()) if r.size else 0.0


def assert_attn_close(got_bf16, ref64, E, units, name="", slack=0):
    """Every element of the bf16 attention output within units * 2**-8 * E (+ slack * 2**-24 * E
    for the fp32 arithmetic) of the float64 reference: `units` counts the bf16 roundings on the
    way to the element, each at most 2**-8 of the terms it rounds.  A NaN or an infinity fails.
    Returns the worst error in units of 2**-8 * E; on failure reports the worst element."""
    e = np.abs(f64(E))
    unit = np.maximum(BF16_UNIT * e, 2.0 ** -149)
    _close(got_bf16, ref64, (units * BF16_UNIT + slack * F32_UNIT) * e + ATTN_FLUSH, unit,
           name or "attn")
    return attn_units(got_bf16, ref64, E)


def assert_attn_tight(got_bf16, ref64, E, emu64, name="", slack=0, margin=4):
    """The bound the reference sets for itself: every element within margin x the worst error of
    the bf16-rounding emulation `emu64` (in units of 2**-8 * E, over the whole tensor) of the
    float64 reference, + slack * 2**-24 * E.  margin = 4 is what the row-wise tests give an fp32
    evaluation in another order; here it covers another accumulation order and rounding points
    that fall differently.  Returns (the result's worst error, the emulation's) in those units."""
    r_emu = attn_units(emu64, ref64, E)
    assert np.isfinite(r_emu), f"{name}: the emulation itself is off where E = 0"
    e = np.abs(f64(E))
    unit = np.maximum(BF16_UNIT * e, 2.0 ** -149)
    _close(got_bf16, ref64, (margin * r_emu * BF16_UNIT + slack * F32_UNIT) * e + ATTN_FLUSH, unit,
           name or "attn tight")
    return attn_units(got_bf16, ref64, E), r_emu


def check_summary(fx, name, t, rtol):
    """Compare tensor t against the fixture summary of `name` (full or sampled + sums)."""
    a = t.detach().to(torch.float64).cpu().numpy().reshape(-1)
    if name + "#full" in fx:
        e = rel_err(a, fx[name + "#full"])
        assert e < rtol, f"{name}: rel err {e:.3g} >= {rtol}"
    else:
        idx = fx[name + "#idx"]
        e = rel_err(a[idx], fx[name + "#val"])
        assert e < rtol, f"{name}: sampled rel err {e:.3g} >= {rtol}"
    sq = float(fx[name + "#sq"])
    e2 = abs((a * a).sum() - sq) / max(sq, 1e-30)
    assert e2 < 2 * rtol, f"{name}: sum-of-squares rel err {e2:.3g}"


def fixture_name(kind, key):
    """Oracle canonical key for the tied embedding is lm_head.weight."""
    if kind == "gpt" and key == "transformer.wte.weight":
        return "lm_head.weight"
    return key


def named_trainable(kind, meta):
    keys = [k for k, _ in meta[f"{kind}_keys"]]
    if kind == "cross":
        return list(meta["cross_trainable"])
    if kind == "gpt":
        return [k for k in keys if not k.endswith(".attn.bias") and k != "lm_head.weight"]
    return [k for k in keys if k.startswith("bridge.")]


def lr_caption(it, max_lr=1e-3, min_lr=1e-4, warm=5, max_steps=80):
    return OM.O.get_lr(it, max_lr, min_lr, warm, max_steps)


def lr_lm(it):
    return OM.O.get_lr(it, 6e-4, 6e-5, 715, 19073)


def lr_cross(it):
    return OM.O.get_lr(it, 1e-3, 1e-5, 20, 925)
