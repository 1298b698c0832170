"""tests/fn_ref.py checked on the CPU: its restated forwards are stock torch's operations, the
emulation and a differently rounded evaluation pass the per-line bounds, and doctored results
that the model-level criteria accept are rejected by them."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fn_ref as R
from tests import gemm_ref
from tests.helpers import assert_f32_close, f64

F64 = torch.float64
DROP_CASES = [n for n, (_, cfg) in R.CASES.items()
              if cfg.get("drop") or cfg.get("p_attn") or cfg.get("p_out") or n == "qformer"]


def _leaves(name):
    t, c, dout = R.inputs(name)
    return {k: v.to(F64) for k, v in t.items()}, c, dout.to(F64)


def _close(a, b, tol=1e-12):
    a, b = f64(a), f64(b)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# --------------------------------------------------------------- stock torch agreement
def test_layer_norm_is_nn_layernorm():
    t, _, _ = _leaves("layernorm")
    ln = torch.nn.LayerNorm(R.C, eps=1e-5).to(F64)
    with torch.no_grad():
        ln.weight.copy_(t["w"])
        ln.bias.copy_(t["b"])
    _close(R.layer_norm(t["x"], t["w"], t["b"]), ln(t["x"]))


@pytest.mark.parametrize("causal", [False, True])
def test_attention_is_sdpa(causal):
    t, _, _ = _leaves("self_attn")
    qkv = t["qkv"]
    q, k, v = qkv[..., :R.C], qkv[..., R.C:2 * R.C], qkv[..., 2 * R.C:]
    want = F.scaled_dot_product_attention(R.heads(q, R.H), R.heads(k, R.H), R.heads(v, R.H),
                                          is_causal=causal)
    _close(R.attention(R.REF, q, k, v, R.H, causal), want.transpose(1, 2).reshape(q.shape))


@pytest.mark.parametrize("name", ["mha_self", "mha_cross"])
def test_mha_is_nn_multihead_attention(name):
    """Self-attention and cross-attention with the packed in_proj split, + the residual."""
    t, c, _ = _leaves(name)
    mha = torch.nn.MultiheadAttention(R.C, R.H, batch_first=True).to(F64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(t["in_w"])
        mha.in_proj_bias.copy_(t["in_b"])
        mha.out_proj.weight.copy_(t["out_w"])
        mha.out_proj.bias.copy_(t["out_b"])
    kv = t["q_in"] if c["self_attn"] else t["kv_in"]
    want = t["res"] + mha(t["q_in"], kv, kv, need_weights=False)[0]
    _close(R.u_mha(R.REF, t, c)["out"], want)


@pytest.mark.parametrize("act", [1, 2])
def test_gelu_is_nn_gelu(act):
    x = torch.linspace(-6, 6, 1001, dtype=F64)
    stock = torch.nn.GELU(approximate="tanh" if act == 1 else "none")(x)
    _close(R.gelu(R.REF, x, act), stock)
    own = gemm_ref.gelu_tanh64 if act == 1 else gemm_ref.gelu_erf64
    _close(stock, own(x.numpy()), 1e-14)
    # the emulation's value is the same; only its derivative is the rounded one
    xe = x.clone().requires_grad_()
    ye = R.gelu(R.EMU, xe, act)
    _close(ye, stock)
    (g,) = torch.autograd.grad(ye.sum(), xe)
    d = (gemm_ref.dgelu_tanh64 if act == 1 else gemm_ref.dgelu_erf64)(x.numpy())
    assert np.abs(f64(g) - d).max() <= 2.0 ** -8 * 1.13


def test_cross_entropy_is_f_cross_entropy():
    t, c, _ = _leaves("lmhead_520")
    logits = R.linear(t["x"], t["w"])
    tgt = c["tgt"].reshape(-1)
    assert (tgt == -100).sum() >= 3
    want = F.cross_entropy(logits.view(-1, c["V"]), tgt, ignore_index=-100)
    _close(R.ce_loss(R.REF, logits.view(-1, c["V"]), tgt, None, False), want)
    # the rounding-free _CESum (the emulation's node) has the same value and gradient
    x = logits.view(-1, c["V"]).clone().requires_grad_()
    valid = tgt != -100
    s = R._CESum.apply(x, tgt, valid)
    _close(s / valid.sum(), want)


@pytest.mark.parametrize("mask_mode", [False, True])
def test_cross_entropy_mask_semantics(mask_mode):
    """K.cross_entropy: a row counts when target != -100 and mask set; the divisor is the number
    of such rows, or with mask_mode sum(mask) (gpt2_cross-att's masked mean)."""
    t, c, _ = _leaves("lmhead_mask")
    V, off, Tt = c["V"], c["off"], c["tgt"].shape[1]
    rows = R.linear(t["x"], t["w"])[:, off:off + Tt].reshape(-1, V)
    tgt, mk = c["tgt"].reshape(-1), c["mask"].reshape(-1)
    assert (mk & (tgt == -100)).any() and (~mk & (tgt != -100)).any()
    per = F.cross_entropy(rows, tgt.clamp(min=0), reduction="none")
    use = mk & (tgt != -100)
    want = per[use].sum() / (mk.sum() if mask_mode else use.sum())
    _close(R.ce_loss(R.REF, rows, tgt, c["mask"], mask_mode), want)


@pytest.mark.parametrize("name", ["embed", "embed_prefix"])
def test_embed_is_nn_embedding_cat(name):
    t, c, _ = _leaves(name)
    idx = c["idx"]
    assert idx.min() == 0 and idx.max() == c["V"] - 1 and idx.unique().numel() < idx.numel()
    wte = torch.nn.Embedding.from_pretrained(t["wte"])
    wpe = torch.nn.Embedding.from_pretrained(t["wpe"])
    x = wte(idx) + wpe(torch.arange(idx.shape[1]))
    if "prefix" in t:
        x = torch.cat([t["prefix"], x], dim=1)
    _close(R.u_embed(R.REF, t, c)["out"], x)


def test_query_expand_is_expand():
    t, c, _ = _leaves("query_expand")
    _close(R.u_query_expand(R.REF, t, c)["out"], t["q"].unsqueeze(0).expand(R.B, -1, -1))


def test_case_list_covers_the_wiring_edges():
    assert (R.C, R.H, R.B, R.T, R.S_CLIP, R.Q, R.L) == (128, 2, 3, 33, 33, 32, 2)
    assert -(-R.B * R.T // 8) == 13 and R.B * R.T % 8 == 3  # LayerNorm backward blocks
    vs = {cfg["V"] for _, cfg in R.CASES.values() if "V" in cfg}
    assert vs == {520, 517}
    lm = [cfg for u, cfg in R.CASES.values() if u == "lmhead"]
    assert any(c["off"] == 32 and c["S"] == 47 and c["Tt"] == 15 for c in lm)
    assert any(c["off"] == 0 and c["S"] == c["Tt"] for c in lm)
    assert {c.get("mask_mode") for c in lm if c.get("mask")} == {False, True}
    gates = {cfg["gate"] for _, cfg in R.CASES.values() if "gate" in cfg}
    assert gates == {0.3, -4.0}
    assert {cfg["act"] for u, cfg in R.CASES.values() if u == "mlp"} == {1, 2}
    assert R.SEED_OFFSETS[0] == 0 and R.SEED_OFFSETS[1] != 0


# ----------------------------------------------- the emulation passes its own bounds
def _self_check(name, offset):
    ref, emu = R.evaluate(name, "ref", offset), R.evaluate(name, "emu", offset)
    alt = R.evaluate(name, "alt", offset)
    worst = 0.0
    for k in ref:
        if ref[k].ndim == 0 and k == "out":  # the fp32 loss: one step from the stored logits
            for got in (emu, alt):
                want, scale, slack = R.loss_of_logits(name, got["logits"])
                assert_f32_close(np.float32(got[k]), want, scale, slack, name=f"{name} loss")
            continue
        for which, got in (("emu", emu[k]), ("alt", alt[k])):
            n, ratio, units, _ = R.violations(k, got, ref[k], emu[k])
            assert n == 0, f"{name} {which} {k}: {n} elements out of bound, ratio {ratio:.3g}"
            worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", list(R.CASES))
def test_emulation_and_rerounded_variant_within_bounds(name):
    """EMU within its own bound trivially uses <= 1 / MARGIN of it; ALT (fp32 arithmetic, P and dS
    rounded inside attention) must fit too, and must use a visible part of the bound: MARGIN = 4
    is neither vacuous nor too tight."""
    worst = _self_check(name, 0)
    assert worst <= 1.0
    print(f"{name}: worst ratio of emu / alt to the bound {worst:.3f}")
    assert worst >= 0.1, "the bound is vacuous against a re-rounded evaluation"


@pytest.mark.parametrize("name", DROP_CASES)
def test_dropout_cases_at_the_second_seed_offset(name):
    off = R.SEED_OFFSETS[1]
    assert _self_check(name, off) <= 1.0
    # the masks at the two offsets differ: a wrong offset is a wrong mask
    a, b = R.evaluate(name, "ref", 0), R.evaluate(name, "ref", off)
    n, *_ = R.violations("out", b["out"], a["out"], R.evaluate(name, "emu", 0)["out"])
    assert n > 0


# -------------------------------------------------------------------- doctored results
def _doc_gate(name="linear_res_gate"):
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    g = float(R.inputs(name)[0]["gate"].double())
    got = dict(emu)
    got["d_gate"] = emu["d_gate"] / (1.0 - math.tanh(g) ** 2)
    return name, ref, emu, got, ["d_gate"]


def _doc_bias(which):
    """mlp: b2 shares dY with w2 (and b1 with w1): a bias fused into two weight gradients of one
    dY doubles, one fused into none stays at zero."""
    name = "mlp_tanh"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    got = dict(emu)
    got["d_b2"] = emu["d_b2"] * (2.0 if which == "doubled" else 0.0)
    return name, ref, emu, got, ["d_b2"]


def _doc_dx_last_row():
    name = "gpt_block"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    dout = f64(R.inputs(name)[2])
    got = dict(emu)
    dx = emu["d_x"].copy()
    dx[-1, -1] -= dout[-1, -1]  # the residual path of the last row
    got["d_x"] = dx
    return name, ref, emu, got, ["d_x"]


def _doc_ln_last_block():
    name = "layernorm"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    t, _, dout = R.inputs(name)
    x, dy = f64(t["x"]).reshape(-1, R.C)[-3:], f64(dout).reshape(-1, R.C)[-3:]
    d = x - x.mean(1, keepdims=True)
    xh = d / np.sqrt((d * d).mean(1, keepdims=True) + 1e-5)
    got = dict(emu)
    got["d_w"] = emu["d_w"] - (dy * xh).sum(0)
    got["d_b"] = emu["d_b"] - dy.sum(0)
    return name, ref, emu, got, ["d_w", "d_b"]


def _doc_dprefix_shift():
    name = "embed_prefix"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    got = dict(emu)
    got["d_prefix"] = np.roll(emu["d_prefix"].reshape(-1, R.C), 1, axis=0).reshape(emu["d_prefix"].shape)
    return name, ref, emu, got, ["d_prefix"]


def _doc_lm_dx_off():
    name = "lmhead_517_prefix"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    got = dict(emu)
    got["d_x"] = np.roll(emu["d_x"], -1, axis=1)  # the text rows written at off - 1
    return name, ref, emu, got, ["d_x"]


def _doc_tied_half():
    name = "tied"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    half = R.evaluate_with(name, R.EMU, settings=dict(detach_embed=True))
    got = dict(emu)
    got["d_wte"] = half["d_wte"]
    present = np.unique(R.inputs(name)[1]["idx"].numpy())
    absent = np.setdiff1d(np.arange(ref["d_wte"].shape[0]), present)
    assert np.array_equal(half["d_wte"][absent], emu["d_wte"][absent])  # only ids that occur
    return name, ref, emu, got, ["d_wte"]


def _doc_kv_swap():
    """Batch row 1 of the slab with the two layers' column blocks swapped: what CrossKVFn's
    backward then computes for dz and the kv_proj gradients."""
    name = "cross_kv"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    pr = R.evaluate_with(name, R.REF, probe=True)
    t = R.inputs(name)[0]
    z = f64(t["z"])
    d = [pr["p_kvp0"], pr["p_kvp1"]]
    w = [f64(t["kv_w0"]), f64(t["kv_w1"])]
    got = dict(emu)
    b = 1
    for l in range(2):
        delta = d[1 - l][b] - d[l][b]  # what layer l's columns of row b hold instead
        got[f"d_kv_w{l}"] = emu[f"d_kv_w{l}"] + delta.T @ z[b]
        got[f"d_kv_b{l}"] = emu[f"d_kv_b{l}"] + delta.sum(0)
    dz = emu["d_z"].copy()
    dz[b] = d[1][b] @ w[0] + d[0][b] @ w[1]
    got["d_z"] = dz
    return name, ref, emu, got, ["d_z", "d_kv_w0", "d_kv_w1", "d_kv_b0", "d_kv_b1"]


def _doc_pout_mask():
    name = "mha_self_drop"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    wrong = R.keep_rows(R.SEED ^ R.ATTN_XOR, 0, R.B * R.T, R.C, R.DROP_P)
    got = R.evaluate_with(name, R.EMU, settings=dict(kd_out_bwd=wrong))
    np.testing.assert_array_equal(got["out"], emu["out"])  # the forward is untouched
    return name, ref, emu, got, ["d_q_in", "d_in_w", "d_in_b", "d_out_w", "d_out_b"]


def _doc_inproj_operand():
    """in_proj rows [C, 3C) = dkvp^T kv_in; doctored: the q slice's operand q_in in its place
    (for the 32 key rows per sequence that q_in has)."""
    name = "mha_cross"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    pr = R.evaluate_with(name, R.REF, probe=True)
    t = R.inputs(name)[0]
    qi, kvi, d = f64(t["q_in"]), f64(t["kv_in"]), pr["p_kvp"]
    Tq = qi.shape[1]
    rows = sum(d[b, :Tq].T @ qi[b] + d[b, Tq:].T @ kvi[b, Tq:] for b in range(R.B))
    got = dict(emu)
    w = emu["d_in_w"].copy()
    w[R.C:] = rows
    got["d_in_w"] = w
    return name, ref, emu, got, ["d_in_w"]


# name -> (builder, the old criteria also reject it)
DOCTORED = {
    "gate_without_sech2": (_doc_gate, False),
    "bias_doubled_shared_dy": (lambda: _doc_bias("doubled"), True),
    "bias_zero_shared_dy": (lambda: _doc_bias("zero"), True),
    "dx_last_row_without_residual": (_doc_dx_last_row, True),
    "ln_dw_db_without_last_block": (_doc_ln_last_block, True),
    "dprefix_shifted_one_row": (_doc_dprefix_shift, True),
    "lmhead_dx_at_off_minus_1": (_doc_lm_dx_off, True),
    "tied_wte_lm_head_part_only": (_doc_tied_half, True),
    "kv_slab_layers_swapped_in_one_batch_row": (_doc_kv_swap, True),
    "p_out_mask_from_attention_seed": (_doc_pout_mask, True),
    "in_proj_kv_rows_from_q_operand": (_doc_inproj_operand, True),
}


@pytest.mark.parametrize("what", list(DOCTORED))
def test_doctored_result_is_rejected(what):
    build, old_rejects = DOCTORED[what]
    name, ref, emu, got, keys = build()
    rejected = []
    for k in keys:
        n, ratio, units, _ = R.violations(k, got[k], ref[k], emu[k])
        old_t = R.old_tensor_ok(got[k], ref[k])
        print(f"{what}: {name} {k}: new bound {'REJECTS' if n else 'accepts'} ({n} elements, "
              f"ratio {ratio:.3g}); old per-tensor 1.2e-1 of max: {'accepts' if old_t else 'REJECTS'}")
        if n:
            rejected.append(k)
    gk = [k for k in ref if k.startswith("d_")]
    old_a = R.old_arena_ok([got[k] for k in gk], [ref[k] for k in gk])
    old_t_all = all(R.old_tensor_ok(got[k], ref[k]) for k in gk)
    print(f"{what}: old one-number max-norm over all gradients (1e-2): "
          f"{'accepts' if old_a else 'REJECTS'}; old per-tensor over all: "
          f"{'accepts' if old_t_all else 'REJECTS'}")
    assert rejected == keys, f"{what}: the new bound accepts {set(keys) - set(rejected)}"
    # every untouched tensor still passes
    for k in ref:
        if k not in keys and ref[k].ndim:
            assert R.violations(k, got[k], ref[k], emu[k])[0] == 0
    # the old criteria: the plain path was held per tensor, the sink path by the one number; a
    # doctored result "passes today" when either accepts it
    assert (not (old_t_all or old_a)) == old_rejects, \
        f"{what}: old criteria verdict changed (per-tensor {old_t_all}, one-number {old_a})"
