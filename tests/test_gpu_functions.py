"""Per-tensor parity of every fused autograd Function (gvl/functional.py, _SelfAttnFn,
_CrossSDPAFn) on the MI355X against float64 autograd of the same forward (tests/fn_ref.py): each
Function is called alone, at the shared small cases, and every output and every gradient is held
per element to  ulp_bf16(ref) + 4 * U_t * s_i  (s_i the rms of the reference line, U_t the worst
error of the bf16-rounding emulation in those units; fn_ref's docstring) on every path a gradient
can take: returned to autograd, accumulated into a gvl.optim.AdamW arena gradient (immediately or
through the deferred flush, on each of its routes), with frozen inputs, over a retained graph and
with two graphs interleaved.  tests/test_fn_ref_cpu.py shows what these bounds reject.  The
measured ratios go to profiles/fn_margins.json through helpers.margins_out."""
import collections

import numpy as np
import pytest
import torch

from tests import fn_ref as R
from tests.helpers import assert_f32_close, margins_out
from tests.misc_ref import bits

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
INPUT_NAMES = {"x", "z", "res", "q_in", "kv_in", "prefix", "qkv", "kv", "v"}
MAIN = [n for n in R.CASES if n not in ("gpt_stack", "kv_only", "kv_only_99", "lin_lmhead", "mlp_k64")]
DROP_CASES = [n for n, (_, cfg) in R.CASES.items()
              if cfg.get("drop") or cfg.get("p_attn") or cfg.get("p_out") or n == "qformer"]
ROUTES = {}


def _fn():
    from gvl import functional as Fn
    return Fn


def _k():
    from gvl import kernels as K
    return K


def _is_param(unit, k):
    if k == "q":
        return unit == "query_expand"
    return k not in INPUT_NAMES


def _sinks(name, k):
    """Does the Function accumulate parameter k's gradient in place (and fire the ready hook)?
    LinearFn hands its gate gradient to autograd; with a vocabulary that is no multiple of 8 the
    lm_head's weight is pad_vocab's copy, whose gradient autograd slices and adds."""
    unit, cfg = R.CASES[name]
    if unit == "linear":
        return k != "gate" and cfg.get("bias", True)
    if unit == "lmhead":
        return cfg["V"] % 8 == 0
    return True


# ------------------------------------------------------------------------------ calling
def _call(name, t, c, dev):
    """The Function(s) of case `name` over the device leaves t -> dict(out[, logits])."""
    Fn = _fn()
    unit, cfg = R.CASES[name]
    p = R.DROP_P
    if unit == "linear":
        if not cfg.get("bias", True):
            return dict(out=Fn.lm_logits(t["x"], t["w"]))
        return dict(out=Fn.LinearFn.apply(t["x"], t["w"], t["b"], t.get("res"), t.get("gate"),
                                          p if cfg.get("drop") else 0.0, R.SEED))
    if unit == "layernorm":
        return dict(out=Fn.LayerNormFn.apply(t["x"], t["w"], t["b"], 1e-5))
    if unit == "mlp":
        return dict(out=Fn.MLPFn.apply(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], t.get("res"),
                                       cfg["act"], p if cfg.get("drop") else 0.0, R.SEED))
    if unit == "mha":
        kv = t["q_in"] if cfg["self_attn"] else t["kv_in"]
        return dict(out=Fn.MHAFn.apply(t["q_in"], kv, t["in_w"], t["in_b"], t["out_w"], t["out_b"],
                                       t["res"], R.H, cfg["self_attn"], cfg["p_attn"], cfg["p_out"],
                                       R.SEED))
    blk = ("ln1_w", "ln1_b", "attn_w", "attn_b", "aproj_w", "aproj_b", "ln2_w", "ln2_b", "fc_w",
           "fc_b", "mproj_w", "mproj_b")
    if unit == "gpt_block":
        return dict(out=Fn.GPTBlockFn.apply(t["x"], *[t[k] for k in blk], R.H, True))
    if unit == "gpt_stack":
        x = t["x"]
        for l in range(R.L):
            x = Fn.GPTBlockFn.apply(x, *[t[k + str(l)] for k in blk], R.H, True)
        return dict(out=x)
    xa = ("ln_w", "ln_b", "q_w", "q_b")
    if unit == "cross_attn":
        return dict(out=Fn.CrossAttnFn.apply(t["x"], t["z"], *[t[k] for k in xa], t["kv_w"],
                                             t["kv_b"], t["c_w"], t["c_b"], t["gate"], R.H))
    if unit in ("cross_kv", "kv_only"):
        slab = Fn.KVGradSlab(R.L)
        wb = [t[f"kv_{a}{l}"] for l in range(R.L) for a in "wb"]
        kv = Fn.CrossKVFn.apply(t["z"], slab, *wb)
        if unit == "kv_only":
            return dict(out=kv)
        x = t["x"]
        for l in range(R.L):
            s = str(l)
            x = Fn.CrossAttnKVFn.apply(x, kv, l, slab, *[t[k + s] for k in xa], t["c_w" + s],
                                       t["c_b" + s], t["gate" + s], R.H)
        return dict(out=x, slab=slab)
    if unit in ("embed", "tied"):
        x = Fn.EmbedFn.apply(c["idx"].to(dev), t["wte"], t["wpe"], t.get("prefix"))
        if unit == "embed":
            return dict(out=x)
        xn = Fn.LayerNormFn.apply(x, t["ln_w"], t["ln_b"], 1e-5)
        logits, loss = Fn.lm_head_loss(xn, t["wte"], c["tgt"].to(dev), cfg["off"])
        return dict(out=loss, logits=logits)
    if unit == "lmhead":
        mask = c["mask"].to(dev) if "mask" in c else None
        logits, loss = Fn.lm_head_loss(t["x"], t["w"], c["tgt"].to(dev), cfg["off"], mask,
                                       cfg.get("mask_mode", False))
        return dict(out=loss, logits=logits)
    if unit == "lin_lmhead":
        h = Fn.LinearFn.apply(t["x"], t["pw"], t["pb"])
        logits, loss = Fn.lm_head_loss(h, t["w"], c["tgt"].to(dev), 0)
        return dict(out=loss, logits=logits)
    if unit == "query_expand":
        return dict(out=Fn.QueryExpandFn.apply(t["q"], R.B))
    if unit == "self_attn":
        from gvl.gpt2 import _SelfAttnFn
        return dict(out=_SelfAttnFn.apply(t["qkv"], R.H))
    if unit == "cross_sdpa":
        from gvl.cross_att import _CrossSDPAFn
        return dict(out=_CrossSDPAFn.apply(t["q"], t["kv"], R.H))
    if unit == "qformer":  # gvl.caption.QFormerLayer.forward in train mode, seeds given
        s0, s1, s2 = c["seeds"]
        ln = lambda n, x, tape=None: Fn.LayerNormFn.apply(x, t[n + "_w"], t[n + "_b"], 1e-5, tape)
        mha = lambda a, qi, kvi, res, sa, seed: Fn.MHAFn.apply(
            qi, kvi, t[a + "_in_w"], t[a + "_in_b"], t[a + "_out_w"], t[a + "_out_b"], res, R.H, sa,
            p, p, seed)
        q = t["q"]
        tp = Fn.ResTape()
        q2 = ln("ln1", q, tp)
        q = Fn.ResTapFn.apply(mha("sa", q2, q2, q.detach(), True, s0), tp)
        tp = Fn.ResTape()
        q = Fn.ResTapFn.apply(mha("ca", ln("ln2q", q, tp), ln("ln2v", t["v"]), q.detach(), False, s1), tp)
        tp = Fn.ResTape()
        q2 = ln("ln3", q, tp)
        return dict(out=Fn.ResTapFn.apply(
            Fn.MLPFn.apply(q2, t["w1"], t["b1"], t["w2"], t["b2"], q.detach(), 2, p, s2), tp))
    raise KeyError(unit)


class _Offset:
    """K.seed_offset(device) set for the duration, restored to 0 afterwards."""

    def __init__(self, dev, value):
        self.t, self.value = _k().seed_offset(dev), value

    def __enter__(self):
        self.t.fill_(self.value)

    def __exit__(self, *exc):
        self.t.zero_()


def _leaves(name, dev, offset, frozen=()):
    t, c, dout = R.inputs(name, offset)
    leaves = {k: v.to(dev, copy=True).requires_grad_(k not in frozen) for k, v in t.items()}
    return leaves, c, dout.to(dev)


def _g0(name, k, ref):
    """A non-zero bf16 gradient already in the sink: half the reference's rms, seeded."""
    g = torch.Generator().manual_seed(500 + sum(map(ord, name + k)))
    rms = float(np.sqrt((ref * ref).mean())) or 1.0
    return (0.5 * rms * torch.randn(ref.shape, generator=g, dtype=torch.float64)).to(BF)


def _pending_empty():
    Fn = _fn()
    return not (Fn._PENDING or Fn._PENDING_B or Fn._PENDING_LN or Fn._QUEUED)


def _run(name, dev, offset=0, sink=False, frozen=(), before_backward=None):
    """One forward + backward of case `name` -> dict(out, logits, loss, grads: k -> bf16 CPU tensor
    or None, g0, hooks: k -> count, ptr_same: k -> bool)."""
    Fn = _fn()
    unit, _ = R.CASES[name]
    leaves, c, dout = _leaves(name, dev, offset, frozen)
    ref = R.evaluate(name, "ref", offset)
    res = dict(g0={}, hooks={}, ptr_same={})
    params = [k for k in leaves if _is_param(unit, k) and k not in frozen]
    counts = collections.Counter()
    handle = None
    ptrs = {}
    if sink:
        from gvl.optim import AdamW
        for k in params:
            if k.startswith("kv_w") or k.startswith("kv_b"):  # gvl.cross_att: one stacked matrix
                leaves[k]._gvl_stack_key = "xattn.kv_proj." + ("weight" if k[3] == "w" else "bias")
        opt = AdamW([leaves[k] for k in params], lr=0.0)
        opt.grad_arena
        for k in params:
            res["g0"][k] = _g0(name, k, ref["d_" + k])
            leaves[k].grad.copy_(res["g0"][k].to(dev))
            ptrs[k] = leaves[k].grad.data_ptr()
        handle = Fn.register_grad_ready_hook(lambda p: counts.update([id(p)]))
    try:
        with _Offset(dev, offset):
            outs = _call(name, leaves, c, dev)
            out = outs["out"]
            if before_backward is not None:
                before_backward(outs, leaves, dout)
            if out.requires_grad:
                out.backward(dout.to(out.dtype) if out.dim() == 0 else dout)
            torch.cuda.synchronize()
    finally:
        if handle is not None:
            handle.remove()
    assert _pending_empty(), "deferred gradients left in the queue after backward"
    res["out"] = out.detach().cpu()
    if "logits" in outs:
        res["logits"] = outs["logits"].detach().cpu()
    res["grads"] = {k: (None if v.grad is None else v.grad.detach().cpu()) for k, v in leaves.items()}
    for k in params if sink else ():
        res["ptr_same"][k] = leaves[k].grad.data_ptr() == ptrs[k]
        res["hooks"][k] = counts[id(leaves[k])]
    res["params"] = params
    return res


def _check_forward(name, got, offset=0):
    ref, emu = R.evaluate(name, "ref", offset), R.evaluate(name, "emu", offset)
    if "logits" in got:
        V = R.CASES[name][1]["V"]
        assert got["logits"].shape[-1] == V, "the padded logits were not sliced to the vocabulary"
        R.assert_line_close(name, "logits", got["logits"], ref["logits"], emu["logits"], path="fwd")
        want, scale, slack = R.loss_of_logits(name, got["logits"])
        assert got["out"].dtype == torch.float32
        u = assert_f32_close(got["out"], want, scale, slack, name=f"{name} loss")
        R.RATIOS.setdefault(name, {})["fwd:loss_f32_units"] = dict(units=u, slack=slack)
    else:
        assert got["out"].dtype == BF
        R.assert_line_close(name, "out", got["out"], ref["out"], emu["out"], path="fwd")


def _check_grads(name, got, offset=0, path="plain", frozen=()):
    ref, emu = R.evaluate(name, "ref", offset), R.evaluate(name, "emu", offset)
    for k, g in got["grads"].items():
        if k in frozen:
            assert g is None, f"{name}: frozen input {k} received a gradient"
            continue
        if g is None:  # an input the unit does not use (none today)
            assert not ref["d_" + k].any(), f"{name}: no gradient for {k}"
            continue
        assert g.dtype == BF
        g0 = got["g0"].get(k)
        R.assert_line_close(name, "d_" + k, g.reshape(ref["d_" + k].shape), ref["d_" + k],
                            emu["d_" + k], g0=g0, path=path)


_PLAIN = {}


def _plain(name, dev, offset=0):
    """The all-trainable plain-path run, shared (nothing modifies it)."""
    if (name, offset) not in _PLAIN:
        _PLAIN[(name, offset)] = _run(name, dev, offset)
    return _PLAIN[(name, offset)]


def _same_bits(a, b):
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


# ---------------------------------------------------------------- a, b: forward, plain
@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_and_plain_gradients(cuda, name):
    got = _plain(name, cuda)
    _check_forward(name, got)
    _check_grads(name, got)


@pytest.mark.parametrize("name", DROP_CASES)
def test_dropout_sites_at_a_nonzero_seed_offset(cuda, name):
    """f: every dropout site's backward uses its forward's mask, and both follow seed_ptr: the
    reference with the restated masks of offset 977 is met (offset 0: the test above)."""
    off = R.SEED_OFFSETS[1]
    got = _run(name, cuda, off)
    _check_forward(name, got, off)
    _check_grads(name, got, off)
    assert int(_k().seed_offset(cuda).item()) == 0


@pytest.mark.parametrize("name", MAIN)
def test_frozen_inputs_get_none_and_the_rest_keeps_its_bits(cuda, name):
    unit, _ = R.CASES[name]
    t = R.inputs(name)[0]
    params = [k for k in t if _is_param(unit, k)]
    # every other parameter; with one parameter or none, the inputs (but never every leaf: with
    # a single leaf this is a second identical run, which must repeat its bits)
    frozen = tuple(params[::2]) if len(params) > 1 else tuple(k for k in t if not _is_param(unit, k))
    if len(frozen) == len(t):
        frozen = frozen[:-1]
    full = _plain(name, cuda)
    got = _run(name, cuda, frozen=frozen)
    assert _same_bits(got["out"], full["out"])
    for k, g in got["grads"].items():
        if k in frozen:
            assert g is None, f"{name}: frozen {k} received a gradient"
        else:
            assert g is not None and _same_bits(g, full["grads"][k]), \
                f"{name}: {k} differs from the all-trainable run with {frozen} frozen"


# ------------------------------------------------------------------------- c: sink path
SINK_CASES = [n for n in R.CASES if any(_is_param(R.CASES[n][0], k) for k in R.inputs(n)[0])]


@pytest.mark.parametrize("name", SINK_CASES)
def test_sink_path(cuda, name):
    """The leaves in a real gvl.optim.AdamW (lr 0: the kv_proj stack is the production layout),
    .grad pre-filled with g0: p.grad meets the bound around g0 + ref in the same storage, and the
    ready hook fires exactly once per sunk parameter, the packed in_proj and the tied wte (two
    contributions, one notification: after the lm_head's deferred flush) included."""
    unit, _ = R.CASES[name]
    got = _run(name, cuda, sink=True)
    _check_forward(name, got)
    _check_grads(name, got, path="sink")
    for k in got["params"]:
        assert got["ptr_same"][k], f"{name}: {k}.grad was replaced"
        want = 1 if _sinks(name, k) else 0
        assert got["hooks"][k] == want, f"{name}: ready hook of {k} fired {got['hooks'][k]} x, not {want}"
    assert got["params"], name


def test_query_expand_fp32_parameter(cuda):
    """The fp32 query_tokens parameter (cast per call): bf16 output, fp32 gradient."""
    Fn = _fn()
    name = "query_expand"
    ref, emu = R.evaluate(name, "ref"), R.evaluate(name, "emu")
    t, _, dout = R.inputs(name)
    q = t["q"].float().to(cuda).requires_grad_()
    out = Fn.QueryExpandFn.apply(q, R.B)
    out.backward(dout.to(cuda))
    assert out.dtype == BF and q.grad.dtype == torch.float32
    R.assert_line_close(name, "out", out.detach().cpu(), ref["out"], emu["out"], path="fp32")
    R.assert_line_close(name, "d_q", q.grad.cpu(), ref["d_q"], emu["d_q"], path="fp32")


# --------------------------------------------------------------------- d: flush routes
class _Counting:
    """Counting shims over the kernels the flush can take (pytest's monkeypatch restores them)."""
    NAMES = ("gemm_grouped", "gemm_batched", "colsum_batched", "layernorm_finalize_batched", "gemm")

    def __init__(self, monkeypatch):
        K = _k()
        self.n = collections.Counter()
        self.log = []
        for nm in self.NAMES:
            monkeypatch.setattr(K, nm, self._shim(nm, getattr(K, nm)))

    def _shim(self, nm, orig):
        def shim(*a, **kw):
            r = orig(*a, **kw)
            if nm == "gemm":  # only the device-scaled accumulating weight gradient is counted
                if kw.get("alpha_ptr") is not None and kw.get("a_mn") and kw.get("out") is not None:
                    self.n["gemm_scaled_dw"] += 1
                return r
            self.n[nm] += 1
            if nm == "gemm_grouped":
                self.log.append((nm, len(a[0]), kw.get("dbias") is not None, bool(r),
                                 sum(1 for it in a[0] if len(it) > 3 and it[3] is not None)))
            elif nm == "gemm_batched":
                self.log.append((nm, len(a[0]), kw.get("dbias") is not None, r is not False))
            return r
        return shim


def _route(name, rec):
    ROUTES[name] = rec
    R.RATIOS["routes"] = ROUTES
    margins_out("fn_margins", R.RATIOS)


@pytest.mark.parametrize("name", ["kv_only", "kv_only_99"])
def test_flush_single_shape_group_batched(cuda, monkeypatch, name):
    """CrossKVFn alone, L = 2: one shape group -> gemm_batched with the bias sums fused (or, when
    the library declines the shape, the unfused batch + colsum_batched); never the grouped launch."""
    cnt = _Counting(monkeypatch)
    got = _run(name, cuda, sink=True)
    _check_grads(name, got, path="sink-batched")
    assert cnt.n["gemm_grouped"] == 0
    first = cnt.log[0]
    assert first[:3] == ("gemm_batched", R.L, True)
    if first[3]:
        assert cnt.n["gemm_batched"] == 1 and cnt.n["colsum_batched"] == 0
    else:
        assert cnt.n["gemm_batched"] == 2 and cnt.n["colsum_batched"] == 1
    _route(name, dict(fused=first[3], calls=dict(cnt.n)))
    assert all(got["hooks"][k] == 1 for k in got["params"])


def test_flush_one_problem_falls_back_per_problem(cuda, monkeypatch):
    """One LinearFn: a batch of one cannot fuse its bias -> the unfused call (per-problem
    gvl_gemm) and colsum_batched for the bias."""
    cnt = _Counting(monkeypatch)
    got = _run("linear", cuda, sink=True)
    _check_grads("linear", got, path="sink-fallback")
    assert cnt.n["gemm_grouped"] == 0 and cnt.n["gemm_batched"] == 2 and cnt.n["colsum_batched"] == 1
    assert [e[3] for e in cnt.log] == [False, True]
    assert got["hooks"] == {"w": 1, "b": 1}


@pytest.mark.parametrize("name", ["mlp_k64", "mlp_tanh", "mha_cross", "gpt_block"])
def test_flush_several_groups_one_grouped_launch(cuda, monkeypatch, name):
    """Several shape groups under 8192 tokens: ONE gemm_grouped call with the biases fused.  At
    64 rows it launches; at 99 rows (no multiple of the 32-deep K-step) the library declines and
    the groups take the per-shape path, to the same bounds."""
    cnt = _Counting(monkeypatch)
    got = _run(name, cuda, sink=True)
    _check_forward(name, got)
    _check_grads(name, got, path="sink-grouped")
    assert cnt.n["gemm_grouped"] == 1
    g = cnt.log[0]
    assert g[0] == "gemm_grouped" and g[2]
    assert g[3] == (name == "mlp_k64"), f"{name}: grouped launch {'ran' if g[3] else 'declined'}"
    if g[3]:
        assert cnt.n["gemm_batched"] == 0 and cnt.n["colsum_batched"] == 0
    _route(name, dict(grouped=g[3], problems=g[1], calls=dict(cnt.n)))
    assert all(got["hooks"][k] == 1 for k in got["params"])


def test_flush_bias_without_a_queued_weight_gradient(cuda, monkeypatch):
    """Frozen weight, trainable bias: its dY has no weight gradient to ride -> colsum_batched."""
    cnt = _Counting(monkeypatch)
    got = _run("linear", cuda, sink=True, frozen=("w",))
    _check_grads("linear", got, path="sink-colsum", frozen=("w",))
    assert cnt.n["colsum_batched"] == 1 and cnt.n["gemm_batched"] == 0 and cnt.n["gemm_grouped"] == 0
    assert got["hooks"] == {"b": 1}


def test_flush_device_scaled_lm_head_alone(cuda, monkeypatch):
    cnt = _Counting(monkeypatch)
    got = _run("lmhead_520", cuda, sink=True)
    _check_grads("lmhead_520", got, path="sink-scaled")
    assert cnt.n["gemm_scaled_dw"] == 1 and cnt.n["gemm_grouped"] == 0 and cnt.n["gemm_batched"] == 0
    assert got["hooks"] == {"w": 1}


def test_flush_device_scaled_lm_head_inside_a_grouped_launch(cuda, monkeypatch):
    cnt = _Counting(monkeypatch)
    got = _run("lin_lmhead", cuda, sink=True)
    _check_forward("lin_lmhead", got)
    _check_grads("lin_lmhead", got, path="sink-grouped-scaled")
    assert cnt.n["gemm_grouped"] == 1
    g = cnt.log[0]
    assert g[1] == 2 and g[4] == 1, "the scaled entry did not go into the grouped launch"
    assert g[3], "the grouped launch declined"
    assert cnt.n["gemm_scaled_dw"] == 0
    _route("lin_lmhead", dict(grouped=g[3], calls=dict(cnt.n)))
    assert got["hooks"] == {"pw": 1, "pb": 1, "w": 1}


@pytest.mark.parametrize("blocks", [0, 1])
def test_flush_per_block_under_overlap(cuda, monkeypatch, blocks):
    """set_overlap_blocks(1) over two GPTBlockFn: one in-place flush per block; 0: one at the end."""
    Fn = _fn()
    cnt = _Counting(monkeypatch)
    Fn.set_overlap_blocks(blocks)
    try:
        got = _run("gpt_stack", cuda, sink=True)
    finally:
        Fn.set_overlap_blocks(0)
    _check_forward("gpt_stack", got)
    _check_grads("gpt_stack", got, path=f"sink-overlap{blocks}")
    flushes = R.L if blocks else 1
    assert cnt.n["gemm_grouped"] == flushes and cnt.n["layernorm_finalize_batched"] == flushes
    grouped = [e for e in cnt.log if e[0] == "gemm_grouped"]
    assert [e[1] for e in grouped] == [4 * R.L // flushes] * flushes and all(e[3] for e in grouped)
    assert all(got["hooks"][k] == 1 for k in got["params"])
    assert not Fn._BLOCKS_SEEN


# ----------------------------------------------------------- e: shared state, re-entry
@pytest.mark.parametrize("name", ["cross_kv", "gpt_block", "qformer"])
def test_second_backward_over_a_retained_graph(cuda, name):
    """A second backward over the retained graph gives the same gradients bit for bit (the
    KVGradSlab re-arms; the tapes are refilled)."""
    leaves, c, dout = _leaves(name, cuda, 0)
    outs = _call(name, leaves, c, cuda)
    ins = list(leaves.values())
    g1 = torch.autograd.grad(outs["out"], ins, dout, retain_graph=True)
    g2 = torch.autograd.grad(outs["out"], ins, dout)
    torch.cuda.synchronize()
    full = _plain(name, cuda)
    for k, a, b in zip(leaves, g1, g2):
        assert _same_bits(a.cpu(), b.cpu()), f"{name}: {k} changed in the second backward"
        assert _same_bits(a.cpu(), full["grads"][k]), f"{name}: {k} differs from the plain run"
    if "slab" in outs:
        s = outs["slab"]
        assert s.buf is None and s.left == s.layers and s.task is None
    assert _pending_empty()


def test_interleaved_backward_passes_keep_their_queues(cuda):
    """Two independent graphs, both sinking, both built before either backward: torch.autograd.grad
    on the first, then .backward() on the second.  Each pass flushes its own queue entries only."""
    Fn = _fn()
    from gvl.optim import AdamW
    name_a = "mlp_tanh"
    ref, emu = R.evaluate(name_a, "ref"), R.evaluate(name_a, "emu")
    a, a_c, a_dout = _leaves(name_a, cuda, 0)
    pa = ("w1", "b1", "w2", "b2")
    AdamW([a[k] for k in pa], lr=0.0).grad_arena
    g0 = {k: _g0(name_a, k, ref["d_" + k]) for k in pa}
    for k in pa:
        a[k].grad.copy_(g0[k].to(cuda))
    counts = collections.Counter()
    h = Fn.register_grad_ready_hook(lambda p: counts.update([id(p)]))
    held = {}
    try:
        out_a = _call(name_a, a, a_c, cuda)["out"]

        def between(outs_b, leaves_b, dout_b):
            before = {k: v.grad.clone() for k, v in leaves_b.items() if v.grad is not None}
            gs = torch.autograd.grad(out_a, list(a.values()), a_dout, allow_unused=True)
            held.update(zip(a, gs))
            assert _pending_empty(), "graph A's backward left entries in the queue"
            for k, g in before.items():
                assert torch.equal(bits(leaves_b[k].grad), bits(g)), f"A's flush touched B's {k}"

        got_b = _run("linear", cuda, sink=True, before_backward=between)
    finally:
        h.remove()
    R.assert_line_close(name_a, "d_x", held["x"].cpu(), ref["d_x"], emu["d_x"], path="interleaved")
    for k in pa:
        assert held[k] is None, f"{k}: a sunk gradient was also returned"
        R.assert_line_close(name_a, "d_" + k, a[k].grad.cpu(), ref["d_" + k], emu["d_" + k],
                            g0=g0[k], path="sink-interleaved")
        assert counts[id(a[k])] == 1
    _check_grads("linear", got_b, path="sink-interleaved")
    assert got_b["hooks"] == {"w": 1, "b": 1}


# ----------------------------------------------------------------------- 4: empty batch
def _empty_units(dev, Fn, t):
    z = lambda *s: torch.zeros(*s, dtype=BF, device=dev)
    return {
        "linear": lambda: Fn.LinearFn.apply(z(0, R.T, R.C).requires_grad_(), t["w"], t["b"]),
        "layernorm": lambda: Fn.LayerNormFn.apply(z(0, R.T, R.C).requires_grad_(), t["lw"], t["lb"], 1e-5),
        "mlp": lambda: Fn.MLPFn.apply(z(0, R.T, R.C).requires_grad_(), t["w1"], t["b1"], t["w2"],
                                      t["b2"], None, 1, 0.0, 0),
    }


_EMPTY_PARAMS = {"linear": ("w", "b"), "layernorm": ("lw", "lb"), "mlp": ("w1", "b1", "w2", "b2")}


@pytest.mark.parametrize("sink", [False, True])
@pytest.mark.parametrize("unit", ["linear", "layernorm", "mlp"])
def test_empty_batch(cuda, unit, sink):
    """B = 0: empty outputs; sunk gradients keep g0 bit for bit and their hooks fire once; plain
    gradients are zeros of the parameter's shape (a weight gradient over zero rows adds nothing,
    and no GEMM is launched with K = 0)."""
    Fn = _fn()
    g = torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=g).to(BF).to(cuda).requires_grad_()
    t = dict(w=rn(R.C, R.C), b=rn(R.C), lw=rn(R.C), lb=rn(R.C), w1=rn(4 * R.C, R.C), b1=rn(4 * R.C),
             w2=rn(R.C, 4 * R.C), b2=rn(R.C))
    names = _EMPTY_PARAMS[unit]
    g0 = {}
    counts = collections.Counter()
    if sink:
        from gvl.optim import AdamW
        AdamW([t[k] for k in names], lr=0.0).grad_arena
        for k in names:
            g0[k] = torch.randn(t[k].shape, generator=g).to(BF)
            t[k].grad.copy_(g0[k].to(cuda))
    h = Fn.register_grad_ready_hook(lambda p: counts.update([id(p)]))
    try:
        out = _empty_units(cuda, Fn, t)[unit]()
        assert out.shape == (0, R.T, R.C) and out.dtype == BF
        out.backward(torch.zeros_like(out))
        torch.cuda.synchronize()
    finally:
        h.remove()
    assert _pending_empty()
    for k in names:
        got = t[k].grad.cpu()
        assert got.shape == t[k].shape
        if sink:
            assert torch.equal(bits(got), bits(g0[k])), f"{unit}: {k}.grad moved off g0"
            assert counts[id(t[k])] == 1, f"{unit}: ready hook of {k} fired {counts[id(t[k])]} x"
        else:
            assert not got.any(), f"{unit}: {k}.grad is not zero"
