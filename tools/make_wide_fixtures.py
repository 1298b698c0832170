"""Golden fixtures at the GPT-2 large / XL widths (n_embd 1280 / 20 heads, 1600 / 25 heads) from
the REFERENCE model code, with tools/make_fixtures.py's machinery (runs only where the reference
checkout exists; the reference never travels).

Per config and kind (gpt, qformer, cross) the reference's fp32 CPU path gives the loss, the
logits, every trainable gradient and the parameters, losses and gradient norms of three AdamW
steps, as sampled summaries in tests/golden/KIND_wide1280.npz / KIND_wide1600.npz.  The vision
tokens keep the CLIP width (768); z_raw regenerates from its seed.

The same run in the reference's own bf16 path (model.to(bfloat16) + autocast, bf16 AdamW state:
tools/bf16_yardstick.py's recipe, on the CPU) against that fp32 path gives the yardstick of
tests/golden/wide_yardstick.json: per config and kind the relative errors, in the metrics
tests/test_gpu_wide.py asserts, of loss, logits, gradients, parameters after three steps, train
losses and norms.

    python tools/make_wide_fixtures.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_fixtures as MF  # noqa: E402
from tests.helpers import rel_err, save_golden  # noqa: E402

WIDE = {
    "wide1280": dict(block_size=64, vocab_size=512, n_layer=2, n_head=20, n_embd=1280),
    "wide1600": dict(block_size=64, vocab_size=512, n_layer=1, n_head=25, n_embd=1600),
}
ENC = 768  # CLIP width of the vision tokens
SEEDS = {"gpt": 111, "qformer": 212, "cross": 313}
YARD = os.path.join(ROOT, "tests", "golden", "wide_yardstick.json")


def lr_cross(it):
    return MF.lr_caption(it, 1e-3, 1e-5, 20, 925)


def case(kind, cfg, g2, qf, xa):
    """-> (build(), loss_of(model) -> (logits, loss), inputs to store, lr schedule)."""
    V = cfg["vocab_size"]
    if kind == "gpt":
        x, y = MF.inputs_lm(2, 48, V, SEEDS[kind])
        return (lambda: g2["GPT"](g2["GPTConfig"](**cfg)), lambda m: m(x, y),
                dict(x=x.numpy(), y=y.numpy()), MF.lr_lm)
    if kind == "qformer":
        z_raw, x, y, mask = MF.inputs_caption(2, 257, ENC, 24, V, SEEDS[kind])
        labels = y.masked_fill(~mask, -100)
        z = qf.pool_clip_197_to_33_avg_with_cls(z_raw)

        def build():
            return qf.GPT_Caption(enc_dim=ENC, lm=qf.GPT_previous(qf.GPTConfig(**cfg)), m_vis_tokens=32)
        return (build, lambda m: m(z.to(next(m.parameters()).dtype), x, labels=labels),
                dict(x=x.numpy(), y=y.numpy(), mask=mask.numpy(), labels=labels.numpy(),
                     z_seed=np.array(SEEDS[kind]), z_shape=np.array(z_raw.shape)), MF.lr_caption)
    z_raw, x, y, mask = MF.inputs_caption(2, 197, ENC, 24, V, SEEDS[kind])
    z = xa.pool_clip_197_to_33_avg_with_cls(z_raw)
    return (lambda: xa.GPT(xa.GPTConfig(**cfg, img_embd=ENC)),
            lambda m: m(x, z=z.to(next(m.parameters()).dtype), targets=y, target_mask=mask),
            dict(x=x.numpy(), y=y.numpy(), mask=mask.numpy(), z_seed=np.array(SEEDS[kind]),
                 z_shape=np.array(z_raw.shape)), lr_cross)


def run(build, loss_of, lr_of, bf16):
    """Forward, backward and three AdamW steps of the reference -> dict of float64 arrays."""
    model = MF.set_recipe(build())
    model.eval()  # dropout off; gradients still flow
    if bf16:
        model = model.to(torch.bfloat16)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    params = dict(model.named_parameters())

    def fwd():
        with torch.autocast(device_type="cpu", dtype=torch.bfloat16, enabled=bf16):
            return loss_of(model)

    out = {}
    logits, loss = fwd()
    out["logits"], out["loss"] = logits.detach().double(), float(loss)
    loss.backward()
    out["grad"] = {n: params[n].grad.detach().double().clone() for n in names}
    model.zero_grad()
    opt = model.configure_optimizers(weight_decay=0.1, learning_rate=lr_of(0), device="cpu")
    losses, norms = [], []
    for it in range(3):
        opt.zero_grad()
        loss = fwd()[1]
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)))
        for g in opt.param_groups:
            g["lr"] = lr_of(it)
        opt.step()
        losses.append(float(loss))
    out["train_losses"], out["train_norms"] = np.array(losses), np.array(norms)
    out["step3"] = {n: params[n].detach().double().clone() for n in names}
    return out


def summary_err(got, ref):
    """What helpers.check_summary measures against rtol: the max-norm error and half the
    relative error of the sum of squares."""
    a, b = got.numpy().reshape(-1), ref.numpy().reshape(-1)
    sq = float((b * b).sum())
    return max(rel_err(a, b), 0.5 * abs(float((a * a).sum()) - sq) / max(sq, 1e-30))


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    g2 = MF.load_gpt2_classes()
    qf = MF.load_module("gpt2_q_former", "ref_gpt2_q_former_model")
    xa = MF.load_module("gpt2_cross-att", "ref_gpt2_cross_att_model")
    yard = {"recipe": "reference bf16 path (model.to(bfloat16) + autocast, bf16 AdamW state) "
                      "against its fp32 path, same recipe weights and inputs, CPU"}
    for tag, cfg in WIDE.items():
        for kind in ("gpt", "qformer", "cross"):
            build, loss_of, inputs, lr_of = case(kind, cfg, g2, qf, xa)
            ref = run(build, loss_of, lr_of, False)
            out = dict(inputs)
            out["loss"] = np.array(ref["loss"])
            out["logits"] = ref["logits"].numpy().astype(np.float32)
            for n, g in ref["grad"].items():
                MF.summarize("grad:" + n, g, out)
            for n, p in ref["step3"].items():
                MF.summarize("step3:" + n, p, out)
            out["train_losses"], out["train_norms"] = ref["train_losses"], ref["train_norms"]
            paths = save_golden(f"{kind}_{tag}", out, compressed=True, root=MF.OUT)
            bf = run(build, loss_of, lr_of, True)
            yard[f"{tag}:{kind}"] = dict(
                loss=abs(bf["loss"] - ref["loss"]) / abs(ref["loss"]),
                logits=rel_err(bf["logits"].numpy(), ref["logits"].numpy()),
                grads=max(summary_err(bf["grad"][n], g) for n, g in ref["grad"].items()),
                params=max(summary_err(bf["step3"][n], p) for n, p in ref["step3"].items()),
                train_losses=rel_err(bf["train_losses"], ref["train_losses"]),
                train_norms=rel_err(bf["train_norms"], ref["train_norms"]))
            print(tag, kind, ref["loss"], [os.path.getsize(p) for p in paths], yard[f"{tag}:{kind}"],
                  flush=True)
    with open(YARD, "w") as f:
        json.dump(yard, f, indent=1)


if __name__ == "__main__":
    main()
