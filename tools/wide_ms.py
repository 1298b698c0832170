"""Timing of the wide row kernels and of one LM step at the GPT-2 large / XL sizes.
    python tools/wide_ms.py [profiles/wide_ms.json] [--no-steps]

LayerNorm: forward and backward (the LM's form: dx = residual + LN', dw / db accumulated) at
16384 x {1280, 1600, 2048} next to the narrow kernels at 16384 x 1024, all in one process, the
four widths timed in turn within every round (HIP events around a graph replay of 20 launches,
median of 9 rounds).  Each as achieved bytes/s: 4C B per row forward (+ 8 B of statistics), 6C B
per row backward (+ 8 B, + the partials: blocks x 2C floats written and read once), and as the
ratio to the 1024-column kernel's rate in the same run: these kernels are HBM-bound and should
move bytes at its rate.

LM step: tokens/s of one optimizer step of one micro-batch of 16 x 1024 tokens (vocab 50304) at
gpt2-large and gpt2-xl, with the model FLOPs (6 per parameter and token + 12 L C T of attention)
over the bf16 peak.  The parent of this tool cannot run these sizes: there is nothing to compare
with."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gpt2-vision-language_amd")]
from gvl import _lib  # noqa: E402
from gvl import kernels as K  # noqa: E402

PEAK_BF16_TFLOPS = 2516.6
ROWS, WIDTHS, LAUNCHES, ROUNDS = 16384, (1024, 1280, 1600, 2048), 20, 9


def ln_graphs(C, dev):
    g = torch.Generator(device=dev).manual_seed(C)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)  # noqa: E731
    x, w, b, dy, res = rnd(ROWS, C), rnd(C), rnd(C), rnd(ROWS, C), rnd(ROWS, C)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    dw, db = (torch.zeros(C, device=dev, dtype=torch.bfloat16) for _ in range(2))
    _, mean, rstd = K.layernorm_fwd(x, w, b, out=y)
    K.layernorm_bwd(dy, x, w, mean, rstd, dx=dx, dw=dw, db=db, accumulate_wb=True, residual=res)
    torch.cuda.synchronize()
    gf, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gf):
        for _ in range(LAUNCHES):
            K.layernorm_fwd(x, w, b, out=y)
    with torch.cuda.graph(gb):
        for _ in range(LAUNCHES):
            K.layernorm_bwd(dy, x, w, mean, rstd, dx=dx, dw=dw, db=db, accumulate_wb=True, residual=res)
    nblk = int(_lib.load().gvl_layernorm_bwd_blocks(ROWS))
    nbytes = dict(fwd=ROWS * (4 * C + 8), bwd=ROWS * (6 * C + 8) + 2 * nblk * 2 * C * 4)
    return dict(fwd=gf, bwd=gb), nbytes, (x, w, b, dy, res, y, dx, dw, db, mean, rstd)


def us(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES


def layernorm(dev):
    sets = {C: ln_graphs(C, dev) for C in WIDTHS}
    t = {(C, k): [] for C in WIDTHS for k in ("fwd", "bwd")}
    for r in range(ROUNDS + 1):
        for k in ("fwd", "bwd"):
            for C in WIDTHS:
                v = us(sets[C][0][k])
                if r:  # round 0 warms up
                    t[(C, k)].append(v)
    out = {}
    for k in ("fwd", "bwd"):
        rate = {C: sets[C][1][k] / (statistics.median(t[(C, k)]) * 1e-6) / 1e12 for C in WIDTHS}
        for C in WIDTHS:
            out[f"{k}_{ROWS}x{C}"] = dict(us_median=round(statistics.median(t[(C, k)]), 2),
                                          us_min=round(min(t[(C, k)]), 2),
                                          us_max=round(max(t[(C, k)]), 2), bytes=sets[C][1][k],
                                          tb_per_s=round(rate[C], 3),
                                          ratio_to_1024=round(rate[C] / rate[1024], 3))
    return out


def lm_step(name, dev):
    import gvl.gpt2 as g2
    from gvl.train import lm_batch, train_step
    B, T = 16, 1024
    torch.manual_seed(0)
    cfg = g2.GPTConfig.for_size(name, vocab_size=50304)
    model = g2.GPT(cfg).to(dev).to(torch.bfloat16)
    model.train()
    opt = model.configure_optimizers(0.1, 6e-4, "cuda")
    batches = [lm_batch(B, T, step=0, rank=0, device=dev)]
    loss_fn = lambda m, b: m(b[0], b[1])[1]  # noqa: E731
    ms = []
    for it in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = train_step(model, opt, batches, loss_fn, 6e-4)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:  # two warm-up steps
            ms.append(e0.elapsed_time(e1))
    n_params = sum(p.numel() for p in model.parameters())
    flop_per_token = 6.0 * n_params + 12.0 * cfg.n_layer * cfg.n_embd * T
    tok_s = B * T / (statistics.median(ms) * 1e-3)
    return dict(config=[cfg.n_layer, cfg.n_head, cfg.n_embd], parameters=n_params, tokens=B * T,
                step_ms=[round(v, 2) for v in ms], tokens_per_s=round(tok_s, 1),
                flop_per_token=flop_per_token, loss=float(r.loss),
                mfma_frac=round(tok_s * flop_per_token / 1e12 / PEAK_BF16_TFLOPS, 4),
                peak_hbm_gib=round(torch.cuda.max_memory_allocated(dev) / 2**30, 2))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dev = torch.device("cuda:0")
    _lib.load()
    res = dict(device=torch.cuda.get_device_name(0), rows=ROWS, launches_per_replay=LAUNCHES,
               rounds=ROUNDS, layernorm=layernorm(dev))
    for name in ("gpt2-large", "gpt2-xl"):
        res["lm_step_" + name] = "not measured" if "--no-steps" in sys.argv else lm_step(name, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    if args:
        with open(args[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
