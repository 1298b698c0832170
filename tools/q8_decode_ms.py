"""Int8 weight-only decoding against bf16: milliseconds per token, the skinny kernel per shape,
and how far the two models' outputs lie apart.  GPT-2 124M and GPT-2 XL at vocab 50304, bf16,
random weights (no trained checkpoint: the agreement figures say nothing about trained models).

    python tools/q8_decode_ms.py out.json [--sizes gpt2,gpt2-xl] [--no-shapes]
    python tools/q8_decode_ms.py out.json --bf16-only [--tree DIR]     (one tree's bf16 paths)
    python tools/q8_decode_ms.py out.json --ab PARENT_DIR

1. end to end: greedy generate, 128 new tokens after a 64-token prompt, B in {1, 8}, eager and
   graph-replayed (one GraphedGenerate session per configuration, its capture in the warm-up),
   weights=None against a quantize_decoder snapshot, the four paths timed alternately in one
   process.  ms per token = call time / 128, the prefill included.
2. per shape: c_attn, attn.c_proj, c_fc, mlp.c_proj and lm_head of both sizes at M in {1, 8, 32,
   256}: gvl_linear_w8 on int8, its bf16 instance, and K.linear (gvl_gemm).  Each launch of a
   cycle reads another copy of the weight, the copies totalling >= 512 MiB (twice the Infinity
   Cache), so a launch reads HBM; the cycle is captured as one graph and replayed.  Reported:
   us per launch, weight bytes per second, and that rate as a share of 6.29 TB/s (the measured
   copy rate): a bytes-over-bandwidth bound, not a counter reading.
3. agreement of the int8 and the bf16 run on the same model and prompt: the largest logit
   difference over the 128 steps relative to the largest logit, and the greedy tokens that are
   equal (the runs diverge after the first different token).
--ab: PARENT_DIR (a checkout of the parent commit with its built library) and this tree with
--bf16-only in fresh processes, alternating, AB_RUNS each: the parent's run-to-run spread per
configuration and whether this tree's default (bf16) path sits inside it.
Each figure is a host clock around work that ends in a device synchronise; the paths are timed
alternately ROUNDS times after WARM warm-up calls, the median reported with all rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--sizes", default="gpt2,gpt2-xl")
ap.add_argument("--bf16-only", action="store_true")
ap.add_argument("--no-shapes", action="store_true")
ap.add_argument("--tree", default=HERE)
ap.add_argument("--ab", metavar="PARENT_DIR")
cli = ap.parse_args()

WARM, ROUNDS = 2, 5
AB_RUNS = 3  # fresh processes per tree in --ab
N_NEW, PROMPT = 128, 64
HBM_TBS = 6.29
CYCLE_BYTES = 512 << 20
SIZES = cli.sizes.split(",")


def write(res):
    print(json.dumps(res, indent=1))
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, "w") as f:
            json.dump(res, f, indent=1)


def ab(parent):
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(AB_RUNS):
            for name, tree in (("parent", parent), ("this", HERE)):
                path = os.path.join(tmp, f"{name}{i}.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), path, "--bf16-only",
                                "--tree", tree, "--sizes", cli.sizes],
                               check=True, stdout=subprocess.DEVNULL, timeout=500)
                with open(path) as f:
                    runs.append(dict(tree=name, run=i, **json.load(f)))
    summary = {}
    for key in runs[0]["end_to_end"]:
        for path in ("eager", "graphed"):
            med = lambda tree: [r["end_to_end"][key][path]["bf16"]["ms_per_token"]
                                for r in runs if r["tree"] == tree]
            base, this = med("parent"), med("this")
            spread = max(base) / min(base) - 1.0
            summary[f"{key}_{path}"] = dict(
                parent_ms_per_token=base, parent_spread=spread, this_ms_per_token=this,
                this_within_parent_spread=max(this) <= max(base) * (1 + spread))
    write(dict(method="parent and this tree, bf16 paths only, in fresh processes, alternating, "
                      f"{AB_RUNS} each; spread = max / min - 1 of the parent's medians",
               summary=summary, runs=runs))


if cli.ab:
    ab(cli.ab)
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, os.path.join(cli.tree, "gpt2-vision-language_amd"))
import gvl.gpt2 as g2  # noqa: E402
import gvl.kernels as K  # noqa: E402
from gvl import decode  # noqa: E402

dev = torch.device("cuda:0")
BF = torch.bfloat16


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns):
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            times[k].append(clock(fn))
    return times


def end_to_end(size, model, qd):
    out, agree = {}, {}
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        prompt = torch.randint(0, 50257, (B, 16), generator=g).repeat(1, 4).to(dev)
        kinds = dict(bf16=None) if qd is None else dict(bf16=None, int8=qd)
        fns, sessions = {}, []
        for name, w in kinds.items():
            kw = {} if w is None else dict(weights=w)
            ses = decode.GraphedGenerate(model, PROMPT, N_NEW, greedy=True, **kw)
            sessions.append(ses)
            fns[f"eager/{name}"] = lambda kw=kw: decode.generate(model, prompt, N_NEW, greedy=True,
                                                                 **kw)
            fns[f"graphed/{name}"] = lambda ses=ses: ses(prompt)
        times = alternate(fns)
        r = dict(eager={}, graphed={})
        for k, v in times.items():
            path, name = k.split("/")
            call = statistics.median(v)
            r[path][name] = dict(ms_per_call=call, ms_per_token=call / N_NEW, ms_per_call_rounds=v)
        if qd is not None:
            for path in r:
                r[path]["int8_over_bf16"] = (r[path]["int8"]["ms_per_token"] /
                                             r[path]["bf16"]["ms_per_token"])
            ta, la = decode.generate(model, prompt, N_NEW, greedy=True, return_logits=True)
            tb, lb = decode.generate(model, prompt, N_NEW, greedy=True, return_logits=True,
                                     weights=qd)
            first = (ta != tb).any(0).nonzero()
            agree[f"B{B}"] = dict(
                max_rel_logit_diff=float((la - lb).abs().max() / la.abs().max()),
                equal_greedy_tokens=int((ta == tb).sum()), of=int(ta.numel()),
                first_different_step=int(first[0]) if first.numel() else None,
                max_rel_logit_diff_until_then=float(
                    (la - lb)[:, :int(first[0]) + 1 if first.numel() else N_NEW].abs().max() /
                    la.abs().max()))
            del la, lb
        for ses in sessions:
            ses.close()
        out[f"{size}_B{B}"] = r
    return out, agree


def per_shape(size, C, V):
    """us per launch of the three kernels over cycles of distinct weight copies."""
    shapes = dict(c_attn=(3 * C, C), attn_c_proj=(C, C), c_fc=(4 * C, C), mlp_c_proj=(C, 4 * C),
                  lm_head=(V, C))
    big_q = torch.randint(-127, 128, (CYCLE_BYTES + (64 << 20),), dtype=torch.int8, device=dev)
    big_w = torch.empty((CYCLE_BYTES + (128 << 20)) // 2, dtype=BF, device=dev).normal_()
    res = {}
    for name, (N, Kd) in shapes.items():
        nq = -(-CYCLE_BYTES // (N * Kd))
        nw = -(-CYCLE_BYTES // (2 * N * Kd))
        qs = [big_q[i * N * Kd:(i + 1) * N * Kd].view(N, Kd) for i in range(nq)]
        ws = [big_w[i * N * Kd:(i + 1) * N * Kd].view(N, Kd) for i in range(nw)]
        scale = torch.rand(N, device=dev) * 0.01
        bias = None if name == "lm_head" else torch.randn(N, device=dev).to(BF)
        for M in (1, 8, 32, 256):
            x = torch.randn(M, Kd, device=dev).to(BF)
            y = torch.empty(M, N, dtype=BF, device=dev)
            cycles = {
                "w8_int8": (qs, lambda w: K.linear_w8(x, w, scale, bias, out=y), N * Kd + 4 * N),
                "w8_bf16": (ws, lambda w: K.linear_w8(x, w, None, bias, out=y), 2 * N * Kd),
                "gemm_bf16": (ws, lambda w: K.linear(x, w, bias, out=y), 2 * N * Kd),
            }
            fns = {}
            graphs = []
            for k, (copies, fn, _) in cycles.items():
                fn(copies[0])
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for w in copies:
                        fn(w)
                graphs.append(gr)
                fns[k] = gr.replay
            times = alternate(fns)
            r = {}
            for k, v in times.items():
                copies, _, nbytes = cycles[k]
                us = statistics.median(v) * 1e3 / len(copies)
                r[k] = dict(us_per_launch=us, launches_per_cycle=len(copies),
                            weight_bytes=nbytes, weight_TB_per_s=nbytes / us * 1e-6,
                            share_of_hbm_copy_rate=nbytes / us * 1e-6 / HBM_TBS)
            r["int8_over_gemm"] = r["w8_int8"]["us_per_launch"] / r["gemm_bf16"]["us_per_launch"]
            r["w8_bf16_over_gemm"] = r["w8_bf16"]["us_per_launch"] / r["gemm_bf16"]["us_per_launch"]
            res[f"{size}_{name}_M{M}"] = r
            for gr in graphs:
                gr.reset()
    return res


res = dict(models="GPT-2 sizes at vocab 50304, bf16, random weights", prompt_len=PROMPT,
           n_new=N_NEW, warm=WARM, rounds=ROUNDS,
           device=torch.cuda.get_device_name(0), hbm_copy_rate_TB_per_s=HBM_TBS,
           note="random weights: the agreement figures say nothing about trained checkpoints",
           end_to_end={}, agreement={}, per_shape={})
for size in SIZES:
    torch.manual_seed(0)
    cfg = g2.GPTConfig.for_size(size, vocab_size=50304)
    with torch.device(dev):
        model = g2.GPT(cfg)
    model = model.to(BF).eval()
    qd = None
    if not cli.bf16_only:
        from gvl import quant
        qd = quant.quantize_decoder(model)
    e2e, agree = end_to_end(size, model, qd)
    res["end_to_end"].update(e2e)
    if agree:
        res["agreement"][size] = agree
    del model, qd
    torch.cuda.empty_cache()
    if not cli.bf16_only and not cli.no_shapes:
        res["per_shape"].update(per_shape(size, cfg.n_embd, 50304))
        torch.cuda.empty_cache()
write(res)
