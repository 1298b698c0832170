"""Milliseconds and peak memory per scoring call at GPT-2 124M (vocab 50304, bf16): one
HellaSwag-shaped example [4, 128] (a context of 100 tokens, endings of 12..27) and one
perplexity batch [16, 1024] (every token counted), each three ways:
    masked: gvl.score.score(select="masked")   lm_head on the scored rows only
    all:    gvl.score.score(select="all")      lm_head on every shifted row, in chunks
    today:  get_most_likely_row(tokens, mask, model(tokens)[0])   the [N, T, V] logits in fp32
    python tools/score_ms.py [out.json]
Each figure is a host clock around ITERS calls that ends in a device synchronise (every path ends
in a host read of its own, so the calls do not overlap); the three paths are timed alternately
ROUNDS times after WARM warm-up calls each, and the median is reported with the spread.  Peak
memory is torch.cuda.max_memory_allocated over one call, above what was allocated before it."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "gpt2-vision-language_amd"))
import gvl.gpt2 as g2  # noqa: E402
from gvl.data import get_most_likely_row  # noqa: E402
from gvl.score import score  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
WARM, ROUNDS = 3, 5
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = g2.GPT(g2.GPTConfig(vocab_size=50304)).to(dev).to(torch.bfloat16).eval()


def shape(N, T, hellaswag):
    tokens = torch.randint(0, 50257, (N, T), device=dev)
    mask = torch.ones(N, T, dtype=torch.long, device=dev)
    if hellaswag:
        mask.zero_()
        for n in range(N):
            mask[n, 100:112 + 5 * n] = 1
    return tokens, mask


def paths(tokens, mask):
    def today():
        with torch.no_grad():
            return get_most_likely_row(tokens, mask, model(tokens)[0])

    return dict(masked=lambda: int(score(model, tokens, mask, group=1).pred_norm[0]),
                all=lambda: int(score(model, tokens, mask, group=1, select="all").pred_norm[0]),
                today=today)


def clock(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


res = dict(model="GPT-2 124M, vocab 50304, bf16", warm=WARM, rounds=ROUNDS,
           device=torch.cuda.get_device_name(0))
# iterations per window: about half a second of work each
for name, N, T, hs, iters in (("hellaswag_4x128", 4, 128, True, 200), ("ppl_16x1024", 16, 1024, False, 50)):
    tokens, mask = shape(N, T, hs)
    fns = paths(tokens, mask)
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            times[k].append(clock(fn, iters))
    r = dict(N=N, T=T, scored_rows=int(mask[:, 1:].sum()), iters=iters)
    for k, v in times.items():
        r[k + "_ms"] = statistics.median(v)
        r[k + "_ms_min_max"] = [min(v), max(v)]
        r[k + "_peak_mb"] = peak_mb(fns[k])
    res[name] = r
print(json.dumps(res, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
