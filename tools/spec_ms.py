"""Milliseconds per token of KV-cached decoding at GPT-2 124M (vocab 50304, bf16, random
weights), greedy, 128 new tokens after a prompt of 64 (a block of 16 tokens four times), B in
{1, 8}, three ways:
    generate:        gvl.decode.generate                        one token per decoder pass
    spec_lookup:     speculative_generate(draft_len=4, ngram=3)  prompt-lookup draft
    spec_perfect:    speculative_generate(draft_ids=generate's own output)  every guess right
    python tools/spec_ms.py [out.json] [--generate-only] [--tree DIR]
spec_perfect is the ceiling: passes = ceil(127 / 5) = 26, and its time per pass against
generate's time per token says what 5 rows per sequence cost.  --generate-only times generate
alone, and --tree imports gvl from another checkout (with its own built library): together the
A/B of generate against another commit on the same box.
Each figure is a host clock around ITERS calls that ends in a device synchronise; the paths are
timed alternately ROUNDS times after WARM warm-up calls each, and the median is reported with
the spread.  ms per token = call time / 128, the prefill included in all three."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--generate-only", action="store_true")
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
cli = ap.parse_args()
only_generate, tree, out_path = cli.generate_only, cli.tree, cli.out
sys.path.insert(0, os.path.join(tree, "gpt2-vision-language_amd"))
import gvl.gpt2 as g2  # noqa: E402
from gvl import decode  # noqa: E402

WARM, ROUNDS, ITERS = 2, 5, 3
N_NEW, DRAFT_LEN, NGRAM = 128, 4, 3
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = g2.GPT(g2.GPTConfig(vocab_size=50304)).to(dev).to(torch.bfloat16).eval()


def clock(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


res = dict(model="GPT-2 124M, vocab 50304, bf16, random weights", n_new=N_NEW, warm=WARM,
           rounds=ROUNDS, iters=ITERS, draft_len=DRAFT_LEN, ngram=NGRAM,
           tree=os.path.abspath(tree), device=torch.cuda.get_device_name(0))
for B in (1, 8):
    g = torch.Generator().manual_seed(B)
    prompt = torch.randint(0, 50257, (B, 16), generator=g).repeat(1, 4).to(dev)
    own = decode.generate(model, prompt, N_NEW, greedy=True)
    fns = dict(generate=lambda: decode.generate(model, prompt, N_NEW, greedy=True))
    stats = {}
    if not only_generate:
        spec = lambda **kw: decode.speculative_generate(model, prompt, N_NEW, greedy=True,
                                                        draft_len=DRAFT_LEN, ngram=NGRAM,
                                                        return_stats=True, **kw)
        fns["spec_lookup"] = lambda: spec()
        fns["spec_perfect"] = lambda: spec(draft_ids=own)
        for k in ("spec_lookup", "spec_perfect"):
            ids, st = fns[k]()
            drafted, accepted = int(st["drafted"].sum()), int(st["accepted"].sum())
            stats[k] = dict(passes=st["steps"] - 1, drafted=drafted, accepted=accepted,
                            acceptance=accepted / max(drafted, 1),
                            tokens_equal_generate=int((ids == own).sum()), tokens=B * N_NEW)
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            times[k].append(clock(fn, ITERS))
    r = dict(B=B, prompt_len=64)
    for k, v in times.items():
        call = statistics.median(v)
        r[k] = dict(ms_per_call=call, ms_per_call_min_max=[min(v), max(v)],
                    ms_per_token=call / N_NEW, **stats.get(k, {}))
        if k != "generate":
            r[k]["ms_per_pass"] = call / (r[k]["passes"] + 1)  # the prefill counted as a pass
            r[k]["speedup_vs_generate"] = r["generate"]["ms_per_call"] / call
    if not only_generate:  # (more passes: a near-tie that the 5-row pass rounds the other way)
        r["spec_perfect"]["passes_if_every_guess_is_right"] = math.ceil((N_NEW - 1) / (DRAFT_LEN + 1))
    res[f"B{B}"] = r
print(json.dumps(res, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
