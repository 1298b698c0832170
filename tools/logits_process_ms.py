"""Milliseconds per call of gvl_logits_process next to gvl_beam_step on the same logits: R = 40
rows (10 items x 4 beams), V = 50257 (row stride 50304), L = 30 tokens per row (8 prompt + 22
generated, read through a beam table), every control on.
    python tools/logits_process_ms.py [out.json]
Each figure is device events around ITERS back-to-back calls on one stream (so it includes the
launch overhead, like beam_step_call_ms of tools/beam_step_ms.py); the two are timed alternately
ROUNDS times and the median is reported with the spread."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "gpt2-vision-language_amd"))
from gvl import kernels as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
B, Kb, V, LD, P, N_HIST, T0 = 10, 4, 50257, 50304, 8, 22, 40
R, ITERS, ROUNDS = B * Kb, 2000, 5
dev = torch.device("cuda:0")

torch.manual_seed(0)
fresh = (torch.randn(R, LD, device=dev) * 2).to(torch.bfloat16)
logits = fresh.clone()[:, :V]
hist = torch.randint(0, V, (N_HIST, R), device=dev)
prompt = torch.randint(0, V, (B, P), device=dev)
item = torch.arange(R, device=dev) // Kb * Kb
src = (item[:, None] + torch.randint(0, Kb, (R, T0 + N_HIST + 1), device=dev)).to(torch.int32)
bad = torch.tensor([198, 628], dtype=torch.int32, device=dev)
score = torch.randn(R, device=dev) - 3
flen = torch.zeros(R, dtype=torch.int32, device=dev)
len_norm = torch.ones(N_HIST + 2, device=dev)
outs = K.beam_step(logits, score, flen, len_norm, src, Kb, N_HIST, 50256, T0)


def process():
    K.logits_process(logits, hist, N_HIST, src=src, t0=T0, prompt=prompt, rows_per_item=Kb,
                     repetition_penalty=1.2, no_repeat_ngram_size=3, eos=50256, ban_eos=True,
                     bad_tokens=bad, flen=flen)


def step():
    K.beam_step(logits, score, flen, len_norm, src, Kb, N_HIST, 50256, T0, out=outs)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


for fn in (process, step):
    for _ in range(20):
        fn()
times = {"logits_process_call_ms": [], "beam_step_call_ms": []}
for _ in range(ROUNDS):
    times["logits_process_call_ms"].append(events(process))
    times["beam_step_call_ms"].append(events(step))
res = dict(rows=R, V=V, ld=LD, L=P + N_HIST, iters=ITERS, rounds=ROUNDS,
           device=torch.cuda.get_device_name(0))
for k, v in times.items():
    res[k] = statistics.median(v)
    res[k + "_min_max"] = [min(v), max(v)]
print(json.dumps(res, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
