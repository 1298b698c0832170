"""Milliseconds per decode step: beam_search (Q-Former caption model, B items x K beams) next to
generate at B*K rows, and gvl_beam_step alone on the same logits shape.
    python tools/beam_step_ms.py [out.json] [B=64] [K=4]
Per-step time = (time of n_long new tokens - time of n_short) / (n_long - n_short), each a host
clock around a run that ends in a device synchronise, so the prefill cancels out."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "gpt2-vision-language_amd"))
import gvl.caption as cap  # noqa: E402
import gvl.gpt2 as g2  # noqa: E402
from gvl import kernels as K  # noqa: E402
from gvl.decode import beam_search, generate  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
Kb = int(sys.argv[3]) if len(sys.argv) > 3 else 4
R, N_SHORT, N_LONG, REPS = B * Kb, 8, 40, 3
dev = torch.device("cuda:0")

torch.manual_seed(0)
lm = cap.GPT_previous(g2.GPTConfig(vocab_size=50304, block_size=1024))
model = cap.QFormerCaption(enc_dim=768, lm=lm, m_vis_tokens=32).to(dev).to(torch.bfloat16).eval()
z = torch.nn.functional.normalize(torch.randn(R, 33, 768, device=dev), dim=-1)
prompt = torch.randint(0, 50257, (R, 8), device=dev)


def wall(fn):
    fn()  # warm-up of every shape in the window
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def per_step(run):
    return (wall(lambda: run(N_LONG)) - wall(lambda: run(N_SHORT))) / (N_LONG - N_SHORT)


res = dict(B=B, K=Kb, rows=R, n_short=N_SHORT, n_long=N_LONG, reps=REPS, device=torch.cuda.get_device_name(0))
res["generate_greedy_ms_per_step"] = per_step(lambda n: generate(model, prompt, n, z=z, greedy=True))
res["beam_search_ms_per_step"] = per_step(
    lambda n: beam_search(model, prompt[::Kb], n, z=z[::Kb], num_beams=Kb, eos=None))
res["beam_search_eos_check_ms_per_step"] = per_step(  # eos set: one host sync per step
    lambda n: beam_search(model, prompt[::Kb], n, z=z[::Kb], num_beams=Kb, eos=50256))

# the two launches of gvl_beam_step alone, and gvl_sample (greedy) on the same rows
V, T0, STEP = 50304, 40, 20
logits = (torch.randn(R, V, device=dev) * 2).to(torch.bfloat16)
score = torch.randn(R, device=dev) - 3
flen = torch.zeros(R, dtype=torch.int32, device=dev)
len_norm = torch.ones(STEP + 2, device=dev)
src = torch.zeros(R, T0 + STEP + 1, dtype=torch.int32, device=dev)
outs = K.beam_step(logits, score, flen, len_norm, src, Kb, STEP, 50256, T0)
u = torch.zeros(R, device=dev)


def events(fn, iters=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


res["beam_step_call_ms"] = events(
    lambda: K.beam_step(logits, score, flen, len_norm, src, Kb, STEP, 50256, T0, out=outs))
res["sample_greedy_call_ms"] = events(lambda: K.sample(logits, u, 1.0, 1, 1.0))
print(json.dumps(res, indent=1))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
