"""Int8 KV cache against the bf16 cache: graph-replayed milliseconds per token.  GPT-2 124M and
GPT-2 XL at vocab 50304, bf16, random weights.

    python tools/kv8_decode_ms.py out.json [--sizes gpt2,gpt2-xl] [--rows 1,64,beam] [--quick]

Per configuration (model size x rows x cached length x weights) two sessions over the same model
and prompt, kv_cache=None (the default path, untouched by the int8 cache) and kv_cache="int8",
timed alternately in one process:
  rows     1 and 64 sequences through GraphedGenerate (greedy), and 8 items x 8 beams through
           GraphedBeamSearch (eos=None: every step runs);
  length   a prompt of 96 or 864 tokens and N_NEW = 64 new ones: the cache holds about 128 or
           about 896 positions on average over the timed tokens;
  weights  bf16, and a gvl.quant.quantize_decoder snapshot (weights="int8").
ms per token = (a call with N_NEW + 1 new tokens - a call with 1 new token) / N_NEW: both run the
same eager prefill and first token choice, so the difference is N_NEW graph replays.  Each call
is a host clock around work that ends in a device synchronise; after WARM warm-up calls (the
capture among them) the four calls alternate ROUNDS times and the medians are used.  Also
reported: the cache bytes of both formats (gvl.decode.kv_cache_bytes).  The result is written
after every configuration, so a run that is cut short keeps what it measured."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--sizes", default="gpt2,gpt2-xl")
ap.add_argument("--rows", default="1,64,beam")
ap.add_argument("--quick", action="store_true", help="one round, 16 new tokens")
cli = ap.parse_args()

WARM, ROUNDS = (1, 1) if cli.quick else (1, 3)
N_NEW = 16 if cli.quick else 64
PROMPTS = {"~128": 96, "~896": 864}
BEAM = (8, 8)  # items x beams

import torch  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "gpt2-vision-language_amd"))
import gvl.gpt2 as g2  # noqa: E402
from gvl import decode, quant  # noqa: E402

dev = torch.device("cuda:0")
BF = torch.bfloat16


def write(res):
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, "w") as f:
            json.dump(res, f, indent=1)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def session(model, rows, P, w, kv):
    kw = dict(weights=w, kv_cache=kv)
    if rows == "beam":
        return decode.GraphedBeamSearch(model, P, N_NEW + 1, num_beams=BEAM[1], eos=None, **kw)
    return decode.GraphedGenerate(model, P, N_NEW + 1, greedy=True, **kw)


def one(model, cfg, rows, P, w):
    B = BEAM[0] if rows == "beam" else int(rows)
    g = torch.Generator().manual_seed(P + B)
    prompt = torch.randint(0, 50257, (B, P), generator=g).to(dev)
    ses, fns = {}, {}
    for kv in ("bf16", "int8"):
        ses[kv] = s = session(model, rows, P, w, None if kv == "bf16" else "int8")
        fns[f"{kv}/long"] = lambda s=s: s(prompt, N_NEW + 1)
        fns[f"{kv}/short"] = lambda s=s: s(prompt, 1)
    try:
        for fn in fns.values():
            for _ in range(WARM):
                fn()
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                times[k].append(clock(fn))
    finally:
        for s in ses.values():
            s.close()
    r = {}
    for kv in ("bf16", "int8"):
        long_, short = (statistics.median(times[f"{kv}/{n}"]) for n in ("long", "short"))
        r[kv] = dict(ms_per_token=(long_ - short) / N_NEW, ms_long=times[f"{kv}/long"],
                     ms_short=times[f"{kv}/short"])
    r["int8_over_bf16"] = r["int8"]["ms_per_token"] / r["bf16"]["ms_per_token"]
    R = B * (BEAM[1] if rows == "beam" else 1)
    Tmax = P + N_NEW + 1
    r["cache_bytes"] = dict(bf16=decode.kv_cache_bytes(cfg, R, Tmax),
                            int8=decode.kv_cache_bytes(cfg, R, Tmax, kv_cache="int8"))
    return r


res = dict(models="GPT-2 sizes at vocab 50304, bf16, random weights", n_new=N_NEW, warm=WARM,
           rounds=ROUNDS, prompts=PROMPTS, beam=dict(items=BEAM[0], beams=BEAM[1]),
           device=torch.cuda.get_device_name(0),
           method="graph-replayed ms per token = (call with n_new + 1 tokens - call with 1) / "
                  "n_new, medians of alternated rounds; kv_cache=None is the default path",
           results={})
for size in cli.sizes.split(","):
    torch.manual_seed(0)
    cfg = g2.GPTConfig.for_size(size, vocab_size=50304)
    with torch.device(dev):
        model = g2.GPT(cfg)
    model = model.to(BF).eval()
    qd = quant.quantize_decoder(model)
    for rows in cli.rows.split(","):
        for name, P in PROMPTS.items():
            for wname, w in (("bf16", None), ("int8", qd)):
                key = f"{size}_rows{rows}_len{name}_w{wname}"
                res["results"][key] = r = one(model, cfg, rows, P, w)
                print(f"{key}: bf16 cache {r['bf16']['ms_per_token']:.3f} ms/token, int8 cache "
                      f"{r['int8']['ms_per_token']:.3f} ({r['int8_over_bf16']:.3f}x)", flush=True)
                write(res)
                torch.cuda.empty_cache()
    del model, qd
    torch.cuda.empty_cache()
print(json.dumps({k: v["int8_over_bf16"] for k, v in res["results"].items()}, indent=1))
write(res)
