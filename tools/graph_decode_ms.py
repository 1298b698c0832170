"""Milliseconds per token of eager against graph-replayed decoding at GPT-2 124M (vocab 50304,
bf16, random weights), B in {1, 8}, a prompt of 64 (a block of 16 tokens four times):
    generate      greedy, 128 new tokens       gvl.decode.generate
    beam_search   K = 4, 24 new tokens         gvl.decode.beam_search
each three ways:
    eager         the call as it always was
    graphed       one GraphedGenerate / GraphedBeamSearch session called again and again (the
                  capture falls into the warm-up calls; captures and replays are reported)
    graph_call    generate / beam_search(graph=True): a session per call, its capture included
    python tools/graph_decode_ms.py [out.json] [--eager-only] [--tree DIR]
    python tools/graph_decode_ms.py out.json --ab PARENT_DIR
--eager-only times the eager paths alone and --tree imports gvl from another checkout (with its
own built library): the baseline of a tree that has no graphed path.  --ab does the whole
comparison: PARENT_DIR eager-only and this tree, in fresh processes one after the other, twice
each, alternating; out.json then holds every run, the spread of the parent's repeated runs per
configuration (max / min - 1 of its medians), and per configuration whether this tree's eager
path sits inside that spread and whether a graphed path beats the parent by more than it.
Each figure is a host clock around ITERS calls that ends in a device synchronise; the paths are
timed alternately ROUNDS times after WARM warm-up calls each, and the median is reported with
all rounds.  ms per token = call time / new tokens, the prefill included."""
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
ap.add_argument("--eager-only", action="store_true")
ap.add_argument("--tree", default=HERE)
ap.add_argument("--ab", metavar="PARENT_DIR")
cli = ap.parse_args()

WARM, ROUNDS, ITERS = 2, 5, 3
GEN_NEW, BEAM_NEW, BEAMS = 128, 24, 4
CONFIGS = [f"{what}_B{B}" for what in ("generate", "beam_search") for B in (1, 8)]


def write(res):
    print(json.dumps(res, indent=1))
    if cli.out:
        os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
        with open(cli.out, "w") as f:
            json.dump(res, f, indent=1)


def ab(parent):
    """Fresh processes, one at a time: parent, this tree, parent, this tree."""
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(2):
            for name, extra in (("parent", ["--eager-only", "--tree", parent]), ("this", [])):
                path = os.path.join(tmp, f"{name}{i}.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), path] + extra,
                               check=True, stdout=subprocess.DEVNULL, timeout=600)
                with open(path) as f:
                    runs.append(dict(tree=name, run=i, **json.load(f)))
    summary = {}
    for c in CONFIGS:
        med = lambda tree, path: [r[c][path]["ms_per_call"] for r in runs
                                  if r["tree"] == tree and path in r[c]]
        base = med("parent", "eager")
        spread = max(base) / min(base) - 1.0
        s = dict(parent_eager_ms_per_call=base, parent_spread=spread,
                 this_eager_ms_per_call=med("this", "eager"))
        s["this_eager_within_parent_spread"] = max(s["this_eager_ms_per_call"]) <= max(base) * (1 + spread)
        for path in ("graphed", "graph_call"):
            t = med("this", path)
            s[f"{path}_ms_per_call"] = t
            s[f"{path}_speedup_vs_parent"] = statistics.median(base) / statistics.median(t)
            s[f"{path}_faster_beyond_spread"] = max(t) * (1 + spread) < min(base)
        summary[c] = s
    write(dict(method="parent eager-only and this tree in fresh processes, alternating, twice "
                      "each; spread = max / min - 1 of the parent's medians", summary=summary,
               runs=runs))


if cli.ab:
    ab(cli.ab)
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, os.path.join(cli.tree, "gpt2-vision-language_amd"))
import gvl.gpt2 as g2  # noqa: E402
from gvl import decode  # noqa: E402

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


res = dict(model="GPT-2 124M, vocab 50304, bf16, random weights", prompt_len=64, warm=WARM,
           rounds=ROUNDS, iters=ITERS, tree_path=os.path.abspath(cli.tree),
           device=torch.cuda.get_device_name(0))
for what, n_new in (("generate", GEN_NEW), ("beam_search", BEAM_NEW)):
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        prompt = torch.randint(0, 50257, (B, 16), generator=g).repeat(1, 4).to(dev)
        if what == "generate":
            eager = lambda **kw: decode.generate(model, prompt, n_new, greedy=True, **kw)
            session = lambda: decode.GraphedGenerate(model, 64, n_new, greedy=True)
        else:
            eager = lambda **kw: decode.beam_search(model, prompt, n_new, num_beams=BEAMS, **kw)
            session = lambda: decode.GraphedBeamSearch(model, 64, n_new, num_beams=BEAMS)
        fns, ses = dict(eager=eager), None
        if not cli.eager_only:
            ses = session()
            fns["graphed"] = lambda: ses(prompt)
            fns["graph_call"] = lambda: eager(graph=True)
            same = lambda a, b: all(torch.equal(x, y) for x, y in zip(
                *((v if isinstance(v, tuple) else (v,)) for v in (a, b))))
            want = eager()
            equal = dict(graphed=same(ses(prompt), want), graph_call=same(eager(graph=True), want))
        for fn in fns.values():
            for _ in range(WARM):
                fn()
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                times[k].append(clock(fn, ITERS))
        r = dict(B=B, n_new=n_new)
        for k, v in times.items():
            call = statistics.median(v)
            r[k] = dict(ms_per_call=call, ms_per_call_rounds=v, ms_per_token=call / n_new)
            if k != "eager":
                r[k]["speedup_vs_eager"] = r["eager"]["ms_per_call"] / call
                r[k]["equal_eager"] = equal[k]
        if ses is not None:
            r["graphed"].update(ses.stats, calls=1 + WARM + ROUNDS * ITERS)
            ses.close()
        res[f"{what}_B{B}"] = r
write(res)
