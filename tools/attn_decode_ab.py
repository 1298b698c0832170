"""A/B of the single-query decode attention kernels against another commit: what the five
gvl.kernels wrappers (attn_decode, attn_decode_beam, attn_decode_ragged without and with src,
attn_decode_multi) compute, as digests, and how long one launch takes.
    python tools/attn_decode_ab.py [out.json] [--tree DIR]
--tree imports gvl from another checkout (with its own built library); run the tool once per
tree on the same box and compare the two outputs.
Digests: a SHA-256 over the output bytes of every case (for multi, one over the cache bytes
too) on seeded bf16 inputs, B = 3, H = 2.  Tk in {1, 31, 33, 255, 257, 1000, 4096}: 31 / 33
straddle the 32-row value sweep, 255 / 257 the 256-thread score stride, 4096 is the top of the
score array.  Beam: src a random permutation of the rows per column.  Ragged: gap_hi = Tk with
rows (empty, one column, the whole range), and gap_hi = min(Tk, 300) with rows (from gap_hi / 2,
i.e. across 256 from Tk = 257 on; empty; one column), each without and with src.  Multi: Q in {1, 5, 8}, kv_len = (0, 31, 255),
Tmax = 255 + Q.  Equal digests in both trees = the same bits.
Times: B = 8, H = 12, Tk in {64, 1024, 4096} (multi: Q = 5 at kv_len = Tk - 5); a host clock
around ITERS launches that ends in a device synchronise, ROUNDS times after WARM launches;
microseconds per launch, the median with min and max."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
cli = ap.parse_args()
sys.path.insert(0, os.path.join(cli.tree, "gpt2-vision-language_amd"))
import gvl.kernels as Kn  # noqa: E402

WARM, ROUNDS, ITERS = 20, 5, 200
TKS = (1, 31, 33, 255, 257, 1000, 4096)
dev = torch.device("cuda:0")
BF = torch.bfloat16


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def rand(g, *shape):
    return torch.randn(*shape, generator=g).to(BF).to(dev)


def cache_case(g, B, H, Tk):
    """q [B, C] and a packed [B, Tk, 3C] cache (its k and v slices are the strided views)."""
    C = H * 64
    q, cache = rand(g, B, C), rand(g, B, Tk, 3 * C)
    src = torch.stack([torch.randperm(B, generator=g) for _ in range(Tk)], 1).to(torch.int32)
    return q, cache[:, :, C:2 * C], cache[:, :, 2 * C:], src.contiguous().to(dev)


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=dev)


digests = {}
B, H = 3, 2
for Tk in TKS:
    g = torch.Generator().manual_seed(Tk)
    q, k, v, src = cache_case(g, B, H, Tk)
    digests[f"plain Tk={Tk}"] = sha(Kn.attn_decode(q, k, v, H))
    digests[f"beam Tk={Tk}"] = sha(Kn.attn_decode_beam(q, k, v, H, src))
    hi = min(Tk, 300)
    for name, lo, gap_hi in (("end", [Tk, Tk - 1, 0], Tk),
                             ("mid", [hi // 2, hi, hi - 1], hi)):
        for s in (None, src):
            o = Kn.attn_decode_ragged(q, k, v, H, i32(lo), gap_hi, src=s)
            digests[f"ragged{'' if s is None else '+src'} Tk={Tk} gaps={name}"] = sha(o)
kv_len = [0, 31, 255]
for Q in (1, 5, 8):
    g = torch.Generator().manual_seed(100 + Q)
    C = H * 64
    qkv, cache = rand(g, B, Q, 3 * C), rand(g, B, max(kv_len) + Q, 3 * C)
    o = Kn.attn_decode_multi(qkv, cache, i32(kv_len), H)
    digests[f"multi Q={Q} out"] = sha(o)
    digests[f"multi Q={Q} cache"] = sha(cache)


def clock(fn):
    for _ in range(WARM):
        fn()
    us = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / ITERS)
    return dict(us_per_launch=statistics.median(us), us_min_max=[min(us), max(us)])


times = {}
B, H, Q = 8, 12, 5
for Tk in (64, 1024, 4096):
    g = torch.Generator().manual_seed(Tk)
    q, k, v, src = cache_case(g, B, H, Tk)
    out = torch.empty(B, H * 64, dtype=BF, device=dev)
    lo, hi = i32([Tk // 2 - 3] * B), Tk // 2
    qkv, cache = rand(g, B, Q, 3 * H * 64), rand(g, B, Tk, 3 * H * 64)
    lens, mout = i32([Tk - Q] * B), torch.empty(B * Q, H * 64, dtype=BF, device=dev)
    for name, fn in (
            ("plain", lambda: Kn.attn_decode(q, k, v, H, out=out)),
            ("beam", lambda: Kn.attn_decode_beam(q, k, v, H, src, out=out)),
            ("ragged", lambda: Kn.attn_decode_ragged(q, k, v, H, lo, hi, out=out)),
            ("ragged+src", lambda: Kn.attn_decode_ragged(q, k, v, H, lo, hi, src=src, out=out)),
            ("multi", lambda: Kn.attn_decode_multi(qkv, cache, lens, H, out=mout))):
        times[f"{name} Tk={Tk}"] = clock(fn)

res = dict(tree=os.path.abspath(cli.tree), device=torch.cuda.get_device_name(0), warm=WARM,
           rounds=ROUNDS, iters=ITERS, digests=digests, times=times)
print(json.dumps(res, indent=1))
if cli.out:
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as f:
        json.dump(res, f, indent=1)
