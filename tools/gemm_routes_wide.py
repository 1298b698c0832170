"""Route table of gvl_gemm at the GPT-2 large / XL widths (n_embd 1280 and 1600): every product
of an LM step at 16384, 64 and 8 token rows with the epilogues the model runs on it, asked of
gvl_gemm_kernel_name through tools/gemm_routes.py's query (no GPU), in that table's format.

  python tools/gemm_routes_wide.py                                  one line per cell
  python tools/gemm_routes_wide.py --json tests/data/gemm_routes_wide.json

tests/test_wide_cpu.py holds the built library to the committed table."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_routes as R  # noqa: E402

WIDTHS = (1280, 1600)
TOKENS = (16384, 64, 8)
VOCAB = 50304


def descriptors():
    """(M, N, K, a_mn, b_mn, epilogue): forward, dX and dW of c_attn, attn.c_proj, c_fc, mlp.c_proj
    and lm_head, with tools/gemm_routes.py's epilogues per leaf."""
    out = []
    for C in WIDTHS:
        for T in TOKENS:
            fwd = [("c_attn", 3 * C, C), ("attn.c_proj", C, C), ("c_fc", 4 * C, C),
                   ("mlp.c_proj", C, 4 * C), ("lm_head", VOCAB, C)]
            for leaf, N, K in fwd:
                if leaf in ("attn.c_proj", "mlp.c_proj"):
                    epis = ["bias", "bias_res", "drop_res"]
                elif leaf == "c_fc":
                    epis = ["bias", "bias_act1", "bias_act_d"]
                elif leaf == "lm_head":
                    epis = ["plain", "c_fp32"]
                else:
                    epis = ["plain", "bias"]
                out += [(T, N, K, 0, 0, e) for e in epis]
                # dX = dY @ W (MN-contiguous B), dW = dY^T @ X (both MN-contiguous, accumulated)
                out += [(T, K, N, 0, 1, e)
                        for e in ["plain", "res_inplace"] + (["dact"] if leaf == "mlp.c_proj" else [])]
                out += [(N, K, T, 1, 1, e) for e in ("plain", "res_inplace")]
    seen = set()
    return [r for r in out if not (r in seen or seen.add(r))]


def table(lib):
    names, rows = [], []

    def idx(n):
        if n not in names:
            names.append(n)
        return names.index(n)

    for r in descriptors():
        M, N, K, a, b, epi = r
        rows.append(dict(m=M, n=N, k=K, a_mn=a, b_mn=b, epi=epi,
                         ws=[idx(R.query(lib, s, r, True)) for s in R.SETTINGS],
                         nows=[idx(R.query(lib, s, r, False)) for s in R.SETTINGS]))
    return dict(settings=["%d:%d" % s for s in R.SETTINGS], names=names, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    t = table(R._lib.load(a.lib))
    if a.json:
        with open(a.json, "w") as f:
            f.write('{"settings": %s,\n "names": [\n  %s],\n "rows": [\n  %s]}\n' % (
                json.dumps(t["settings"]), ",\n  ".join(json.dumps(n) for n in t["names"]),
                ",\n  ".join(json.dumps(r) for r in t["rows"])))
        return
    for (M, N, K, am, bm, epi, s, w), name in R.cells(t).items():
        print(f"{s:6s} {M:6d} {N:6d} {K:6d} {am} {bm} {epi:14s} {w:4s} {name}")


if __name__ == "__main__":
    main()
