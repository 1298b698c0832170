"""Route table of gvl_gemm: which kernel instance every (tune setting, descriptor) gets, asked
of gvl_gemm_kernel_name on a host without a GPU (the query touches no device; the CU count
falls back to 256, the MI355X's).

  python tools/gemm_routes.py [--lib libgvl.so]            one line per (setting, descriptor, ws)
  python tools/gemm_routes.py --json tests/data/gemm_routes.json [--base old.json]

The JSON keeps one row per descriptor: the kernel per setting with ("ws") and without ("nows")
workspace + tickets, as indices into "names".  --base: a table of an earlier library; cells that
differ from it are listed under the row's "was" ("<setting>/<ws|nows>": the earlier name).
tests/test_gemm_routes_cpu.py holds the built library to the committed table."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "gpt2-vision-language_amd"))
from gvl import _lib  # noqa: E402

SETTINGS = [(3, -1), (3, 3), (3, 10), (3, 11), (3, 12), (3, 13), (2, -1), (2, 6), (2, 7), (2, 8),
            (2, 9), (1, -1), (0, -1)]
# dummy operands: distinct 16-byte aligned addresses, never dereferenced by the name query
A_, B_, C_, AUX, BIAS, GATE, WS, TK = (0x10000 * i for i in range(1, 9))

# epilogue name -> descriptor fields, as gvl.kernels.gemm fills them (ld's: N)
EPIS = {
    "plain": {},
    "bias": dict(bias=BIAS),
    "bias_res": dict(bias=BIAS, residual=AUX),
    "res_inplace": dict(residual=C_),
    "bias_act1": dict(bias=BIAS, act=1, pre_out=AUX),
    "bias_act2": dict(bias=BIAS, act=2, pre_out=AUX),
    "bias_act_d": dict(bias=BIAS, act=3, pre_out=AUX),
    "bias_act_erf_d": dict(bias=BIAS, act=4, pre_out=AUX),
    "dact": dict(dact=1, pre_in=AUX),
    "dact_erf": dict(dact=2, pre_in=AUX),
    "mul": dict(dact=3, pre_in=AUX),
    "drop_res": dict(bias=BIAS, residual=AUX, drop_p=0.1, seed=1),
    "gate_res": dict(bias=BIAS, residual=AUX, gate=GATE, pre_out=C_ + 0x8000),
    "qgelu": dict(bias=BIAS, act=5),
    "c_fp32": dict(c_fp32=1),
    "odd_ldc": dict(ldc_pad=4),  # ldc = N + 4: no 16-byte row stores
}


def _model_rows():
    """Every shape of tools/gemm_shapes.py with the epilogues the models run on it."""
    spec = importlib.util.spec_from_file_location("gemm_shapes", os.path.join(ROOT, "tools", "gemm_shapes.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    rows = []
    for name, M, N, K, am, bm in S.LM + S.QF + S.XA + S.BIG:
        leaf = name.split(".", 1)[-1] if name[:2] in ("q.", "x.") else name
        if am:
            epis = ["plain", "res_inplace"]
        elif bm:
            epis = ["plain", "res_inplace"] + (["dact", "dact_erf", "mul"] if "mlp.c_proj" in leaf else [])
        elif leaf in ("c_proj", "attn.c_proj", "mlp.c_proj"):
            epis = ["bias", "bias_res", "drop_res", "gate_res"]
        elif leaf == "c_fc":
            epis = ["bias", "bias_act1", "bias_act2", "bias_act_d", "bias_act_erf_d", "qgelu"]
        elif leaf == "lm_head":
            epis = ["plain", "c_fp32"]
        else:
            epis = ["plain", "bias"]
        rows += [(M, N, K, am, bm, e) for e in epis]
    return rows


def _test_rows():
    """Every (shape, epilogue) tests/test_gpu_kernels.py asks gvl_gemm_kernel_name about."""
    rows = []
    lay = [(0, 0), (0, 1), (1, 0), (1, 1)]
    rows += [(8192, 768, K, 0, b, e) for K, b, e in [(3072, 1, "plain"), (2304, 1, "plain"), (768, 1, "plain"),
                                                      (3072, 0, "bias_res"), (768, 0, "bias_res")]]
    rows += [(8064, 768, 3072, 0, 1, "plain"), (8064, 768, 3072, 0, 0, "plain"), (4096, 768, 3072, 0, 1, "plain")]
    for s in [(16384, 768, 3072), (16384, 768, 768), (1000, 776, 160), (4096, 2304, 96), (512, 768, 64),
              (16384, 3072, 768), (8064, 768, 3072), (8064, 768, 768)]:
        rows += [s + (0, b, e) for b in (0, 1) for e in ("plain", "bias_res")]
    for s in [(8064, 3072, 768), (7999, 2240, 768), (16384, 768, 3072), (4096, 2304, 768), (2048, 50304, 768)]:
        rows += [s + (0, 0, e) for e in ("plain", "bias", "bias_act_d")]
    rows += [(50304, 768, 4096, 1, 1, "res_inplace"), (16000, 768, 4096, 1, 1, "res_inplace")]
    for s in [(16384, 768, 768), (12000, 1536, 320), (16384, 2304, 32), (8064, 768, 3072), (8064, 768, 768),
              (7992, 768, 2304)]:
        rows += [s + ab + ("plain",) for ab in lay]
    for s in [(8064, 768, 3072), (8064, 768, 768), (7992, 768, 32)]:
        rows += [s + ab + (e,) for ab in lay
                 for e in ("plain", "bias_res", "res_inplace", "bias_act_d", "mul", "dact")]
    for s in [(8064, 768, 3072), (8064, 768, 2304), (7992, 776, 192), (16384, 768, 384), (300, 128, 192),
              (8064, 3072, 768), (3968, 768, 3072), (4096, 768, 768), (3970, 776, 192), (7992, 776, 384),
              (3970, 904, 768), (3968, 744, 768)]:
        rows += [s + (0, b, e) for b in (0, 1)
                 for e in ("plain", "bias", "bias_res", "res_inplace", "bias_act_d", "mul", "dact_erf")]
    rows += [s + (0, 0, "gate_res") for s in [(3968, 768, 768), (3970, 776, 192), (300, 128, 192), (8064, 768, 768)]]
    rows += [s + (0, 0, "drop_res") for s in [(4096, 768, 768), (4096, 3072, 768), (200, 136, 72), (4096, 768, 3072)]]
    rows += [s + (0, 0, "qgelu") for s in [(4096, 4096, 1024), (2056, 3072, 1024), (300, 136, 72)]]
    return rows


EXTRA = [
    (520, 264, 72, 0, 0, "plain"), (520, 264, 72, 1, 1, "plain"),  # K % 32 != 0: gemm_bf16_kernel
    (512, 512, 96, 0, 0, "bias"),                                 # K % 64 != 0: no gemm_lds_kernel
    (4096, 768, 768, 0, 0, "odd_ldc"), (16384, 3072, 768, 0, 1, "odd_ldc"),
    # the three routes the name query used to report wrongly
    (7680, 2048, 4096, 1, 0, "res_inplace"), (3456, 768, 768, 0, 0, "bias"), (256, 256, 256, 1, 1, "plain"),
]


def descriptors():
    seen, out = set(), []
    for r in _model_rows() + _test_rows() + EXTRA:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def fill(M, N, K, a_mn, b_mn, epi, ws):
    f = dict(EPIS[epi])
    d = _lib.GemmDesc()
    d.a, d.b, d.c = A_, B_, C_
    d.m, d.n, d.k = M, N, K
    d.lda, d.ldb, d.ldc = (M if a_mn else K), (N if b_mn else K), N + f.pop("ldc_pad", 0)
    d.a_mn, d.b_mn, d.alpha = a_mn, b_mn, 1.0
    d.ldp = N if ("pre_out" in f or "pre_in" in f) else 0
    d.ldr = N if "residual" in f else 0
    for k, v in f.items():
        setattr(d, k, v)
    if ws:
        d.workspace, d.workspace_bytes = WS, 64 << 20
        d.tickets, d.ticket_count = TK, 1 << 16
    return d


def query(lib, setting, row, ws):
    lib.gvl_gemm_tune(*setting)
    buf = C.create_string_buffer(128)
    try:
        lib.gvl_gemm_kernel_name(C.byref(fill(*row, ws)), buf, 128)
    finally:
        lib.gvl_gemm_tune(3, -1)
    return buf.value.decode()


def table(lib):
    names, rows = [], []

    def idx(n):
        if n not in names:
            names.append(n)
        return names.index(n)

    for r in descriptors():
        M, N, K, a, b, epi = r
        rows.append(dict(m=M, n=N, k=K, a_mn=a, b_mn=b, epi=epi,
                         ws=[idx(query(lib, s, r, True)) for s in SETTINGS],
                         nows=[idx(query(lib, s, r, False)) for s in SETTINGS]))
    return dict(settings=["%d:%d" % s for s in SETTINGS], names=names, rows=rows)


def cells(t):
    """{(descriptor, setting, ws|nows): name} of a table."""
    out = {}
    for r in t["rows"]:
        key = (r["m"], r["n"], r["k"], r["a_mn"], r["b_mn"], r["epi"])
        for w in ("ws", "nows"):
            for s, i in zip(t["settings"], r[w]):
                out[key + (s, w)] = t["names"][i]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--base", default=None)
    a = ap.parse_args()
    lib = _lib.load(a.lib)
    t = table(lib)
    if a.base:
        old = cells(json.load(open(a.base)))
        for r in t["rows"]:
            key = (r["m"], r["n"], r["k"], r["a_mn"], r["b_mn"], r["epi"])
            was = {f"{s}/{w}": old[key + (s, w)] for w in ("ws", "nows")
                   for s, i in zip(t["settings"], r[w]) if old[key + (s, w)] != t["names"][i]}
            if was:
                r["was"] = was
    if a.json:
        with open(a.json, "w") as f:
            f.write('{"settings": %s,\n "names": [\n  %s],\n "rows": [\n  %s]}\n' % (
                json.dumps(t["settings"]), ",\n  ".join(json.dumps(n) for n in t["names"]),
                ",\n  ".join(json.dumps(r) for r in t["rows"])))
        return
    for (M, N, K, am, bm, epi, s, w), name in cells(t).items():
        print(f"{s:6s} {M:6d} {N:6d} {K:6d} {am} {bm} {epi:14s} {w:4s} {name}")


if __name__ == "__main__":
    main()
