"""Ties the reported GEMM kernel names to what the hardware ran.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_route_trace.py > names.txt
  python tools/gemm_route_trace.py --check DIR names.txt

The first form launches every model row of tools/gemm_routes.py (the shapes of
tools/gemm_shapes.py with the epilogues the models run on them) once under the default routing,
through gvl.kernels.gemm with a KernelTimer, and prints the name the timer recorded per launch
(and the route table's name for the row).  The second compares, in launch order, those names
with the GEMM kernels of the trace (shortened as tools/pmc_traffic.py does; the split-K reduce
kernel that follows a slab split is skipped)."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_routes as R  # noqa: E402


def launch_all():
    import json

    import torch
    from gvl import kernels as K

    table = json.load(open(os.path.join(R.ROOT, "tests", "data", "gemm_routes.json")))
    want = R.cells(table)
    dev = torch.device("cuda:0")
    timer = K.KernelTimer()
    K.set_kernel_timer(timer)
    bf = torch.bfloat16
    for M, N, Kd, am, bm, epi in R._model_rows():
        A = torch.empty((Kd, M) if am else (M, Kd), dtype=bf, device=dev)
        B = torch.empty((Kd, N) if bm else (N, Kd), dtype=bf, device=dev)
        out = torch.empty(M, N, dtype=torch.float32 if epi == "c_fp32" else bf, device=dev)
        aux = (lambda: torch.empty(M, N, dtype=bf, device=dev))
        bias = torch.empty(N, dtype=bf, device=dev)
        kw = {"plain": {}, "c_fp32": {}, "bias": dict(bias=bias),
              "bias_res": dict(bias=bias, residual=aux()), "res_inplace": dict(residual=out),
              "drop_res": dict(bias=bias, residual=aux(), drop_p=0.1, seed=1),
              "gate_res": dict(bias=bias, residual=aux(), gate=bias[:1], pre_out=aux()),
              "qgelu": dict(bias=bias, act=5)}.get(epi)
        if kw is None and epi.startswith("bias_act"):
            kw = dict(bias=bias, act={"bias_act1": 1, "bias_act2": 2, "bias_act_d": 3, "bias_act_erf_d": 4}[epi],
                      pre_out=aux())
        elif kw is None:
            kw = dict(dact={"dact": 1, "dact_erf": 2, "mul": 3}[epi], pre_in=aux())
        K.gemm(A, B, a_mn=bool(am), b_mn=bool(bm), out=out, **kw)
        torch.cuda.synchronize()
        name = timer.records[-1][0]
        ok = name == want[(M, N, Kd, am, bm, epi, "3:-1", "ws")]
        print(f"{M} {N} {Kd} {am} {bm} {epi}\t{name}\t{'table' if ok else 'NOT-THE-TABLE'}", flush=True)
        del A, B, out, kw, bias
    K.set_kernel_timer(None)


def check(trace_dir, names_file):
    from pmc_traffic import short
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), short(r["Kernel_Name"])) for r in csv.DictReader(fh)]
    ran = [n for _, n in sorted(rows) if n.startswith("gemm_") and not n.startswith("gemm_splitk_reduce")]
    said = [ln.rstrip("\n").split("\t") for ln in open(names_file) if "\t" in ln]
    bad = 0
    for i, s in enumerate(said):
        got = ran[i] if i < len(ran) else "(none)"
        flag = "ok" if got == s[1] and s[2] == "table" else "MISMATCH"
        bad += flag != "ok"
        print(f"{s[0]:44s} reported {s[1]:52s} traced {got:52s} {flag}")
    print(f"{len(said)} launches reported, {len(ran)} GEMM kernels traced, {bad} mismatches")
    return 1 if bad or len(said) != len(ran) else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        sys.exit(check(sys.argv[2], sys.argv[3]))
    launch_all()
