#!/bin/bash
# rocprofv3 kernel-trace + stats of the bench workloads (run on the GPU box via gpurun).
# Each profiled run has its own time limit; the script stops at the first failing step.
# Output goes to $GVL_OUT (default: prof_out/ in the repository root).
set -e
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"
TAG=${1:-r1}
O=${GVL_OUT:-$R/prof_out}; mkdir -p "$O"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_qf_$TAG" -o qf -- \
  python bench.py --full --workload qformer --steps 10 --warmup 3 --no-cpu-baseline > "$O/prof_qf_$TAG.json" 2> "$O/prof_qf_$TAG.err"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_lm_$TAG" -o lm -- \
  python bench.py --full --steps 1 --warmup 1 --no-secondary --no-cpu-baseline > "$O/prof_lm_$TAG.json" 2> "$O/prof_lm_$TAG.err"
