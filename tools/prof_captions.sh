#!/bin/bash
# rocprofv3 kernel-trace + stats of the linear and cross-att caption steps (bench workloads).
# Output goes to $GVL_OUT (default: prof_out/ in the repository root).
set -e
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}; cd "$R"; TAG=${1:-x}
O=${GVL_OUT:-$R/prof_out}; mkdir -p "$O"
for w in cross linear; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_${w}_$TAG" -o $w -- \
    python bench.py --full --workload $w --steps 10 --warmup 3 --no-cpu-baseline > "$O/prof_${w}_$TAG.json" 2> "$O/prof_${w}_$TAG.err"
done
