#!/bin/bash
# Whole bench line + rocprofv3 kernel trace/stats of the bench step (outputs under $OUT, default prof_out/).
#   [OUT=<dir>] bash tools/prof_bench.sh <tag>
set -o pipefail
tag=${1:-run}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
O=${OUT:-prof_out}
mkdir -p "$O"
timeout -k 10 240 python3 -u bench.py --full > "$O/bench_$tag.json" 2> "$O/bench_$tag.err" || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_$tag" -o run -- \
  python3 bench.py --steps 10 --warmup 3 > "$O/bench_${tag}_underprof.json" 2> "$O/prof_$tag.err"
