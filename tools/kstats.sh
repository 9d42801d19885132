#!/bin/bash
# tools/kstats.sh [bench args]  -- rocprofv3 kernel statistics (top lines) of one bench batch
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
O=${GBP_OUT:-out}/kstats; rm -rf $O; mkdir -p $O
timeout 300 rocprofv3 --kernel-trace --stats -f csv -d $O -o run -- python bench.py --full --no-cpu-baseline --single-batch "$@" > $O/bench.log 2>&1
head -4 $(find $O -name "*kernel_stats.csv" | head -1) | cut -c1-140
