#!/bin/bash
# Ordered kernel list of one training step (rocprofv3 --kernel-trace of a short bench run): bash tools/run_list.sh TAG
set -o pipefail
tag=${1:-list}
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
out=${CARA_OUT:-bench_out}   # where the runs' files go
mkdir -p $out
timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d $out/prof_${tag} -- python3 bench.py --full --steps 8 --warmup 3 --no-cpu-baseline --no-info-legs \
  > $out/${tag}_bench.json 2> $out/${tag}_rocprof.err || exit 1
python3 tools/timeline.py $out/prof_${tag} --steps 4 --skip-last 3 --list > $out/${tag}_steplist.txt 2>&1
rm -rf $out/prof_${tag}
head -3 $out/${tag}_steplist.txt
