#!/bin/bash
# One round's evidence: the default bench line, the same command under rocprofv3 --kernel-trace --stats, and the
# idle-gap analysis of that trace.  Usage (on the GPU box): bash tools/profile_round.sh r01_h
set -o pipefail
tag=${1:-rXX}
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
out=${CARA_OUT:-bench_out}   # where the runs' files go
mkdir -p $out
timeout -k 10 400 python3 bench.py --full > $out/${tag}_bench_default_run.json 2> $out/${tag}_bench.err || exit 1
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_${tag} -- python3 bench.py --full --no-cpu-baseline --no-info-legs --no-precision-matched \
  > $out/${tag}_bench_under_rocprof.json 2> $out/${tag}_rocprof.err || exit 1
f=$(find $out/prof_${tag} -name '*kernel_stats.csv' | head -1)
cp "$f" $out/${tag}_kernel_stats_final.csv
python3 tools/timeline.py $out/prof_${tag} --steps 10 --skip-last 3 > $out/${tag}_timeline.txt 2>&1
rm -rf $out/prof_${tag}
tail -c 400 $out/${tag}_bench_default_run.json; echo; head -5 $out/${tag}_timeline.txt
