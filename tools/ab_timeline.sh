#!/bin/bash
# Idle-gap analysis (tools/timeline.py) of the bench under two environments.
# Usage (GPU box): bash tools/ab_timeline.sh "ENV_A=.." "ENV_B=.."
set -o pipefail
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT" || exit 1
out=${CARA_OUT:-bench_out}   # where the runs' files go
mkdir -p $out
i=0
for envs in "$1" "$2" "$1" "$2"; do
  i=$((i+1))
  ( export $envs; timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d $out/abt_$i -- python3 bench.py --full --no-cpu-baseline --no-info-legs --steps 10 --warmup 3 > $out/abt_$i.log 2>&1 ) || exit 1
  echo "== $envs: $(grep -h '^{"metric"' $out/abt_$i.log | tail -1 | python3 -c 'import sys,json; d=json.loads(sys.stdin.read()); print(d["ms_per_step"], "ms/step, forward only", d["config"]["forward_only_ms"])')"
  python3 tools/timeline.py $out/abt_$i --steps 8 > $out/abt_$i.txt 2>&1; sed -n 1,8p $out/abt_$i.txt
  rm -rf $out/abt_$i
done
