cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
out=${CARA_OUT:-bench_out}   # where the runs' files go
mkdir -p $out
timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d $out/tl -- python3 bench.py --full --no-cpu-baseline --no-info-legs --steps 8 --warmup 3 > $out/tl.log 2>&1 && python3 tools/timeline.py $out/tl --steps 5 > $out/tl.txt 2>&1; tail -1 $out/tl.log | cut -c1-200; cat $out/tl.txt; rm -rf $out/tl
