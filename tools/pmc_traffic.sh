cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
# HBM traffic of the bracketed kernel sites (bench.py roofline.traffic reads profiles/pmc_traffic_by_site.json):
# FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 --pmc passes (TCC slots), kernel-trace only.
export TMPDIR=/tmp
out=${CARA_OUT:-bench_out}   # where the runs' files go
mkdir -p $out
timeout -k 10 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $out/pmc_fetch --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-info-legs --no-precision-matched > $out/pmc_fetch.log 2>&1 || echo fetch pass failed
timeout -k 10 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $out/pmc_write --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-info-legs --no-precision-matched > $out/pmc_write.log 2>&1 || echo write pass failed
ls $out/pmc_fetch/*/ $out/pmc_write/*/ | head
python3 tools/pmc_sites.py $out/pmc_fetch $out/pmc_write $out/pmc_traffic_by_site.json > $out/pmc_traffic_summary.txt 2>&1; cat $out/pmc_traffic_summary.txt
rm -rf $out/pmc_fetch/*/*kernel_trace.csv $out/pmc_write/*/*kernel_trace.csv
