export TMPDIR=/tmp
out=${CARA_OUT:-bench_out}   # where the runs' files go
mkdir -p $out
for gmv in 1 8; do
CARA_GEMM_GROUPM=$gmv timeout -k 10 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $out/pmc_fetch_g$gmv --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-info-legs > $out/pmc_fetch_g$gmv.log 2>&1 || echo pass failed
done
