#!/bin/bash
# rocprofv3 kernel stats of the commit+open of short rows (2^16 mainnet row, 2^12 testnet row)
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/out}
cd $R; mkdir -p $OUT/prof
for lg in 16 12; do
  rocprofv3 --kernel-trace --stats -d $OUT/prof/kzg$lg -o kzg$lg --output-format csv -- python3 bench.py --full --workload kzg22 --log-n $lg --steps 50 --warmup 5 --no-cpu-baseline > $OUT/prof/bench_kzg${lg}_under_rocprof.json 2> $OUT/prof/rocprof_kzg$lg.err
done
