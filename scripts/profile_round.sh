#!/bin/bash
# Round evidence on the GPU box: default bench line (what the driver runs), msm26 / kzg22 workloads, rocprofv3 kernel
# stats of the headline and of the 2^22 commit+open.  Outputs under $OUT/prof (default: out/prof in the repository); copy what is judged to profiles/.
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/out}
mkdir -p $OUT/prof
cd $R
python bench.py --full > $OUT/prof/bench_default.json 2> $OUT/prof/bench_default.err
python bench.py --full --workload kzg22 --steps 10 --warmup 3 > $OUT/prof/bench_kzg22.json 2> $OUT/prof/bench_kzg22.err
python bench.py --full --workload msm26 --steps 10 --warmup 2 > $OUT/prof/bench_msm26.json 2> $OUT/prof/bench_msm26.err
rocprofv3 --kernel-trace --stats -d $OUT/prof/msm20 -o msm20 --output-format csv -- python3 bench.py --full --headline-only > $OUT/prof/bench_msm20_under_rocprof.json 2> $OUT/prof/rocprof_msm20.err
rocprofv3 --kernel-trace --stats -d $OUT/prof/kzg22 -o kzg22 --output-format csv -- python3 bench.py --full --workload kzg22 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/prof/bench_kzg22_under_rocprof.json 2> $OUT/prof/rocprof_kzg22.err
find $OUT/prof -name "*kernel_stats.csv" | head
