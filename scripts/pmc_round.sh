#!/bin/bash
# PMC passes for the default bench (2^20 MSM): one rocprofv3 --pmc pass per counter group, kernel-trace only
# (MI355X_MICROARCH.md "rocprofv3 PMC slots": FETCH_SIZE and WRITE_SIZE do not fit one pass).  Run on the GPU box:
#   bash scripts/pmc_round.sh ; python scripts/pmc_summarise.py $OUT/pmc profiles/<round>_msm20_pmc.csv
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/out}
cd $R
mkdir -p $OUT/pmc
ARGS="bench.py --full --steps 3 --warmup 1 --headline-only"
for grp in "FETCH_SIZE" "WRITE_SIZE" "SQ_INSTS_VALU SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY" "GRBM_GUI_ACTIVE"; do
  tag=$(echo $grp | cut -d' ' -f1)
  rocprofv3 --pmc $grp --kernel-trace -d $OUT/pmc/$tag -o p --output-format csv -- python3 $ARGS > $OUT/pmc/$tag.json 2> $OUT/pmc/$tag.err
done
ls $OUT/pmc/*/
