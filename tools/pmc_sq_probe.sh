#!/bin/bash
# Where do the waves of each kernel spend their cycles?  One rocprofv3 --pmc pass (SQ block, 8 slots, kernel trace only) of
# one bench window:  tools/pmc_sq_probe.sh <tag> [bench.py flags]  ->  $OUT/<tag>_pmc_sq_wait.json (default OUT: profile_out/)
TAG=${1:-probe}; shift
R=$(pwd); OUT=${OUT:-$R/profile_out}; mkdir -p $OUT; OUT=$(cd $OUT && pwd); export TMPDIR=/tmp; cd /tmp
timeout 600 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU --kernel-trace --output-format csv -d $OUT/pmcw_$TAG -- python $R/bench.py --full --no-cpu-baseline --no-parity --steps 1 --warmup 1 "$@" > $OUT/${TAG}_pmc_sq_wait.log 2>&1
python $R/tools/pmc_summary.py $OUT/${TAG}_pmc_sq_wait.json 3 "rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU (one pass) of bench.py $*: totals per window (3 full windows in the trace) and per-launch averages by grid. WAIT_ANY = wave parked at s_waitcnt / barrier, WAIT_INST_ANY = issue stall, ACTIVE_INST_ANY = issuing; quad-cycles on gfx950." $OUT/pmcw_$TAG
tail -2 $OUT/${TAG}_pmc_sq_wait.log
rm -rf $OUT/pmcw_$TAG
