#!/bin/bash
export OUT=${OUT:-prof_out}; mkdir -p "$OUT"   # output folder of this script and the ones it calls
# SQ counters of the bench's kernels (run on the GPU box from the repo root):  tools/prof_sq.sh <tag>
# one rocprofv3 --pmc pass (8 SQ slots): wave cycles, busy / wait breakdown, MFMA busy cycles, LDS activity and bank conflicts
tag=$1
R=$PWD; cd /tmp && export TMPDIR=/tmp; cd $R
rm -rf $OUT/sq_$tag
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT \
  --output-format csv -d $OUT/sq_$tag -o p -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-parity-path --no-other-configs > $OUT/sq_$tag.log 2>&1
csv=$(find $OUT/sq_$tag -name "*counter_collection.csv" | head -1)
python3 tools/pmc_stats.py $csv > $OUT/sq_$tag.txt
head -30 $OUT/sq_$tag.txt
find $OUT/sq_$tag -name "*.csv" -size +1M -delete
