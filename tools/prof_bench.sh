#!/bin/bash
export OUT=${OUT:-prof_out}; mkdir -p "$OUT"   # output folder of this script and the ones it calls
# rocprofv3 kernel trace of the default bench (run on the GPU box from the repo root):  tools/prof_bench.sh <tag> [bench args]
# -> $OUT/prof_<tag>/ (rocpd db) + $OUT/kstats_<tag>.txt (per-kernel table, tools/rocpd_stats.py)
tag=$1; shift
R=$PWD; cd /tmp && export TMPDIR=/tmp; cd $R
rm -rf $OUT/prof_$tag
rocprofv3 --kernel-trace -d $OUT/prof_$tag -o b -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-other-configs "$@" > $OUT/prof_$tag.log 2>&1
db=$(find $OUT/prof_$tag -name "*.db" | head -1)
python3 tools/rocpd_stats.py $db 13 > $OUT/kstats_$tag.txt
head -40 $OUT/kstats_$tag.txt
