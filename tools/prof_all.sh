#!/bin/bash
export OUT=${OUT:-prof_out}; mkdir -p "$OUT"   # output folder of this script and the ones it calls
# Everything profiles/<tag>_* holds, regenerated on the library as built (run on the GPU box from the repo root):  tools/prof_all.sh r06
# then, back in the container:  tools/collect_profiles.sh r06
tag=$1
tools/prof_round.sh $tag > $OUT/${tag}_prof_round.log 2>&1
tools/prof_bench.sh ${tag}nf --model NestFuse --batch 4 --size 512 --no-parity-path > /dev/null 2>&1
cp $OUT/kstats_${tag}nf.txt $OUT/${tag}_kernel_stats_nestfuse_b4_512_bf16.txt
tools/prof_bench.sh ${tag}rf --model RFNNest --batch 4 --size 512 --no-parity-path > /dev/null 2>&1
cp $OUT/kstats_${tag}rf.txt $OUT/${tag}_kernel_stats_rfnnest_b4_512_bf16.txt
tools/prof_bench.sh ${tag}df --model DenseFuse --no-parity-path > /dev/null 2>&1
cp $OUT/kstats_${tag}df.txt $OUT/${tag}_kernel_stats_densefuse_b32_256_bf16.txt
tools/prof_bench.sh ${tag}inf --mode infer --batch 1 --size 1024 --width 1224 > /dev/null 2>&1
cp $OUT/kstats_${tag}inf.txt $OUT/${tag}_kernel_stats_infer_1224x1024_bf16.txt
tools/sweep_configs.sh > $OUT/${tag}_config_sweep.txt 2>&1
cp $OUT/${tag}_traffic.json profiles/${tag}_traffic.json   # (on the box's copy: the bench line below reads the counter pass of THIS build)
python3 bench.py --full > $OUT/${tag}_bench_line.json 2> $OUT/${tag}_bench.err
tail -c 1500 $OUT/${tag}_bench_line.json
cat $OUT/${tag}_config_sweep.txt
rm -rf $OUT/prof_${tag}*/ $OUT/prof_bp_*/ $OUT/pmc_${tag}*/ $OUT/sq_${tag}*/ 2>/dev/null
du -sh $OUT
