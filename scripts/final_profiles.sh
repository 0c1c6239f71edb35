#!/bin/bash
# Per-round evidence: kernel stats (rocprofv3 --kernel-trace --stats), PMC passes (scripts/pmc_run.sh), bench lines of every
# BASELINE config.   bash scripts/final_profiles.sh r2_k   ->   $OUT/r2_k_*
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export OUT=${OUT:-bench_out}; mkdir -p $OUT     # where the results go, relative to the repository root
TAG=$1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu > $OUT/prof_$TAG.log 2>&1
f=$(find $OUT/prof_$TAG -name '*kernel_stats.csv' | head -1)
(head -1 $f; grep smm:: $f) > $OUT/${TAG}_kernel_stats.csv
bash scripts/pmc_run.sh $TAG > /dev/null 2>&1
python3 bench.py --full > $OUT/${TAG}_bench_c1.json 2> $OUT/${TAG}_bench.err
python3 bench.py --full --exact --steps 5 > $OUT/${TAG}_bench_c1_exact.json 2>> $OUT/${TAG}_bench.err
python3 bench.py --config c2 --steps 5 > $OUT/${TAG}_bench_c2.json 2>> $OUT/${TAG}_bench.err
python3 bench.py --config c2 --steps 5 --exact > $OUT/${TAG}_bench_c2_exact.json 2>> $OUT/${TAG}_bench.err
python3 bench.py --config c3 --steps 3 --warmup 1 > $OUT/${TAG}_bench_c3.json 2>> $OUT/${TAG}_bench.err
python3 bench.py --config c3 --steps 3 --warmup 1 --exact > $OUT/${TAG}_bench_c3_exact.json 2>> $OUT/${TAG}_bench.err
python3 bench.py --config c4 --steps 3 --warmup 1 --no-cpu > $OUT/${TAG}_bench_c4.json 2>> $OUT/${TAG}_bench.err
bash scripts/pmc_run.sh ${TAG}_c3 --config c3 > /dev/null 2>&1
# only the summaries are kept
rm -rf $OUT/pmc_$TAG $OUT/pmc_${TAG}_c3 $OUT/prof_$TAG
cut -c1-160 $OUT/${TAG}_kernel_stats.csv | head -8
for f in $OUT/${TAG}_bench_c*.json; do echo $f; cut -c1-330 $f; done
