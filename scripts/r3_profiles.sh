#!/bin/bash
# Round-3 evidence: bash scripts/r3_profiles.sh r3_z  ->  $OUT/r3_z_*  (copied into profiles/ afterwards)
#   kernel stats of the default bench command (headline + extra_configs), PMC passes of configs[1] and of the configs[4] share,
#   the bench lines (default = what the driver runs, and --exact), the end-to-end API timings.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export OUT=${OUT:-bench_out}; mkdir -p $OUT     # where the results go, relative to the repository root
TAG=$1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu > $OUT/prof_$TAG.log 2>&1
f=$(find $OUT/prof_$TAG -name '*kernel_stats.csv' | head -1)
(head -1 $f; grep smm:: $f) > $OUT/${TAG}_kernel_stats.csv
echo "kernel stats done"; cut -c1-150 $OUT/${TAG}_kernel_stats.csv | head -12
bash scripts/pmc_run.sh $TAG --no-extra > /dev/null 2>&1
echo "pmc c1 done"
bash scripts/pmc_run.sh ${TAG}_c4 --no-extra --config c4 > /dev/null 2>&1
echo "pmc c4 done"
python3 bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
python3 bench.py --full --exact --steps 5 --no-extra > $OUT/${TAG}_bench_exact.json 2>> $OUT/${TAG}_bench.err
python3 bench.py --config c3 --steps 3 --warmup 1 --exact > $OUT/${TAG}_bench_c3_exact.json 2>> $OUT/${TAG}_bench.err
echo "bench lines done"
python3 scripts/api_e2e.py big > $OUT/${TAG}_api_e2e.jsonl 2>> $OUT/${TAG}_bench.err
cat $OUT/${TAG}_api_e2e.jsonl
rm -rf $OUT/pmc_$TAG $OUT/pmc_${TAG}_c4 $OUT/prof_$TAG
for f in $OUT/${TAG}_bench*.json; do echo $f; cut -c1-400 $f; done
