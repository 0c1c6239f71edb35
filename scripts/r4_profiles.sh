#!/bin/bash
# Round-4 evidence: bash scripts/r4_profiles.sh r4_z  ->  $OUT/r4_z_*  (copied into profiles/ afterwards)
#   kernel stats of the default bench command (headline + extra_configs), PMC passes of configs[1], the bench lines
#   (default = what the driver runs, and --exact).
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export OUT=${OUT:-bench_out}; mkdir -p $OUT     # where the results go, relative to the repository root
TAG=$1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu > $OUT/prof_$TAG.log 2>&1
f=$(find $OUT/prof_$TAG -name '*kernel_stats.csv' | head -1)
(head -1 $f; grep smm:: $f) > $OUT/${TAG}_kernel_stats.csv
echo "kernel stats done"; cut -c1-150 $OUT/${TAG}_kernel_stats.csv | head -12
bash scripts/pmc_run.sh $TAG --no-extra > /dev/null 2>&1
echo "pmc c1 done"
python3 bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
python3 bench.py --full --exact --steps 5 --no-extra > $OUT/${TAG}_bench_exact.json 2>> $OUT/${TAG}_bench.err
echo "bench lines done"
rm -rf $OUT/pmc_$TAG $OUT/prof_$TAG
for f in $OUT/${TAG}_bench*.json; do echo $f; cut -c1-300 $f; done
