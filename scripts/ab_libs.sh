#!/bin/bash
# A/B of library builds on the bench: bash scripts/ab_libs.sh <out-prefix> <config> <name>=<lib.so> ...
# (SMM_LIB_PATH selects the build; each arm runs REPS times (default 2), interleaved, so that box drift shows; even
#  repetitions run the arms in reverse order.  STEPS / WARMUP (default 8 / 2) and BENCH_ARGS go to bench.py; every run
#  has its own time limit and the first failure ends the script)
out=$1; cfg=$2; shift 2
arms=("$@")
rev=()
for ((i=${#arms[@]}-1; i>=0; i--)); do rev+=("${arms[i]}"); done
for rep in $(seq 1 ${REPS:-2}); do
  if (( rep % 2 )); then order=("${arms[@]}"); else order=("${rev[@]}"); fi
  for arm in "${order[@]}"; do
    name=${arm%%=*}; lib=${arm#*=}
    SMM_LIB_PATH=$lib timeout -k 10 ${RUN_LIMIT:-300} python bench.py --config $cfg --steps ${STEPS:-8} --warmup ${WARMUP:-2} --no-cpu $BENCH_ARGS \
      > ${out}_${cfg}_${name}_${rep}.json 2>> ${out}.err || exit 1
  done
done
