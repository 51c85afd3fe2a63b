#!/bin/bash
# the round's measurement set on one machine.  usage: bash profiles/scripts/evidence.sh <tag>   (writes <tag>_* files: the bench line,
# --full with roofline and cpu_baseline, under $OUT; the rest beside the profiler output of the scripts it calls)
TAG=${1:-r02z}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-bench_results}
cd $R
mkdir -p $OUT
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench_default_run.json 2> $OUT/${TAG}_bench_default_run.err; echo "bench rc=$?"
cut -c1-300 $OUT/${TAG}_bench_default_run.json
bash profiles/scripts/table.sh > gpurun_out/${TAG}_throughput_table.txt 2>&1; cat gpurun_out/${TAG}_throughput_table.txt
bash profiles/scripts/rocprof_bench.sh $TAG
bash profiles/scripts/pmc_traffic.sh $TAG 2>&1 | tail -12
bash profiles/scripts/exposed_run.sh $TAG 2>&1 | tail -30
