#!/bin/bash
# Produces the rocprofv3 evidence for bench.py's numbers (run on the GPU box):
#   $OUT/prof_<tag>/   --kernel-trace --stats of the full bench command (every workload)
#   $OUT/pmc_fetch_<tag>/, pmc_write_<tag>/   separate --pmc passes (HBM traffic)
# usage: tools/profile_round.sh <tag> [output directory, default prof_out/ in the repository]
TAG=$1
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$R/prof_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o s -- python $R/bench.py --full --no-cpu-baseline > $OUT/prof_$TAG.json 2> $OUT/prof_$TAG.err
timeout 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch_$TAG -o s -- python $R/bench.py --full --no-cpu-baseline --steps 200 --warmup 50 > /dev/null 2>&1
timeout 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write_$TAG -o s -- python $R/bench.py --full --no-cpu-baseline --steps 200 --warmup 50 > /dev/null 2>&1
ls $OUT/prof_$TAG $OUT/pmc_fetch_$TAG $OUT/pmc_write_$TAG
tail -1 $OUT/prof_$TAG.json | cut -c1-200
