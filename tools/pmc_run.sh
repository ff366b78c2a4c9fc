#!/bin/bash
# HBM traffic per kernel: two separate rocprofv3 counter passes (FETCH_SIZE, WRITE_SIZE) over a
# short bench run, then tools/pmc_traffic.py -> profiles/<tag>_pmc_traffic.json.
#   bash tools/pmc_run.sh r01            (PMC_CMD: the profiled program; default a short C2 bench
#                                         with every section; PMC_OUT: where the passes are kept)
set -e
TAG=${1:-r01}
OUT=${PMC_OUT:-pmc_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 600 rocprofv3 --pmc $C -d "$OUT/pmc_$C" -o run --output-format csv -- \
    ${PMC_CMD:-python3 bench.py --full --steps 5 --warmup 3 --no-cpu-baseline --no-score --infer-pairs 64} > "$OUT/pmc_$C.log" 2>&1
done
python3 tools/pmc_traffic.py "$OUT/pmc_FETCH_SIZE" "$OUT/pmc_WRITE_SIZE" \
  profiles/${TAG}_pmc_traffic.json
