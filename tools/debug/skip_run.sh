#!/bin/bash
# tools/debug/skip_elem_patch.py must have been applied and built: one bench line per skipped kernel family
#   bash tools/debug/skip_run.sh OUTDIR MASK [MASK...]
set -e
OUT=$1; shift
mkdir -p "$OUT"
for mask in "$@"; do
  CMOOP_DEBUG_SKIP_ELEM=$mask python3 bench.py --warmup 1 --no-cpu-baseline > "$OUT/skip_$mask.json" 2> "$OUT/skip_$mask.err" || { tail -5 "$OUT/skip_$mask.err"; exit 1; }
  python3 -c "
import json
d=json.loads(open('$OUT/skip_$mask.json').read().strip().splitlines()[-1])
print('skip mask $mask evals/h', d['value'], 'ms/step', d['ms_per_step'], 'aggregate', d['whole_job_tflops'], flush=True)"
done
