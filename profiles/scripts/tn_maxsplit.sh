#!/bin/bash
# The switch was removed from the code after this measurement; kept as the record of how it was measured.
# cap on the weight-gradient (TN) kernel's split count (EG_TN_MAXSPLIT): the image-side layers have ONE output tile, so the cap is their grid size
for w in "celeba bf16 128" "colored f16 512" "dsprites bf16 128"; do set -- $w; for v in 128 256 512 128 512; do
  out=$(env EG_TN_MAXSPLIT=$v timeout -k 10 120 python bench.py --no-probe --workload $1 --dtype $2 --batch $3 --steps 60 --warmup 10 --no-cpu-baseline --no-roofline 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], d['value'])" 2>/dev/null)
  echo "$1 EG_TN_MAXSPLIT=$v -> $out"
done; done
