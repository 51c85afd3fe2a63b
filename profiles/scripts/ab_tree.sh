#!/bin/bash
# A/B of two built source trees on one box, alternating -- for changes that touch the C ABI or the Python side too, where swapping the
# library alone (ab_lib.sh) cannot work:  bash ab_tree.sh BEFORE_DIR AFTER_DIR [bench args]
# Runs `python bench.py --no-probe --steps 50 --warmup 10 [bench args]` (no capture probe child: twelve runs, every one captures directly);
# bench.py's own messages stay on stderr.  Stops at the first run that does not end with a result line.
A=$1; B=$2; shift 2
for rep in 1 2 3; do for v in before after; do
  d=$A; [ $v = after ] && d=$B
  out=$(cd "$d" && timeout -k 10 180 python bench.py --no-probe --steps 50 --warmup 10 "$@" | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d['ms_per_step'], d['value'])") || { echo "$v -> FAILED"; exit 1; }
  echo "$v -> $out"
done; done
