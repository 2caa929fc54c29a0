#!/bin/bash
# Step time of two or more builds of the library on ONE box, alternating:  [REPS=2] [STEPS=40] [WARMUP=10] tools/ab_lib.sh [--precision bf16x3] name1 name2 ...
# (names of fabric_amd/csrc/variants/lib_<name>.so, e.g. built by tools/build_lib_variant.sh); one line per run: name, ms/step, pairs/s.
# Stops at the first run that fails (a fault on the card must not be followed by more runs).
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root"
extra=""
if [ "$1" == "--precision" ]; then extra="--precision $2"; shift 2; fi
for rep in $(seq 1 ${REPS:-2}); do
for v in "$@"; do
  out=$(BIDATE_LIB=$root/fabric_amd/csrc/variants/lib_$v.so timeout -k 10 300 python bench.py --steps ${STEPS:-40} --warmup ${WARMUP:-10} --no-extras --no-roofline --no-cpu-baseline $extra 2>/dev/null) || { echo "$v FAILED (exit $?)"; exit 1; }
  echo "$out" | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', d['ms_per_step'], d['value'])"
done; done
