#!/bin/bash
# A/B two builds of libmdm_hip.so on ONE box, interleaved: ab_libs.sh libA.so libB.so [rounds]   (results in $OUT_DIR, default bench_out/)
A=$1; B=$2; R=${3:-3}; O=${OUT_DIR:-bench_out}; mkdir -p $O; : > $O/ab.txt
for i in $(seq 1 $R); do
  for L in $A $B; do
    MDM_LIB_PATH=$PWD/$L timeout -k 10 300 python bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-sampler > $O/ab.json 2> $O/ab.err || { echo "$L failed"; tail -3 $O/ab.err; exit 1; }
    python - "$L" "$O" <<'PY' | tee -a $O/ab.txt
import json, sys
j = json.loads(open(sys.argv[2] + "/ab.json").read().strip().splitlines()[-1])
print(f"{sys.argv[1]:40s} {j['ms_per_step']:.4f} ms/step  family {j['roofline']['kernel_ms_per_step']} ms")
PY
  done
done
