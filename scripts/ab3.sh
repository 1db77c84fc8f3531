#!/bin/bash
# A/B/C of several builds on ONE box, interleaved: ab3.sh rounds lib1 lib2 ...   (results in $OUT_DIR, default bench_out/)
R=$1; shift; O=${OUT_DIR:-bench_out}; mkdir -p $O; : > $O/ab.txt
for i in $(seq 1 $R); do
  for L in "$@"; do
    MDM_LIB_PATH=$PWD/$L timeout -k 10 300 python bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-sampler > $O/ab.json 2> $O/ab.err || { echo "$L failed"; tail -3 $O/ab.err; exit 1; }
    python - "$L" "$O" <<'PY' | tee -a $O/ab.txt
import json, sys
j = json.loads(open(sys.argv[2] + "/ab.json").read().strip().splitlines()[-1])
print(f"{sys.argv[1]:40s} {j['ms_per_step']:.4f} ms/step  family {j['roofline']['kernel_ms_per_step']} ms  loss {j['config']['final_loss']}")
PY
  done
done
