#!/bin/bash
# usage: bench_sweep.sh "<bench args 1>" "<bench args 2>" ...  -> one short line per run in $OUT_DIR/sweep.txt (default bench_out/)
O=${OUT_DIR:-bench_out}; mkdir -p $O; : > $O/sweep.txt
for a in "$@"; do
  timeout -k 10 300 python bench.py --full --steps 40 --warmup 8 --no-cpu-baseline --no-sampler $a > $O/sw.json 2> $O/sw.err
  rc=$?
  python - "$a" $rc "$O" <<'PY' | tee -a $O/sweep.txt
import json, sys
try:
    j = json.loads(open(sys.argv[3] + "/sw.json").read().strip().splitlines()[-1])
    print(f"{sys.argv[1]!r:40s} rc={sys.argv[2]} ms/step {j['ms_per_step']:.4f} img/s {j['value']:.0f} fam {j['roofline']['kernel_ms_per_step']} ms {j['roofline']['launches_per_step']} launches")
except Exception as e:
    print(f"{sys.argv[1]!r:40s} rc={sys.argv[2]} FAILED {e}")
PY
  if [ $rc -eq 124 ] || [ $rc -ge 128 ]; then exit $rc; fi
done
