#!/bin/bash
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${TUNE_OUT:-$ROOT/tune_out}  # (per-variant build logs and bench lines)
cd "$ROOT"
mkdir -p "$OUT"
for W in 256 512 1024 1536 2048; do
  PCLEAN_WAVE_WGS=$W timeout 600 python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-full-iteration > "$OUT/w_$W.json" 2> "$OUT/w_$W.log"
  python - <<PY
import json
d=json.loads(open("$OUT/w_$W.json").read().strip().splitlines()[-1])
ph=d["phases_ms"]
print("WGS=$W: root %.3f ms, slot_scan %.3f, step %.2f ms, device %.2f" % (d["roofline"]["avg_launch_ms"], ph["slot_scan"]["ms"], d["ms_per_step"], d["config"]["device_ms_per_step"]))
PY
done
