#!/bin/bash
# bench.py --full (every secondary record) + the whole -m gpu suite + smoke: the round-end check.
# Usage: scripts/gpu_final_check.sh OUTDIR
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT=${1:?usage: gpu_final_check.sh OUTDIR}
mkdir -p "$OUT"
export TMPDIR=/tmp
s=$(date +%s)
timeout 1500 python bench.py --full --steps 20 --warmup 5 > "$OUT/bench.json" 2> "$OUT/bench.err"
echo "bench rc=$? wall=$(( $(date +%s) - s )) s"
python - "$OUT" <<'PY'
import json,sys
d=json.loads(open(sys.argv[1]+"/bench.json").read().strip().splitlines()[-1])
print("c3", d["ms_per_step"], d["value"], d["roofline"]["frac"], d["roofline"]["avg_launch_ms"])
for k,v in d["secondary"].items():
    print(k, v.get("error") or (v.get("ms_per_step"), v.get("value"), v.get("unit")))
print(d["summary"])
PY
s=$(date +%s)
timeout 2400 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.txt" 2>&1
echo "pytest rc=$? wall=$(( $(date +%s) - s )) s"; tail -3 "$OUT/pytest_gpu.txt"
timeout 300 python __graft_entry__.py smoke > "$OUT/smoke.txt" 2>&1; echo "smoke rc=$?"; tail -3 "$OUT/smoke.txt"
