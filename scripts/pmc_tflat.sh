#!/bin/bash
# FETCH_SIZE / WRITE_SIZE of the flat read-in fill `k_tflat_move` (separate counter passes, no tracing; FETCH_SIZE x2 on
# gfx950, KiB) of the checkout this script lies in.  Usage: pmc_tflat.sh OUTDIR [cells]; prints one line per dispatch.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "$1" && cd "$1" && pwd)
CELLS=${2:-1000000}
export TMPDIR=/tmp
cd /tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 420 rocprofv3 --pmc $c -d "$OUT/$c" -o pmc --output-format csv -- python "$ROOT/scripts/probes/tflat_traffic.py" "$CELLS" > "$OUT/$c.log" 2>&1
  rc=$?
  echo "$c rc=$rc"
  [ $rc -eq 0 ] || { tail -5 "$OUT/$c.log"; exit $rc; }
done
python - "$OUT" <<'PY'
import csv, glob, sys, collections
out = sys.argv[1]
for c in ("FETCH_SIZE", "WRITE_SIZE"):
    agg = collections.OrderedDict()
    for f in glob.glob(out + f"/{c}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_tflat_move" in r["Kernel_Name"] and r["Counter_Name"] == c:
                agg[int(r["Dispatch_Id"])] = agg.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    for d, v in sorted(agg.items()):
        gb = v * 1024 * (2 if c == "FETCH_SIZE" else 1) / 1e9
        print(f"k_tflat_move dispatch {d:6d} {c:11s} raw {v:.4e} KiB -> {gb:7.1f} GB")
PY
find "$OUT" -name "*.csv" -size +2M -delete
