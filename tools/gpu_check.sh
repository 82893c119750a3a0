#!/bin/bash
# GPU-box iteration step: selected -m gpu tests (one process, per-test timeout), then the C2 bench line.
#   [OUT=<dir>] bash tools/gpu_check.sh "<pytest -k expr or test files>" [bench args...]
set -euo pipefail
OUT=${OUT:-$(mktemp -d)}
mkdir -p "$OUT"
echo "logs in $OUT"
T=${1:-tests}; shift || true
timeout -k 10 900 python3 -u -m pytest $T -x -q -m gpu --timeout 120 --timeout-method thread > "$OUT/tests.log" 2>&1 \
  || { tail -30 "$OUT/tests.log"; exit 1; }
tail -3 "$OUT/tests.log"
if [ "${BENCH:-1}" = 1 ]; then
  # --full: the per-kernel table printed below comes from the live kernel timer
  timeout -k 10 300 python3 bench.py --full --no-c4-ref --no-cpu-baseline "$@" > "$OUT/bench.json" 2> "$OUT/bench.err"
  python3 - "$OUT/bench.json" <<'PY'
import json, sys
d = json.loads([x for x in open(sys.argv[1]) if x.startswith("{")][-1])
print("ms_per_step", d["ms_per_step"], "value", d["value"])
for k, v in sorted(d.get("kernels", {}).items(), key=lambda kv: -kv[1]["ms"])[:12]:
    print(f"  {k:28s} {v['ms']:7.3f} ms  x{v['launches']:3d}  {v['bound']} {v['frac']}")
PY
fi
