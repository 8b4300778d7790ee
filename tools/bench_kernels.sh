#!/bin/bash
# headline step only (no variants / other configs): ms per step, eager, the probed gather kernels
set -eu
out=$(mktemp)
python bench.py --full --no-variants --no-configs "$@" 2>&1 | tail -1 > "$out"
python - "$out" <<PY
import json, sys
o=json.load(open(sys.argv[1]))
print("ms/step", round(o["ms_per_step"],4), "eager", round(o["repeats"]["eager_ms_per_step"],4), {k:round(v["ms"],4) for k,v in o.get("kernels",{}).items()})
PY
