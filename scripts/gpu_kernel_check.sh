#!/bin/bash
set -u
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=$R/gpurun_out/kernel_check
mkdir -p "$OUT"
cd "$R"
timeout 600 python -m pytest tests/test_gpu_hourglass.py -m gpu -x -q -k "${K:-layer1}" > "$OUT/pytest.log" 2>&1; echo "pytest rc=$?" >> "$OUT/pytest.log"
tail -15 "$OUT/pytest.log"
for dt in ${DTYPES:-bf16}; do
timeout 400 python bench.py --dtype $dt --full --whole-record --no-cpu-baseline --no-bf16-leg > "$OUT/bench_$dt.log" 2>&1
python - <<PY
import json
l=[x for x in open("$OUT/bench_$dt.log") if x.startswith("{")]
if l:
    d=json.loads(l[-1]); print("$dt frames/s", round(d["value"],1), "ms/step", round(d["ms_per_step"],2))
    for k in d["roofline"]["kernels"][:9]: print("  ", k["kernel"], k["launches"], round(k["avg_us"],1), round(k["tflops"],1))
else:
    print(open("$OUT/bench_$dt.log").read()[-2000:])
PY
done
