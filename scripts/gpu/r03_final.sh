#!/bin/bash
# usage: r03_final.sh <output dir>  -> bench.py --full (all workloads) + stage benches and timelines
set -o pipefail
OUT=${1:?usage: r03_final.sh <output dir>}
mkdir -p "$OUT"
python bench.py --full > "$OUT/r3_bench_full.log" 2> "$OUT/r3_bench_full.err"
rc=$?
grep "bench +" "$OUT/r3_bench_full.err"
python - "$OUT/r3_bench_full.log" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("value", d["value"], "ms", d["ms_per_step"], d["windows_ms_per_step"])
print("roofline", {k: d["roofline"][k] for k in ("kernel","achieved","frac","traffic","achieved_counter","walked_bytes","achieved_walked","avg_launch_us","empty_bracket_us")})
for k,v in d["roofline"]["blend_launches"].items(): print(" ", k, v["frac"], v["avg_launch_us"], v["achieved_counter"])
print("secondary", d["secondary_rooflines"])
print("kernels", d["kernels_us"])
for k in ("stable_targets","host_frames","reference_schedule","c3_phase_with_density_control","cpu_baseline"):
    v=d.get(k); 
    if v: print(k, {kk: vv for kk, vv in v.items() if kk not in ("workload","sample")})
PY
bash scripts/gpu/r03_stages.sh > "$OUT/r3_stages_out.log" 2>&1; head -12 "$OUT/r3_stages_out.log"
exit $rc
