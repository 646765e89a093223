#!/bin/bash
# Scratch: wall time of the --full bench.py run and of --steps 1 --warmup 0.  Output under $1 (default logs/walltime).
OUT=${1:-logs/walltime}
mkdir -p "$OUT"
t0=$(date +%s.%N)
timeout -k 10 600 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err" || exit 1
t1=$(date +%s.%N)
timeout -k 10 300 python bench.py --steps 1 --warmup 0 --full --no-cpu-baseline > "$OUT/bench_s1.json" 2> "$OUT/bench_s1.err" || exit 1
t2=$(date +%s.%N)
python - <<PY
import json
d = json.loads(open("$OUT/bench_default.json").read().strip().splitlines()[-1])
print("--full run: wall %.1f s" % ($t1 - $t0), {k: d[k] for k in ("value", "ms_per_step", "steps", "warmup", "world_size", "collectives_per_step")})
print("  frac", d["roofline"]["frac"], "cpu", d["cpu_baseline"]["value"], "clock", d["calibration"].get("k1_core_clock_mhz"), "hard eig share", d["hard_spectrum"]["eig_share"])
d = json.loads(open("$OUT/bench_s1.json").read().strip().splitlines()[-1])
print("steps 1 warmup 0: wall %.1f s" % ($t2 - $t1), {k: d[k] for k in ("value", "ms_per_step", "steps", "warmup")}, d["roofline"]["frac"])
PY
