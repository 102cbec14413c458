#!/bin/bash
# end-of-round evidence: 2-rank rehearsal of bench.py --gpus (gloo, both ranks on cuda:0), profiles of every workload, the full bench line
O=${OUT_DIR:-bench_out}; mkdir -p "$O"
FFTW_AMD_BENCH_REHEARSE=1 python bench.py --gpus 2 --batch 64 --steps 3 --warmup 1 > "$O/r03_rehearse2.json" 2> "$O/r03_rehearse2.err"
tail -c 400 "$O/r03_rehearse2.json"; echo; tail -3 "$O/r03_rehearse2.err"
timeout -k 10 900 tools/perf/profile_r03.sh > "$O/profile_r03.log" 2>&1
grep "traffic / alg" "$O/profile_r03.log"
SECONDS=0; python bench.py --full > "$O/r03_bench_3.json" 2> "$O/r03_bench_3.err"
echo "bench wall ${SECONDS} s"
python - "$O/r03_bench_3.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["traffic"], d["roofline"]["per_launch"]["avg_launch_ms"])
for l in d["config"]["legs"]:
    print(l["workload"], l["ms_per_step"], l["roofline"]["frac"], l["roofline"]["traffic"], l["roofline"]["per_launch"]["avg_launch_ms"])
PY
