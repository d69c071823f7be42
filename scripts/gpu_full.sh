#!/bin/bash
# GPU tests, smoke and the benchmark with everything it measures (--full: roofline, CPU baseline, `also` block) into OUT:
#   bash scripts/gpu_full.sh OUT
OUT=${1:?usage: bash scripts/gpu_full.sh OUT}; mkdir -p $OUT
python -m pytest tests -m gpu -x -q > $OUT/pytest.log 2>&1; tail -4 $OUT/pytest.log
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; tail -2 $OUT/smoke.log
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err; python - $OUT/bench.json <<'P'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["ms_per_step"], d["value"], d["roofline"]["frac"], d["cpu_baseline"]["value"], d["also"]["demucs_fwd"]["stages"]["stft"])
P
