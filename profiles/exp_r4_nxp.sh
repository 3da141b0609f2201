#!/bin/bash
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd $ROOT && mkdir -p bench_out
for cfg in c5 c4 c5 c4; do
  timeout -k 10 300 python bench.py --full --config $cfg --steps 100 --warmup 20 --no-cpu-baseline > bench_out/nxp_$cfg.json 2> bench_out/nxp_$cfg.err || echo "$cfg failed"
  python3 -c "
import json,sys
j=json.loads(open('bench_out/nxp_$cfg.json').read().strip().splitlines()[-1]); print('$cfg', j['ms_per_step'], j['kernel_ms'], j['roofline']['frac'], j['roofline']['fwd_plus_bwd_frac'])"
done
timeout -k 10 900 python -m pytest tests -x -q -m gpu 2>&1 | tail -4
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep smoke
