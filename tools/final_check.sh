#!/bin/bash
export OUT=${OUT:-prof_out}; mkdir -p "$OUT"   # output folder of this script and the ones it calls
mkdir -p $OUT
timeout 3400 python -m pytest tests -x -q -m gpu > $OUT/r06z_tests.log 2>&1
tail -6 $OUT/r06z_tests.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3
for i in 1 2; do
python3 bench.py --full > $OUT/r06_bench_line.json 2> $OUT/r06_bench.err
python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['OUT'], 'r06_bench_line.json')).read().strip().splitlines()[-1])
print('headline', round(d['value'],1), round(d['ms_per_step'],3), 'frac', round(d['step_frac_of_ideal'],3), 'roof', round(d['roofline']['frac'],3), d['roofline']['traffic'], 'parity', round(d['parity_path']['value'],1), {k: round(v['value'],1) for k,v in d['other_configs'].items()})
PY
done
