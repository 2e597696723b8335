#!/bin/bash
# GPU tests, smoke, the full bench line and bench variants, the kernel timeline.  Usage: bash tools/gpu_validate.sh <output dir>
out=${1:?usage: bash tools/gpu_validate.sh <output dir>}
mkdir -p $out
timeout 900 python -m pytest tests -x -q -m gpu 2>&1 | tail -5 > $out/t_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $out/smoke.log 2>&1
timeout 600 python bench.py --full > $out/bench_n1.json 2> $out/bench_n1.err
rm -f $out/b_var.log
for a in "--batch 8192" "--batch 8192 --n 120" "--batch 4096 --n 200" "--batch 4096 --n 200 --polish-max-rounds 8" "--batch 1024 --n 120" "--profile varied"; do
  echo "== $a" >> $out/b_var.log
  timeout 300 python bench.py --full --no-cpu-baseline --steps 20 $a 2>&1 | tail -1 >> $out/b_var.log
done
python tools/kernel_timeline.py 1024 80 > $out/timeline.log 2>&1
cat $out/t_gpu.log; tail -2 $out/smoke.log; cat $out/bench_n1.json
B_VAR=$out/b_var.log python - <<'PY'
import json, os
for l in open(os.environ['B_VAR']):
    if l.startswith('=='): print(l.strip()); continue
    try:
        d=json.loads(l); print(round(d['value']), round(d['roofline']['kernel_ms'],3), round(d['roofline']['frac'],3), d['kkt_solves'], d['factorisations'], d['solved'], d['polished'])
    except Exception as e: print(l[:300])
PY
cat $out/timeline.log
