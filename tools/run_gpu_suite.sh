set -e
export OUT=${OUT:-out}      # where the logs and result lines go
mkdir -p $OUT
python -m pytest tests -x -q -m gpu > $OUT/r5_gpu_tests.log 2>&1 || { tail -40 $OUT/r5_gpu_tests.log; exit 1; }
tail -3 $OUT/r5_gpu_tests.log
python bench.py --full --no-frame --no-extra-legs --no-cpu-baseline > $OUT/r5_bench.json 2> $OUT/r5_bench.err || { tail -20 $OUT/r5_bench.err; exit 1; }
python - <<'PY'
import json, os
d=json.loads(open(os.environ['OUT'] + '/r5_bench.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['kernel_ms'], d['roofline'].get('stages_ms'), d.get('batches_in_flight'))
if d.get('legs_failed'):
    raise SystemExit('bench legs failed: %s' % d['legs_failed'])
PY
