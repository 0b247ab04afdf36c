# GPU box, one call: parity suite on the product library, then the bench line.
#   bash scripts/run_round_checks.sh <tag>
TAG=${1:-r04a}
OUT=${CHECKS_OUT:-checks_out}  # where the logs and the bench record go
mkdir -p "$OUT"
timeout 600 python -m pytest tests -m gpu -x -q > "$OUT/pytest_$TAG.log" 2>&1; tail -5 "$OUT/pytest_$TAG.log"
timeout 420 python bench.py --full --steps 20 --warmup 5 > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"; tail -3 "$OUT/bench_$TAG.err"
python - <<PY
import json
try:
    d = json.load(open('$OUT/bench_$TAG.json'))
    print('value %.1f M  ms %.4f  rep %s' % (d['value'] / 1e6, d['ms_per_step'], [round(x, 4) for x in d['repeats']['ms_per_step_all']]))
    for k in ('roofline_stft', 'roofline_istft'):
        print(k, round(d[k]['launch_ms'], 4), round(d[k]['frac'], 4), d[k].get('round_trip_snr_db_min'))
    print('stream', json.dumps(d.get('stream_ceiling'))[:600])
    print('power', json.dumps(d.get('board_power'))[:600])
    print('cpu', json.dumps(d.get('cpu_baseline'))[:500]); print('cpu_all', json.dumps(d.get('cpu_baseline_all_cores'))[:300]); print('parity', d.get('parity'))
    print('cqt', json.dumps(d.get('cqt_lite'))[:900]); print('e2e', json.dumps(d.get('end_to_end_numpy'))[:400]); print('gl', json.dumps(d.get('griffinlim'))[:200])
except Exception as e:
    print('bench parse failed', e)
PY
