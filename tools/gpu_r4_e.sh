cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/gpu_r4_e.sh <output dir>}; mkdir -p "$OUT"
python -m pytest tests -m gpu -q 2>&1 | tail -n 8
python bench.py --full --no-cpu-baseline > "$OUT/r4_bench2.json" 2> "$OUT/r4_bench2.err"; tail -c 300 "$OUT/r4_bench2.err"
python3 - <<PY
import json
d=json.load(open('$OUT/r4_bench2.json'))
print('value', round(d['value']), 'ms', round(d['ms_per_step'],2), 'roofline', round(d['roofline']['frac'],3))
e=d['extra']
print({k: round(v,3) for k,v in e['stage_ms_per_step'].items() if v})
for k in ('nrms_train_step_B64','standard_train_step_B64','naml_train_step_B64'):
    t=e[k]; print(k, round(t['ms'],2))
print('news_only', {k: (round(v['ms'],3), round(v['frac_fp32_mfma'],3)) for k,v in e['news_encoder_only_1024'].items()})
print('latency', e['latency_one_impression'])
PY
