# all five BASELINE.json configs back to back on one GPU (bash tools/gpu/all_configs.sh [DIR]): one summary line per config, JSON lines under DIR (default bench_out/all_configs/)
cd "$(dirname "$0")/../.."; out=${1:-bench_out/all_configs}; mkdir -p "$out"
for c in 1 2 3 4 5; do
  python bench.py --full --config $c --steps 20 --warmup 3 --no-pmc --no-cpu-baseline > "$out/config$c.json" 2> "$out/config$c.err"
  python - <<PY
import json
d=json.load(open('$out/config$c.json'))
r=d['roofline']
print('config $c: %.2f %s  %.3f ms/step  clock %s  roofline %s frac %.4f  step %s' % (d['value'], d['unit'], d['ms_per_step'], d['sustained_shader_clock_ghz_each'], r.get('bound'), r.get('frac') or 0, r.get('step')))
PY
done
rm -rf gpurun_out/step_trace_config*
