#!/bin/bash
# One GPU call that produces what a round is judged by: smoke, the whole GPU test suite, the bench line as the driver asks for it
# (python bench.py --gpus 1 --steps 20 --warmup 5) and the same line with --full (every side workload and baseline).
# Every GPU step runs under its own time limit, and the script stops at the first step that does not exit 0: nothing more is started
# on a card after a failure.  Logs go to $LOGS (default: a new temporary directory).
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
set -o pipefail
LOGS=${LOGS:-$(mktemp -d)}; mkdir -p "$LOGS"; echo "logs in $LOGS"
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > "$LOGS/smoke.log" 2>&1; rc=$?; echo "smoke rc=$rc"
tail -2 "$LOGS/smoke.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 2400 python -m pytest tests -m gpu -q > "$LOGS/pytest_gpu.log" 2>&1; rc=$?; echo "pytest rc=$rc"
tail -8 "$LOGS/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 > "$LOGS/bench_plain.log" 2> "$LOGS/bench_plain.err"; rc=$?; echo "plain bench rc=$rc"
tail -1 "$LOGS/bench_plain.log" | cut -c1-400; [ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$LOGS/bench.log" 2> "$LOGS/bench.err"; rc=$?; echo "bench --full rc=$rc"
[ $rc -eq 0 ] || exit $rc
tail -1 "$LOGS/bench.log" | wc -c
tail -1 "$LOGS/bench.log" | python -c "
import json,sys
j=json.loads(sys.stdin.read())
print('headline %.4g %s  ms/step %.4f %s frac %.3f (kernel %.3f)  one-launch %.4f' % (j['value'], j['unit'], j['ms_per_step'], j['config']['region_ms_per_step'], j['roofline']['frac'], j['roofline']['frac_kernel'], j['roofline'].get('one_launch_ms', 0)))
for k,v in j.get('workloads',{}).items():
    print(' ', k, ('%.4g ms/step %.4f frac %.3f one-launch %s cpu %s' % (v['value'], v['ms_per_step'], v['roofline']['frac'], v['roofline'].get('one_launch_ms'), v.get('cpu_baseline',{}).get('value'))) if 'value' in v else v)
print('cpu_baseline', j.get('cpu_baseline',{}).get('value'))
"
