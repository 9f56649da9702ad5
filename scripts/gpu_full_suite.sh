#!/bin/bash
# the whole GPU suite (what the driver runs at round end), then smoke() and one short bench line with its --full measurements
#   usage: scripts/gpu_full_suite.sh [output directory, default suite_out]
cd "$(dirname "$0")/.." && export TMPDIR=/tmp || exit 1
OUT=${1:-suite_out}
mkdir -p "$OUT"
timeout -k 10 1000 python -m pytest tests -q -m gpu -x --durations=15 > "$OUT/full_suite.log" 2>&1; rc=$?; tail -28 "$OUT/full_suite.log"; echo "suite rc=$rc"
[ $rc = 0 ] || exit 1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
timeout -k 10 300 python bench.py --full --steps 4 --warmup 1 --no-cpu-baseline > "$OUT/full_suite_bench.json" 2> "$OUT/full_suite_bench.err" && python -c "import json, sys; d=json.load(open(sys.argv[1])); print('ms_per_step %.1f' % d['ms_per_step'], 'frac %.3f' % d['roofline']['frac'], [round(l['frac_of_peak'],3) for l in d['amg_levels']], 'hbm', d['config']['hbm_used_gb'])" "$OUT/full_suite_bench.json"
