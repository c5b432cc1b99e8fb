#!/bin/bash
# One measurement session on the GPU box, per config in $CONFIGS (default "C2"):
#   PMC passes (tools/pmc.sh) → gpurun_out/<cfg>_traffic.json, copied into profiles/ so bench.py
#   finds the traffic of this very build → rocprofv3 kernel stats of bench.py → bench.py (with the
#   CPU baseline unless NOCPU is set).  Any failing step ends the session.
set -u
ROOT="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
cd "$ROOT"
OUT=$ROOT/gpurun_out
mkdir -p "$OUT"
for cfg in ${CONFIGS:-C2}; do
  lc=$(echo "$cfg" | tr 'A-Z' 'a-z')
  if [ -z "${NOPMC:-}" ]; then
    CONFIG=$cfg PMC_OUT=$OUT/pmc_$lc bash tools/pmc.sh || { echo "pmc $cfg failed"; exit 3; }
    python3 tools/summarize_prof.py - "$OUT/pmc_$lc" --json="$OUT/${lc}_traffic.json" > "$OUT/${lc}_pmc.md" || exit 3
    cp "$OUT/${lc}_traffic.json" profiles/
  fi
  if [ -z "${NOPROF:-}" ]; then
    (cd /tmp && export TMPDIR=/tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv \
        -d "$OUT/prof_$lc" -o run -- python3 "$ROOT/bench.py" --full --config "$cfg" --steps 3 --warmup 1 --no-cpu-baseline --no-model) \
        > "$OUT/prof_$lc.log" 2>&1 || { echo "rocprof $cfg failed"; exit 4; }
  fi
  timeout -k 10 900 python3 bench.py --full --config "$cfg" ${NOCPU:+--no-cpu-baseline} ${BENCH_ARGS:-} > "$OUT/bench_$lc.log" 2>&1 \
      || { echo "bench $cfg failed"; tail -5 "$OUT/bench_$lc.log"; exit 5; }
  tail -1 "$OUT/bench_$lc.log" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); r=d['roofline']; print('BENCH', d['config']['workload'], d['ms_per_step'], 'ms', d['value'], 'Msamples/s; dominant', r['kernel'], 'frac', r['frac'], 'traffic_frac', r['traffic_frac'], 'cpu', (d.get('cpu_baseline') or {}).get('value'))"
done
echo measure done
