#!/bin/bash
# same-box A/B of library / engine variants: each line "NAME|ENV..." runs bench.py --no-extras REPS times (default 2), alternating
# usage: [REPS=4] [STEPS=30] [BENCH_FLAGS="--depth 50"] scripts/ab_bench.sh "A|" "B|DAFNE_FUSE_GNFIN=0" ...
# every run has its own time limit; the first one that fails ends the script
cd ${GRAFT_REPO_ROOT:-/root/repo}
for rep in $(seq 1 ${REPS:-2}); do
  for spec in "$@"; do
    name=${spec%%|*}; envs=${spec#*|}
    out=$(env $envs timeout -k 10 240 python bench.py --steps ${STEPS:-30} --warmup 5 --no-extras --no-cpu-baseline ${BENCH_FLAGS:-} 2>/dev/null) || { echo "$rep $name: bench.py failed ($?)"; exit 1; }
    v=$(echo "$out" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('%.1f img/s %.3f ms' % (d['value'], d['ms_per_step']))")
    echo "$rep $name: $v"
  done
done
