#!/bin/bash
# What the driver runs at a round's end and a little more, from the repo root on the GPU box; logs go to $OUT (default
# out/final_check).  Every step has a time limit of its own and the script stops at the first step that fails.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out/final_check}; mkdir -p "$OUT"
run() {  # run <name> <seconds> <command...>: stdout to $OUT/<name>.out, stderr to $OUT/<name>.err
  local name=$1 secs=$2; shift 2
  timeout -k 10 "$secs" "$@" > "$OUT/$name.out" 2> "$OUT/$name.err"; local rc=$?
  echo "$name rc $rc"
  [ $rc -eq 0 ] || { tail -5 "$OUT/$name.out" "$OUT/$name.err"; exit $rc; }
}
run tests 600 python -m pytest tests -m gpu -x -q; tail -3 "$OUT/tests.out"
run smoke 100 python -c "import __graft_entry__ as g; g.smoke()"; tail -2 "$OUT/smoke.out"
run dist 200 python bench.py --force-dist --steps 20 --warmup 5 --full --no-cpu-baseline --no-extras --no-e2e; cut -c1-200 "$OUT/dist.out"
run strong4 300 python bench.py --strong --config 4 --loci 20000 --steps 8 --warmup 2 --full --no-cpu-baseline --no-extras --no-e2e
python3 -c "import json,sys;j=json.load(open(sys.argv[1]));print(round(j['value']/1e6,2), j.get('strong_scaling_check'), j['parity_check'])" "$OUT/strong4.out"
run bench 120 python bench.py --steps 20 --warmup 5
python3 -c "import json,sys;j=json.load(open(sys.argv[1]));print(round(j['value']/1e6,2), j['ms_per_step'])" "$OUT/bench.out"
run bench_full 600 python bench.py --steps 20 --warmup 5 --full
python3 -c "import json,sys;j=json.load(open(sys.argv[1]));print(round(j['value']/1e6,2), j['ms_per_step'], j['parity_check'], {k:round(v['value']/1e6,2) for k,v in j['configs'].items()})" "$OUT/bench_full.out"
