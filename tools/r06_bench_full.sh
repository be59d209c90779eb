#!/bin/bash
# the whole line (--full) and its blocks; OUT = a directory for the results
: "${OUT:?set OUT to a results directory}"; OUT=$(realpath -m "$OUT"); export OUT
mkdir -p $OUT
timeout 1500 python bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err; echo "rc $?" >> $OUT/bench_full.err
tail -3 $OUT/bench_full.err
python - <<'PY'
import json, os
line = open(os.path.join(os.environ["OUT"], "bench_full.json")).read().strip().splitlines()[-1]
print("line length", len(line))
d = json.loads(line)
print("value", d["value"], "frac", d["roofline"]["frac"])
print(json.dumps(d.get("e2e_host"), indent=0)[:1500])
for k, v in d.get("configs", {}).items():
    print(k, json.dumps({a: b for a, b in v.items() if a != "cpu"}))
PY
