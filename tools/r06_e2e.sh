: "${OUT:?set OUT to a results directory}"; OUT=$(realpath -m "$OUT"); export OUT
mkdir -p $OUT
timeout 900 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-other-configs --no-second-dtype --no-ess > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc $?" >> $OUT/bench.err
tail -3 $OUT/bench.err
python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "bench.json")).read().strip().splitlines()[-1])
print(json.dumps(d.get("e2e_host"), indent=1))
PY
