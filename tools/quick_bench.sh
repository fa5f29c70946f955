# usage: bash tools/quick_bench.sh <name> [extra bench args]  -> $OUT/<name>.json (OUT default: bench_out/) + a one-line summary
N=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
mkdir -p "$OUT"
python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-rccl-smoke "$@" > "$OUT/$N.json" 2> "$OUT/$N.err" || tail -c 2000 "$OUT/$N.err"
python - <<PY
import json
l=json.loads(open("$OUT/$N.json").read().strip().splitlines()[-1])
print("value", l["value"], "ms", l["ms_per_step"], "median", l["repeat_ms_per_step"]["median"], "kernels", l.get("kernels_per_step"), "selfcheck ok", l.get("selfcheck", {}).get("ok"))
if "shard_sweep" in l: print("shards", {k:v["graph_ms"] for k,v in l["shard_sweep"].items()})
if "contact_loss_eval" in l: print("cle", {k:v for k,v in l["contact_loss_eval"].items() if "step" in k})
PY
