# Run ON THE GPU BOX: the bench line under a list of option sets.  bash tools/bench_variants.sh tag "opts1" "opts2" ...
# Output under ${ORB_OUT:-build/out}/<tag>/.
T=$1; shift
O=${ORB_OUT:-build/out}/$T
mkdir -p $O
i=0
for o in "$@"; do
  python bench.py --full --no-cpu-baseline --no-host-fed $o > $O/v$i.json 2>$O/v$i.err || { echo "variant $i failed"; tail -3 $O/v$i.err; exit 1; }
  python - <<P
import json; d=json.load(open("$O/v$i.json")); print("$o", "->", d["value"], d.get("verified_frames"), d["roofline"]["stage_ms_per_batch"])
P
  i=$((i+1))
done
