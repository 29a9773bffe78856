# Run ON THE GPU BOX: the bench line with each of the given library builds (ORBHIP_LIB).  bash tools/lib_variants.sh tag lib1.so lib2.so ...
# Output under ${ORB_OUT:-build/out}/<tag>/.
T=$1; shift
O=${ORB_OUT:-build/out}/$T
mkdir -p $O
for l in "$@"; do
  n=$(basename $l .so)
  ORBHIP_LIB=$PWD/$l python bench.py --full --no-cpu-baseline --no-host-fed $BENCH_OPTS > $O/$n.json 2>$O/$n.err || { echo "$l failed"; tail -3 $O/$n.err; exit 1; }
  python - <<P
import json; d=json.load(open("$O/$n.json")); print("$n", "->", d["value"], d["roofline"]["stage_ms_per_batch"])
P
done
