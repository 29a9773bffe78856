# Run ON THE GPU BOX: extractor parity tests + one-stream stage times of the bench step.  bash tools/quick_stage.sh [tag] [pytest targets...]
# Output under ${ORB_OUT:-build/out}/<tag>/.
T=${1:-q}; shift
O=${ORB_OUT:-build/out}/$T
mkdir -p $O
timeout -k 10 300 python -m pytest ${@:-tests/test_gpu_extract.py tests/test_gpu_fuzz.py} -x -q -m gpu > $O/pytest.log 2>&1; rc=$?
echo "pytest rc=$rc"; tail -3 $O/pytest.log
[ $rc -eq 0 ] || exit $rc
python bench.py --full --streams 1 --steps 3 --warmup 1 --no-cpu-baseline --no-host-fed > $O/s1.json 2>/dev/null || exit 1
python - <<P
import json; d=json.load(open("$O/s1.json")); print(d["value"], d["roofline"]["stage_ms_per_batch"])
P
