# Run ON THE GPU BOX from the repo root:  bash tools/profile_round.sh [tag]
# bench lines (both workloads, --full), rocprofv3 kernel-trace stats of the same bench command, HBM traffic passes, SQ counter
# passes, vector-issue calibration -> ${ORB_OUT:-build/out}/<tag>_*  (copy what is to be kept into profiles/).
set -e
R=$PWD
T=${1:-r03}
mkdir -p ${ORB_OUT:-build/out}
export ORB_OUT=$(cd ${ORB_OUT:-build/out} && pwd)     # absolute: the rocprofv3 runs below start in /tmp
O=$ORB_OUT
python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
echo "bench euroc done"
python bench.py --full --config tumvi > $O/${T}_bench_tumvi.json 2> $O/${T}_bench_tumvi.err
echo "bench tumvi done"
cd /tmp && export TMPDIR=/tmp
rm -rf $O/${T}_prof
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_prof -- python3 $R/bench.py --full --no-cpu-baseline --no-host-fed > $O/${T}_prof.log 2>&1
# one pipeline, synchronised nowhere but at the step ends: the HIP-event stage times of the bench line and rocprofv3's dispatch
# durations must agree here (with four streams the events also see the wait for CUs held by the other streams)
rm -rf $O/${T}_s1_prof
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_s1_prof -- python3 $R/bench.py --full --streams 1 --steps 4 --warmup 1 --no-cpu-baseline --no-host-fed > $O/${T}_s1_bench.json 2> $O/${T}_s1_prof.log
cd $R
cp $(ls $O/${T}_s1_prof/*/*kernel_stats.csv | head -1) $O/${T}_s1_kernel_stats.csv
rm -rf $O/${T}_s1_prof
python bench.py --full --no-match --no-cpu-baseline --no-host-fed > $O/${T}_bench_extract_only.json 2> /dev/null
echo "kernel trace done"
cp $(ls $O/${T}_prof/*/*kernel_stats.csv | head -1) $O/${T}_kernel_stats.csv
rm -rf $O/${T}_prof      # the per-dispatch trace is large; the summary is what is kept
python tools/collect_traffic.py > $O/${T}_traffic.log 2>&1
cp $O/traffic.json $O/${T}_traffic.json
echo "traffic done"
python tools/collect_sq.py > $O/${T}_sq.log 2>&1
cp $O/sq_counters.json $O/${T}_sq_counters.json
echo "sq done"
python tools/collect_valu_calib.py --out $O/${T}_valu_calib.json > $O/${T}_valu_calib.log 2>&1
echo "calib done"
