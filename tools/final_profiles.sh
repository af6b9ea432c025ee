# Round profiles: the driver's bench command, bench lines per precision, rocprofv3 kernel stats, PMC traffic / SQ counters, shapes.
# usage (GPU box, from the repo root): bash tools/final_profiles.sh [a|b|c] (parts that each fit one 20-minute gpurun call; default a and b) ; then python tools/collect_profiles.py r06 here
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${OUT:-runs}        # where the logs and profiles go (the repository ignores runs/)
mkdir -p $OUT/final
PART=${1:-ab}
if [[ $PART == *a* ]]; then
# the driver's exact command, and the two short warm-ups VERDICT r3 asked about
timeout 600 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 --detail-out $OUT/final/bench_driver_cmd_detail.json > $OUT/final/bench_driver_cmd.log 2>&1
grep "^{" $OUT/final/bench_driver_cmd.log | tail -1 > $OUT/final/bench_driver_cmd.json      # (the compact line; the full record of the same run beside it)
for w in 0 1; do
  timeout 300 python3 bench.py --full --gpus 1 --steps 20 --warmup $w --cpu-frames 0 --single-stream 0 --extras 0 2> /dev/null | grep "^{" | tail -1 > $OUT/final/bench_warmup$w.json
done
# rocprofv3 kernel trace of the driver's command (the configs[1] / configs[3] / spread extras off: they launch the same kernels on other shapes)
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final/rocprof_driver -- python3 bench.py --full --gpus 1 --steps 20 --warmup 5 --cpu-frames 0 --single-stream 0 --extras 0 > $OUT/final/rocprof_driver.log 2>&1
python3 tools/summarize_rocprof.py $OUT/final/rocprof_driver $OUT/final/kernel_stats_driver_cmd.csv > /dev/null; rm -rf $OUT/final/rocprof_driver
for p in adaptive fp16x3; do
  timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final/rocprof_$p -- python3 bench.py --full --steps 100 --warmup 20 --cpu-frames 0 --single-stream 0 --extras 0 --precision $p > $OUT/final/rocprof_$p.log 2>&1
  python3 tools/summarize_rocprof.py $OUT/final/rocprof_$p $OUT/final/kernel_stats_$p.csv > /dev/null; rm -rf $OUT/final/rocprof_$p
done
timeout 900 python bench.py --full --print-record > $OUT/final/bench_adaptive.log 2>&1
timeout 300 python bench.py --full --print-record --arrays 128 --frames 256 --cpu-frames 0 --single-stream 0 --extras 0 > $OUT/final/bench_128x256.log 2>&1
grep "^{" $OUT/final/bench_128x256.log | tail -1 > $OUT/final/bench_128x256.json
timeout 900 python bench.py --full --print-record --precision fp16x3 --cpu-frames 0 --extras 0 > $OUT/final/bench_fp16x3.log 2>&1
timeout 900 python bench.py --full --print-record --precision fp16 --cpu-frames 0 --extras 0 > $OUT/final/bench_fp16.log 2>&1
timeout 900 python bench.py --full --print-record --precision fp32 --cpu-frames 0 --extras 0 --steps 30 --warmup 5 > $OUT/final/bench_fp32.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/final/rocprof_mvdr -- python3 bench.py --full --config mvdr --steps 20 --warmup 5 --cpu-frames 0 > $OUT/final/rocprof_mvdr.log 2>&1
python3 tools/summarize_rocprof.py $OUT/final/rocprof_mvdr $OUT/final/kernel_stats_mvdr.csv > /dev/null; rm -rf $OUT/final/rocprof_mvdr
timeout 300 python bench.py --full --print-record --config mvdr > $OUT/final/bench_mvdr.log 2>&1
fi
if [[ $PART == *b* ]]; then
bash tools/pmc_traffic.sh adaptive $OUT/pmc_traffic_adaptive > $OUT/final/pmc_traffic.log 2>&1
bash tools/pmc_sq.sh adaptive $OUT/pmc_sq > $OUT/final/pmc_sq.log 2>&1
timeout 600 python tools/precision_report.py > $OUT/final/precision_report.json 2> $OUT/final/precision_report.log
timeout 300 python tools/host_path_rate.py > $OUT/final/host_path.log 2>&1
python tools/bench_fallback.py 2>&1 | grep -v amdgpu.ids > $OUT/final/fallback.log
(python tools/bench_shapes.py; python tools/bench_shapes.py m16; python tools/bench_shapes.py sources; python tools/bench_shapes.py gate; python tools/bench_shapes.py n2048; python tools/bench_shapes.py n512; echo "--- the any-length kernels at 2048-sample frames (MCA_HIP_NO_N2048=1):"; MCA_HIP_NO_N2048=1 python tools/bench_shapes.py n2048) 2>&1 | grep -v amdgpu.ids > $OUT/final/shapes.log
timeout 300 python tools/stream_latency.py 2>&1 | grep -v amdgpu.ids > $OUT/final/stream_latency.log
fi
if [[ $PART == *c* ]]; then
# round 5: the MVDR kernels' PMC passes, the adaptive mode against FP16X3 at sizes the oracle cannot reach, the per-kernel
# breakdown of the repair chain on three shapes, the kernel timeline of one step
bash tools/r05_profiles_mvdr.sh > $OUT/final/pmc_mvdr.log 2>&1
timeout 900 python tools/adaptive_check.py 40 2026 > $OUT/final/adaptive_check.json 2> $OUT/final/adaptive_check.log
bash tools/repair_breakdown.sh > $OUT/final/repair_breakdown.log 2>&1
bash tools/timeline.sh > $OUT/final/timeline.log 2>&1
fi
tail -c 300 $OUT/final/bench_driver_cmd.json
cat $OUT/final/kernel_stats_driver_cmd.csv
