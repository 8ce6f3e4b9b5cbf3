R=r04
OUT=$(realpath -m "${OUT:-profile_out}"); ROOT=$(pwd); mkdir -p $OUT
export VDN_SIDE_STREAM=0 VDN_OVERLAP=0
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${R}_trace -- python3 bench.py --full --headline-only --no-cpu-baseline --no-roofline --steps 20 > $OUT/${R}_trace_bench.json 2> $OUT/${R}_trace.log
find $OUT/${R}_trace -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/${R}_train_bf16_kernel_stats_whole_run.csv
find $OUT/${R}_trace -name "*kernel_trace.csv" | head -1 | xargs -I{} python3 tools/steady_stats.py {} 0.3 $OUT/${R}_trace_bench.json > $OUT/${R}_train_bf16_kernel_stats.csv
rm -rf $OUT/${R}_trace
unset VDN_SIDE_STREAM VDN_OVERLAP
rocprofv3 --kernel-trace --output-format csv -d $OUT/${R}_trace2 -- python3 bench.py --full --headline-only --no-cpu-baseline --no-roofline --steps 20 > $OUT/${R}_trace2_bench.json 2> $OUT/${R}_trace2.log
find $OUT/${R}_trace2 -name "*kernel_trace.csv" | head -1 | xargs -I{} python3 tools/steady_stats.py {} 0.3 $OUT/${R}_trace2_bench.json > $OUT/${R}_train_bf16_kernel_stats_two_streams.csv
rm -rf $OUT/${R}_trace2
python3 bench.py --full > $OUT/${R}_bench_train_bf16.json 2> $OUT/${R}_bench.err
echo traces done
