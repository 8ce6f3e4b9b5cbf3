OUT=$(realpath -m "${OUT:-profile_out}"); ROOT=$(pwd); mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
rocprofv3 --kernel-trace -d $OUT/tl -o tl --output-format csv -- python3 bench.py --full --headline-only --no-cpu-baseline --steps 30 --warmup 10 > $OUT/tl.log 2>&1
f=$(find $OUT/tl -name '*kernel_trace.csv' | head -1)
python3 tools/dev/timeline.py $f -600 > $OUT/tl_step.txt
python3 tools/dev/timeline.py $f -601 > $OUT/tl_step5.txt
rm -rf $OUT/tl
