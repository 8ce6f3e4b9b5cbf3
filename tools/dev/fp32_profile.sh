OUT=$(realpath -m "${OUT:-profile_out}"); ROOT=$(pwd); mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
export VDN_SIDE_STREAM=0 VDN_OVERLAP=0
rocprofv3 --kernel-trace --stats -d $OUT/fp -o fp --output-format csv -- python3 bench.py --full --precision fp32 --headline-only --no-cpu-baseline --no-roofline --steps 10 > $OUT/fp.log 2>&1
tail -c 400 $OUT/fp.log
f=$(find $OUT/fp -name '*kernel_stats.csv' | head -1)
cp $f $OUT/fp32_kernel_stats.csv
rm -rf $OUT/fp
