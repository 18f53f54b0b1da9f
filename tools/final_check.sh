set -e
# usage: tools/final_check.sh [OUTDIR]   (default bench_out; run from anywhere, on a machine with an MI355X)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd $ROOT
OUT=${1:-bench_out}
mkdir -p $OUT && OUT=$(cd $OUT && pwd)
mkdir -p $OUT/prof
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/t.log 2>&1
tail -2 $OUT/t.log
timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/b.json 2> $OUT/b.err
grep "timed region" $OUT/b.err
for B in 16 8 4; do timeout -k 10 200 python bench.py --child --batch $B --steps 20 --warmup 5 --no-cpu-baseline --no-roofline --no-parity > $OUT/b_$B.json 2> $OUT/b_$B.err; grep "timed region" $OUT/b_$B.err; done
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r02 -- python3 $ROOT/bench.py --child --steps 3 --warmup 2 --no-cpu-baseline --no-roofline --secondary --no-parity > $OUT/prof.log 2>&1
cd $ROOT
python tools/trace_step.py $OUT/prof 70 > $OUT/last_step_by_kernel.txt
python tools/trace_step.py $OUT/prof 80 grid > $OUT/last_step_by_kernel_and_grid.txt
head -3 $OUT/last_step_by_kernel.txt
rm -f $OUT/prof/*kernel_trace.csv $OUT/prof/*/*kernel_trace.csv
ls -la $OUT/prof $OUT/prof/* | head
