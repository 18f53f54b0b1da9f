# round-3 measurement script (run on the GPU box from the repo root): driver-flag bench, local-batch sweep, rocprofv3
# kernel trace of the bench child at B = 32 and B = 4, two --pmc passes for the dominant kernel template
set -e
# usage: tools/final_check_r03.sh [OUTDIR]   (default bench_out; run from anywhere, on a machine with an MI355X)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd $ROOT
OUT=${1:-bench_out}
mkdir -p $OUT && OUT=$(cd $OUT && pwd)
mkdir -p $OUT/prof $OUT/prof4 $OUT/pmc_f $OUT/pmc_w
timeout -k 10 400 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/b.json 2> $OUT/b.err
grep "timed region" $OUT/b.err
cp bench_out/bench_kernel_table.json $OUT/b_kernel_table.json
for B in 16 8 4; do timeout -k 10 200 python bench.py --child --batch $B --steps 20 --warmup 5 --no-cpu-baseline --no-roofline --no-parity > $OUT/b_$B.json 2> $OUT/b_$B.err; grep "timed region" $OUT/b_$B.err; done
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r03 -- python3 $ROOT/bench.py --child --steps 3 --warmup 2 --no-cpu-baseline --no-roofline --secondary --no-parity > $OUT/prof.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof4 -o r03b4 -- python3 $ROOT/bench.py --child --batch 4 --steps 3 --warmup 2 --no-cpu-baseline --no-roofline --secondary --no-parity > $OUT/prof4.log 2>&1
cd $ROOT
python tools/trace_step.py $OUT/prof 70 > $OUT/last_step_by_kernel.txt
python tools/trace_step.py $OUT/prof 60 template > $OUT/last_step_by_template.txt
python tools/trace_step.py $OUT/prof 80 grid > $OUT/last_step_by_kernel_and_grid.txt
python tools/trace_step.py $OUT/prof4 75 > $OUT/last_step_b4.txt
head -3 $OUT/last_step_by_kernel.txt; head -3 $OUT/last_step_b4.txt
rm -f $OUT/prof/*kernel_trace.csv $OUT/prof/*/*kernel_trace.csv $OUT/prof4/*kernel_trace.csv $OUT/prof4/*/*kernel_trace.csv
cd /tmp
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_f -o f -- python3 $ROOT/bench.py --child --steps 2 --warmup 2 --no-graph --no-cpu-baseline --no-roofline --secondary --no-parity > $OUT/pmc_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_w -o w -- python3 $ROOT/bench.py --child --steps 2 --warmup 2 --no-graph --no-cpu-baseline --no-roofline --secondary --no-parity > $OUT/pmc_w.log 2>&1
cd $ROOT
DOM=$(python -c "import json; print(json.loads(open('$OUT/b.json').read().strip().splitlines()[-1])['roofline']['kernel'])")
echo "dominant kernel template: $DOM"
python tools/pmc_traffic.py $OUT/pmc_f $OUT/pmc_w "$DOM" $OUT/pmc_dominant_traffic.json
rm -f $OUT/pmc_f/*/*counter_collection.csv $OUT/pmc_w/*/*counter_collection.csv
# matrix-pipe utilisation per kernel (SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE): one more --pmc pass
mkdir -p $OUT/pmc_m
cd /tmp
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_m -o m -- python3 $ROOT/bench.py --child --steps 2 --warmup 2 --no-graph --no-cpu-baseline --no-roofline --secondary --no-parity > $OUT/pmc_m.log 2>&1
cd $ROOT
python tools/pmc_mfma.py $OUT/pmc_m $OUT/pmc_mfma_by_kernel.csv
rm -f $OUT/pmc_m/*/*counter_collection.csv $OUT/pmc_m/*counter_collection.csv
