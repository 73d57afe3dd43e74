# The end-of-round evidence in one run on the GPU machine: GPU test suite, full bench lines of every config, rocprofv3 kernel
# stats and the per-dispatch timeline of the default bench command (outputs under $OUT, default out/; copy what is judged
# into profiles/).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(realpath -m "${OUT:-$R/out}")
cd $R
mkdir -p $out
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $out/full_gpu.log 2>&1 || { tail -30 $out/full_gpu.log; exit 1; }
tail -3 $out/full_gpu.log
timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 > $out/bench_c2.json
for c in c1 c3 c5; do timeout -k 10 200 python bench.py --full --config $c --steps 20 --warmup 5 --no-cpu-baseline > $out/bench_$c.json; done
timeout -k 10 200 python bench.py --full --ragged --steps 20 --warmup 5 --no-cpu-baseline > $out/bench_c2_ragged.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats_v2 -o st -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $out/stats_bench.log 2>&1
find $out/stats_v2 -name "*kernel_stats.csv" -exec cp {} $out/r02_c2_default_bench_kernel_stats_v2.csv \;
timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $out/tl -o tl -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > /dev/null 2>&1 && python3 $R/tools/timeline.py $out/tl > $out/r02_c2_step_timeline_v2.txt
rm -rf $out/stats_v2 $out/tl
for f in c2 c1 c3 c5 c2_ragged; do python3 -c "import json,sys; d=json.loads(open('$out/bench_$f.json').read().strip().splitlines()[-1]); print('$f', d['value'], d['ms_per_step'], d.get('roofline',{}).get('frac'))"; done
