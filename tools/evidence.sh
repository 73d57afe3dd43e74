#!/bin/bash
# The evidence set behind profiles/ in one run on the GPU machine, from the repository root:
#   OUT=<dir> bash tools/evidence.sh <tag>      (outputs <tag>_* under $OUT, default out/; copy what is judged into profiles/)
# Full bench lines of every config (CPU baseline on the default one), per-launch timelines, the chain kernels' phase trace (when
# build/trace.so exists: make -C gcgcn_amd/csrc trace), the rows either side of the path, and rocprofv3 kernel stats + PMC passes
# per workload (tools/profile_all.sh).  Every GPU step has its own time limit; the first failure ends the run.
set -e
tag=${1:?usage: tools/evidence.sh <tag>}
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(realpath -m "${OUT:-$R/out}")
cd $R
mkdir -p $out

bench() {  # <name> [bench.py args]
  local name=$1; shift
  timeout -k 10 400 python bench.py --full "$@" > $out/${tag}_bench_$name.json
}
bench c2
for c in c1 c3 c5; do bench $c --config $c --no-cpu-baseline; done
for c in c1 c2 c3; do bench ${c}_ragged --config $c --ragged --no-cpu-baseline; done
bench c2_ragged_b128 --config c2 --ragged --global-batch 128 --no-cpu-baseline
echo "== bench lines done"

timeline() {  # <name> [bench.py args]: per-dispatch timeline of one step
  local name=$1; shift
  rm -rf $out/tl
  (cd /tmp && TMPDIR=/tmp timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $out/tl -o tl -- \
     python3 $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline "$@" > /dev/null 2>&1)
  python3 tools/timeline.py $out/tl > $out/${tag}_${name}_step_timeline.txt
  rm -rf $out/tl
}
for c in c1 c2 c3 c5; do timeline $c --config $c; done
for c in c2 c3; do timeline ${c}_ragged --config $c --ragged; done
echo "== timelines done"

if [ -f build/trace.so ]; then
  for c in c1 c2 c3; do
    GCGCN_LIB=$R/build/trace.so timeout -k 10 120 python tools/trace_chain.py --config $c --iters 2 > $out/${tag}_chain_phase_trace_$c.txt 2>&1
  done
  echo "== trace done"
fi

row() {  # <name> <script> [args]: the rows either side of the path
  local name=$1; shift
  timeout -k 10 300 python "$@" > $out/${tag}_$name.json 2>/dev/null
}
row tail_bench_ragged tools/tail_bench.py --ragged --steps 20
row tail_bench_ragged_bert tools/tail_bench.py --ragged --steps 20 --layers 4 --heads 4
row head_bench_ragged tools/head_bench.py --ragged --steps 20
row head_bench_n64 tools/head_bench.py --steps 10
row producer_bench tools/producer_bench.py --ids uint8 --steps 20
row train_step_bench tools/train_step_bench.py --steps 10
echo "== row benches done"

OUT=$out bash tools/profile_all.sh $tag c2 c3 c5 c2_ragged producer tail_ragged head_ragged
