# GPU test suite, then the full bench line of every config, on the GPU machine from the repository root:
#   OUT=<dir> bash tools/gpu_round.sh tests bench      (any subset of: tests bench; outputs under $OUT, default out/)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(realpath -m "${OUT:-$R/out}")
cd $R
mkdir -p $out
for what in "$@"; do
  case $what in
    tests)
      timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $out/full_gpu.log 2>&1 || { tail -40 $out/full_gpu.log; exit 1; }
      tail -3 $out/full_gpu.log;;
    bench)
      timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 > $out/bench_c2.json
      for c in c1 c3 c5; do timeout -k 10 200 python bench.py --full --config $c --steps 20 --warmup 5 --no-cpu-baseline > $out/bench_$c.json; done
      timeout -k 10 200 python bench.py --full --ragged --steps 20 --warmup 5 --no-cpu-baseline > $out/bench_c2_ragged.json
      for f in c2 c1 c3 c5 c2_ragged; do python3 -c "import json,sys; d=json.loads(open('$out/bench_$f.json').read().strip().splitlines()[-1]); print('$f', d['value'], d['ms_per_step'], d.get('roofline',{}).get('frac'), {k: v['ms_per_step'] for k, v in d['time_shares_ms_per_step'].items()})"; done;;
  esac
done
