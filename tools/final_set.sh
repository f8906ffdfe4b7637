set -e
bash tools/run_profile.sh ${1:-r3v7}
bash tools/sq_counters.sh ${1:-r3v7} || true
python bench.py --full --steps 8 --warmup 3 --no-cpu-baseline --dtype fp8 > ${MDT_OUT:-out}/${1:-r3v7}_bench_fp8.log 2>&1 || true
python bench.py --full --steps 8 --warmup 3 --no-cpu-baseline > ${MDT_OUT:-out}/${1:-r3v7}_bench_bf16_same_call.log 2>&1 || true
python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --config large > ${MDT_OUT:-out}/${1:-r3v7}_bench_large.log 2>&1 || true
tail -c 400 ${MDT_OUT:-out}/${1:-r3v7}_bench.log
