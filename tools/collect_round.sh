# On the GPU box: every profile / bench file of a round that DESIGN.md and profiles/README.md quote, into $1 (default out/;
# copy the summaries to profiles/).  The kernel traces of tools/collect_profiles.sh go where that script puts them.
cd "$(dirname "$0")/.."
O="${1:-out}"
mkdir -p "$O/r06"
bash tools/collect_profiles.sh r06 > "$O/r06/collect.log" 2>&1
python bench.py --full > "$O/r06_bench_local.json" 2> "$O/r06/bench_local.err"
python bench.py --full --steps 20 --warmup 5 --no-extra --no-strict --no-cpu-baseline > "$O/r06_bench_20steps.json" 2> /dev/null
python bench.py --full --no-strict --no-extra --no-cpu-baseline --no-parity --steps 8 --dump-kernels "$O/r06_conv_shapes.txt" > /dev/null 2>&1
python tools/lookup_sweep.py --fused > "$O/r06_lookup_sweep.txt" 2>&1
python tools/lc1_bench.py 0 1 > "$O/r06_lc1_bench.txt" 2>&1
tail -c 1500 "$O/r06_bench_local.json"
