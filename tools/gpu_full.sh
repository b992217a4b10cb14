cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
out="${1:?usage: tools/gpu_full.sh OUT_DIR}"; mkdir -p "$out"
timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -15 > "$out/gpu_tests.log"
cat "$out/gpu_tests.log"
( time python bench.py --full ) > "$out/bench_default.log" 2> "$out/bench_default.err"
tail -c 600 "$out/bench_default.err"
tail -c 4200 "$out/bench_default.log"
cp bench_extras.json "$out/bench_default_run.json"
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
