cd $GRAFT_REPO_ROOT
out=${OUT:-bench_out}
mkdir -p $out
s=$(date +%s)
python bench.py --full > $out/r05_bench_timed.json 2> $out/r05_bench_timed.err
e=$(date +%s)
echo "default bench wall: $((e-s)) s" > $out/r05_bench_timed.txt
grep -E "^\[bench" $out/r05_bench_timed.err | tail -40 >> $out/r05_bench_timed.txt
