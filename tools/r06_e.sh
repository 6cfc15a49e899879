set -x
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
out=${OUT:-bench_out}
mkdir -p $out
timeout 900 python bench.py --full --no-cpu-baseline --no-train-leg --no-oxford-leg --no-pinned-leg > $out/r06_e_bench.json 2> $out/r06_e_bench.err
tail -3 $out/r06_e_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $out/r06_e_prof_x6 -- python bench.py --gemm x6 --no-extras --no-cpu-baseline --steps 10 --warmup 3 > $out/r06_e_prof_x6.log 2>&1
find $out/r06_e_prof_x6 -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $out/r06_e_x6_kernel_stats.csv
python tools/summarize_rocprof.py $out/r06_e_x6_kernel_stats.csv 13 > $out/r06_e_x6_summary_table.md 2>&1 || true
head -40 $out/r06_e_x6_summary_table.md
rm -rf $out/r06_e_prof_x6
