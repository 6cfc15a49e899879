set -x
cd $GRAFT_REPO_ROOT
out=${OUT:-bench_out}
mkdir -p $out
timeout 600 python bench.py --full --no-cpu-baseline --no-train-leg --no-oxford-leg --no-pinned-leg > $out/r05_z_bench.json 2> $out/r05_z_bench.err
