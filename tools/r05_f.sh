set -x
cd $GRAFT_REPO_ROOT
out=${OUT:-bench_out}
mkdir -p $out
timeout 1500 python -m pytest tests -x -q -m gpu 2>&1 | tail -12 > $out/r05_f_gputest.log
timeout 300 python tools/host_issue_probe.py > $out/r05_f_graph_probe.log 2>&1
timeout 900 python bench.py --full > $out/r05_f_bench.json 2> $out/r05_f_bench.err
tail -c 300 $out/r05_f_bench.err
