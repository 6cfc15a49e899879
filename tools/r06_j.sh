set -x
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
out=${OUT:-bench_out}
mkdir -p $out
timeout 900 python bench.py --full --no-cpu-baseline --no-train-leg --no-oxford-leg --no-pinned-leg > $out/r06_j_bench.json 2> $out/r06_j_bench.err
tail -4 $out/r06_j_bench.err
python - "$out/r06_j_bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print('value', d['value'], 'matched', d['matched_precision']['value'], d['matched_precision']['ms_per_step'], 'lib', d['matched_precision']['fp32_library_gemm']['value'], 'x6 frac', d['matched_precision']['roofline']['frac'])
PY
