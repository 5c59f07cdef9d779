#!/bin/bash
# Same-box A/B of two builds / settings of the benchmark (boxes differ by +-3 %, so nothing is compared across gpurun calls):
#   tools/ab.sh "<env A>" "<env B>" [rounds] [extra bench args]     e.g.  tools/ab.sh "ACCFLOW_HIP_LIB=tools/bin/lib_ref/libaccflow_hip.so" ""
# prints ms/step (pipelined), conv family TFLOP/s and ms/step one sequence at a time for every run.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
A="$1"; B="$2"; R="${3:-2}"; shift; shift; shift || true
O="${AB_OUT:-out/ab}"   # the last run of A and of B: JSON line, stderr, per-shape table
mkdir -p "$O"
for i in $(seq 1 $R); do
  for v in A B; do
    if [ $v = A ]; then E="$A"; else E="$B"; fi
    env $E timeout 600 python bench.py --full --no-strict --no-extra --no-cpu-baseline --no-parity --steps 8 "$@" --dump-kernels "$O/conv_shapes_$v.txt" > "$O/bench_$v.json" 2> "$O/bench_$v.err" || echo "run $v failed"
    python - "$v" "$E" "$O" <<'PY'
import json, sys
v, e, o = sys.argv[1], sys.argv[2], sys.argv[3]
try:
    d = json.loads([l for l in open("%s/bench_%s.json" % (o, v)).read().strip().splitlines() if l.startswith("{")][-1])
    print("%s [%s]  %.3f ms/step  %.1f TFLOP/s conv  %.3f ms one-at-a-time" % (v, e, d["ms_per_step"], d["roofline"]["achieved"], d["one_sequence_at_a_time"]["ms_per_step"]))
except Exception as ex:
    print(v, "ERR", ex)
PY
  done
done
