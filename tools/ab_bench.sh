# A/B of two builds of the library in ONE gpurun call (box-to-box variance is larger than most single changes):
#   cp graph_pooling_amd/libdiffpool_hip.so graph_pooling_amd/libdiffpool_hip_base.so   (the baseline build)
#   ... rebuild with the change ...
#   gpurun -- 'bash tools/ab_bench.sh [bench args]'
# alternates base / new three times (AB_PAIRS=n: n times) and prints ms_per_step of each run.  Every run has a time
# limit of its own (AB_RUN_LIMIT seconds, default 180), and the first run that fails ends the script: nothing more is
# started on a GPU that a run may have left in a bad state.
R=${GRAFT_REPO_ROOT:-.}
cd $R
for i in $(seq ${AB_PAIRS:-3}); do
  for v in base new; do
    if [ $v = base ]; then L=$R/graph_pooling_amd/libdiffpool_hip_base.so; else L=$R/graph_pooling_amd/libdiffpool_hip.so; fi
    out=$(DP_LIB=$L timeout -k 10 ${AB_RUN_LIMIT:-180} python3 bench.py --no-cpu-baseline "$@" 2>/dev/null)
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v run failed (exit $rc): stopping"; exit $rc; fi
    ms=$(echo "$out" | python3 -c "import json,sys; print(json.loads(sys.stdin.read())['ms_per_step'])") || exit 1
    echo "$v $ms"
  done
done
