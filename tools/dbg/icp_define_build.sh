#!/bin/bash
# Developer tool: variants of the library that differ in -D flags of ONE source (default icp.hip), built in the build container
# from the cached objects of the product build (icp_flow_amd/csrc/_obj) -- no GPU minutes spent compiling:
#   bash tools/dbg/icp_define_build.sh "ICPFLOW_SHARE_MIN_W=128 ICPFLOW_SHARE_PART_MIN=64" "ICPFLOW_PROBE_MAX=32" ...
#   SWEEP_SRC=icp_plan.hip bash tools/dbg/icp_define_build.sh "ICPFLOW_TEAM_CHAIN=2" "ICPFLOW_TEAM_CHAIN=3" ...
# writes tools/dbg/sweep_<k>.so (+ sweep_<k>.txt with the flags); run them with tools/dbg/icp_define_run.sh in one gpurun call.
# SWEEP_SRC selects the ONE source that sees the flags, so a knob has to be swept with the source that reads it:
#   icp.hip (the default)       the knobs of the loop and its launch policy: ICPFLOW_PROBE_*, ICPFLOW_WIDE_WINDOW, ICPFLOW_SHARE_MIN_W,
#                               ICPFLOW_SHARE_PART_MIN, ICPFLOW_SHARE_MIN_N, ICPFLOW_HALF_CU_MIN_N, ICPFLOW_DRAIN_AT
#   SWEEP_SRC=icp_epilogue.hip  ICPFLOW_DEBUG_EXECUTED (the history epilogue reports the iterations a pair executed)
#   SWEEP_SRC=icp_plan.hip      the team plan's: ICPFLOW_TEAM_CHAIN, ICPFLOW_TEAM_MIN_SHARE, and ICPFLOW_SHARE_LAUNCH_MIN_N (icp_team_shares)
# (a knob of a header several sources read, ICPFLOW_MAX_TEAM of kernels.hpp among them, wants a whole variant: build.py --define)
cd "$(dirname "$0")/../.."
SRC=${SWEEP_SRC:-icp.hip}
C=icp_flow_amd/csrc
python icp_flow_amd/build.py --force > /dev/null || exit 1   # (every object of the product in the cache; only what is missing compiles)
# the compile flags and the product's other objects are build.py's: nothing is repeated here
BUILD='import sys; sys.path.insert(0, "icp_flow_amd"); import build'
CFLAGS=$(python -c "$BUILD; print(*build.CFLAGS)")
OTHERS=$(python -c "$BUILD; print(*[argv[-1] for src, argv in build.plan()['compile'].items() if src != '$SRC'])")
rm -f tools/dbg/sweep_*.so tools/dbg/sweep_*.txt
k=0
for DEFS in "$@"; do
  k=$((k+1))
  FLAGS=""; for d in $DEFS; do FLAGS="$FLAGS -D$d"; done
  echo "$DEFS" > tools/dbg/sweep_$k.txt
  ( /opt/rocm/bin/hipcc $CFLAGS $FLAGS -c $C/$SRC -o /tmp/sweep_$k.o 2>&1 | grep -v warning | head -5
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OTHERS /tmp/sweep_$k.o -o tools/dbg/sweep_$k.so && echo "built sweep_$k [$DEFS]" ) &
  [ $((k % ${SWEEP_JOBS:-6})) -eq 0 ] && wait
done
wait
