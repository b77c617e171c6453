#!/bin/bash
# Developer tool: build a debug variant of the library next to the product one.
#   tools/dbg/build_debug.sh ICPFLOW_CERT_STATS tools/dbg/libicpflow_dbg.so ; ICPFLOW_HIP_LIB=tools/dbg/libicpflow_dbg.so python tools/dbg/...
set -e
cd "$(dirname "$0")/../.."
DEF=$1; OUT=${2:-tools/dbg/libicpflow_dbg.so}
python icp_flow_amd/build.py --define "$DEF" --out "$OUT" > /dev/null   # (sources, headers and flags: build.py's, the only list)
echo built $OUT
