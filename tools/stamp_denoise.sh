#!/bin/bash
# Per-op cycle stamps of one denoise step (diagnostic build).  Run from the repo root on a machine with the MI355X:
#   bash tools/stamp_denoise.sh [tag]      -> graspldm_amd/csrc/build/stamp_<tag>.txt
# builds graspldm_amd/csrc/build/libgldm_hip_dbg.so (-DGLDM_DEBUG_KNOBS, plus $EXTRA_DEFS) and runs it: one stamped launch,
# then one plain launch of the benchmark's shape; the second does not start when the first fails or runs out of time.
set -e
tag=${1:-cur}
out=graspldm_amd/csrc/build/stamp_$tag.txt
# make does not see a change of EXTRA_DEFS: drop the objects of every source that includes a header of the r1d family
for f in $(grep -lE '#include "(r1d_|quad_narrow|quad16_narrow|diffusion_step)' graspldm_amd/csrc/*.hip); do
  rm -f graspldm_amd/csrc/build/dbg/$(basename $f .hip).o
done
make -C graspldm_amd/csrc EXTRA="-DGLDM_DEBUG_KNOBS $EXTRA_DEFS" BUILD=$PWD/graspldm_amd/csrc/build/dbg OUT=$PWD/graspldm_amd/csrc/build/libgldm_hip_dbg.so -j4 2>&1 | grep -i "error\|warning: v" || true
export GLDM_LIB=graspldm_amd/csrc/build/libgldm_hip_dbg.so
GLDM_R1D_STAMP=1 timeout -k 10 240 python tools/run_denoise_once.py 4096 20 > $out 2>&1 &&
  timeout -k 10 240 python tools/run_denoise_once.py 5120 100 >> $out 2>&1 || { echo "a run failed: see $out"; tail -5 $out; exit 1; }
tail -45 $out
