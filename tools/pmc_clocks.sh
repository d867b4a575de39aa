#!/bin/bash
# Effective shader clock and MFMA-pipe occupancy per kernel of one bench pass (one PMC run, kernel trace only):
#   bash tools/pmc_clocks.sh <tag> [out_dir]   -> <out_dir>/clk_<tag>.txt (out_dir: pmc_out/ in the repo root)
tag=${1:-x}
R=${GRAFT_REPO_ROOT:-$PWD}
out=${2:-$R/pmc_out}
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --output-format csv --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES -d $out/clk_$tag -o run -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --streams 1 > $out/clk_$tag.log 2>&1
cd $R
python3 tools/pmc_clocks.py $out/clk_$tag | tee $out/clk_$tag.txt
