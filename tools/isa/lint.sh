#!/bin/bash
# ISA lint of the hot kernels (no GPU needed: cross-compiles the device code, ~2 min).  From the repo root:
#   bash tools/isa/lint.sh
# Prints, per kernel, prefetches the scheduler has sunk to their first use (waits on a load issued <= 16 instructions
# earlier, near MFMAs) and the 200-instruction windows with >= 20 branches (wave-uniform tests left in per-value code).
set -e
tmp=$(mktemp -d)
dis() {  # source file -> listing
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Iinclude --cuda-device-only -c $1 -o $tmp/x.co
  /opt/rocm/lib/llvm/bin/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/x.co --output=$tmp/x.elf --unbundle
  /opt/rocm/lib/llvm/bin/llvm-objdump -d --no-show-raw-insn $tmp/x.elf > $2
}
dis graspldm_amd/csrc/resnet1d.hip $tmp/r1d.s   # r1d_kernel: the source includes every header of the family (r1d_*.h, quad*_narrow.h)
dis graspldm_amd/csrc/sa_mlp.hip $tmp/sa.s
dis graspldm_amd/csrc/pointwise_mlp.hip $tmp/pw.s
dis graspldm_amd/csrc/conv3d.hip $tmp/c3.s
dis graspldm_amd/csrc/voxel_norm.hip $tmp/vn.s
dis graspldm_amd/csrc/pointwise_small.hip $tmp/ps.s
dis graspldm_amd/csrc/point_attention.hip $tmp/pa.s
dis graspldm_amd/csrc/grasp_classifier.hip $tmp/gc.s
lst() {  # kernel -> the listing that holds it
  case $1 in r1d_*) echo $tmp/r1d.s;; sa_*) echo $tmp/sa.s;; pointwise_mlp*) echo $tmp/pw.s;; pointwise_*|linear_*|bias_*) echo $tmp/ps.s;; conv3d_*) echo $tmp/c3.s;; gn_*|groupnorm_*|se_*|devoxelize_*) echo $tmp/vn.s;; attn_*) echo $tmp/pa.s;; cls_*) echo $tmp/gc.s;; esac
}
for k in r1d_kernelILi64ELi4 r1d_kernelILi32ELi16 pointwise_mlp_sp_kernel attn_gemm_kernelILb0ELb0 attn_gemm_kernelILb0ELb1 cls_head_kernelILb0 cls_head_kernelILb1; do python3 tools/isa/sunk_prefetch_scan.py $(lst $k) $k; python3 tools/isa/branch_density.py $(lst $k) $k; done
# hand-written DPP blocks (quad_narrow.h, quad16_narrow.h, mfma_prims.h): no VALU write closer than 2 wait states in front of a DPP read
# of the same register -- nothing checks that inside an asm statement; fails the lint on any hit
rc=0
for k in r1d_kernelILi64ELi4 r1d_kernelILi64ELi16 r1d_kernelILi32ELi4 r1d_kernelILi32ELi16 sa_mlp3_kernel sa_mlp2_kernel pointwise_mlp_sp_kernel attn_gemm_kernelILb0ELb0 attn_gemm_kernelILb0ELb1 attn_gemm_kernelILb1ELb0 cls_head_kernelILb0 cls_head_kernelILb1; do
  python3 tools/isa/dpp_hazard_scan.py $(lst $k) $k || rc=1
done
python3 tools/isa/dpp_hazard_scan.py $(lst conv3d_k3) conv3d_k3 || rc=1
for k in conv3d_k3_pl_kernelILi3ELi24ELi24ELi8ELb1 conv3d_k3_pl_kernelILi6ELi12ELi12ELi4ELb0 conv3d_k3_kernelILi3ELi6ELi4; do python3 tools/isa/sunk_prefetch_scan.py $(lst $k) $k; python3 tools/isa/branch_density.py $(lst $k) $k; done
rm -rf $tmp
exit $rc
