// voxel_geom.h -- the geometry that the voxel convs (conv3d.hip) and what reads their results (voxel_norm.hip) agree on.
#pragma once

namespace {

// A conv workgroup owns a brick of kBrick x kBrick x r output voxels (the whole z axis) for all output channels and
// leaves the brick's per-channel statistics for GroupNorm:
//   partial[cloud][brick = bx * bricks_per_axis + by][channel][sum | sum of squares]        (f32)
// which the norm kernels add in f64, bricks in index order.  gldm_conv3d_partial_floats sizes it.
constexpr int kBrick = 4;
constexpr int bricks_per_axis(int r) { return (r + kBrick - 1) / kBrick; }   // edge bricks are partial where r % kBrick != 0
constexpr int bricks_per_cloud(int r) { return bricks_per_axis(r) * bricks_per_axis(r); }

// The SE squeeze over a channel-last tensor leaves kSumParts partial sums per (cloud, channel), added in index order
// by the gate kernel (gldm_squeeze_parts tells the caller).
constexpr int kSumParts = 8;

}  // namespace
