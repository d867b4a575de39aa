// voxel_geom.h -- the geometry that the voxel convs (conv3d.hip) and what reads their results (voxel_norm.hip) agree on,
// and the trilinear cell that the three devoxelize kernels (voxel_points.hip, voxel_norm.hip) agree on.
#pragma once
#include <hip/hip_runtime.h>

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

// Trilinear devoxelize: the 8 corners of the voxel cell around a point (x, y, z) in grid units of an r^3 grid
// (coordinates already clamped to [0, r - 1]), corner k = 4 dx + 2 dy + dz: its weight and its flat index
// (x r^2 + y r + z).  A point ON a voxel face along an axis (fraction 0) has no upper neighbour there: the upper
// corners take the lower index (the `> 0` tests), so x = r - 1 never reads outside the grid; their weight is 0 anyway.
// Products, single subtractions and integer arithmetic only: the same bits with and without fp contraction.  The 8-term
// sum is each kernel's own.
__device__ __forceinline__ void trilinear_corners(float x, float y, float z, int r, float (&w)[8], int (&idx)[8]) {
  const int r2 = r * r;
  const float xl = floorf(x), yl = floorf(y), zl = floorf(z);
  const float xd1 = x - xl, yd1 = y - yl, zd1 = z - zl;
  const float xd0 = 1.0f - xd1, yd0 = 1.0f - yd1, zd0 = 1.0f - zd1;
  w[0] = xd0 * yd0 * zd0; w[1] = xd0 * yd0 * zd1; w[2] = xd0 * yd1 * zd0; w[3] = xd0 * yd1 * zd1;
  w[4] = xd1 * yd0 * zd0; w[5] = xd1 * yd0 * zd1; w[6] = xd1 * yd1 * zd0; w[7] = xd1 * yd1 * zd1;
  const int zh = zd1 > 0 ? 1 : 0, yh = yd1 > 0 ? r : 0, xh = xd1 > 0 ? r2 : 0;
  idx[0] = (int)xl * r2 + (int)yl * r + (int)zl;
  idx[1] = idx[0] + zh; idx[2] = idx[0] + yh; idx[3] = idx[2] + zh;
  idx[4] = idx[0] + xh; idx[5] = idx[4] + zh; idx[6] = idx[4] + yh; idx[7] = idx[6] + zh;
}

}  // namespace
