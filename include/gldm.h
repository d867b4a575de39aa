/*
 * gldm.h -- C ABI of libgldm_hip.so: the MI355X (gfx950) implementation of
 * GraspLDM's grasp-generation hot path.
 *
 * This is the drop-in boundary.  Every entry point takes
 * raw DEVICE pointers, plain sizes and an explicit HIP stream; outputs are
 * caller-allocated; nothing here allocates, frees, synchronises or exits the
 * process.  Return value: 0 = launched, negative = gldm_status (below).  All
 * tensors are dense, row-major, f32 / int32 exactly as in the reference:
 * coords [B,3,N], features [B,C,N], indices int32.
 *
 * "ref:" lines cite the reference interface each function replaces, relative
 * to /root/reference/grasp_ldm/models/modules/ext/pvcnn/modules/functional/src/
 * unless they start with grasp_ldm/ or tools/.
 */
#ifndef GLDM_H_
#define GLDM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *gldm_stream_t; /* hipStream_t; NULL = the null stream */

enum gldm_status {
  GLDM_OK = 0,
  GLDM_ERR_INVALID_ARG = -1, /* null pointer, non-positive size, unsupported shape */
  GLDM_ERR_LAUNCH = -2,      /* hipGetLastError() after the launch was not hipSuccess */
  GLDM_ERR_UNSUPPORTED = -3, /* shape outside what the kernels were built for */
  GLDM_ERR_WORKSPACE = -4    /* caller workspace too small */
};

/* ABI version (bumped on any signature change) and a static message per status.  gldm_abi_version() returns the
 * GLDM_ABI_VERSION the library was built with; the Python binding (graspldm_amd/_abi.py) is derived from this header and
 * compares the two, so a library built from another revision of the header is refused. */
#define GLDM_ABI_VERSION 15
int gldm_abi_version(void);
const char *gldm_status_string(int status);

/* ---------------------------------------------------------------- point ops */

/* ref: ball_query/ball_query.hpp:6-8, ball_query.cu:19-59 (pybind `ball_query`).
 * First `u` points (ascending index) with |p - c|^2 < radius^2 (strict, f32, no
 * FMA contraction); slots beyond the hit count repeat the first hit; all zero
 * when the ball is empty.  Writes every slot of out[b,m,u]. */
int gldm_ball_query(const float *centers /*[b,3,m]*/, const float *points /*[b,3,n]*/,
                    int b, int n, int m, float radius, int u,
                    int32_t *out /*[b,m,u]*/, gldm_stream_t stream);

/* ref: grouping/grouping.hpp:6, grouping.cu:18-44 (pybind `grouping_forward`).
 * out[b,c,j,k] = features[b,c,idx[b,j,k]]. */
int gldm_grouping_forward(const float *features /*[b,c,n]*/, const int32_t *idx /*[b,m,u]*/,
                          int b, int c, int n, int m, int u,
                          float *out /*[b,c,m,u]*/, gldm_stream_t stream);

/* ref: sampling/sampling.hpp:6, sampling.cu:17-39 (pybind `gather_features_forward`).
 * out[b,c,j] = features[b,c,idx[b,j]]. */
int gldm_gather_features_forward(const float *features /*[b,c,n]*/, const int32_t *idx /*[b,m]*/,
                                 int b, int c, int n, int m,
                                 float *out /*[b,c,m]*/, gldm_stream_t stream);

/* ref: sampling/sampling.hpp:10, sampling.cpp:43-58, sampling.cu:86-174
 * (pybind `furthest_point_sampling`).  Iterative FPS from index 0; tie rule of
 * the reference's 512-thread tree (max distance, then min (k mod 512), then
 * min k).  Distances live on chip; no scratch buffer.  n <= 8192. */
int gldm_furthest_point_sampling(const float *coords /*[b,3,n]*/, int b, int n, int m,
                                 int32_t *out_idx /*[b,m]*/, gldm_stream_t stream);

/* ref: interpolate/neighbor_interpolate.hpp:7-10, neighbor_interpolate.cu:20-131
 * (pybind `three_nearest_neighbors_interpolate_forward`). */
int gldm_three_nn_interpolate_forward(const float *points /*[b,3,n]*/, const float *centers /*[b,3,m]*/,
                                      const float *center_features /*[b,c,m]*/,
                                      int b, int c, int m, int n,
                                      float *out /*[b,c,n]*/, int32_t *idx /*[b,3,n]*/, float *wgt /*[b,3,n]*/,
                                      gldm_stream_t stream);

/* ref: voxelization/vox.hpp:7-9, vox.cpp:17-43, vox.cu:18-72,112-119
 * (pybind `avg_voxelize_forward`).  Deterministic: each voxel's mean is summed
 * in ascending point index (the reference uses f32 atomics in arbitrary order).
 * Writes all of out/ind/cnt (no pre-zeroing needed).  n <= 8192, r <= 64. */
int gldm_avg_voxelize_forward(const float *features /*[b,c,n]*/, const int32_t *vox_coords /*[b,3,n]*/,
                              int b, int c, int n, int r,
                              float *out /*[b,c,r^3]*/, int32_t *ind /*[b,n]*/, int32_t *cnt /*[b,r^3]*/,
                              gldm_stream_t stream);

/* ref: interpolate/trilinear_devox.hpp:7-10, trilinear_devox.cpp:18-55,
 * trilinear_devox.cu:21-105 (pybind `trilinear_devoxelize_forward`).
 * inds/wgts [b,8,n] are written only when is_training != 0 (may be NULL otherwise). */
int gldm_trilinear_devoxelize_forward(const float *coords /*[b,3,n]*/, const float *features /*[b,c,r^3]*/,
                                      int b, int c, int n, int r, int is_training,
                                      float *out /*[b,c,n]*/, int32_t *inds, float *wgts,
                                      gldm_stream_t stream);

/* ref: grasp_ldm/models/modules/ext/pvcnn/modules/voxelization.py:16-35
 * (Voxelization.forward before F.avg_voxelize): mean-centre, scale to [0,r-1]
 * (normalize != 0: divide by 2*max|p| + eps and add 0.5; else (p+1)/2), clamp,
 * round-half-even.  The per-axis mean is accumulated in f64 in a fixed tree. */
int gldm_voxel_coords(const float *coords /*[b,3,n]*/, int b, int n, int r, int normalize, float eps,
                      float *norm_coords /*[b,3,n]*/, int32_t *vox_coords /*[b,3,n]*/,
                      gldm_stream_t stream);

/* ------------------------------------------------ raw-cloud front end */

/* ref: grasp_ldm/utils/pointcloud_helpers.py:160-217 (PointCloudHelpers.farthest_points with
 * distance_by_translation_point :219-223, as called by regularize_pc_point_count :124-158): greedy
 * farthest-point selection on a sensor-layout cloud [b,n,3].  First centre = index 0 (np.argmax of
 * the all-1e7 start vector), distance = sqrt((dx^2 + dy^2) + dz^2) in f32, ties -> lowest index.
 * m <= n <= 8192.  Bit-identical indices to the numpy routine on f32 input. */
int gldm_farthest_points_euclid(const float *points /*[b,n,3]*/, int b, int n, int m,
                                int32_t *out_idx /*[b,m]*/, gldm_stream_t stream);

/* The same selection for clouds beyond one workgroup: 8192 < n <= 2^22 rows per cloud, 1 <= m <= min(n, 8192)
 * (GLDM_ERR_UNSUPPORTED outside, checked before any pointer; m = 0 is a no-op).  ref: pointcloud_helpers.py:162-223, the
 * contract of gldm_farthest_points_euclid word for word: start at index 0, sqrt((dx^2 + dy^2) + dz^2) in f32, running
 * minimum from 1e7, pick = largest distance, lowest index on ties; bit-identical indices.
 * counts [b] (device, may be NULL = every cloud has n rows): the live rows of each cloud, all with row stride n, so the
 * frames of one gldm_depth_to_cloud call go through one call; no row past counts[b] is read.  A cloud with counts[b] <= m
 * gets 0 .. counts[b]-1 followed by -1 (the reference's nclusters >= N -> arange, :185-191).
 * workspace: gldm_farthest_points_euclid_large_workspace_bytes(b, n) bytes, 8-byte aligned, uninitialised, private to the
 * stream until the work has finished (running minima [b, n] f32 + two sets of one 64-bit key per slice); smaller:
 * GLDM_ERR_WORKSPACE.  The bytes query returns a negative GLDM_ERR_* status for a shape outside the envelope.
 * One launch per round over (slices, b), enqueued back to back; returns without synchronising.
 * gldm_farthest_points_euclid_large_slice(n): the rows per slice (= per workgroup) at this n. */
long long gldm_farthest_points_euclid_large_workspace_bytes(int b, int n);
int gldm_farthest_points_euclid_large_slice(int n);
int gldm_farthest_points_euclid_large(const float *points /*[b,n,3]*/, const int32_t *counts /*[b] or NULL*/, int b, int n,
                                      int m, void *workspace, long long workspace_bytes, int32_t *out_idx /*[b,m]*/,
                                      gldm_stream_t stream);

/* The same selection over clouds of different sizes in one call: cloud i is rows start[i] .. start[i] + min(count[i], n_max)
 * of points [rows,3] (start / count: device int32 [b]; n_max: a host upper bound of the counts, counts above it are
 * clamped).  The rule of gldm_farthest_points_euclid word for word (start at the cloud's row 0, sqrt((dx^2 + dy^2) + dz^2)
 * in f32, minima from 1e7, largest distance, lowest index on ties, the same 64-bit key), so out_idx [b,m] holds, relative to
 * the cloud's start, exactly the indices the two entries above return for that cloud alone.  A cloud with count <= m gets
 * 0 .. count-1 followed by -1, count <= 0 all -1.  No row outside a cloud's range is read.
 * Envelope, checked before any pointer: 1 <= b <= 65535, 1 <= n_max <= 2^22, 0 <= m <= 8192 (GLDM_ERR_UNSUPPORTED beyond;
 * m = 0 is a no-op).  One launch serves every cloud of at most 8192 rows (one workgroup each); with n_max > 8192, m further
 * launches, one per round over (slices(n_max), b), serve the larger ones.  Returns without synchronising.
 * workspace: gldm_farthest_points_euclid_ragged_workspace_bytes(b, n_max) bytes, 8-byte aligned, uninitialised, private to
 * the stream until the work has finished; 0 for n_max <= 8192, and workspace may then be NULL. */
long long gldm_farthest_points_euclid_ragged_workspace_bytes(int b, int n_max);
int gldm_farthest_points_euclid_ragged(const float *points /*[rows,3]*/, const int32_t *start /*[b]*/,
                                       const int32_t *count /*[b]*/, int b, int n_max, int m, void *workspace,
                                       long long workspace_bytes, int32_t *out_idx /*[b,m]*/, gldm_stream_t stream);

/* ref: grasp_ldm/utils/camera.py:176-215 (Camera.depth_to_pointcloud_torch): depth frames -> ordered clouds.
 * depth [frames,h,w]: f32 metres (depth_is_u16 = 0) or u16 raw units (1; d = f32(raw) * depth_scale).  mask [frames,h,w]
 * u8 or NULL, nonzero = keep.  A pixel (u, v) is kept iff d > z_min && d <= z_max (NaN never passes; z_max = FLT_MAX drops
 * inf), the mask is nonzero, and, with a box, lo <= p' <= hi on all three axes.  Each step rounds once in f32 (no
 * contraction, IEEE division):  x = ((f32(u) - cx) * d) / fx,  y = ((f32(v) - cy) * d) / fy,  z = d;  with cam_to_world
 * (host, 3 x 4 row major, or NULL)  p'_i = ((R_i0*x + R_i1*y) + R_i2*z) + t_i.  box_lo / box_hi (host [3], both or
 * neither) are in the output frame.
 * Kept pixels of a frame come out in ascending pixel index v*w + u (the row-major order of torch.where(depth > 0)):
 * points [frames, h*w, 3] rows 0 .. count[f]-1, rows past count[f] are not written; count [frames] int32; pixel
 * [frames, h*w] int32 (the source pixel of every row) or NULL.
 * Envelope, checked before any pointer or the device is touched: frames >= 1, 1 <= h*w <= 2^24, frames <= 65535
 * (GLDM_ERR_UNSUPPORTED beyond), fx, fy != 0, z_min < z_max (GLDM_ERR_INVALID_ARG).
 * workspace: gldm_depth_to_cloud_workspace_bytes(frames, h, w) bytes (one int32 per tile; a negative GLDM_ERR_* status for a
 * shape outside the envelope), uninitialised, private to the stream until the work has finished.  Two launches, no
 * workgroup waits for another.  gldm_depth_to_cloud_tile_pixels(): the pixels per tile (= per workgroup). */
long long gldm_depth_to_cloud_workspace_bytes(int frames, int h, int w);
int gldm_depth_to_cloud_tile_pixels(void);
int gldm_depth_to_cloud(const void *depth /*[frames,h,w] f32 or u16*/, int depth_is_u16, float depth_scale,
                        const uint8_t *mask /*[frames,h,w] or NULL*/, int frames, int h, int w,
                        float fx, float fy, float cx, float cy, float z_min, float z_max,
                        const float *cam_to_world /*host [12] or NULL*/, const float *box_lo /*host [3] or NULL*/,
                        const float *box_hi /*host [3] or NULL*/, void *workspace, long long workspace_bytes,
                        float *points /*[frames,h*w,3]*/, int32_t *count /*[frames]*/, int32_t *pixel /*[frames,h*w] or NULL*/,
                        gldm_stream_t stream);

/* Labelled frames: every object's ordered cloud in one pass (additive; the reference has no counterpart).  Everything of
 * gldm_depth_to_cloud plus labels [frames,h,w] int32 and num_labels K: a pixel belongs to object k (1 .. K) iff its label
 * is k and gldm_depth_to_cloud's predicate keeps it; labels <= 0 or > K are background.
 * points [frames, h*w, 3]: inside a frame the objects lie one after another in ascending label, inside an object the
 * pixels in ascending pixel index; start / count [frames, K] int32: object (f, k+1) is rows start[f][k] .. + count[f][k] of
 * frame f (start relative to the frame's row 0; an absent label has count 0); pixel [frames, h*w] int32 or NULL.  Rows past
 * a frame's total are not written.  The rows, count and pixels of object (f, k) are bit-identical to what
 * gldm_depth_to_cloud writes for frame f with mask = (labels == k) & mask (the same inlined arithmetic).
 * Envelope, checked before any pointer or the device is touched: gldm_depth_to_cloud's, and 1 <= K (GLDM_ERR_INVALID_ARG)
 * <= 64 (GLDM_ERR_UNSUPPORTED).
 * workspace: gldm_depth_to_objects_workspace_bytes(frames, h, w, K) bytes (one int32 per (label, tile); a negative
 * GLDM_ERR_* status outside the envelope), uninitialised, private to the stream until the work has finished.  Three
 * launches (per-tile per-label counts, a scan over the tiles of every (frame, label), the write pass); no workgroup waits
 * for another. */
long long gldm_depth_to_objects_workspace_bytes(int frames, int h, int w, int num_labels);
int gldm_depth_to_objects(const void *depth /*[frames,h,w] f32 or u16*/, int depth_is_u16, float depth_scale,
                          const uint8_t *mask /*[frames,h,w] or NULL*/, const int32_t *labels /*[frames,h,w]*/,
                          int num_labels, int frames, int h, int w, float fx, float fy, float cx, float cy, float z_min,
                          float z_max, const float *cam_to_world /*host [12] or NULL*/,
                          const float *box_lo /*host [3] or NULL*/, const float *box_hi /*host [3] or NULL*/,
                          void *workspace, long long workspace_bytes, float *points /*[frames,h*w,3]*/,
                          int32_t *start /*[frames,K]*/, int32_t *count /*[frames,K]*/,
                          int32_t *pixel /*[frames,h*w] or NULL*/, gldm_stream_t stream);

/* ------------------------------------------------ tabletop segmentation (the reference has no counterpart)
 * Arithmetic of all three entries: f32, every product, difference, sum, quotient and square root rounds once, in the written
 * order (no contraction, IEEE division and sqrt).  A point q is an INLIER of plane (nx, ny, nz, d) iff
 *   fabsf(((nx*qx + ny*qy) + nz*qz) + d) <= tol        (NaN never passes).
 *
 * gldm_plane_ransac: T plane hypotheses against N points.  points [n,3] f32; triples [t,3] int32 (device).  For the triple
 * (i, j, k) with p0, p1, p2 the points at i, j, k:  e1 = p1 - p0, e2 = p2 - p0,
 *   c = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x),  l2 = (cx*cx + cy*cy) + cz*cz,  n = c / sqrtf(l2),
 *   d = -((nx*p0x + ny*p0y) + nz*p0z).
 * out_plane [t,4] = (nx, ny, nz, d), out_count [t] = the exact number of inliers among the n points.  A hypothesis with a
 * repeated index, an index outside [0, n) or !(l2 >= min_cross2) is degenerate: plane 0, count -1.
 * Envelope, checked before any pointer or the device is touched: 1 <= n (GLDM_ERR_INVALID_ARG) <= 2^24
 * (GLDM_ERR_UNSUPPORTED), 1 <= t (INVALID_ARG) <= 4096 (UNSUPPORTED), tol and min_cross2 not NaN (INVALID_ARG).
 * workspace: gldm_plane_ransac_workspace_bytes(n, t) bytes (a negative GLDM_ERR_* status outside the envelope),
 * uninitialised, private to the stream until the work has finished.  Two launches; counts are combined with integer
 * atomics, so two calls are bitwise equal; no workgroup waits for another.  gldm_plane_ransac_tile_points(): the points
 * per workgroup of the count launch. */
long long gldm_plane_ransac_workspace_bytes(int n, int t);
int gldm_plane_ransac_tile_points(void);
int gldm_plane_ransac(const float *points /*[n,3]*/, int n, const int32_t *triples /*[t,3]*/, int t, float tol,
                      float min_cross2, void *workspace, long long workspace_bytes, float *out_plane /*[t,4]*/,
                      int32_t *out_count /*[t]*/, gldm_stream_t stream);

/* Moments of the inliers of one plane (host [4]) for a least-squares refit: out [10] f64 (device) = count, Sx, Sy, Sz, Sxx,
 * Sxy, Sxz, Syy, Syz, Szz.  Products are taken in f64 from the f32 coordinates (exact).  The order of summation is fixed:
 * per-tile partial sums in a fixed tree, then one workgroup over the tiles in ascending order, so two calls are bitwise
 * equal.  Envelope: 1 <= n <= 2^24 as above, tol not NaN.  workspace: gldm_plane_moments_workspace_bytes(n) bytes (10 f64
 * per tile), 8-byte aligned, uninitialised.  Two launches. */
long long gldm_plane_moments_workspace_bytes(int n);
int gldm_plane_moments(const float *points /*[n,3]*/, int n, const float *plane /*host [4]*/, float tol, void *workspace,
                       long long workspace_bytes, double *out /*[10]*/, gldm_stream_t stream);

/* One depth frame -> an instance-label image of the objects standing on a table.  depth / mask / intrinsics / window /
 * cam_to_world / box: those of gldm_depth_to_cloud with frames = 1 (the same inlined predicate and deprojection).
 *   foreground  the pixel is kept by that predicate and hgt = ((a*x + b*y) + c*z) + d of its point (x, y, z) under
 *               plane = (a, b, c, d) (host [4]) satisfies hgt > h_min && hgt <= h_max
 *   links       two 4-neighbours are linked iff both are foreground and ((dx*dx + dy*dy) + dz*dz) <= link2, dx, dy, dz the
 *               differences of their points, link2 = link_dist * link_dist formed once in f32 on the host
 *   components  the transitive closure of the links; a component's root is its lowest pixel index v*w + u
 *   labels      components of at least min_pixels pixels, ranked by falling pixel count, ties to the lower root; the first
 *               max_labels of them are labels 1 .. K, every other pixel is 0
 * labels [h,w] int32: every pixel written; num_labels [1] = K; label_pixels / label_root [max_labels]: pixel count and root
 * of label k + 1, 0 / -1 past K.  All four are exact and independent of the execution order.
 * Envelope, checked before any pointer or the device is touched: h, w >= 1 (GLDM_ERR_INVALID_ARG), h*w <= 2^24
 * (GLDM_ERR_UNSUPPORTED), gldm_depth_to_cloud's conditions on fx, fy, cx, cy, z_min, z_max, h_min < h_max, link_dist >= 0
 * (inf allowed), min_pixels >= 1, 1 <= max_labels (INVALID_ARG) <= 64 (UNSUPPORTED), no NaN in plane.
 * workspace: gldm_segment_tabletop_workspace_bytes(h, w) bytes (16 per pixel + 8), 8-byte aligned, uninitialised, private
 * to the stream until the work has finished.  Six launches back to back (union-find inside tiles in LDS, unions across
 * tile edges, flatten + sizes, candidate roots, top-K selection in one workgroup, write), no host round trip.  Unions hang
 * the higher root under the lower, so every find / union loop ends on its own data and no workgroup waits for another.
 * gldm_segment_tile_shape: the tile of the first launch (pixels wide, pixels high). */
long long gldm_segment_tabletop_workspace_bytes(int h, int w);
int gldm_segment_tile_shape(int *tw, int *th);
int gldm_segment_tabletop(const void *depth /*[h,w] f32 or u16*/, int depth_is_u16, float depth_scale,
                          const uint8_t *mask /*[h,w] or NULL*/, int h, int w, float fx, float fy, float cx, float cy,
                          float z_min, float z_max, const float *cam_to_world /*host [12] or NULL*/,
                          const float *box_lo /*host [3] or NULL*/, const float *box_hi /*host [3] or NULL*/,
                          const float *plane /*host [4]*/, float h_min, float h_max, float link_dist, int min_pixels,
                          int max_labels, void *workspace, long long workspace_bytes, int32_t *labels /*[h,w]*/,
                          int32_t *num_labels /*[1]*/, int32_t *label_pixels /*[max_labels]*/,
                          int32_t *label_root /*[max_labels]*/, gldm_stream_t stream);

/* ref: tools/inference.py:570-591 (InferenceLDM.normalize_input) and
 * grasp_ldm/inference/inference_base.py:181-212: pc_out = ((pc - mean_points(pc)) - shift) / scale
 * per axis (shift = _INPUT_PC_SHIFT, scale = _INPUT_PC_SCALE of set_normalization_params :103-130),
 * mean_out[b,:] = per-cloud mean (f64 accumulation, rounded once). */
int gldm_normalize_cloud(const float *pc /*[b,n,3]*/, int b, int n, float shift_x, float shift_y, float shift_z,
                         float scale_x, float scale_y, float scale_z,
                         float *pc_out /*[b,n,3]*/, float *mean_out /*[b,3]*/, gldm_stream_t stream);

/* out[b,j,:] = pc[b,idx[b,j],:]  (row gather behind every point-count regularisation:
 * pointcloud_helpers.py:40-71,124-158). */
int gldm_gather_points(const float *pc /*[b,n,3]*/, const int32_t *idx /*[b,m]*/, int b, int n, int m,
                       float *out /*[b,m,3]*/, gldm_stream_t stream);

/* ------------------------------------------------------- set abstraction */

/* ref: grasp_ldm/models/modules/ext/pvcnn/modules/ball_query.py:16-34
 * (BallQuery.forward = ball_query + grouping(coords) - centre + grouping(features)
 * + concat) as ONE kernel: the "set-abstraction gather".  features may be NULL
 * (c = 0).  out[b, 0:3, j, k] = p[idx] - centre_j ; out[b, 3:3+c, j, k] = f[idx].
 * idx_out [b,m,u] is optional (NULL to skip). */
int gldm_sa_group(const float *points /*[b,3,n]*/, const float *centers /*[b,3,m]*/,
                  const float *features /*[b,c,n] or NULL*/,
                  int b, int c, int n, int m, float radius, int u,
                  float *out /*[b,3+c,m,u]*/, int32_t *idx_out, gldm_stream_t stream);

/* Multi-scale set abstraction (pointnet.py:49-114 with lists of radii): replaces ball_query.cu:19-59 run once per
 * scale.  ONE scan of a cloud's points per centre for n_scales radii (1..4); out[s] [b,m,u[s]] is bit-identical to
 * gldm_ball_query(radius[s], u[s]).  radius, u and out are HOST arrays of n_scales entries (out: device pointers). */
int gldm_ball_query_multi(const float *centers /*[b,3,m]*/, const float *points /*[b,3,n]*/, int b, int n, int m,
                          int n_scales, const float *radius, const int32_t *u, int32_t *const *out,
                          gldm_stream_t stream);

/* Replaces pointnet.py:104-109 (the max over a scale's neighbours where a U = 64 h neighbourhood ran as h centres of
 * 64, and the torch.cat of the scales): out[b, c0 + r, j] = max over part[b, r, j h .. j h + h - 1], h in {1, 2, 4};
 * the other rows of out [b,ctot,m] are not touched. */
int gldm_group_max_concat(const float *part /*[b,c,m*h]*/, int b, int c, int m, int h,
                          float *out /*[b,ctot,m]*/, int c0, int ctot, gldm_stream_t stream);


/* ------------------------------------- 1-D ResNet engine (denoiser, decoder) */

/* Architecture descriptor of one ResNet1D / TimeConditionedResNet1D instance
 * (ref: grasp_ldm/models/modules/resnets.py:263-424,427-616) plus offsets, in
 * floats, into ONE packed weight buffer prepared on the host at load time
 * (graspldm_amd/r1d_pack.py): weight-standardised conv weights, MFMA
 * A-fragment order, combined scale/shift biases.  Plain C struct, filled by the
 * host side; the kernels never parse checkpoints. */
#define GLDM_R1D_MAX_LEVELS 6
#define GLDM_R1D_MAX_RESBLOCKS (2 * GLDM_R1D_MAX_LEVELS + 1)

typedef struct gldm_r1d_resblock {
  int32_t c1_w, c1_b;   /* block1.proj  (packed A fragments), bias [C]            */
  int32_t n1_w, n1_b;   /* block1.norm  gamma/beta [C]                            */
  int32_t c2_w, c2_b;   /* block2.proj                                            */
  int32_t n2_w, n2_b;   /* block2.norm                                            */
  int32_t ss_w, ss_b;   /* mlp.1 as a [2C x E] GEMM (packed A fragments) and the
                           combined bias R*b (+R on the C scale rows): [2C]       */
  int32_t c1_w3, c2_w3; /* ABI 5: the two conv weights again as split-f16 fragments (see below);
                           0 = absent                                              */
  int32_t c1_wq, c2_wq; /* ABI 9: the same fragments with the columns of every 32-channel block in
                           "quad" order (see below); 0 = absent                    */
} gldm_r1d_resblock;

typedef struct gldm_r1d_level {
  int32_t ln_g;         /* PreNorm LayerNorm gain [C]                             */
  int32_t qkv_w[2];     /* to_qkv rows for heads {0,1} and {2,3}: 192 x C packed  */
  int32_t out_w, out_b; /* to_out.0 [C x 128] packed, bias [C]                    */
  int32_t ln2_g;        /* to_out.1 LayerNorm gain [C]                            */
  int32_t down_w, down_b; /* Conv1d(C -> C', k=3) packed, bias [C']               */
  int32_t qkvn_w;       /* ABI 4: to_qkv with the PreNorm gain folded in, W' = W diag(g), in to_qkv's own
                           row order (q | k | v, head h at rows 32 h of each third): 384 x C packed;
                           0 / negative = absent (the position-major engine is then not used)       */
  int32_t qkvn_s;       /* ABI 4: row sums of W' [384] (the mean term of the folded LayerNorm)     */
  int32_t qkvn_w3, out_w3, down_w3; /* ABI 5: qkvn_w / out_w / down_w as split-f16 fragments; 0 = absent */
  int32_t qkvn_wq, out_wq, down_wq; /* ABI 9: the same in quad column order; out_wq of a 4-channel level has
                                       channel ch in row 4 ch of its one m-tile; qkvn_wq = W' = W diag(g) with
                                       its q and k rows (the first 256) times log2(e): the engine multiplies it
                                       with the normalised column and exponentiates with 2^x; 0 = absent   */
} gldm_r1d_level;

/* Quad column order (ABI 9; r1d_pack.quad_perm32): the wave-local engine of the narrow levels (csrc/quad_narrow.h) feeds
 * a GEMM's B operand straight from the accumulator layout of the previous one -- lane (column, g) holds rows 4 g + r of
 * m-tiles 2 kb and 2 kb + 1 -- so k-slot 8 g + j of a 32-channel block kb stands for channel 32 kb + 16 (j >> 2) + 4 g +
 * (j & 3), and the weights' columns are stored in that order: W_q[:, 32 kb + 8 g + j] = W[:, 32 kb + 16 (j >> 2) + 4 g + (j & 3)].
 * 16-position nets (round 6, csrc/quad16_narrow.h: the 16 / 32 / 64-channel levels in front of a 128-channel one; one wave =
 * one sample's 16 positions): the same copies, taken from the weights with every tap's channels padded to whole 32-channel
 * blocks first (a 16-channel level is one block whose k-slots j >= 4 are zero): quad_perm32(pad_cin32(W, C, taps)).  Packers
 * that leave them 0 get the barrier-separated phases of the 64-column engine instead: same results, ~20 % slower. */

/* Split-f16 weight fragments (layout since ABI 5, two f16 planes since ABI 9; graspldm_amd/r1d_pack.py:
 * mfma_a_fragments_f16x2).  Every f32 weight is written as hi + lo, two f16 numbers (hi = f16(w), lo = f16(w - hi):
 * 2 x 11 significant bits, |w - hi - lo| <= 2^-22 |w|; |w| < 65504 or the packer raises); the matrix [M, K]
 * (K % 32 == 0) is stored as [M/16][K/32][plane hi|lo][lane 64][8 f16] = 2 KiB per fragment, lane l holding
 * W[16 mt + (l & 15)][32 kb + 8 (l >> 4) + j], j = 0..7: the A operand of v_mfma_f32_16x16x32_f16.  The 64-column
 * engines compute every f32 product as the three partial products hi*hi + hi*lo + lo*hi on the f16 matrix pipe with f32
 * accumulation (the pipe keeps f16 subnormals); the dropped lo*lo term is <= 2^-22 of |a||b| per product, the order of an
 * f32 rounding, at 3/16 of the f32-MFMA time.  (ABI 5-8 stored three bf16 planes, hi|mid|lo, for six products.) */

typedef struct gldm_r1d_desc {
  int32_t seq_len;      /* L: 4 (latent denoiser) or 16 (pose decoder)            */
  int32_t n_levels;
  int32_t dims[GLDM_R1D_MAX_LEVELS + 1]; /* channel widths; dims[0] = init_dim    */
  int32_t emb_dim;      /* E = 4 * dim                                            */
  int32_t cond_rows;    /* R: rows of the conditioning latent (3), 1 if 2-D       */
  int32_t groups;       /* GroupNorm groups (resnet_block_groups)                 */
  int32_t init_w, init_b; /* init_conv [C0][7], [C0]                              */
  int32_t ss_rows;      /* 2 * max(dims) (unused since ABI 2: the scale/shift rows are
                           computed in the conv epilogue; kept for layout)        */
  gldm_r1d_resblock rb[GLDM_R1D_MAX_RESBLOCKS]; /* 2 per level, then final        */
  gldm_r1d_level lv[GLDM_R1D_MAX_LEVELS];
  int32_t final_w, final_b; /* final_conv [dims[n_levels]], [1]                   */
  /* decoder only (ref: grasp_ldm/models/grasp_vae.py:358-436) */
  int32_t latent_dim;   /* D of z_h; 0 for the denoiser                           */
  int32_t in_w, in_b;   /* in_layer [L][D], [L]                                   */
  int32_t head_w, head_b; /* rows tmrp(6) then class_logits(1): [7][L], [7]       */
  int32_t n_head;       /* 7 (decoder) or 2 * latent size (encoder)               */
  int32_t head_kind;    /* ABI 11: GLDM_HEAD_DECODER (0: rows 0..5 tmrp, row 6 logit) or GLDM_HEAD_ENCODER: n_head = 2 Lz
                           rows [2 Lz][L], rows 0..Lz-1 = W_mu W_out, rows Lz..2 Lz-1 = W_logvar W_out, biases folded
                           likewise (grasp_vae.py:113-115,532-536: nothing sits between out_layer and the bottleneck);
                           Lz <= GLDM_R1D_MAX_LATENT */
} gldm_r1d_desc;
enum gldm_head_kind { GLDM_HEAD_DECODER = 0, GLDM_HEAD_ENCODER = 1 };
#define GLDM_R1D_MAX_LATENT 32

enum gldm_sched_kind { GLDM_SCHED_NONE = 0, GLDM_SCHED_DDIM = 1, GLDM_SCHED_DDPM = 2, GLDM_SCHED_DPMPP = 3 };
#define GLDM_SCHED_COEF_STRIDE 8
/* per-step coefficient row (f32, the table 16-byte aligned; computed on the host exactly like the
 * scheduler library does on 0-dim f32 tensors):
 *   [0] sqrt(1-abar_t) [1] sqrt(abar_t)
 *   DDIM: [2] sqrt(abar_prev) [3] sqrt(1-abar_prev-sigma^2)
 *   DDPM: [4] coef_x0 [5] coef_xt [6] sqrt(variance) [7] 1 if noise is added (t>0)
 * GLDM_SCHED_DPMPP (ref: grasp_ldm/models/diffusion/elucidated_diffusion.py:259-313, DPM-Solver++(2M) of
 * ElucidatedDiffusion; the network sees c_in x and time = c_noise(sigma), so `temb` holds one row per STEP and
 * timesteps = 0..n_steps-1; clip_sample = the sampler's `clamp`):
 *   [0] c_in [1] c_skip [2] c_out [3] 1-gamma [4] gamma [5] sigma_fn(t_next)/sigma_fn(t) [6] expm1(-h)
 *   [7] 1 if the previous step's denoised row is blended in (not on the first step, not when sigma_next = 0) */

/* ref: resnets.py:484-494,587-594 (input_emb_layers = Linear + SiLU on z_cond).
 * cemb[i,r,:] = silu(W z_cond[i,r,:] + b). */
int gldm_r1d_cond_embed(const float *z_cond /*[n_cond,R,Dc]*/, const float *w /*[E,Dc]*/, const float *b /*[E]*/,
                        int n_cond, int rows, int dc, int e, float *cemb /*[n_cond,R,E]*/, gldm_stream_t stream);

/* Bytes of workspace gldm_denoise / gldm_decode need for n_samples (-1 if the descriptor is not
 * supported: groups must be 4, widths powers of two in {4, 16, 32, 64, 128, 256}, at most 128 on levels
 * with attention, emb_dim % 16 == 0).  A step stays on chip; the workspace carries only the
 * work-distribution header (GLDM_R1D_WS_*: 256 bytes) and one 8-byte {latent value, tag} hand-off
 * granule per activation column, used when a batch does not fill whole rounds of workgroups and the
 * left-over tiles are split along the step axis over several workgroups.  For a pose-decoder descriptor
 * (seq_len 16, latent_dim > 0, emb_dim >= 32) it also holds, behind those, the ResnetBlocks' scale/shift
 * rows per conditioning cloud (4 bytes x n_samples x sum of 2 C over the blocks: sized for one grasp per
 * cloud), written by gldm_decode itself before the fused launch.  For a 16-position latent-denoiser
 * descriptor (the `ppc` experiment) of the 64-column engine whose last level has 256 channels it holds, behind the granules
 * (256-byte aligned), 64 KiB of scratch per workgroup of the launch (min(tiles, compute units)): the level's residual
 * stream is parked there, by the lanes that re-load it, while LDS holds its padded split-f16 planes (the 4-position
 * engine keeps both in LDS since ABI 9 and needs header + granules only).
 * Contract: the caller ZEROES the workspace once, when it allocates it; a workspace is used by one
 * launch at a time (launches on the same stream may share it, concurrent streams may not); the
 * library re-arms it at the end of every launch.  The 32-bit word at byte GLDM_R1D_WS_ERROR is set
 * to 1 if a hand-off wait ever ran into its (seconds long) bound: outputs of that launch are invalid. */
#define GLDM_R1D_WS_ERROR 12
long long gldm_r1d_workspace_bytes(const gldm_r1d_desc *desc, int n_samples);

/* Which engine gldm_denoise / gldm_decode run this descriptor on: 64 = the position-major engine (64-column tiles = 16
 * samples x 4 positions, or 4 samples x 16 positions; GEMMs as split-f16 products on the f16 matrix pipe: nets packed with
 * the split fields), 32 = the sample-major engine (32-column tiles, f32 matrix pipe: every other supported shape), or a negative GLDM_ERR_* status for a descriptor no engine takes.  No reference
 * counterpart: reporting only (bench.py labels its roofline record with it). */
int gldm_r1d_tile_columns(const gldm_r1d_desc *desc);

/* ref: grasp_ldm/models/diffusion/gaussian_diffusion.py:232-277 (sample loop:
 * eps = model(x, t, z_cond); x = scheduler.step(eps, t, x)) and
 * resnets.py:558-616 (TimeConditionedResNet1D.forward), fused: ONE launch runs
 * all n_steps for every latent; x stays on chip between steps.
 *  - sched_kind NONE with n_steps = 1 returns eps (= the module's forward);
 *    sample_t (optional, [n]) then gives a per-sample timestep.
 *  - temb is the host-precomputed time_mlp table [T, E] (resnets.py:517-522).
 *  - sample i is conditioned on cemb[i / samples_per_cond].
 *  - step_noise [n_steps, n, D] is read by DDPM steps with coef[7] != 0.
 *  - sample_emb [n, E] (optional) is added to the time embedding of each sample before the
 *    conditioning embedding: the class embedding of ClassTimeConditionedResNet1D
 *    (grasp_ldm/models/modules/class_conditioned_resnet.py:43-46,99-101). */
int gldm_denoise(const gldm_r1d_desc *desc, const float *weights, const float *temb, const float *cemb,
                 int samples_per_cond, const float *x_in /*[n,1,L]*/, int n_samples,
                 const int32_t *timesteps /*[n_steps]*/, const int32_t *sample_t, int n_steps,
                 int sched_kind, int clip_sample, const float *sched_coef /*[n_steps,8]*/,
                 const float *step_noise, const float *sample_emb, float *x_out /*[n,1,L]*/, void *workspace,
                 gldm_stream_t stream);

/* gldm_denoise for DDPM throughput runs with the per-step noise drawn IN the kernel (ABI 9): the reference draws one
 * [n,1,D] normal tensor per step on the device (gaussian_diffusion.py:258-272); a fused launch fed from memory needs all of
 * them up front ([steps,n,1,D]: 205 MB per 12,800-latent batch of BASELINE configs[4]).  Here every (latent, position,
 * step) gets its unit normal from Philox4x32-10 + Box-Muller keyed on `noise_seed`, counter = (noise_base + latent index,
 * position / 4, step): results depend on the seed and on a latent's GLOBAL index only -- not on tiling, batch splits or the
 * world size (a rank passes the global index of its first latent as noise_base).  Not bit-compatible with torch's stream:
 * parity tests use gldm_denoise with recorded noise.  Arguments as gldm_denoise (DDPM, no per-sample timesteps). */
int gldm_denoise_rng(const gldm_r1d_desc *desc, const float *weights, const float *temb, const float *cemb,
                     int samples_per_cond, const float *x_in /*[n,1,L]*/, int n_samples,
                     const int32_t *timesteps /*[n_steps]*/, int n_steps, int clip_sample,
                     const float *sched_coef /*[n_steps,8]*/, unsigned long long noise_seed, long long noise_base,
                     const float *sample_emb, float *x_out /*[n,1,L]*/, void *workspace, gldm_stream_t stream);
/* The same generator on its own: out[i][l] = the normal gldm_denoise_rng adds to latent noise_base + i, position l, at
 * step `step` (statistical tests; no reference counterpart). */
int gldm_step_noise_rng(unsigned long long noise_seed, long long noise_base, int step, int n_samples, int seq_len,
                        float *out /*[n,L]*/, gldm_stream_t stream);

/* ref: grasp_ldm/models/grasp_vae.py:401-436 (ConditionalGraspPoseDecoder.forward:
 * in_layer -> ResNet1D -> tmrp / class_logits heads). */
int gldm_decode(const gldm_r1d_desc *desc, const float *weights, const float *cemb, int samples_per_cond,
                const float *z_h /*[n,D]*/, int n_samples, float *tmrp /*[n,6]*/, float *logit /*[n,1]*/,
                void *workspace, gldm_stream_t stream);

/* ref: grasp_ldm/models/grasp_vae.py:104-117 (GraspCVAE.encode) = :518-536 (ConditionalGraspPoseEncoder.forward:
 * in_layer -> ResNet1D -> out_layer) + :552-574 (VAEBottleneck.forward and .reparameterize), one engine launch on the
 * engine gldm_decode takes for the same descriptor.  `desc` carries the encoder head (GLDM_HEAD_ENCODER, Lz = n_head / 2);
 * h [n, latent_dim] is the normalised grasp row [t, mrp(, label)].  mu / logvar [n, Lz]; when z is given,
 *   z = mix_mu * mu + mix_eps * eps * (eps_times_std ? exp(0.5 * logvar) : 1)      (eps NULL: z = mix_mu * mu)
 * (1, 1, 1) is reparameterize; (sqrt(abar_t), sqrt(1 - abar_t), 0) is the scheduler's add_noise of mu to timestep t,
 * the start of a partial reverse diffusion.  Workspace as gldm_decode.  A decoder descriptor is GLDM_ERR_INVALID_ARG
 * (and gldm_decode rejects an encoder one). */
int gldm_encode(const gldm_r1d_desc *desc, const float *weights, const float *cemb, int samples_per_cond,
                const float *h /*[n,latent_dim]*/, int n_samples, const float *eps /*[n,Lz] or NULL*/, float mix_mu,
                float mix_eps, int eps_times_std, float *mu /*[n,Lz]*/, float *logvar /*[n,Lz]*/,
                float *z /*[n,Lz] or NULL*/, void *workspace, gldm_stream_t stream);

/* ref: grasp_ldm/utils/rotations.py:305-309 (H_to_tmrp) with :115-163 (rotmat_to_mrp: arg-max over R00, R11, R22, trace
 * with the first maximum winning a tie, the SciPy branch formulas, normalise, q.xyz / (1 + q.w); NOT canonicalised: the
 * shadow set |m| > 1 comes back when the chosen branch gives w < 0) + the dataset's normalisation, the inverse of
 * gldm_pose_epilogue:  h[i, 0..5] = ((t, mrp) - mean) / std,  h[i, 6] = label[i] when label is given (width 7, else 6).
 * mean / std per cloud as in gldm_pose_epilogue. */
int gldm_pose_prologue(const float *H /*[n,4,4]*/, const float *label /*[n] or NULL*/, const float *grasp_mean,
                       const float *grasp_std, int n, int grasps_per_cloud, int n_clouds, float *h /*[n,6|7]*/,
                       gldm_stream_t stream);

/* ref: tools/inference.py:64-94,628-647 + grasp_ldm/utils/rotations.py:171-302:
 * un = tmrp*std+mean; H = tmrp_to_H(un); conf = sigmoid(logit).  mean AND std are
 * per cloud, [n_clouds,6] each (a caller holding the reference's broadcastable [1,6] std expands
 * it first); grasp i belongs to cloud i / grasps_per_cloud; n <= n_clouds * grasps_per_cloud is
 * checked (GLDM_ERR_INVALID_ARG). */
int gldm_pose_epilogue(const float *tmrp /*[n,6]*/, const float *logit /*[n]*/, const float *grasp_mean,
                       const float *grasp_std, int n, int grasps_per_cloud, int n_clouds, float *H /*[n,4,4]*/,
                       float *tmrp_unnorm /*[n,6]*/, float *confidence /*[n]*/, gldm_stream_t stream);

/* ref: grasp_ldm/models/modules/ext/pvcnn/modules/pointnet.py:100-111 (PointNetSAModule.forward
 * after FPS + ball query): neighbour gather + grouped SharedMLP2d (Conv2d k1 + eval BatchNorm
 * folded + ReLU, shared_mlp.py:6-35) + max over the U neighbours, fused; the grouped tensor
 * never reaches HBM.  `weights` holds, per layer l, the folded weight [cout x cin_pad] in MFMA
 * A-fragment order at w_off[l] and the folded bias at b_off[l] (graspldm_amd/sa_pack.py);
 * cin_pad[0] = roundup(3 + c, 16), u must divide 64, cout <= 256. */
int gldm_sa_mlp_forward(const float *points /*[b,3,n]*/, const float *centers /*[b,3,m]*/,
                        const float *features /*[b,c,n] or NULL*/, const int32_t *idx /*[b,m,u]*/,
                        const float *weights, int b, int c, int n, int m, int u, int n_layers,
                        const int32_t *cin_pad, const int32_t *cout, const int32_t *w_off, const int32_t *b_off,
                        float *out /*[b,cout_last,m]*/, gldm_stream_t stream);

/* The same module core with the GEMMs on the f16 matrix pipe (every f32 product as three f16 partial products of the
 * hi / lo splits of both operands, f32 accumulation: the arithmetic of the denoiser engines): 64-column tiles whose
 * gathered rows and hidden-layer outputs live in LDS as pre-split planes.  `weights` holds, per layer, the split-f16 A
 * fragments of [cout x cin_pad] at w3_off[l] (graspldm_amd/r1d_pack.py: mfma_a_fragments_f16x2; cin_pad a multiple of 32,
 * zero beyond the real rows) and the folded bias at b_off[l].  Shapes: cin_pad[0] <= 288, hidden widths multiples of 32
 * (32 / 64 / 128 / 256), U in {16, 32, 64}; GLDM_ERR_UNSUPPORTED otherwise (callers then use gldm_sa_mlp_forward).
 * `range_gain` (HOST memory, [n_layers][2] = per layer the largest row sum of |W| and the largest |bias|, BatchNorm folded;
 * ABI 10): f16 has 5 exponent bits, so every 64-column tile is split as x / s with s a power of two taken from the tile's
 * largest gathered magnitude, the hidden layers' planes with one taken from the bound gain_r * max|in| + gain_b, and s is
 * folded back on the accumulators (exact; s = 1, i.e. every bit as without it, while 2^-8 <= magnitude < 2^14).  NULL: no
 * scales -- the caller vouches for |values| < 65504 everywhere. */
int gldm_sa_mlp_forward_f16x2(const float *points /*[b,3,n]*/, const float *centers /*[b,3,m]*/,
                               const float *features /*[b,c,n] or NULL*/, const int32_t *idx /*[b,m,u]*/,
                               const float *weights, int b, int c, int n, int m, int u, int n_layers,
                               const int32_t *cin_pad, const int32_t *cout, const int32_t *w3_off, const int32_t *b_off,
                               const float *range_gain /*host [n_layers][2] or NULL*/,
                               float *out /*[b,cout_last,m]*/, gldm_stream_t stream);

/* The same launch with the module's FIRST layer hoisted out of the (centre, neighbour) pairs (ABI 10).  Its input is the
 * concatenation [x - centre; f] (ball_query.py:21-33), so  W1 [x - c; f] + b1 = W1a (x - c) + (W1b f + b1)  and the second
 * term depends on the point only: the caller computes pre = W1b f + b1 once per cloud, POINT-major [b, n, c1]
 * (gldm_pointwise_mlp_f16x2_pm; every point sits in ~m u / n balls, 16 at SSG-SA2: a neighbour's rows are then one run of
 * c1 floats and a gather thread's four rows one 16-byte load), the gather fetches a neighbour's rows of `pre` instead of its
 * features, adds the three coordinate products (W1a [c1][4] = columns x, y, z, 0 at float index wa_off of `weights`) and
 * applies the ReLU.  The layer tables describe layers 2.. of the module (cin_pad[0] = c1 = rows of pre, a multiple of 32;
 * rows the module does not have carry zero weights and zero pre).  pre_broadcast != 0: a module WITHOUT features -- its first
 * layer is W1a (x - c) + b1, `pre` is the one row b1 [c1] shared by every point.  Same arithmetic for layers 2.., the first layer's
 * products are f32 (VALU) + the caller's GEMM: results differ from gldm_sa_mlp_forward_f16x2 in the last bits. */
int gldm_sa_mlp_forward_f16x2_pre(const float *points /*[b,3,n]*/, const float *centers /*[b,3,m]*/,
                                   const float *pre /*[b,n,c1]; [c1] with pre_broadcast*/, int pre_broadcast,
                                   const int32_t *idx /*[b,m,u]*/, const float *weights,
                                   int wa_off, int b, int n, int m, int u, int n_layers,
                                   const int32_t *cin_pad, const int32_t *cout, const int32_t *w3_off, const int32_t *b_off,
                                   const float *range_gain /*host [n_layers][2] or NULL*/,
                                   float *out /*[b,cout_last,m]*/, gldm_stream_t stream);

/* Shape queries of the three launches above (ABI 15): each is the launch's own planner behind a thin wrapper, a pure
 * function of the sizes and the HOST tables (no device pointer, nothing launched), and answers the status the launch gives
 * the same shape before it looks at gains or launches.
 * gldm_sa_mlp_supported: GLDM_OK where gldm_sa_mlp_forward runs (c, u, n_layers, cin_pad[], cout[]), else its status
 * (GLDM_ERR_UNSUPPORTED; GLDM_ERR_INVALID_ARG for a null table, u <= 0, c < 0, cin_pad[l] != cout[l - 1] or cin_pad[0] < 3 + c).
 * gldm_sa_mlp_f16x2_lds_bytes: the dynamic LDS of the single-tile launch of gldm_sa_mlp_forward_f16x2 (pre == 0) or
 * gldm_sa_mlp_forward_f16x2_pre (pre != 0: c = 0, cin_pad[0] = rows of `pre`): the two plane regions + the eight range words +
 * the staged run of output rows, in bytes; a negative GLDM_ERR_* status where the launch takes no such shape (the
 * *_workspace_bytes convention).  plane_bytes (optional): the plane regions' share of that figure. */
int gldm_sa_mlp_supported(int c, int u, int n_layers, const int32_t *cin_pad, const int32_t *cout);
long long gldm_sa_mlp_f16x2_lds_bytes(int pre, int c, int u, int n_layers, const int32_t *cin_pad, const int32_t *cout,
                                      long long *plane_bytes /*or NULL*/);

/* ref: grasp_ldm/models/modules/ext/pvcnn/modules/shared_mlp.py:6-35 (Conv1d k = 1 + eval BatchNorm folded + ReLU),
 * one layer, in the native [b, c, n] layout: y = act(W x + bias).  `w_packed` = the folded weight [cout, cin] in MFMA
 * A-fragment order (graspldm_amd/r1d_pack.py: mfma_a_fragments).  Optional fused head on the accumulators:
 * z = Wh y + bh with hout <= 16 rows (grasp_ldm/models/modules/pc_encoders.py:104-111: conv_downscale and out_layer[0]
 * folded into one [hout x cout] matrix); `head_w_packed` = [16, cout] in A-fragment order with the k index of every
 * 16-block permuted k' = 4 (k % 4) + k / 4 (graspldm_amd/dense.py: pack_head).  With a head, y may be NULL and the
 * [b, cout, n] tensor never reaches HBM.  cin % 32 == 0, cout % 256 == 0, n % 32 == 0, 4 (32 cin + 4096) <= 160 KiB. */
int gldm_pointwise_mlp(const float *x /*[b,cin,n]*/, const float *w_packed, const float *bias /*[cout]*/,
                       int b, int cin, int cout, int n, int relu,
                       const float *head_w_packed, const float *head_bias /*[hout] or NULL*/, int hout,
                       float *y /*[b,cout,n] or NULL*/, float *z /*[b,hout,n] or NULL*/, gldm_stream_t stream);

/* Two consecutive SharedMLP layers (both with ReLU) and the optional head in ONE launch: the first layer's output
 * (x [b,cin0,n] -> [b,cin,n]) is produced tile by tile in LDS as the second layer's input and never reaches HBM
 * (the shipped encoder's 96 -> 768 -> 1536 -> head: 0.8 GB less written and read per 256 clouds).
 * cin0 % 32 == 0, cin % 256 == 0, other constraints as gldm_pointwise_mlp, 4 (32 (cin + cin0) + 4096) <= 160 KiB. */
int gldm_pointwise_mlp2(const float *x /*[b,cin0,n]*/, const float *w0_packed, const float *bias0 /*[cin]*/, int cin0,
                        const float *w_packed, const float *bias /*[cout]*/, int b, int cin, int cout, int n,
                        const float *head_w_packed, const float *head_bias, int hout,
                        float *y /*[b,cout,n] or NULL*/, float *z /*[b,hout,n] or NULL*/, gldm_stream_t stream);

/* ref: shared_mlp.py:6-35 for NARROW layers (the PVConv point branches 3 -> 48, 48 -> 96): y = act(W x + bias) over
 * [b, cin, n] with W [cout, cin] row major (BatchNorm folded by the caller); cin in {3, 6, 16, 24, 32, 48, 64}.
 * VALU kernel (lane = point), k-ordered fma chain from the bias. */
int gldm_pointwise_small(const float *x /*[b,cin,n]*/, const float *w /*[cout,cin]*/, const float *bias /*[cout] or NULL*/,
                         int b, int cin, int cout, long long n, int relu, float *y /*[b,cout,n]*/, gldm_stream_t stream);

/* ref: the same module for EVERY other shape (ext/pvcnn/modules/shared_mlp.py:6-35, ext/pvcnn/modules/pointnet.py:117-135:
 * the feature-propagation SharedMLPs of PointNet++ / PVCNN2, e.g. 384 -> 256 over 128 centres): any cin, cout, n; weights
 * [cout][cin] as stored (BatchNorm folded by the caller), exact f32 products on the f32 matrix pipe, 64 x 64 output tiles.
 * These layers went to the GEMM library (rocBLAS / MIOpen through F.conv1d) + gldm_bias_act before ABI 7. */
int gldm_pointwise_any(const float *x /*[b,cin,n]*/, const float *w /*[cout,cin]*/, const float *bias /*[cout] or NULL*/,
                       int b, int cin, int cout, long long n, int relu, float *y /*[b,cout,n]*/, gldm_stream_t stream);

/* ref: pc_encoders.py:60-82,104-111: out_layer[1] = nn.Linear(n_points, latent) applied over the POINT axis of
 * [B, C, N]: y[row, :] = W x[row, :] + bias for rows = B * C; n % 4 == 0, n <= 16384. */
int gldm_linear_rows(const float *x /*[rows,n]*/, const float *w /*[nout,n]*/, const float *bias /*[nout] or NULL*/,
                     int rows, int n, int nout, float *y /*[rows,nout]*/, gldm_stream_t stream);

/* The same two entry points with the MAIN layer's weights as split-f16 fragments (graspldm_amd/r1d_pack.py:
 * mfma_a_fragments_f16x2; layout above): the GEMM runs on the f16 matrix pipe with three partial products per f32
 * product and f32 accumulation (error of the order of one f32 rounding per product, 3/16 of the f32-MFMA time).  The
 * input tile is split once while it is staged.  Since ABI 6 the front layer's weights `w0_split` are split-f16 fragments
 * too (cin0 % 32 == 0, cin0 <= 96; its f32 input tile is split once per wave into registers); `head_w_packed` stays f32
 * fragments.  cin % 128 == 0, cout % 32 == 0 (with a front layer or a head: % 256; fewer than 256 output rows leave waves
 * idle), n % 16 == 0, the tile's two f16 planes (128 bytes per channel of a 32-point tile) + the front layer's f32 tile
 * + 64 bytes <= 160 KiB: cin <= 1152 (until ABI 8 three bf16 planes, 4 (48 cin + 32 cin0) + 16 bytes).  The exact rule is
 * gldm_pointwise_mlp_supported's answer. */
/* (ABI 10: without a front layer cin may be any multiple of 8 -- `w_split` then holds the fragments of W zero-padded to a
 * multiple of 128 columns, the K the launch walks; cout any multiple of 16 below 256 rows, of 32 from there.) */
int gldm_pointwise_mlp_f16x2(const float *x /*[b,cin,n]*/, const float *w_split, const float *bias /*[cout]*/,
                              int b, int cin, int cout, int n, int relu,
                              const float *head_w_packed, const float *head_bias, int hout,
                              float *y /*[b,cout,n] or NULL*/, float *z /*[b,hout,n] or NULL*/, gldm_stream_t stream);

/* The same launch with an addend in front of the activation: y = act(W x + bias + add), add[cloud * add_cloud_stride +
 * row * add_row_stride + col * add_col_stride] -- a per-cloud bias (strides cout, 1, 0) or a [b, cout, n] tensor
 * (cout * n, n, 1).  It serves layers whose input is a concatenation (pointnet.py:117-135 PointNetFPModule, :11-46
 * PointNetAModule): W [x1; x2] = W1 x1 + W2 x2, the wide part here, the other part (three coordinate rows, or one centre's
 * feature vector broadcast to every point) as the addend, and the concatenated tensor is never built. */
/* gldm_pointwise_mlp_f16x2 writing y POINT-major, [b, n, cout] (a lane's four consecutive output rows of a point: one
 * 16-byte store): the layout gldm_sa_mlp_forward_f16x2_pre gathers from. */
int gldm_pointwise_mlp_f16x2_pm(const float *x /*[b,cin,n]*/, const float *w_split, const float *bias /*[cout]*/, int b, int cin,
                                 int cout, int n, int relu, float *y_point_major /*[b,n,cout]*/, gldm_stream_t stream);
int gldm_pointwise_mlp_f16x2_add(const float *x /*[b,cin,n]*/, const float *w_split, const float *bias /*[cout]*/,
                                  const float *add, long long add_cloud_stride, long long add_row_stride,
                                  long long add_col_stride, int b, int cin, int cout, int n, int relu,
                                  float *y /*[b,cout,n]*/, gldm_stream_t stream);
/* Range of the split operands (ABI 10): the one-layer launches above split every input tile as x / s, s a power of two from
 * the tile's largest magnitude (1 while 2^-8 <= magnitude < 2^14: then every bit is as without it), and fold s back on the
 * accumulators.  The two-layer launch below does the same for its input tile and scales the front layer's output planes by
 * the bound front_gain[0] * max|x| + front_gain[1] (HOST memory: largest row sum of |W0|, largest |bias0|); front_gain ==
 * NULL: no scales in that launch -- the caller vouches for |values| < 65504. */
int gldm_pointwise_mlp2_f16x2(const float *x /*[b,cin0,n]*/, const float *w0_split, const float *bias0, int cin0,
                               const float *w_split, const float *bias /*[cout]*/, int b, int cin, int cout, int n,
                               const float *head_w_packed, const float *head_bias, int hout,
                               const float *front_gain /*host [2] or NULL*/,
                               float *y /*[b,cout,n] or NULL*/, float *z /*[b,hout,n] or NULL*/, gldm_stream_t stream);

/* Shape query of the six gldm_pointwise_mlp* launches (ABI 15): their common planner behind a thin wrapper, a pure function of
 * the sizes and the form.  split_f16: the *_f16x2 forms; cin0: rows of the front layer's input (gldm_pointwise_mlp2*), 0 for no
 * front layer; hout: rows of the head, 0 for none; with_addend / point_major: the _add / _pm forms (split only).  GLDM_OK
 * where the launch of that form runs the shape, GLDM_ERR_UNSUPPORTED otherwise (a non-positive size included). */
int gldm_pointwise_mlp_supported(int split_f16, int cin0, int cin, int cout, int n, int hout, int with_addend, int point_major);

/* ref: grasp_ldm/models/modules/ext/pvcnn/modules/pointnet.py:40-44 (PointNetAModule: `features.max(dim=-1)`, the global
 * pooling over a cloud's centres).  out[row] = max over x[row][0..n) for rows = b * c; NaN propagates as in torch.max. */
int gldm_row_max(const float *x /*[rows,n]*/, long long rows, int n, float *out /*[rows]*/, gldm_stream_t stream);

/* ---------------------------------------------------------- voxel branch of PVConv */

/* ref: grasp_ldm/models/modules/ext/pvcnn/modules/pvconv.py:48-66 (nn.Conv3d k=3 p=1 on the
 * [b, c, r, r, r] voxel grid).  Implicit GEMM on f32 MFMA; `w_packed` = weight [cout, cin, 3,3,3]
 * re-laid as [cout, 27 * cin_pad] (k = tap * cin_pad + ci, tap = (dx*3+dy)*3+dz, cin_pad =
 * roundup(cin,16)) in MFMA A-fragment order (graspldm_amd/voxel.py).  Also writes, per 4x4xr
 * brick and output channel, (sum, sum of squares) of the outputs to `partial`
 * [gldm_conv3d_partial_floats()] for the following GroupNorm.  r % 4 == 0. */
long long gldm_conv3d_partial_floats(int b, int cout, int r);
int gldm_conv3d_k3(const float *x /*[b,cin,r^3]*/, const float *w_packed, const float *bias /*[cout]*/,
                   int b, int cin, int cout, int r, float *y /*[b,cout,r^3]*/, float *partial,
                   gldm_stream_t stream);

/* gldm_conv3d_k3 writing its output channel-last, [b, r^3, cout] (the layout gldm_gn_swish_chan_sum_cl and
 * gldm_devoxelize_gn_cl_fused read: a voxel stack's last conv); cout % 4 == 0. */
int gldm_conv3d_k3_cl(const float *x /*[b,cin,r^3]*/, const float *w_packed, const float *bias /*[cout]*/, int b, int cin,
                      int cout, int r, float *y_cl /*[b,r^3,cout]*/, float *partial, gldm_stream_t stream);

/* The same conv for ANY channel counts (r % 4 == 0) with the weight as nn.Conv3d stores it, [cout, cin, 27] f32: a
 * direct VALU kernel for voxel shapes the MFMA kernels are not instantiated for (PVCNN2's 256 ch @ 8^3, 128 ch @ 16^3);
 * same `partial` layout.  A correctness path: no shape of the shipped encoder uses it. */
int gldm_conv3d_k3_generic(const float *x /*[b,cin,r^3]*/, const float *w /*[cout,cin,27]*/, const float *bias,
                           int b, int cin, int cout, int r, float *y /*[b,cout,r^3]*/, float *partial,
                           gldm_stream_t stream);

/* The same conv with split-f16 weights (graspldm_amd/voxel.py: pack_conv3d_f16x2: [cout, cblocks * 14 * 32] with
 * k = ((16-channel block) * 14 + tap pair) * 32 + 16 (tap - 2 pair) + channel, as mfma_a_fragments_f16x2 fragments):
 * three f16 partial products per f32 product on the f16 matrix pipe, f32 accumulation.  Built for the shipped
 * encoder's shapes (cout 48 at r = 24, cout 96 at r = 12 with cin % 16 == 0; and the first conv, cin = 3 -> 48 at r = 24,
 * whose weights are packed tap-major without padding between taps, k = tap * 3 + ci < 81 in three 32-deep blocks:
 * pack_conv3d_fewch_f16x2); GLDM_ERR_UNSUPPORTED otherwise. */
int gldm_conv3d_k3_f16x2(const float *x /*[b,cin,r^3]*/, const float *w_split, const float *bias /*[cout]*/,
                          int b, int cin, int cout, int r, float *y /*[b,cout,r^3]*/, float *partial,
                          gldm_stream_t stream);

/* Shape query of the MFMA convs (ABI 15): GLDM_OK where gldm_conv3d_k3 / _cl (GLDM_CONV3D_F32: any cin, the listed
 * (m-tiles of cout, r)) or gldm_conv3d_k3_f16x2 / _gn (GLDM_CONV3D_F16X2: the listed (cout, r) with cin % 16 == 0, and
 * 3 -> 48 at r = 24) has an instantiation, GLDM_ERR_UNSUPPORTED otherwise; another kind: GLDM_ERR_INVALID_ARG.  It reads the
 * list the dispatch reads (csrc/conv3d.hip).  The forms' own conditions (_cl: cout % 4 == 0; _gn: cin % 16 == 0) stay with
 * the entries. */
enum gldm_conv3d_kind { GLDM_CONV3D_F32 = 0, GLDM_CONV3D_F16X2 = 1 };
int gldm_conv3d_k3_supported(int kind, int cin, int cout, int r);

/* ref: pvconv.py:57-66 (Conv3d -> GroupNorm(8) -> Swish -> Conv3d): a conv of the voxel stack with its neighbours' work
 * folded in.  in_coef [b, cin, 2] (optional) = (a, s) from gldm_groupnorm_coef: x is the previous conv's RAW output and
 * x' = swish(a x + s) is applied per in-grid element while the bricks are staged (the activated tensor is never written).
 * out_channel_last != 0: y is written [b, r^3, cout] (a voxel's channels as one run: the layout the squeeze and
 * devoxelize passes below read; `partial` is unchanged).  cin % 16 == 0, the cout / r of gldm_conv3d_k3_f16x2. */
int gldm_conv3d_k3_f16x2_gn(const float *x /*[b,cin,r^3] raw*/, const float *in_coef /*[b,cin,2] or NULL*/,
                             const float *w_split, const float *bias /*[cout]*/, int b, int cin, int cout, int r,
                             float *y /*[b,cout,r^3] or [b,r^3,cout]*/, float *partial, int out_channel_last,
                             gldm_stream_t stream);

/* ref: pvconv.py:57-66 (nn.GroupNorm(8, c)) as per-(cloud, channel) coefficients: GN(x) = a x + s, a = gamma rstd,
 * s = beta - mean a, statistics from a conv's `partial` (combined in f64 in a fixed order, as gldm_groupnorm_swish).
 * c / groups <= 128. */
int gldm_groupnorm_coef(const float *partial, const float *gamma, const float *beta, int b, int c, int r, int groups,
                        float eps, float *coef /*[b,c,2]*/, gldm_stream_t stream);

/* chan_sum[b,c] = sum over the r^3 voxels of swish(a y + s): the SE squeeze (se.py:12-25) of a GroupNorm + Swish output
 * that is never written (read-only pass over the raw conv output). */
int gldm_gn_swish_chan_sum(const float *y /*[b,c,r^3] raw*/, const float *coef /*[b,c,2]*/, int b, int c, int r,
                           float *chan_sum /*[b,c]*/, gldm_stream_t stream);

/* The same squeeze over a channel-last tensor, as gldm_squeeze_parts() partial sums per cloud (fixed split of the voxels,
 * added in index order by gldm_se_gate_parts: deterministic, no atomics).  c % 4 == 0. */
int gldm_squeeze_parts(void);
int gldm_gn_swish_chan_sum_cl(const float *y /*[b,r^3,c] raw*/, const float *coef /*[b,c,2]*/, int b, int c, int r,
                              float *chan_parts /*[b,parts,c]*/, gldm_stream_t stream);

/* ref: pvconv.py:57-66 (nn.GroupNorm(8, c) + Swish), in place on y; statistics from `partial`
 * (combined in f64 in a fixed order).  chan_sum [b,c] (optional) receives the per-channel sum of
 * the OUTPUT: the squeeze of the SE block that follows. */
int gldm_groupnorm_swish(float *y /*[b,c,r^3]*/, const float *partial, const float *gamma, const float *beta,
                         int b, int c, int r, int groups, float eps, float *chan_sum, gldm_stream_t stream);

/* ref: grasp_ldm/models/modules/ext/pvcnn/modules/se.py:12-25: gate = sigmoid(W2 act(W1 mean)),
 * act = ReLU (use_relu) or Swish. */
int gldm_se_gate(const float *chan_sum /*[b,c]*/, const float *w1 /*[hidden,c]*/, const float *w2 /*[c,hidden]*/,
                 int b, int c, int hidden, int r, int use_relu, float *gate /*[b,c]*/, gldm_stream_t stream);
int gldm_se_gate_parts(const float *chan_parts /*[b,parts,c]*/, int parts, const float *w1, const float *w2, int b, int c,
                       int hidden, int r, int use_relu, float *gate /*[b,c]*/, gldm_stream_t stream);

/* ref: pvconv.py:79-83: trilinear_devoxelize(SE(v)) + point_features(x) in one pass:
 * out = gate[b,c] * trilinear(V) + add  (gate / add may be NULL). */
int gldm_devoxelize_fused(const float *coords /*[b,3,n]*/, const float *features /*[b,c,r^3]*/,
                          const float *gate /*[b,c]*/, const float *add /*[b,c,n]*/, int b, int c, int n, int r,
                          float *out /*[b,c,n]*/, gldm_stream_t stream);

/* The same pass over a RAW conv output: GroupNorm + Swish (coef [b,c,2] from gldm_groupnorm_coef) applied to the eight
 * corner values of every point before the trilinear blend: out = gate * trilinear(swish(a V + s)) + add. */
int gldm_devoxelize_gn_fused(const float *coords /*[b,3,n]*/, const float *features /*[b,c,r^3] raw*/,
                             const float *coef /*[b,c,2]*/, const float *gate /*[b,c]*/, const float *add /*[b,c,n]*/,
                             int b, int c, int n, int r, float *out /*[b,c,n]*/, gldm_stream_t stream);
/* ... and over a channel-LAST raw conv output: a point's corner is one run of c floats (16-byte loads by neighbouring
 * lanes) instead of c gathers from c cache lines.  c % 4 == 0, c <= 256. */
int gldm_devoxelize_gn_cl_fused(const float *coords /*[b,3,n]*/, const float *features_cl /*[b,r^3,c] raw*/,
                                const float *coef /*[b,c,2]*/, const float *gate /*[b,c]*/, const float *add /*[b,c,n]*/,
                                int b, int c, int n, int r, float *out /*[b,c,n]*/, gldm_stream_t stream);

/* y[b, c, :] = act(y[b, c, :] + bias[c]) in place (relu != 0: ReLU).  Epilogue of the k = 1 Conv1d /
 * Conv2d + BatchNorm(eval, folded) + ReLU of ext/pvcnn/modules/shared_mlp.py:24-36 when the GEMM itself
 * runs as a plain library call.  n % 4 == 0 (rows stay 16-byte aligned). */
int gldm_bias_act(float *y /*[b,c,n]*/, const float *bias /*[c]*/, int b, int c, long long n, int relu,
                  gldm_stream_t stream);

/* ------------------------------------------------ point attention (ABI 12) */

/* ref: grasp_ldm/models/modules/modules.py:10-54 (the PVD `Attention` block) between its k = 1 convs: dense softmax
 * attention of every point over every point, WITHOUT a 1 / sqrt(c) factor (modules.py:42):
 *   out[b,c,i] = sum_j v[b,c,j] softmax_j( sum_c' q[b,c',i] k[b,c',j] ).
 * q, k, v are [b,c,n] f32 and may alias one another (with the k and v projections folded into q and the out conv, k = v =
 * the block's input).  c % 16 == 0, 16 <= c <= 1024; n % 32 == 0, 32 <= n <= 4096; GLDM_ERR_UNSUPPORTED otherwise.
 * Default arithmetic: both products as three v_mfma_f32_16x16x32_f16 over hi / lo f16 pieces, f32 accumulation; every
 * 16-row group of an operand is split as x / s (s a power of two from the group's largest magnitude, folded back on the
 * accumulators) and P is split as 2^14 P.  exact_f32 != 0: the same stages on v_mfma_f32_16x16x4_f32, partial sums of 128
 * channels (keys) added in K order, so that no f32 chain is longer than 32 steps plus K / 128 totals.  Softmax subtracts
 * the row maximum and divides once per row.  Deterministic (fixed summation order, no atomics); a cloud's result does
 * not depend on b or on its position in the batch.
 * `workspace`: at least gldm_point_attention_workspace_bytes(b, c, n) bytes (at most 256 MiB, or one cloud's need where
 * that is more: operand fragments, scores and probabilities of a chunk of clouds; the entry point loops over chunks),
 * 16-byte aligned, private to the stream until the call's work has finished.  A missing / smaller workspace or a
 * pointer that is not 16-byte aligned: GLDM_ERR_INVALID_ARG, nothing launched.  The bytes query returns -1 for an
 * unsupported shape. */
long long gldm_point_attention_workspace_bytes(int b, int c, int n);
int gldm_point_attention(const float *q /*[b,c,n]*/, const float *k /*[b,c,n]*/, const float *v /*[b,c,n]*/,
                         int b, int c, int n, int exact_f32, void *workspace, long long workspace_bytes,
                         float *out /*[b,c,n]*/, gldm_stream_t stream);

/* ref: modules.py:50-52 (`x = h + x; x = nonlin(norm(x))`): out = swish(GroupNorm(groups, eps, affine)(x + add)) over
 * [b,c,n]; add may be NULL, out may be x.  Statistics from the tensor itself, combined in f64 in a fixed order (as
 * gldm_groupnorm_swish does for voxel grids).  c % groups == 0, c / groups <= 128, n % 4 == 0, b <= 65535
 * (GLDM_ERR_UNSUPPORTED otherwise); x, add and out 16-byte aligned (GLDM_ERR_INVALID_ARG otherwise). */
int gldm_groupnorm_swish_points(const float *x /*[b,c,n]*/, const float *add /*[b,c,n] or NULL*/, const float *gamma /*[c]*/,
                                const float *beta /*[c]*/, int b, int c, int n, int groups, float eps,
                                float *out /*[b,c,n]*/, gldm_stream_t stream);

/* ref: grasp_ldm/models/modules/pc_encoders.py:72-77,111 (out_layer[0] = Conv1d(C -> out_channels, k = 1)) where it cannot be
 * folded into conv_downscale (global attention on): y = W x + bias for a FEW output rows, hout <= 8, over [b, cin, n]; W
 * [hout, cin] row major.  One pass over x, k-ordered fma chain from the bias.  n % 4 == 0, b <= 65535
 * (GLDM_ERR_UNSUPPORTED otherwise); x and y 16-byte aligned (GLDM_ERR_INVALID_ARG otherwise). */
int gldm_pointwise_rows(const float *x /*[b,cin,n]*/, const float *w /*[hout,cin]*/, const float *bias /*[hout] or NULL*/,
                        int b, int cin, int hout, int n, float *y /*[b,hout,n]*/, gldm_stream_t stream);

/* ------------------------------------------------ voxel attention inside PVConv (ABI 14) */

/* ref: grasp_ldm/models/modules/modules.py:39-48 (the PVD `Attention` block between its k = 1 convs) where the tokens are the
 * r^3 voxels of a PVConv (ext/pvcnn/modules/pvconv.py:68-69): the contract of gldm_point_attention,
 *   out[b,c,i] = sum_j v[b,c,j] softmax_j( sum_c' q[b,c',i] k[b,c',j] ),   no 1 / sqrt(c) factor,
 * for many tokens at few channels, in ONE launch that never writes an n x n tensor and takes no workspace: a workgroup
 * keeps the q of 128 queries in registers, walks the keys in staged tiles of 32 and carries a running maximum and sum per
 * query (online softmax; one division per row at the end).  q, k, v are [b,c,n] f32 and may alias one another; out may
 * not alias them.  c % 16 == 0, 32 <= c <= 128; n % 32 == 0, 32 <= n <= 4096; b <= 65535 (GLDM_ERR_UNSUPPORTED otherwise).
 * Default arithmetic: both products as three v_mfma_f32_16x16x32_f16 over hi / lo f16 pieces with f32 accumulation; q is
 * split as q / s per 16-query tile, every staged tile of k and of v as x / s (s a power of two from the tile's largest
 * magnitude, 1 for anything ordinary, folded back on the accumulators), probabilities as 2^14 p.  exact_f32 != 0: the same
 * stages on v_mfma_f32_16x16x4_f32.  Deterministic (fixed summation order, no atomics, nothing waits on another
 * workgroup); a cloud's result does not depend on b, on its position in the batch or on the stream.  A null or not
 * 16-byte aligned pointer, or a non-positive size: GLDM_ERR_INVALID_ARG, nothing launched.  Those two are the only
 * statuses the entry decides itself; a launch the runtime refuses is GLDM_ERR_LAUNCH, as for every entry point here. */
int gldm_point_attention_fused(const float *q /*[b,c,n]*/, const float *k /*[b,c,n]*/, const float *v /*[b,c,n]*/,
                               int b, int c, int n, int exact_f32, float *out /*[b,c,n]*/, gldm_stream_t stream);

/* ref: pvconv.py:64-69 (the second conv's nn.GroupNorm(8, c) where `Attention` follows it instead of Swish): x = a y + s per
 * (cloud, channel) over a channel-major voxel grid, (a, s) = coef [b,c,2] from gldm_groupnorm_coef; no activation.
 * r^3 % 4 == 0, r <= 64 (GLDM_ERR_UNSUPPORTED otherwise); y and x 16-byte aligned (GLDM_ERR_INVALID_ARG otherwise); x may
 * be y. */
int gldm_groupnorm_affine(const float *y /*[b,c,r^3] raw*/, const float *coef /*[b,c,2]*/, int b, int c, int r,
                          float *x /*[b,c,r^3]*/, gldm_stream_t stream);

/* ref: modules.py:50-52 followed by se.py:12-25: gldm_groupnorm_swish_points with the SE squeeze on its way:
 * chan_sum[b,c] = sum over n of the OUTPUT, a wave per channel, lanes in index order (f64), a fixed tree over the lanes.
 * Same shapes and statuses as gldm_groupnorm_swish_points; chan_sum must not be NULL. */
int gldm_groupnorm_swish_points_sum(const float *x /*[b,c,n]*/, const float *add /*[b,c,n] or NULL*/, const float *gamma /*[c]*/,
                                    const float *beta /*[c]*/, int b, int c, int n, int groups, float eps,
                                    float *out /*[b,c,n]*/, float *chan_sum /*[b,c]*/, gldm_stream_t stream);

/* ------------------------------------------------ grasp success classifier (ABI 13) */

/* ref: grasp_ldm/dataset/acronym/acronym_grasp_points.py:25-28,107,117 (gripper points placed at a pose, centred on the
 * cloud's mean, normalised) + grasp_ldm/models/grasp_classifier.py:71-80 (label channel, merge, channel-first): the input of
 * every (cloud, pose) scene in one pass.  pc [bc,np,3] normalised clouds; H [bc*g,4,4] row-major poses in the un-normalised
 * cloud frame, row c*g + i belongs to cloud c (repeat_interleave order); gripper [ng,3] control points; pc_mean [bc,3] or
 * NULL (the points are then placed in the frame as given).  x [bc*g, 4, np+ng]: columns < np hold the cloud's xyz (bit
 * copies) and label 0, columns >= np hold (R p + t - pc_mean - pc_shift) / pc_scale and label 1,
 * evaluated in the reference's order (k-ordered fma chain of R p, then + t, - pc_mean, - pc_shift, one IEEE division).  pc_scale zero or NaN,
 * a null pointer or a non-positive count: GLDM_ERR_INVALID_ARG. */
int gldm_grasp_scene(const float *pc /*[bc,np,3]*/, const float *H /*[bc*g,4,4]*/, const float *gripper /*[ng,3]*/,
                     const float *pc_mean /*[bc,3] or NULL*/, float pc_shift, float pc_scale, int bc, int g, int np, int ng,
                     float *x /*[bc*g,4,np+ng]*/, gldm_stream_t stream);

/* ref: grasp_ldm/models/grasp_classifier.py:40-52,86-92: the `classifier` Sequential (SharedMLP(c -> rows) with its
 * BatchNorm(eval) folded, Dropout(eval), Conv1d(rows -> 1), Linear(n -> 1)) and the sigmoid on features x [b,c,n]:
 *   logit[b] = c0 + sum_n l[n] (w2 . relu(W1' x[b,:,n] + b1')),   prob = 1 / (1 + exp(-logit)),
 * c0 = lb + b2 sum_n l[n] from the caller.  `w1`: exact_f32 == 0: split-f16 A fragments of W1' with K zero-padded to a
 * multiple of 32 ([rows/16][K/32][plane][lane][8 f16], see "Split-f16 weight fragments"); exact_f32 != 0: f32 A fragments
 * [rows/16][c/16][lane][4].  16-byte aligned.  The GEMM runs on the matrix pipe (three f16 products per f32 product, the
 * 64-point tile split as x / s with s the power of two that brings its largest magnitude into [2^13, 2^14); or
 * v_mfma_f32_16x16x4_f32 with partial sums of 128 channels added in K order); ReLU, w2 and
 * l[n] are applied on the accumulators, neither [b,rows,n] nor [b,1,n] is written.  The sum over points runs in a fixed
 * order (lanes, waves, then one partial per 64-point tile in `workspace`, added in tile order by a second launch): no
 * atomics, bitwise repeatable, independent of b and of a scene's position.
 * c % 16 == 0, 16 <= c <= 2048; rows % 16 == 0, 16 <= rows <= 512; 1 <= n <= 2^20 (any n: tail columns are masked), b *
 * ceil(n / 64) < 2^31: GLDM_ERR_UNSUPPORTED otherwise.  `workspace`: gldm_cls_head_workspace_bytes(b, c, rows, n) bytes
 * (-1 for an unsupported shape), private to the stream until the work has finished; smaller: GLDM_ERR_WORKSPACE. */
long long gldm_cls_head_workspace_bytes(int b, int c, int rows, int n);
int gldm_cls_head(const float *x /*[b,c,n]*/, const void *w1, const float *b1 /*[rows]*/, const float *w2 /*[rows]*/,
                  const float *l /*[n]*/, float c0, int b, int c, int rows, int n, int exact_f32, void *workspace,
                  long long workspace_bytes, float *logit /*[b]*/, float *prob /*[b]*/, gldm_stream_t stream);

/* ------------------------------------------------ surface normals (additive, ABI 14; csrc/normals.hip) */

/* The search of estimate_normals_cam_from_pc (grasp_ldm/utils/pointcloud_helpers.py:74-97: cKDTree.query(k,
 * distance_upper_bound)).  pc [b,n,3] f32, finite.  For every point i of every cloud: the up to k points j of the same cloud
 * with the smallest squared distances among those with d2 <= r2, the point itself included, where
 *   d2(i, j) = (dx*dx + dy*dy) + dz*dz  in f32, differences first, one rounding per operation;  r2 = max_radius * max_radius
 * ordered by (d2, j) ascending (ties to the lower index).  idx [b,n,k] int32, d2 [b,n,k] f32 (or NULL), found [b,n] int32 =
 * the number of neighbours; slots behind found carry idx = n and d2 = +inf (scipy's convention).  A pure function of the
 * inputs: bitwise repeatable, independent of the launch shape and of the broad phase (boxes of 256-point chunks in the
 * workspace; a chunk is skipped only when the box-to-box distance, formed in the arithmetic of d2, exceeds the bound, which
 * no point pair can then meet).  A cloud in pixel order (gldm_depth_to_cloud) skips most chunks; a shuffled one degrades to
 * the full scan.  Two launches; no workgroup waits for another.
 * Envelope, checked before any pointer or the device is touched: b, n >= 1, max_radius >= 0 with a finite
 * r2 (GLDM_ERR_INVALID_ARG: +inf is the padding of d2, so no real neighbour may carry it);
 * 1 <= k <= 16, n <= 2^20 (GLDM_ERR_UNSUPPORTED).  workspace: gldm_knn_radius_workspace_bytes(b, n) bytes (a negative
 * GLDM_ERR_* status outside the envelope), uninitialised, private to the stream until the work has finished. */
long long gldm_knn_radius_workspace_bytes(int b, int n);
int gldm_knn_radius(const float *pc /*[b,n,3]*/, int b, int n, int k, float max_radius, void *workspace,
                    long long workspace_bytes, int32_t *idx /*[b,n,k]*/, float *d2 /*[b,n,k] or NULL*/,
                    int32_t *found /*[b,n]*/, gldm_stream_t stream);

/* vectorized_normal_computation (pointcloud_helpers.py:99-122).  Exactly one of idx [b,n,k] (gldm_knn_radius's; a slot
 * with idx outside [0, n) counts as the point itself) and neighbors [b,n,k,3] is given.  Per point: diffs = neighbour -
 * point in f32; the six sums of diffs^T diffs in f64 (products of f32 values are exact there; the reference's division by
 * k^2 does not change a direction and is dropped); the eigenvector of the smallest eigenvalue by cyclic Jacobi in f64, a
 * fixed number of sweeps; normalised; negated where dot(normal, point - view) >= 0 (view: HOST [3]; 0 = the reference's
 * "towards the camera", :120-121); rounded to f32.  Where fewer than 3 slots are live (idx form: inside [0, n); neighbors
 * form: all k) no plane is defined and the normal is the zero vector; the reference returns an arbitrary eigenvector of a
 * rank-deficient matrix there.  Envelope: that of gldm_knn_radius; view finite. */
int gldm_point_normals(const float *pc /*[b,n,3]*/, const int32_t *idx /*[b,n,k] or NULL*/,
                       const float *neighbors /*[b,n,k,3] or NULL*/, int b, int n, int k, const float *view /*host [3]*/,
                       float *normals /*[b,n,3]*/, gldm_stream_t stream);

/* ------------------------------------------------ sensor-cloud cleanup (additive; csrc/cloud_filter.hip) */

/* Outlier removal on ragged clouds (Open3D's remove_radius_outlier / remove_statistical_outlier; the reference has no
 * counterpart).  Layout of both entries: the one gldm_depth_to_objects writes and gldm_farthest_points_euclid_ragged reads:
 * points [rows,3] f32; cloud i is rows start[i] .. start[i] + min(count[i], n_max) (start / count: device int32 [b]; n_max:
 * a host upper bound of the counts; a negative count is 0, and a cloud whose range leaves [0, rows) is empty).  The ranges
 * do not overlap.  Rows outside every range are never read and their outputs never written; the gaps may hold anything.
 * Inside the ranges the points are finite.
 *
 * gldm_neighbor_stats: for every point i of every cloud, the up to k OTHER points j of its cloud (j != i by index, so a
 * duplicate is a neighbour at distance 0) with the smallest d2 among those with d2 <= r2, where
 *   d2(i, j) = (dx*dx + dy*dy) + dz*dz  in f32, differences first, one rounding per operation;  r2 = max_radius * max_radius
 * (gldm_knn_radius's arithmetic).  neighbors [rows] int32 = their number (<= k); score [rows] f32 = their mean distance,
 *   (float)(sum_s (double)sqrtf(d2_s) / (double)neighbors),  summed in f64 in ascending d2, sqrtf and the division IEEE;
 * +inf where neighbors = 0.  A pure function of the inputs: bitwise repeatable, independent of the launch shape and of the
 * broad phase (gldm_knn_radius's: boxes of the 256-row chunks of every cloud, counted from the cloud's own start; a chunk is
 * skipped only when its exact box-to-box distance exceeds the bound).  Two launches; no workgroup waits for another.
 * Envelope, checked before any pointer or the device is touched: b >= 1, n_max >= 0, rows >= 0, max_radius >= 0 with a
 * finite r2 (GLDM_ERR_INVALID_ARG); b <= 65535, n_max <= 2^20, 1 <= k <= 16 (GLDM_ERR_UNSUPPORTED).  n_max = 0 or rows = 0
 * is a no-op.  workspace: gldm_neighbor_stats_workspace_bytes(b, n_max) bytes (a negative GLDM_ERR_* status outside the
 * envelope), uninitialised, private to the stream until the work has finished. */
long long gldm_neighbor_stats_workspace_bytes(int b, int n_max);
int gldm_neighbor_stats(const float *points /*[rows,3]*/, const int32_t *start /*[b]*/, const int32_t *count /*[b]*/, int b,
                        int n_max, int rows, int k, float max_radius, void *workspace, long long workspace_bytes,
                        int32_t *neighbors /*[rows]*/, float *score /*[rows]*/, gldm_stream_t stream);

/* The keep rule on gldm_neighbor_stats' outputs and the ordered compaction.  Per cloud, over the points with neighbors >=
 * max(min_neighbors, 1):  N = their number,  mu = S1 / N with S1 = sum (double)score,  sigma = sqrt(sum ((double)score -
 * mu)^2 / (N - 1))  (the sample deviation; 0 for N < 2; mu = 0 for N = 0), all in f64 in a fixed order: inside a 256-row
 * chunk a fixed tree (the other points count as +0.0; a butterfly over each 64 rows with offsets 32, 16, .. 1, then
 * (w0 + w1) + (w2 + w3)), then the chunks in ascending order, two passes (gldm_plane_moments' rule).  stats [b,2] f64 = mu,
 * sigma.  A point is kept iff neighbors >= min_neighbors and, when the statistical rule is on (std_ratio >= 0; a negative
 * value switches it off), neighbors >= 1 and (double)score <= mu + (double)std_ratio * sigma.
 * The kept rows of every cloud go out in ascending row order, packed: cloud i is rows out_start[i] .. + out_count[i] of
 * out_points (out_start = the exclusive sum of out_count; rows copied bit for bit); kept [.] int32 = the source row of every
 * output row, relative to its cloud's start.  out_points [sum count, 3] and kept [sum count] are written up to the total
 * only.  Six or seven launches (per-chunk sums, per-cloud moments, twice; per-chunk counts, a scan, the write pass); no
 * atomics; no workgroup waits for another; two calls are bitwise equal.
 * Envelope, checked before any pointer or the device is touched: gldm_neighbor_stats' on b, n_max, rows, k; 0 <=
 * min_neighbors <= k, std_ratio not NaN (GLDM_ERR_INVALID_ARG).  With n_max = 0 or rows = 0 only out_start, out_count and
 * stats are written.  workspace: gldm_filter_outliers_workspace_bytes(b, n_max) bytes, 8-byte aligned, uninitialised, private
 * to the stream until the work has finished. */
long long gldm_filter_outliers_workspace_bytes(int b, int n_max);
int gldm_filter_outliers(const float *points /*[rows,3]*/, const int32_t *neighbors /*[rows]*/, const float *score /*[rows]*/,
                         const int32_t *start /*[b]*/, const int32_t *count /*[b]*/, int b, int n_max, int rows, int k,
                         int min_neighbors, float std_ratio, void *workspace, long long workspace_bytes,
                         float *out_points /*[sum count,3]*/, int32_t *out_start /*[b]*/, int32_t *out_count /*[b]*/,
                         int32_t *kept /*[sum count]*/, double *stats /*[b,2]*/, gldm_stream_t stream);

/* ------------------------------------------------ voxel-grid downsampling (additive; csrc/cloud_downsample.hip) */

/* One output row per occupied voxel of every cloud (Open3D's voxel_down_sample, PCL's VoxelGrid; the reference has no
 * counterpart).  Layout: that of gldm_neighbor_stats / gldm_filter_outliers above, word for word (points [rows,3] f32; start /
 * count device int32 [b]; host n_max; the ranges do not overlap; the gaps are never read; a range that leaves [0, rows) is
 * empty; inside the ranges the points are finite).
 * Per point and per axis, in f64:  t = (double)p / (double)voxel_size (IEEE division);  cell = floor(t);  q = rint(t * 65536.0)
 * (round-half-even).  The lattice is anchored at the ORIGIN, not at the cloud's min bound as in Open3D: the same voxel
 * means the same place in every frame and in every cloud.  Precondition: |t| < 2^20; beyond it cell is clamped to [-2^20,
 * 2^20 - 1] and q to [-2^36, 2^36], so addresses and sums stay safe whatever the data holds (the Python layer raises).
 * An output row is one occupied voxel of one cloud:  members = the number of its points;  first = the lowest source row among
 * them, relative to the cloud's start;  centroid per axis =
 *   (float)(((double)sum_q / (double)members) / 65536.0 * (double)voxel_size),  sum_q the exact int64 sum of q
 * (|q| <= 2^36 and members <= 2^22 give 2^58: no overflow).  The quantum is voxel_size * 2^-16 (30 nm at a 2 mm voxel).
 * Count, min and integer sums commute exactly, so nothing depends on execution order: two calls are bitwise equal and
 * numpy restates every bit (tests/cloud_downsample_ref.py).
 * The voxels of a cloud go out in ascending `first` (order of first appearance), packed as gldm_filter_outliers packs: cloud
 * i is rows out_start[i] .. + out_count[i] of out_points (out_start = the exclusive sum of out_count); first [.] and members
 * [.] int32 carry one entry per output row; voxel [rows] int32 (NULL allowed) = the output row of every source row,
 * relative to its cloud's out_start.  Rows past the total are never written; the gaps of voxel are never written.
 * A hash build (one table region of 2 * count slots per cloud, linear probing, vector atomics: compare-and-swap on the key,
 * 64-bit adds, add, min) and the ordered compaction of gldm_filter_outliers: five launches, six with voxel; no sort; no
 * workgroup waits for another.
 * Envelope, checked before any pointer or the device is touched: b >= 1, n_max >= 0, rows >= 0, voxel_size finite and > 0
 * (GLDM_ERR_INVALID_ARG); b <= 65535, n_max <= 2^22, rows <= 2^24 (GLDM_ERR_UNSUPPORTED).  With n_max = 0 or rows = 0 only
 * out_start and out_count are written.  workspace: gldm_voxel_downsample_workspace_bytes(b, n_max, rows) bytes (a negative
 * GLDM_ERR_* status outside the envelope), 8-byte aligned, uninitialised, private to the stream until the work has finished. */
long long gldm_voxel_downsample_workspace_bytes(int b, int n_max, int rows);
int gldm_voxel_downsample(const float *points /*[rows,3]*/, const int32_t *start /*[b]*/, const int32_t *count /*[b]*/, int b,
                          int n_max, int rows, float voxel_size, void *workspace, long long workspace_bytes,
                          float *out_points /*[sum count,3]*/, int32_t *out_start /*[b]*/, int32_t *out_count /*[b]*/,
                          int32_t *first /*[sum count]*/, int32_t *members /*[sum count]*/, int32_t *voxel /*[rows] or NULL*/,
                          gldm_stream_t stream);

/* ------------------------------------------------ Euclidean clustering (additive; csrc/cloud_cluster.hip) */

/* Connected components of an unorganised cloud under "closer than link_dist" (PCL's EuclideanClusterExtraction, Open3D's
 * cluster_dbscan with min_points = 1; the reference has no counterpart), for every cloud of a ragged batch.  Layout: that of
 * gldm_voxel_downsample above (points [rows,3] f32; start / count device int32 [b]; host n_max; the ranges do not overlap;
 * the gaps are never read; a range that leaves [0, rows) is empty), except that the points may hold anything.
 * Cell size.  cs = (double)link_dist * (1 + 2^-10).
 * Active row.  A row is active when all of these hold:
 *   - its three coordinates are finite;
 *   - per axis, floor((double)p / cs) lies strictly inside (-2^20, 2^20 - 1);
 *   - if plane is given, hgt = ((a*x + b*y) + c*z) + d satisfies hgt > h_min && hgt <= h_max (gldm_segment_tabletop's formula
 *     and rule, in f32).
 * Link.  Two active rows i, j of the same cloud are linked iff ((dx*dx + dy*dy) + dz*dz) <= link2, dx = xi - xj in f32,
 * link2 = link_dist * link_dist computed once in f32 on the host.
 * Components.  The transitive closure of links.  The root of a component is its lowest row, relative to the cloud's start.
 * Ranking.  Per cloud, components of at least min_points >= 1 rows are ranked by falling size, ties to the lower root.  The
 * first max_labels (1..64) become labels 1..K.
 * Outputs.  labels[row] is the label of the row's component, or 0; every row of every valid cloud range is written, rows
 * outside all ranges are left alone.  num_labels[i] = K.  label_points [b, max_labels] holds the sizes and label_root
 * [b, max_labels] the roots; past K they hold 0 and -1.
 * Every output is a pure function of the inputs: the components are a property of the link graph, the root is a minimum,
 * the sizes are counts; two calls are bitwise equal and numpy restates every value (tests/cloud_cluster_ref.py).
 * Why the grid may not lose a link.  The reference is the all-pairs test.  The rows are binned by cell = floor((double)p / cs)
 * and a row is tested against the rows of the 27 cells around its own.  The f32 test can admit a pair whose true per-axis
 * distance D exceeds link_dist L by a few ulp: |dx| = |fl(xi - xj)| >= |D| (1 - 2^-24), each of the product and the two sums of
 * non-negative terms loses at most another factor (1 - 2^-24), and link2 <= L^2 (1 + 2^-24), so an admitted pair has
 * D^2 <= L^2 (1 + 2^-24) / (1 - 2^-24)^5 and |D| < L (1 + 2^-21).  With the 2^-10 margin on cs:
 *   - every admitted pair has |D| < cs * (1 - 2^-11)   [(1 + 2^-10)(1 - 2^-11) = 1 + 2^-11 - 2^-21 > 1 + 2^-21];
 *   - the f64 quotients carry at most 2^-33 absolute error inside the lattice (|p / cs| < 2^20, one rounding of 2^-53 relative);
 *   - so the two quotients differ by less than 1 - 2^-11 + 2^-32 < 1 and their floors differ by at most 1.
 * link_dist must lie in [2^-60, 2^60]: then link2 is a normal f32, and a dx whose square underflows is far below cs.
 * Cost: about (rows of a 27-cell neighbourhood) distance tests per row.  A cloud with all its rows in one cell is
 * inherently quadratic: downsample first (gldm_voxel_downsample at a voxel below link_dist).
 * Eleven launches on one stream (csrc/cloud_cluster.hip names them); vector atomics only (compare-and-swap, add, min); no
 * host round trip; no workgroup waits for another; every loop is bounded by the data it walks.
 * Envelope, checked before any pointer or the device is touched: b >= 1, n_max >= 0, rows >= 0, min_points >= 1, max_labels
 * >= 1, link_dist in [2^-60, 2^60] (NaN fails), with a plane: no NaN in it and h_min < h_max (GLDM_ERR_INVALID_ARG); b <=
 * 65535, n_max <= 2^22, rows <= 2^24, max_labels <= 64 (GLDM_ERR_UNSUPPORTED).  With n_max = 0 or rows = 0 only num_labels,
 * label_points and label_root are written.  workspace: gldm_cluster_cloud_workspace_bytes(b, n_max, rows) bytes (a negative
 * GLDM_ERR_* status outside the envelope; 84 per row, 4 per chunk, 12 per cloud), 16-BYTE aligned, uninitialised, private to
 * the stream until the work has finished. */
long long gldm_cluster_cloud_workspace_bytes(int b, int n_max, int rows);
int gldm_cluster_cloud(const float *points /*[rows,3]*/, const int32_t *start /*[b]*/, const int32_t *count /*[b]*/, int b,
                       int n_max, int rows, float link_dist, const float *plane /*host [4] or NULL*/, float h_min, float h_max,
                       int min_points, int max_labels, void *workspace, long long workspace_bytes, int32_t *labels /*[rows]*/,
                       int32_t *num_labels /*[b]*/, int32_t *label_points /*[b,max_labels]*/,
                       int32_t *label_root /*[b,max_labels]*/, gldm_stream_t stream);

/* The ordered split of labelled clouds into their objects.  Layout as above; labels [rows] int32 is read inside the cloud
 * ranges only.  The rows with label 1..max_labels are packed cloud-major, then by ascending label, then by ascending row,
 * densely from row 0 of out_points (bit copies); rows with any other label (0, negative, above max_labels) are dropped.
 * out_row [.] is the source row relative to its cloud; obj_count [b, max_labels] the rows of (cloud, label); obj_start
 * [b, max_labels] their first row, absolute in out_points: the exclusive sum of obj_count in (cloud, label) order, so a
 * count of 0 keeps the running start; out_total [1] the rows written.  out_points / out_row past the total are never
 * written.  (out_points, obj_start, obj_count) is a ragged batch of b * max_labels clouds in the layout above.
 * Four launches: per-chunk per-label counts, a scan over the chunks of every (cloud, label), a scan over the (cloud, label)
 * table, and a write pass that ranks by ballot and popcount among equal labels.  No atomics: bitwise a pure function of the
 * inputs.
 * Envelope, checked before any pointer or the device is touched: b >= 1, n_max >= 0, rows >= 0, max_labels >= 1
 * (GLDM_ERR_INVALID_ARG); b <= 65535, n_max <= 2^22, rows <= 2^24, max_labels <= 64 and, because the counters are dense,
 * b * ceil(n_max / 256) * max_labels <= 2^24 (GLDM_ERR_UNSUPPORTED): one cloud of 2^22 rows or 256 clouds of 8192 at 64 labels
 * use 2^20 and 2^19 of them.  With n_max = 0 or rows = 0 only obj_start, obj_count and out_total are written.  workspace:
 * gldm_split_labels_workspace_bytes(b, n_max, rows, max_labels) bytes (4 per counter), 8-byte aligned, uninitialised. */
long long gldm_split_labels_workspace_bytes(int b, int n_max, int rows, int max_labels);
int gldm_split_labels(const float *points /*[rows,3]*/, const int32_t *labels /*[rows]*/, const int32_t *start /*[b]*/,
                      const int32_t *count /*[b]*/, int b, int n_max, int rows, int max_labels, void *workspace,
                      long long workspace_bytes, float *out_points /*[rows,3]*/, int32_t *out_row /*[rows]*/,
                      int32_t *obj_start /*[b,max_labels]*/, int32_t *obj_count /*[b,max_labels]*/, int32_t *out_total /*[1]*/,
                      gldm_stream_t stream);

/* ------------------------------------------------ meshes (additive; csrc/mesh_sample.hip, csrc/mesh_render.hip) */

/* A ragged batch of b triangle meshes.  vertices [n_verts,3] f32 and faces [n_faces,3] int32 are packed; mesh i owns the
 * vertex rows vert_start[i] .. + vert_count[i] and the face rows face_start[i] .. + face_count[i] (device int32 [b]); the
 * indices of a face are local to its mesh.  A face count is clamped to [0, 2^22] (and to f_max where an entry takes one);
 * a range that leaves its array is empty; a face with an index outside [0, vert_count) is DEGENERATE: its vertices are never
 * read, it has no area and draws nothing.  Nothing outside the arrays is ever addressed, whatever they hold.
 *
 * gldm_mesh_sample_surface: n points on every mesh, each on a face drawn with probability proportional to its area (the
 * rule of trimesh.sample.sample_surface; ref: grasp_ldm/dataset/acronym/acronym_pointclouds.py:173-176), made exact.
 * Face weight.  In f64 from the f32 vertices: e1 = v1 - v0, e2 = v2 - v0 per component; c = (e1y e2z - e1z e2y,
 *   e1z e2x - e1x e2z, e1x e2y - e1y e2x); n2 = (cx cx + cy cy) + cz cz; A = 0.5 * sqrt(n2).  A degenerate face, and one
 *   whose A is not a positive finite number, has A = 0.  Amax = the largest A of the mesh = m 2^e with m in [0.5, 1)
 *   (frexp).  q = (uint64) rint(ldexp(A, 40 - e)): the largest face weighs 2^39 .. 2^40, at most 2^22 faces sum below 2^62;
 *   every q is 0 when Amax is 0.  cum[f] = q[0] + .. + q[f] in the mesh's face order, total = cum[last]: integer sums.
 * Uniforms.  (u0, u1, u2) of sample i of mesh j, multiples of 2^-24 in [0, 1):
 *   - rand != NULL: rand[(j n + i) 3 + 0..2] (device f32), each first brought into [0, 1 - 2^-24] with
 *     fminf(fmaxf(u, 0), 1 - 2^-24) (a NaN becomes 0); k0 = (uint32)(u0 * 2^24), truncated;
 *   - rand == NULL: the words (x0, x1, x2, x3) of Philox4x32-10 with key = seed (low, high) and counter = (i, j, 0, 0)
 *     (the generator of gldm_denoise_rng; oracle/philox.py); k0 = x0 >> 8, u1 = (float)(x1 >> 8) * 2^-24, u2 likewise.
 * Face.  t = (k0 * total) >> 24 (an 88-bit product); the sample lies on the first face of the mesh with cum > t.
 * Point.  In f32, one rounding per written operation: if (u1 + u2 > 1) { u1 = 1 - u1; u2 = 1 - u2; } then per component
 *   p = v0 + ((v1 - v0) * u1 + (v2 - v0) * u2).
 * Outputs.  points [b,n,3]; face [b,n] (optional): the row of the packed face array; normals [b,n,3] (optional): (float)(c
 * / sqrt(n2)) per component, the f64 cross product above.  A mesh whose total is 0 (no faces, all degenerate) gets zero
 * points, zero normals and face -1.  Every element is written; two calls are bitwise equal; numpy restates every bit
 * (tests/mesh_ref.py).
 * Four launches on one stream (clear, areas with a vector atomicMax on the bits of non-negative doubles, weights + scan with
 * one workgroup per mesh, samples); no host round trip.
 * Envelope, checked before any pointer or the device is touched: b >= 1, f_max, n_verts, n_faces, n >= 0
 * (GLDM_ERR_INVALID_ARG); b <= 65535, f_max <= 2^22, n_verts <= 2^24, n_faces <= 2^24, n <= 2^24, b n <= 2^28
 * (GLDM_ERR_UNSUPPORTED).  f_max: at least the largest face_count (host).  n = 0 writes nothing.  workspace:
 * gldm_mesh_sample_surface_workspace_bytes(...) bytes (a negative GLDM_ERR_* status outside the envelope; 16 per face, 16 per
 * mesh), 8-byte aligned, uninitialised, private to the stream until the work has finished. */
long long gldm_mesh_sample_surface_workspace_bytes(int b, int f_max, int n_verts, int n_faces, int n);
int gldm_mesh_sample_surface(const float *vertices /*[n_verts,3]*/, const int32_t *faces /*[n_faces,3]*/,
                             const int32_t *vert_start /*[b]*/, const int32_t *vert_count /*[b]*/,
                             const int32_t *face_start /*[b]*/, const int32_t *face_count /*[b]*/, int b, int f_max, int n_verts,
                             int n_faces, int n, const float *rand /*[b,n,3] or NULL*/, unsigned long long seed, void *workspace,
                             long long workspace_bytes, float *points /*[b,n,3]*/, int32_t *face /*[b,n] or NULL*/,
                             float *normals /*[b,n,3] or NULL*/, gldm_stream_t stream);

/* gldm_render_depth: `frames` frames of h x w pixels of the meshes above seen by a pinhole camera at the origin looking down
 * +z with +x right and +y down -- the frame of gldm_depth_to_cloud, so that deprojecting a rendered frame lands on the
 * surface (ref: the pyrender depth frames of grasp_ldm/dataset/acronym/acronym_partial_pointclouds.py:521-581).
 * Instances.  Row k of the instance table (device arrays of n_inst rows) draws mesh inst_mesh[k] under the rigid transform
 * inst_xf[k] (obj_to_cam, 3 x 4 row major, f32) with label inst_label[k]; inst_tri[k] is its first RECORD: the caller's
 * exclusive sum of the face counts in table order, n_tris their total.  Record r belongs to the last instance with inst_tri <=
 * r and is face r - inst_tri of its mesh; a record whose instance has no such face, or a mesh id outside [0, b), draws
 * nothing.  Frame f draws the records from inst_tri[frame_start[f]] up to the first record of instance frame_start[f] +
 * frame_count[f] (n_tris behind the last); a frame whose instance range leaves the table is empty.
 * Vertex.  X = ((m00 x + m01 y) + m02 z) + m03, Y and Z likewise (gldm_depth_to_cloud's expression); px = (X * fx) / Z + cx,
 * py = (Y * fy) / Z + cy; f32, one rounding each.
 * Dropped triangles.  A triangle with a vertex for which Z >= z_near does not hold (NaN included), or with a projected
 * coordinate that is not finite, is dropped whole -- there is no clipping -- and counted in dropped[f].  Degenerate faces
 * (above) are skipped without being counted.
 * Coverage.  Pixel (u, v) is sampled at its integer coordinates (gldm_depth_to_cloud's convention; an OpenGL renderer samples
 * at u + 0.5, v + 0.5: shift cx, cy by 0.5 to compare).  For an edge a -> b, E_ab = (bx - ax)(v - ay) - (by - ay)(u - ax) in
 * f64 from the f32 projections, when (ax, ay) <= (bx, by) lexicographically; otherwise E_ab = -E_ba, E_ba evaluated that
 * way: the two triangles on a shared edge see bitwise opposite values, which leaves no cracks and draws no pixel of an
 * interior edge less than once.  w0 = E_bc, w1 = E_ca, w2 = E_ab, S = (w0 + w1) + w2.  The pixel is inside when min(px) <=
 * u <= max(px) and min(py) <= v <= max(py) (f32 comparisons; implied by the rest in exact arithmetic, stated so that the
 * broad phase is exact), all three w are >= 0 or all three are <= 0, and S != 0.  There is no back-face culling.
 * Depth.  z = (float)(1 / (((w0 / za + w1 / zb) + w2 / zc) / S)) in f64, za .. zc the vertices' Z; kept iff z_near <= z <=
 * z_far.
 * Resolve.  The pixel takes the minimum of (bits(z) << 32) | r over the kept records r of its frame: the nearest surface,
 * coincident surfaces to the lower record.
 * Outputs.  depth [frames,h,w] f32, 0 where empty; label (optional) int32, the instance's label, 0 where empty; face
 * (optional) int32, the row of the packed face array, -1 where empty; dropped [frames] int32.  Every element is written;
 * bitwise a pure function of the inputs (tests/mesh_ref.py restates every bit).
 * Two launches: one record and one pixel box per (instance, face); then one workgroup per 16 x 16 pixel tile, which walks its
 * frame's boxes 256 at a time, stages the records whose box meets the tile in LDS and keeps every pixel's minimum in
 * registers.  No atomics on device memory, no initialising pass, no workgroup waits for another.
 * Envelope, checked before any pointer or the device is touched: b, frames, h, w >= 1, n_verts, n_faces, n_inst, n_tris >= 0,
 * fx, fy finite and != 0, cx, cy finite, 0 < z_near < z_far < inf (GLDM_ERR_INVALID_ARG); b <= 65535, n_verts, n_faces <=
 * 2^24, n_inst <= 65535, n_tris <= 2^24, frames <= 65535, h w <= 2^24 (GLDM_ERR_UNSUPPORTED).  workspace:
 * gldm_render_depth_workspace_bytes(...) bytes (64 per record), 16-BYTE aligned, uninitialised. */
long long gldm_render_depth_workspace_bytes(int b, int n_verts, int n_faces, int n_inst, int n_tris, int frames, int h, int w);
int gldm_render_depth(const float *vertices /*[n_verts,3]*/, const int32_t *faces /*[n_faces,3]*/,
                      const int32_t *vert_start /*[b]*/, const int32_t *vert_count /*[b]*/, const int32_t *face_start /*[b]*/,
                      const int32_t *face_count /*[b]*/, int b, int n_verts, int n_faces, const int32_t *inst_mesh /*[n_inst]*/,
                      const float *inst_xf /*[n_inst,12]*/, const int32_t *inst_label /*[n_inst]*/,
                      const int32_t *inst_tri /*[n_inst]*/, int n_inst, int n_tris, const int32_t *frame_start /*[frames]*/,
                      const int32_t *frame_count /*[frames]*/, int frames, int h, int w, float fx, float fy, float cx, float cy,
                      float z_near, float z_far, void *workspace, long long workspace_bytes, float *depth /*[frames,h,w]*/,
                      int32_t *label /*[frames,h,w] or NULL*/, int32_t *face /*[frames,h,w] or NULL*/,
                      int32_t *dropped /*[frames]*/, gldm_stream_t stream);

/* ------------------------------------------------ grasp selection (additive, ABI 14; csrc/grasp_select.hip) */

/* Gripper clearance and finger-sweep contacts of every pose against a whole scene cloud.  The geometry is the
 * reference's (grasp_ldm/utils/gripper.py:26-47: the four segments of the open gripper and the two "finger sweep"
 * segments between the finger tips; :80-128 wraps both in tubes "for checking collisions in the grasp area"); the
 * reference only draws them.  scene [b,ns,3] f32 in the frame of the poses; H [b*g,4,4] row-major, row c*g + i belongs
 * to cloud c.  `body` [sb,2,3] and `sweep` [ss,2,3] are HOST arrays of segments (a, b) in the gripper frame (as radius
 * and u of gldm_ball_query_multi: they travel as kernel arguments).  For a pose (R, t) a scene point p becomes
 * q = R^T (p - t); its distance to a segment is |q - a - u (b - a)|, u = clamp((q - a).(b - a) / |b - a|^2, 0, 1).
 *   clearance[c*g + i] = min(cap, min over points and body segments of that distance)
 *   contacts[c*g + i]  = points whose smallest SQUARED distance to a sweep segment is <= r_sweep^2 (0 when ss = 0)
 * A point farther than rho + max(cap, r_sweep) (plus a margin) from the centre of the gripper's bounding sphere of radius
 * rho changes neither output and is skipped, a staged chunk of gldm_grasp_clearance_chunk() points at a time.  Both
 * reductions are exact (min of non-negative floats through their integer views, integer sum; device atomics behind an
 * initialising launch): bitwise repeatable, independent of b, of a pose's position and of how the scene is split.  No FMA
 * contraction.  Inputs must be finite (the caller checks).
 * Envelope, checked before any pointer or the device is touched: 1 <= ns <= 2^24, 1 <= sb <= 8, 0 <= ss <= 8 or
 * GLDM_ERR_UNSUPPORTED; b, g >= 1, cap > 0, r_sweep >= 0, no null pointer or GLDM_ERR_INVALID_ARG. */
int gldm_grasp_clearance_chunk(void);
int gldm_grasp_clearance(const float *scene /*[b,ns,3]*/, const float *H /*[b*g,4,4]*/, int b, int g, int ns,
                         const float *body /*host [sb,2,3]*/, int sb, const float *sweep /*host [ss,2,3] or NULL*/, int ss,
                         float r_sweep, float cap, float *clearance /*[b*g]*/, int32_t *contacts /*[b*g]*/,
                         gldm_stream_t stream);

/* The contacts of gldm_grasp_clearance judged by the friction cone (additive, ABI 14).  normals [b,ns,3]: unit surface
 * normals of the scene points (gldm_point_normals; a zero vector = no normal).  The contact set is that of
 * gldm_grasp_clearance -- points whose smallest squared distance to a sweep segment is <= r_sweep^2, q = R^T (p - t) formed
 * by the same instructions -- split by finger: side 0 is q.x > 0 (the left finger of the open gripper, gripper.py:26-31),
 * side 1 the rest.
 *   contacts_side[(c*g + i)*2 + s] = contacts of side s; the two sum to gldm_grasp_clearance's contacts, bit for bit
 *   aligned[(c*g + i)*2 + s]       = those with fabsf((R00*nx + R10*ny) + R20*nz) >= cos_friction and n != 0: the normal
 *                                    lies within the friction angle of the pose's closing axis (first column of R), either
 *                                    way round, so the frame in which the normals were oriented does not matter
 * Integer sums behind a clearing memset: exact, bitwise repeatable, independent of how the scene is split.  One scan with
 * gldm_grasp_clearance (a template flag of the same kernel); the broad phase uses the sweep family's own bounding sphere.
 * Envelope as gldm_grasp_clearance (1 <= ns <= 2^24, 0 <= ss <= 8 or GLDM_ERR_UNSUPPORTED); 0 <= cos_friction <= 1. */
int gldm_grasp_contact_normals(const float *scene /*[b,ns,3]*/, const float *normals /*[b,ns,3]*/,
                               const float *H /*[b*g,4,4]*/, int b, int g, int ns, const float *sweep /*host [ss,2,3] or NULL*/,
                               int ss, float r_sweep, float cos_friction, int32_t *contacts_side /*[b,g,2]*/,
                               int32_t *aligned /*[b,g,2]*/, gldm_stream_t stream);

/* Which k of a cloud's g candidate poses to keep: one workgroup per cloud, the rounds run inside the launch.
 * score [b*g] f32 (finite); keep [b*g] uint8 or NULL (all); ctrl [np,3]: HOST array of gripper control points.
 * mode 0 (top-k): the kept candidates in the order (score falling, index rising); gap is written 0.
 * mode 1 (diverse): greedy farthest-pose selection under the reference's control-point distance
 *   D(i, j) = (1/np) sum_k |H_i c_k - H_j c_k|^2      (grasp_ldm/losses/loss.py:77-127)
 * evaluated in closed form around the control points' centroid cb:
 *   D = |dt + dR cb|^2 + tr(dR Me dR^T),  dt, dR = differences of the two poses, Me = (1/np) sum (c - cb)(c - cb)^T.
 * First pick: highest score, lowest index on a tie.  m_j = min over the picks so far of D(pick, j); every later pick
 * maximises m_j, lowest index on a tie.  Picking stops after k picks, when no candidate is left, or when the best
 * m_j < min_separation^2.  gap = sqrt(m) of a pick when it was taken (RMS control-point distance to the nearest earlier
 * pick, metres); +inf for the first pick.
 * index [b,k]: -1 behind the last pick; count [b]; gap [b,k]: 0 behind the last pick.  Every slot is written.
 * Envelope: 1 <= k <= g <= 2048, 1 <= np <= 64 or GLDM_ERR_UNSUPPORTED (checked first, as above). */
int gldm_select_grasps(const float *H /*[b*g,4,4]*/, const float *score /*[b*g]*/, const uint8_t *keep /*[b*g] or NULL*/,
                       int b, int g, const float *ctrl /*host [np,3]*/, int np, int k, int mode, float min_separation,
                       int32_t *index /*[b,k]*/, int32_t *count /*[b]*/, float *gap /*[b,k]*/, gldm_stream_t stream);

/* ---- Unet1D (additive; ref: grasp_ldm/models/modules/resnets.py:622-857) ------------------------------------------------
 * One kernel carries a tile of `tile_samples` samples through the whole U-net and through every sampler step; the skip
 * stack, the stem's output and the residual stream stay in LDS (csrc/unet1d.hip).  The packed buffer holds the weights and,
 * at `prog_off`, the network as a PROGRAM of n_ops ops of GLDM_UNET1D_OP_INTS int32 each, the first the op's code (enum
 * gldm_unet1d_op; graspldm_amd/unet1d_pack.py writes and bounds-checks it; LDS offsets in floats, weight offsets in floats from the buffer's start, -1 = absent):
 *   CONV  {1, src0, c0, pitch_in, src1, c1, dst, pitch_out, M, mode, taps, Lin, Lout, w, bias, add}
 *         dst[M][col] = W im2col(src0 | src1) + bias + add.  mode 0: taps centred (k = 1 / 3, resnets.py:130,191,748,767);
 *         1: k = 4, stride 2, pad 1 (Downsample, :75-76); 2: nearest x2 then k = 3, pad 1 (Upsample, :68-72).  A second
 *         source is the popped skip of an up block (:843-847) or `r` (:854): the concatenation is never built.  W is
 *         [M/16][K/32][hi|lo][64][8 f16] (split-f16, the layout above) or, with exact_f32, [M/16][K/32][64][8 f32], K running
 *         over [source][tap][channels padded to 32 with zero columns].  Also computes every ResnetBlock's scale/shift rows
 *         (:193-202) from the tile's summed SiLU(embedding) columns (Lin = Lout = 1).
 *   GN    {2, buf, C, pitch, L, gamma, beta, use_scale_shift, add, out, groups}   Block.norm + scale/shift + SiLU (:160-177)
 *   ATT   {3, x, C, pitch, L, out, ln_buf, y_buf, ln_g, qkv_w, out_w, out_b, ln2_g}  Residual(PreNorm(LinearAttention))
 *         (:211-235), or with ln2_g = -1 Residual(PreNorm(Attention)) (:238-261); qkv_w rows in head-major order
 *         [head][q|k|v][32], out_w one [C x 32] matrix per head
 *   FINAL {4, x, C, pitch, w, b}  final_conv (:776,857)        STEM {5, dst, C, pitch, w, b}  init_conv (:681,805) */
enum gldm_unet1d_op {
  GLDM_UNET1D_OP_CONV = 1, GLDM_UNET1D_OP_GN = 2, GLDM_UNET1D_OP_ATT = 3, GLDM_UNET1D_OP_FINAL = 4, GLDM_UNET1D_OP_STEM = 5
};
#define GLDM_UNET1D_OP_INTS 16   /* int32 per op */
/* Pitch of the o_emb rows: 16 columns + 2 (the four lane groups of a B read fall into different banks). */
#define GLDM_UNET1D_EMB_PITCH 18
#define GLDM_UNET1D_MAX_LEVELS 4
typedef struct gldm_unet1d_desc {
  int32_t dim, n_levels;
  int32_t widths[GLDM_UNET1D_MAX_LEVELS + 1]; /* init_dim, then dim * dim_mults                                 */
  int32_t groups, emb_dim;
  int32_t cond_rows;    /* R of z_cond [n, R, Dc]; 1 for [n, Dc]; 0 without input conditioning                  */
  int32_t time_cond;    /* is_time_conditioned (then cond_rows <= 1: :816-822 adds the two embeddings untiled)  */
  int32_t has_emb;      /* time_cond || cond_rows > 0: the ResnetBlocks apply scale/shift                       */
  int32_t exact_f32;    /* packed under numerics.f32_only(): f32 fragments, v_mfma_f32_16x16x4_f32              */
  int32_t seq_len;      /* L the program's LDS map was laid out for                                             */
  int32_t tile_samples; /* samples per workgroup, sized on the host from the LDS the net needs                  */
  int32_t lds_floats;   /* dynamic LDS of a workgroup                                                           */
  int32_t prog_off, n_ops;
  int32_t o_lat, o_eps; /* [tile_samples][L] current latent row / network output                                */
  int32_t o_emb;        /* [emb_dim][GLDM_UNET1D_EMB_PITCH] summed SiLU(embedding) per sample column            */
  int32_t o_ss;         /* [2 C][tile_samples] scale (+1, summed over R) and shift rows of the running block    */
  int32_t o_qkv, o_o, o_a; /* attention: one head's q|k|v rows [96][pitch], its output [32][pitch], A [S][L][L]  */
  int32_t n_floats;     /* length of the packed buffer                                                          */
} gldm_unet1d_desc;

/* 0 if gldm_unet1d runs this architecture at this length, GLDM_ERR_UNSUPPORTED otherwise (GLDM_ERR_INVALID_ARG for a null
 * descriptor); decided from the header fields alone, before any HIP call.  dim in {16, 32}; 2..4 levels; widths
 * multiples of 16, at most 256; groups 4 or 8; emb_dim = 4 dim; cond_rows <= 4 (<= 1 with time conditioning); 2 <= L <= 16
 * with L % 2^(levels-1) == 0 (the reference fails at the first skip concat otherwise, :843). */
int gldm_unet1d_supported(const gldm_unet1d_desc *desc, int seq_len);

/* ref: resnets.py:779-857 (Unet1D.forward) and gaussian_diffusion.py:232-277 (the sample loop), fused like gldm_denoise:
 * ONE launch runs all n_steps for every row.  sched_kind NONE with n_steps = 1 returns the module's output (sample_t
 * [n] then gives a per-sample timestep); DDIM / DDPM read the coefficient rows documented at GLDM_SCHED_COEF_STRIDE;
 * step_noise [n_steps, n, L] is read by DDPM steps with coef[7] != 0.  temb [T, emb_dim] is the host-evaluated time_mlp
 * table (:710-715), cemb [n_cond, R, emb_dim] = input_emb_layers(z_cond) (:724-728), row i conditioned on
 * cemb[i / samples_per_cond]; either is NULL when the net has no such conditioning.  No workspace. */
int gldm_unet1d(const gldm_unet1d_desc *desc, const float *weights, const float *temb, const float *cemb,
                int samples_per_cond, const float *x_in /*[n,1,L]*/, int n_samples, int seq_len,
                const int32_t *timesteps /*[n_steps]*/, const int32_t *sample_t, int n_steps, int sched_kind,
                int clip_sample, const float *sched_coef /*[n_steps,8]*/, const float *step_noise,
                float *x_out /*[n,1,L]*/, gldm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLDM_H_ */
