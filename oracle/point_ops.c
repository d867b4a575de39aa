/*
 * oracle/point_ops.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Scalar, single-threaded C restatement of the nine forward point-cloud kernels
 * of the reference's `_pvcnn_backend` CUDA extension.  The reference has no
 * host implementation of these ops (every entry point is CHECK_CUDA-guarded),
 * so this file defines the canonical CPU semantics the HIP kernels are checked
 * against:  f32 arithmetic in the source's written operation order, no FMA
 * contraction (build with -ffp-contract=off), int32 indices, and for the
 * float-atomic voxel scatter the canonical order "ascending point index".
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library.  Parity status: pinned to the reference's own kernels,
 * compiled unmodified for gfx950 (oracle/ref_build.py) and run on an MI355X:
 * bit-equal on every case of tests/test_ref_kernels_gpu.py, and replayed from
 * tests/golden/ref_point_ops.npz in tests/test_oracle_point_ops.py, which also
 * cross-checks an independent torch formulation.
 *
 * All paths cited are relative to
 *   /root/reference/grasp_ldm/models/modules/ext/pvcnn/modules/functional/src/
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORACLE_API __attribute__((visibility("default")))

/* ball_query/ball_query.cu:19-50.  out must be zero-initialised by the caller
 * (ball_query.cpp:20-22 uses torch::zeros). */
ORACLE_API void oracle_ball_query(int b, int n, int m, float r2, int u,
                                  const float *centers, const float *points,
                                  int32_t *out) {
  for (int bi = 0; bi < b; ++bi) {
    const float *pc = points + (size_t)bi * n * 3;
    const float *cc = centers + (size_t)bi * m * 3;
    int32_t *o = out + (size_t)bi * m * u;
    for (int j = 0; j < m; ++j) {
      float cx = cc[j], cy = cc[j + m], cz = cc[j + m + m];
      for (int k = 0, cnt = 0; k < n && cnt < u; ++k) {
        float dx = cx - pc[k];
        float dy = cy - pc[k + n];
        float dz = cz - pc[k + n + n];
        float d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < r2) {
          if (cnt == 0)
            for (int v = 0; v < u; ++v) o[j * u + v] = k;
          o[j * u + cnt] = k;
          ++cnt;
        }
      }
    }
  }
}

/* grouping/grouping.cu:18-36 */
ORACLE_API void oracle_grouping(int b, int c, int n, int m, int u,
                                const float *feat, const int32_t *idx,
                                float *out) {
  for (int bi = 0; bi < b; ++bi) {
    const float *f = feat + (size_t)bi * n * c;
    const int32_t *id = idx + (size_t)bi * m * u;
    float *o = out + (size_t)bi * m * u * c;
    for (int l = 0; l < c; ++l)
      for (int j = 0; j < m; ++j)
        for (int k = 0; k < u; ++k)
          o[((size_t)l * m + j) * u + k] = f[(size_t)l * n + id[j * u + k]];
  }
}

/* sampling/sampling.cu:17-31 */
ORACLE_API void oracle_gather(int b, int c, int n, int m, const float *feat,
                              const int32_t *idx, float *out) {
  for (int bi = 0; bi < b; ++bi)
    for (int l = 0; l < c; ++l) {
      const float *f = feat + ((size_t)bi * c + l) * n;
      const int32_t *id = idx + (size_t)bi * m;
      float *o = out + ((size_t)bi * c + l) * m;
      for (int j = 0; j < m; ++j) o[j] = f[id[j]];
    }
}

/* sampling/sampling.cu:86-167 with the launch shape of :169-174 (512 threads)
 * and the 1e38 distance initialisation of sampling.cpp:53-54.  The 512-slot
 * strided scan and the shared-memory tree are emulated literally so that ties
 * resolve exactly as on the device: strict '>' inside a thread (lowest k wins),
 * strict '<' in the tree (lower slot wins). */
ORACLE_API void oracle_fps(int b, int n, int m, const float *coords,
                           float *dist_scratch, int32_t *out) {
  enum { BS = 512 };
  float dists[BS];
  int dists_i[BS];
  if (m <= 0) return;
  for (int bi = 0; bi < b; ++bi) {
    const float *xyz = coords + (size_t)bi * n * 3;
    float *dist = dist_scratch + (size_t)bi * n;
    int32_t *o = out + (size_t)bi * m;
    for (int k = 0; k < n; ++k) dist[k] = 1e38f;
    int old = 0;
    o[0] = old;
    for (int j = 1; j < m; ++j) {
      float x1 = xyz[old], y1 = xyz[old + n], z1 = xyz[old + n + n];
      for (int t = 0; t < BS; ++t) {
        int besti = 0;
        float best = -1.0f;
        for (int k = t; k < n; k += BS) {
          float td = dist[k];
          float x2 = xyz[k], y2 = xyz[k + n], z2 = xyz[k + n + n];
          float d = (x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1) +
                    (z2 - z1) * (z2 - z1);
          float d2 = d < td ? d : td; /* min(d, td) */
          if (d2 != td) dist[k] = d2;
          if (d2 > best) {
            best = d2;
            besti = k;
          }
        }
        dists[t] = best;
        dists_i[t] = besti;
      }
      for (int s = 0; (1 << s) < BS; ++s) {
        int active = BS >> (s + 1);
        for (int t = 0; t < active; ++t) {
          int i1 = (t * 2) << s, i2 = (t * 2 + 1) << s;
          if (dists[i1] < dists[i2]) {
            dists[i1] = dists[i2];
            dists_i[i1] = dists_i[i2];
          }
        }
      }
      old = dists_i[0];
      o[j] = old;
    }
  }
}

/* interpolate/neighbor_interpolate.cu:20-75 (3-NN search + weights) and
 * :90-116 (weighted gather).  Running bests are double, d is f32. */
ORACLE_API void oracle_three_nn_interpolate(int b, int c, int m, int n,
                                            const float *points,
                                            const float *centers,
                                            const float *cfeat, int32_t *idx,
                                            float *wgt, float *out) {
  for (int bi = 0; bi < b; ++bi) {
    const float *pc = points + (size_t)bi * 3 * n;
    const float *cc = centers + (size_t)bi * 3 * m;
    float *w = wgt + (size_t)bi * 3 * n;
    int32_t *id = idx + (size_t)bi * 3 * n;
    for (int j = 0; j < n; ++j) {
      float ux = pc[j], uy = pc[j + n], uz = pc[j + n + n];
      double best0 = 1e40, best1 = 1e40, best2 = 1e40;
      int i0 = 0, i1 = 0, i2 = 0;
      for (int k = 0; k < m; ++k) {
        float x = cc[k], y = cc[k + m], z = cc[k + m + m];
        float d = (ux - x) * (ux - x) + (uy - y) * (uy - y) +
                  (uz - z) * (uz - z);
        if (d < best2) {
          best2 = d; i2 = k;
          if (d < best1) {
            best2 = best1; i2 = i1;
            best1 = d; i1 = k;
            if (d < best0) {
              best1 = best0; i1 = i0;
              best0 = d; i0 = k;
            }
          }
        }
      }
      best0 = fmax(fmin((double)1e10f, best0), (double)1e-10f);
      best1 = fmax(fmin((double)1e10f, best1), (double)1e-10f);
      best2 = fmax(fmin((double)1e10f, best2), (double)1e-10f);
      float d0d1 = (float)(best0 * best1);
      float d0d2 = (float)(best0 * best2);
      float d1d2 = (float)(best1 * best2);
      float inv = 1.0f / (d0d1 + d0d2 + d1d2);
      w[j] = d1d2 * inv;          id[j] = i0;
      w[j + n] = d0d2 * inv;      id[j + n] = i1;
      w[j + n + n] = d0d1 * inv;  id[j + n + n] = i2;
    }
    const float *cf = cfeat + (size_t)bi * m * c;
    float *o = out + (size_t)bi * n * c;
    for (int l = 0; l < c; ++l)
      for (int j = 0; j < n; ++j) {
        float w1 = w[j], w2 = w[j + n], w3 = w[j + n + n];
        int a1 = id[j], a2 = id[j + n], a3 = id[j + n + n];
        o[(size_t)l * n + j] = cf[(size_t)l * m + a1] * w1 +
                               cf[(size_t)l * m + a2] * w2 +
                               cf[(size_t)l * m + a3] * w3;
      }
  }
}

/* voxelization/vox.cu:18-34 (grid_stats) + :48-72 (avg_voxelize).  ind/cnt/out
 * must be zero-initialised (vox.cpp:31-36).  The reference accumulates with
 * f32 atomicAdd in unspecified order; the canonical order here is ascending
 * point index i. */
ORACLE_API void oracle_avg_voxelize(int b, int c, int n, int r,
                                    const float *feat, const int32_t *coords,
                                    int32_t *ind, int32_t *cnt, float *out) {
  int r2 = r * r, r3 = r2 * r;
  for (int bi = 0; bi < b; ++bi) {
    const int32_t *co = coords + (size_t)bi * n * 3;
    int32_t *in = ind + (size_t)bi * n;
    int32_t *cn = cnt + (size_t)bi * r3;
    const float *f = feat + (size_t)bi * c * n;
    float *o = out + (size_t)bi * c * r3;
    for (int i = 0; i < n; ++i) {
      in[i] = co[i] * r2 + co[i + n] * r + co[i + n + n];
      cn[in[i]] += 1;
    }
    for (int i = 0; i < n; ++i) {
      int pos = in[i];
      int cur = cn[pos];
      if (cur > 0) {
        float div = (float)(1.0 / (double)(float)cur);
        for (int j = 0; j < c; ++j)
          o[(size_t)j * r3 + pos] += f[(size_t)j * n + i] * div;
      }
    }
  }
}

/* interpolate/trilinear_devox.cu:21-105, eval branch (is_training == false
 * skips the inds/wgts stores; pass NULL).  When inds/wgts are non-NULL the
 * training-mode side outputs [b,8,n] are written too. */
ORACLE_API void oracle_trilinear_devoxelize(int b, int c, int n, int r,
                                            const float *coords,
                                            const float *feat, int32_t *inds,
                                            float *wgts, float *outs) {
  int r2 = r * r, r3 = r2 * r;
  for (int bi = 0; bi < b; ++bi) {
    const float *co = coords + (size_t)bi * n * 3;
    const float *f = feat + (size_t)bi * c * r3;
    float *o = outs + (size_t)bi * c * n;
    for (int i = 0; i < n; ++i) {
      float x = co[i], y = co[i + n], z = co[i + n + n];
      float xl = floorf(x), yl = floorf(y), zl = floorf(z);
      float xd1 = x - xl, yd1 = y - yl, zd1 = z - zl;
      float xd0 = 1.0f - xd1, yd0 = 1.0f - yd1, zd0 = 1.0f - zd1;
      float w000 = xd0 * yd0 * zd0, w001 = xd0 * yd0 * zd1;
      float w010 = xd0 * yd1 * zd0, w011 = xd0 * yd1 * zd1;
      float w100 = xd1 * yd0 * zd0, w101 = xd1 * yd0 * zd1;
      float w110 = xd1 * yd1 * zd0, w111 = xd1 * yd1 * zd1;
      int xlo = (int)xl, ylo = (int)yl, zlo = (int)zl;
      int xhi = (xd1 > 0) ? -1 : 0;
      int yhi = (yd1 > 0) ? -1 : 0;
      int zhi = (zd1 > 0) ? 1 : 0;
      int i000 = xlo * r2 + ylo * r + zlo;
      int i001 = i000 + zhi;
      int i010 = i000 + (yhi & r);
      int i011 = i010 + zhi;
      int i100 = i000 + (xhi & r2);
      int i101 = i100 + zhi;
      int i110 = i100 + (yhi & r);
      int i111 = i110 + zhi;
      if (inds && wgts) {
        float *w = wgts + (size_t)bi * n * 8;
        int32_t *id = inds + (size_t)bi * n * 8;
        w[i] = w000; w[i + n] = w001; w[i + n * 2] = w010; w[i + n * 3] = w011;
        w[i + n * 4] = w100; w[i + n * 5] = w101; w[i + n * 6] = w110;
        w[i + n * 7] = w111;
        id[i] = i000; id[i + n] = i001; id[i + n * 2] = i010;
        id[i + n * 3] = i011; id[i + n * 4] = i100; id[i + n * 5] = i101;
        id[i + n * 6] = i110; id[i + n * 7] = i111;
      }
      for (int j = 0; j < c; ++j) {
        const float *fj = f + (size_t)j * r3;
        o[(size_t)j * n + i] =
            w000 * fj[i000] + w001 * fj[i001] + w010 * fj[i010] +
            w011 * fj[i011] + w100 * fj[i100] + w101 * fj[i101] +
            w110 * fj[i110] + w111 * fj[i111];
      }
    }
  }
}
