// point_attention_fused.hip -- the attention core for MANY tokens at FEW channels (voxel attention inside PVConv: n = r^3
// up to 4096 at c <= 128).  The norms of the voxel attention stack around it (gldm_groupnorm_affine,
// gldm_groupnorm_swish_points_sum) are voxel_norm.hip's.
//
//   out[b, c, i] = sum_j v[b, c, j] softmax_j( sum_c' q[b, c', i] k[b, c', j] )          (no 1 / sqrt(c) factor)
//
// The contract of gldm_point_attention (point_attention.hip), which materialises the n x n scores and probabilities in a
// workspace; this kernel never writes an n x n tensor and takes no workspace.  A workgroup of four waves owns 128
// queries of one cloud, a wave 32 of them (two 16-query column tiles); the wave's q lives in REGISTERS as the B fragments
// of the scores product for the whole kernel.  Keys are walked in tiles of 32, staged once per workgroup in LDS (double
// buffered, one barrier per tile) in the two fragment orders the two products read:
//   A1  rows = keys, K = channels      (scores, transposed: S^T = k^T q, rows = keys, columns = queries)
//   A2  rows = channels, K = keys      (apply: out = v P^T), the keys of a K block in the order the accumulators of the two
//       16-key score tiles leave them in a lane: K index 8 g + t  <->  key 4 g + t (t < 4), 16 + 4 g + t - 4 (t >= 4).
// The score accumulators of a lane are therefore, after exp, the B fragment of the apply product as they stand: P never
// leaves the registers (the "B operands made in place from the accumulators with K-permuted weights" of quad_narrow.h).
// Softmax is ONLINE: a running maximum and sum per query; when the maximum grows the accumulators are rescaled by
// exp(old - new).  A row's maximum is in-lane over 8 scores and two permlane swaps across the four 16-lane groups.  One
// division per row at the end.
// Split arithmetic (default): products as three v_mfma_f32_16x16x32_f16 over hi / lo pieces.  q is split as q / s per
// 16-query tile, a staged k tile and a staged v tile as x / s per TILE (s a power of two from the tile's largest magnitude,
// range_pow2: 1 for anything ordinary), folded back on the accumulators; probabilities are split as 2^14 p.
// exact_f32: the same stages on v_mfma_f32_16x16x4_f32 from f32 tiles in LDS, no scales.
// Fixed summation order, no atomics, nothing waits on another workgroup; a cloud's bits do not depend on b, on its
// position in the batch or on the stream.
#include "mfma_prims.h"

namespace {

constexpr int kFusedKeys = 32;      // keys per staged tile
constexpr int kFusedNT = 2;         // 16-query tiles per wave
constexpr int kFusedQ = 4 * 16 * kFusedNT;   // queries per workgroup
constexpr float kFPScale = 16384.f, kFPScaleInv = 1.f / 16384.f;
constexpr float kLog2e = 1.44269504088896340736f;

inline bool fused_shape_ok(int c, int n) { return c % 16 == 0 && c >= 32 && c <= 128 && n % 32 == 0 && n >= 32 && n <= 4096; }

// LDS map (bytes).  Split: per buffer A1 = [key tile 2][K block KB][plane 2][lane 64] x 16 bytes, then A2 = [channel tile
// CT][plane 2][lane 64] x 16 bytes.  Exact: per buffer k [C][33] and v [C][33] floats.  Behind the two buffers: the
// per-wave magnitudes of the tile in flight, [parity 2][wave 4][k | v].
template <int CT, bool EX>
struct FusedLds {
  static constexpr int C = 16 * CT, KB = (CT + 1) / 2;
  static constexpr int kA2 = 4 * KB * 64 * 16;                                       // offset of A2 inside a buffer
  static constexpr int kBuf = EX ? 2 * C * 33 * 4 : kA2 + 2 * CT * 64 * 16;
  static constexpr int kSlots = 2 * kBuf;
  static constexpr int kBytes = kSlots + 2 * 4 * 2 * 4;
};
static_assert(FusedLds<8, false>::kBytes * 2 <= 160 * 1024 && FusedLds<8, true>::kBytes * 2 <= 160 * 1024, "two workgroups per CU");

template <int CT, bool EX>
__global__ __launch_bounds__(256) void attn_fused_kernel(const float *__restrict__ q, const float *k, const float *v, int n,
                                                         float *__restrict__ out) {
  extern __shared__ float lds[];
  using LY = FusedLds<CT, EX>;
  constexpr int C = LY::C, KB = LY::KB, NT = kFusedNT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  const size_t cloud = (size_t)blockIdx.y * C * n;
  q += cloud;
  k += cloud;
  v += cloud;
  out += cloud;
  const int T = n / kFusedKeys;
  const int q0 = blockIdx.x * kFusedQ + wave * 16 * NT;
  const bool active = q0 < n;          // whole waves: a wave past the last query only stages
  char *base = (char *)lds;
  float *slots = (float *)(base + LY::kSlots);

  // ---- staging: a thread owns a PAIR of channels (2 cp, 2 cp + 1) x the 8 keys {4 sg .. + 3, 16 + 4 sg .. + 3} of a tile
  const int cp = tid >> 2, sg = tid & 3;
  const bool item = cp < C / 2;
  const bool same = k == v;
  f32x4 kr[2][2], vr[2][2];            // [channel of the pair][key chunk]
#pragma unroll
  for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
    for (int h = 0; h < 2; ++h) kr[c2][h] = vr[c2][h] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto load_tile = [&](int t) {
    if (!item) return;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const size_t o = (size_t)(2 * cp + c2) * n + kFusedKeys * t + 16 * h + 4 * sg;
        kr[c2][h] = *(const f32x4 *)(k + o);
        vr[c2][h] = same ? kr[c2][h] : *(const f32x4 *)(v + o);
      }
  };
  auto publish = [&](int par) {        // this wave's largest |k| and |v| of the tile in its registers
    if constexpr (!EX) {
      float mk = 0.f, mv = 0.f;
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            mk = fmaxf(mk, fabsf(kr[c2][h][e]));
            mv = fmaxf(mv, fabsf(vr[c2][h][e]));
          }
      mk = wave_max(mk);
      mv = wave_max(mv);
      if (lane == 0) {
        slots[(par * 4 + wave) * 2] = mk;
        slots[(par * 4 + wave) * 2 + 1] = mv;
      }
    }
  };
  auto read_scale = [&](int par, float &sk, float &sv) {
    sk = sv = 1.0f;
    if constexpr (!EX) {
      float mk = 0.f, mv = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        mk = fmaxf(mk, slots[(par * 4 + w) * 2]);
        mv = fmaxf(mv, slots[(par * 4 + w) * 2 + 1]);
      }
      sk = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(range_pow2(mk))));
      sv = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(range_pow2(mv))));
    }
  };
  auto stage = [&](int buf, float sk, float sv) {
    if (!item) return;
    if constexpr (EX) {
      float *kt = (float *)(base + buf * LY::kBuf), *vt = kt + C * 33;
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            kt[(2 * cp + c2) * 33 + 16 * h + 4 * sg + e] = kr[c2][h][e];
            vt[(2 * cp + c2) * 33 + 16 * h + 4 * sg + e] = vr[c2][h][e];
          }
    } else {
      unsigned *a1 = (unsigned *)(base + buf * LY::kBuf);
      u32x4 *a2 = (u32x4 *)(base + buf * LY::kBuf + LY::kA2);
      const float ik = pow2_inv(sk), iv = pow2_inv(sv);
      // A1: the pair's two channels of one key are one dword (f16 x 2) of the fragment of lane (g' = channel octet, key)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned hi, lo;
          split_f16x2(kr[0][h][e] * ik, kr[1][h][e] * ik, hi, lo);
          const int d = ((h * KB + (cp >> 4)) * 2) * 256 + (((cp >> 2) & 3) * 16 + 4 * sg + e) * 4 + (cp & 3);
          a1[d] = hi;
          a1[d + 256] = lo;
        }
      // A2: a channel's 8 keys are the whole fragment entry of lane (g = sg, channel)
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const float x8[8] = {vr[c2][0][0] * iv, vr[c2][0][1] * iv, vr[c2][0][2] * iv, vr[c2][0][3] * iv,
                             vr[c2][1][0] * iv, vr[c2][1][1] * iv, vr[c2][1][2] * iv, vr[c2][1][3] * iv};
        u32x4 pl[kSplit];
        split_planes8(x8, pl);
        const int ch = 2 * cp + c2, idx = ((ch >> 4) * 2) * 64 + sg * 16 + (ch & 15);
        a2[idx] = pl[0];
        a2[idx + 64] = pl[1];
      }
    }
  };

  // ---- prologue: tile 0 staged, tile 1 in registers, q in registers
  if constexpr (!EX) {   // K padding of an odd channel-tile count (C = 48, 80, 112) stays zero: nobody writes it
    for (int i = tid; i < 2 * LY::kBuf / 16; i += 256) ((u32x4 *)base)[i] = u32x4{0u, 0u, 0u, 0u};
  }
  load_tile(0);
  publish(0);
  __syncthreads();
  float sk_c, sv_c;
  read_scale(0, sk_c, sv_c);
  stage(0, sk_c, sv_c);
  if (T > 1) {
    load_tile(1);
    publish(1);
  }

  u32x4 qf[NT][KB][kSplit];   // split: B fragments of q (K = channels, column = query)
  float qx[NT][C / 4];        // exact: B values of q, step j = channel 4 j + g
  float sq[NT];
  if (active) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float *qp = q + q0 + 16 * nt + col;
      sq[nt] = 1.0f;
      if constexpr (EX) {
#pragma unroll
        for (int j = 0; j < C / 4; ++j) qx[nt][j] = qp[(size_t)(4 * j + g) * n];
      } else {
        float val[KB][8], m = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const int ch = 32 * kb + 8 * g + t;
            val[kb][t] = ch < C ? qp[(size_t)ch * n] : 0.f;
            m = fmaxf(m, fabsf(val[kb][t]));
          }
        const float s = range_pow2(wave_max(m)), inv = pow2_inv(s);
        sq[nt] = s;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
          for (int t = 0; t < 8; ++t) val[kb][t] *= inv;
          split_planes8(val[kb], qf[nt][kb]);
        }
      }
    }
  }

  float mrun[NT], lrun[NT];
  f32x4 acc[CT][NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    mrun[nt] = -__builtin_inff();
    lrun[nt] = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  auto compute = [&](int buf, float sk, float sv) {
    f32x4 sc[2][NT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) sc[s][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ---- scores, transposed: rows = the tile's keys, columns = this wave's queries
    if constexpr (EX) {
      const float *kt = (const float *)(base + buf * LY::kBuf);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < C / 4; ++j) {
          const float a = kt[(4 * j + g) * 33 + 16 * s + col];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) sc[s][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, qx[nt][j], sc[s][nt], 0, 0, 0);
        }
    } else {
      const u32x4 *a1 = (const u32x4 *)(base + buf * LY::kBuf) + lane;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
          const u32x4 a[kSplit] = {a1[((s * KB + kb) * 2) * 64], a1[((s * KB + kb) * 2 + 1) * 64]};
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) sc[s][nt] = mfma_split(a, qf[nt][kb], sc[s][nt]);
        }
    }
    // ---- online softmax over the tile's 32 keys; P stays in the lanes that hold the scores
    u32x4 pb[NT][kSplit];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float tm = -__builtin_inff();
      const float f = sq[nt] * sk;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (!EX) sc[s][nt][r] *= f;
          tm = fmaxf(tm, sc[s][nt][r]);
        }
      tm = half_max(row_pair_max(tm));   // the query's four lanes (keys 4 g + r of both key tiles)
      const float mn = fmaxf(mrun[nt], tm);
      const float alpha = __builtin_amdgcn_exp2f((mrun[nt] - mn) * kLog2e);   // first tile: exp(-inf) = 0
      mrun[nt] = mn;
      float ps = 0.f, p8[8];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f((sc[s][nt][r] - mn) * kLog2e);
          ps += p;
          p8[4 * s + r] = p * kFPScale;
          sc[s][nt][r] = p;
        }
      lrun[nt] = __builtin_fmaf(lrun[nt], alpha, ps);   // this lane's keys; the four lanes are added once, at the end
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct][nt] *= alpha;
      if constexpr (!EX) split_planes8(p8, pb[nt]);
    }
    // ---- apply: rows = channels, columns = queries, K = the tile's keys
    if constexpr (EX) {
      const float *vt = (const float *)(base + buf * LY::kBuf) + C * 33;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            const float a = vt[(16 * ct + col) * 33 + 16 * s + 4 * g + r];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[ct][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sc[s][nt][r], acc[ct][nt], 0, 0, 0);
          }
    } else {
      const u32x4 *a2 = (const u32x4 *)(base + buf * LY::kBuf + LY::kA2) + lane;
      if (sv == 1.0f) {   // wave uniform; the ordinary case accumulates in place
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const u32x4 a[kSplit] = {a2[(ct * 2) * 64], a2[(ct * 2 + 1) * 64]};
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[ct][nt] = mfma_split(a, pb[nt], acc[ct][nt]);
        }
      } else {            // the tile's v scale goes back on the tile's own product
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const u32x4 a[kSplit] = {a2[(ct * 2) * 64], a2[(ct * 2 + 1) * 64]};
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const f32x4 t = mfma_split(a, pb[nt], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ct][nt][r] = __builtin_fmaf(t[r], sv, acc[ct][nt][r]);
          }
        }
      }
    }
  };

  // ---- key tiles: tile t is computed from buffer t & 1 while tile t + 1 is written to the other and tile t + 2 is in flight
  for (int t = 0; t < T; ++t) {
    __syncthreads();   // tile t staged, the magnitudes of tile t + 1 published, buffer (t + 1) & 1 free
    float sk_n = 1.0f, sv_n = 1.0f;
    if (t + 1 < T) {
      read_scale((t + 1) & 1, sk_n, sv_n);
      stage((t + 1) & 1, sk_n, sv_n);
    }
    if (t + 2 < T) load_tile(t + 2);
    if (active) compute(t & 1, sk_c, sv_c);
    if (t + 2 < T) publish(t & 1);   // slot parity t was last read in front of this trip's barrier
    sk_c = sk_n;
    sv_c = sv_n;
  }

  if (active) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float l = half_sum(row_pair_sum(lrun[nt]));
      const float inv = (EX ? 1.0f : kFPScaleInv) / l;   // the row's one division
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(16 * ct + 4 * g + r) * n + q0 + 16 * nt + col] = acc[ct][nt][r] * inv;
    }
  }
}

template <int CT, bool EX>
int launch_fused(const float *q, const float *k, const float *v, int b, int c, int n, float *out, hipStream_t st) {
  if constexpr (CT > 8) {
    return GLDM_ERR_UNSUPPORTED;
  } else {
    if (c != 16 * CT) return launch_fused<CT + 1, EX>(q, k, v, b, c, n, out, st);
    constexpr int bytes = FusedLds<CT, EX>::kBytes;
    gldm_dev::launch_dynamic_lds<attn_fused_kernel<CT, EX>>(dim3((n + kFusedQ - 1) / kFusedQ, b), dim3(256), bytes, bytes, st, q, k,
                                                            v, n, out);
    return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
  }
}

}  // namespace

GLDM_API int gldm_point_attention_fused(const float *q, const float *k, const float *v, int b, int c, int n, int exact_f32,
                                        float *out, gldm_stream_t stream) {
  if (!q || !k || !v || !out || b <= 0 || c <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (!fused_shape_ok(c, n) || b > 65535) return GLDM_ERR_UNSUPPORTED;
  if ((((size_t)q | (size_t)k | (size_t)v | (size_t)out) & 15)) return GLDM_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return exact_f32 ? launch_fused<2, true>(q, k, v, b, c, n, out, st) : launch_fused<2, false>(q, k, v, b, c, n, out, st);
}
