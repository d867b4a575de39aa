// point_attention.hip -- dense softmax attention of every point over every point (the PVD Attention block of
// grasp_ldm/models/modules/modules.py:10-54, without its k = 1 convs; the GroupNorm + Swish behind it is voxel_norm.hip's
// gldm_groupnorm_swish_points, the few-row out_layer conv pointwise_small.hip's gldm_pointwise_rows).
//
//   out[b, c, i] = sum_j v[b, c, j] softmax_j( sum_c' q[b, c', i] k[b, c', j] )          (no 1 / sqrt(c) factor)
//
// Both products multiply ACTIVATIONS by activations, so neither operand arrives pre-packed as the weights of every other
// GEMM here do.  Structure, per chunk of clouds (the scores live in the caller's workspace, at most 256 MiB of it):
//   pack     q, k (K = channel, the slow axis) and v (K = point, the fast axis) are re-laid ONCE as MFMA fragments: a
//            16-row group of the operand x a 32-deep K block = [plane hi|lo][lane 64][8 f16], the fragment of
//            v_mfma_f32_16x16x32_f16 (the layout the weight fragments have).  Each 16-row group is split as x / s with s a
//            power of two from the group's largest magnitude over ALL of K (range_pow2: 1 for anything ordinary), so the
//            scale is constant along a product's K loop and is folded back once, on the accumulators.
//   scores   S = q^T k, a batched GEMM whose waves read both operands as whole fragments (16-byte loads, L2 -> VGPR, as
//            wstream.h reads weights): no LDS, no barrier, 64 x 64 outputs per wave, 128 x 128 per workgroup.
//   softmax  one wave per row: maximum, sum of exp(s - max) in a fixed order, ONE reciprocal, and P written straight as
//            the B fragments of the next product, multiplied by 2^14 in front of the split (a flat row of 1024 keys is all
//            2^-10: scaled, its lo piece is a normal f16); 2^-14 goes back on the accumulators.
//   apply    out = v P^T, the same GEMM kernel (A = v fragments, B = P fragments).
// exact_f32: the same four stages with f32 fragments ([lane 64][4 f32] per 16-deep K block) on v_mfma_f32_16x16x4_f32, no
// scales.  Fixed summation order everywhere, no atomics, nothing waits on another workgroup; a cloud's result does not
// depend on its position in the batch, on b or on the chunking.
#include "mfma_prims.h"

namespace {

constexpr long long kAttnWsCap = 256ll << 20;   // scores + fragments of one chunk of clouds
constexpr float kPScale = 16384.f, kPScaleInv = 1.f / 16384.f;
constexpr int kAttnMT = 4, kAttnNT = 4;          // 16 x 16 tiles per wave; a workgroup is 2 x 2 waves
constexpr int kAttnFoldKb = 8;                   // exact_f32: 16-deep K blocks per partial sum (an even number: two per trip)

inline bool attn_shape_ok(int c, int n) { return c % 16 == 0 && c >= 16 && c <= 1024 && n % 32 == 0 && n >= 32 && n <= 4096; }

// One cloud's block of the workspace (bytes; every part a multiple of 256)
struct AttnWs {
  long long qf, kf, vf, s, pf, sq, sk, sv, total;
};
inline AttnWs attn_ws(int c, int n) {
  const long long kc = (c + 31) / 32 * 32;   // K of the scores product, zero-padded to the f16 MFMA depth
  auto up = [](long long x) { return (x + 255) / 256 * 256; };
  AttnWs w;
  long long o = 0;
  w.qf = o; o += up(4ll * n * kc);
  w.kf = o; o += up(4ll * n * kc);
  w.vf = o; o += up(4ll * c * n);
  w.s = o;  o += up(4ll * n * n);
  w.pf = o; o += up(4ll * n * n);
  w.sq = o; o += up(4ll * (n / 16));
  w.sk = o; o += up(4ll * (n / 16));
  w.sv = o; o += up(4ll * (c / 16));
  w.total = o;
  return w;
}
inline int attn_chunk(int b, int c, int n) {
  const long long fit = kAttnWsCap / attn_ws(c, n).total;
  return (int)(fit < 1 ? 1 : (fit < b ? fit : b));
}

// ---- pack: K on the SLOW axis (q and k of the scores product: x [c][n], a group = 16 points, K = channels) -------------
// One wave per group; lane = (g = K octet, r = point).  frag [groups][kblocks][EX ? 64 : 2 x 64] x 16 bytes.
template <bool EX>
__global__ __launch_bounds__(256) void attn_pack_kslow_kernel(const float *__restrict__ x, int c, int n, int kblocks,
                                                              u32x4 *__restrict__ frag, float *__restrict__ scale,
                                                              long long ws_cloud_bytes) {
  const int grp = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
  if (grp >= n / 16) return;
  const float *p = x + (size_t)blockIdx.y * c * n + 16 * grp + r;
  frag = (u32x4 *)((char *)frag + blockIdx.y * ws_cloud_bytes) + (size_t)grp * kblocks * (EX ? 64 : 128) + lane;
  if constexpr (EX) {
    for (int kb = 0; kb < kblocks; ++kb) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = p[(size_t)(16 * kb + 4 * j + g) * n];
      frag[(size_t)kb * 64] = __builtin_bit_cast(u32x4, v);
    }
  } else {
    float m = 0.f;
#pragma unroll 8   // one 4-byte load per trip: without several in flight the pass is one round trip per channel quad
    for (int ch = g; ch < c; ch += 4) m = fmaxf(m, fabsf(p[(size_t)ch * n]));
    const float s = range_pow2(wave_max(m)), inv = pow2_inv(s);
    if (lane == 0) ((float *)((char *)scale + blockIdx.y * ws_cloud_bytes))[grp] = s;
    for (int kb = 0; kb < kblocks; ++kb) {
      float v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int ch = 32 * kb + 8 * g + t;
        v[t] = ch < c ? p[(size_t)ch * n] * inv : 0.f;   // K zero-padded to the MFMA depth
      }
      u32x4 pl[kSplit];
      split_planes8(v, pl);
      frag[(size_t)kb * 128] = pl[0];
      frag[(size_t)kb * 128 + 64] = pl[1];
    }
  }
}

// ---- pack: K on the FAST axis (v of the apply product: x [c][n], a group = 16 channels, K = points) ---------------------
template <bool EX>
__global__ __launch_bounds__(256) void attn_pack_kfast_kernel(const float *__restrict__ x, int c, int n, int kblocks,
                                                              u32x4 *__restrict__ frag, float *__restrict__ scale,
                                                              long long ws_cloud_bytes) {
  const int grp = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
  if (grp >= c / 16) return;
  const float *p = x + (size_t)blockIdx.y * c * n + (size_t)(16 * grp + r) * n;
  frag = (u32x4 *)((char *)frag + blockIdx.y * ws_cloud_bytes) + (size_t)grp * kblocks * (EX ? 64 : 128) + lane;
  if constexpr (EX) {
    for (int kb = 0; kb < kblocks; ++kb) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = p[16 * kb + 4 * j + g];
      frag[(size_t)kb * 64] = __builtin_bit_cast(u32x4, v);
    }
  } else {
    float m = 0.f;
    for (int j4 = g; j4 < n / 4; j4 += 4) {
      const f32x4 v = *(const f32x4 *)(p + 4 * j4);
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    const float s = range_pow2(wave_max(m)), inv = pow2_inv(s);
    if (lane == 0) ((float *)((char *)scale + blockIdx.y * ws_cloud_bytes))[grp] = s;
    for (int kb = 0; kb < kblocks; ++kb) {
      const f32x4 lo4 = *(const f32x4 *)(p + 32 * kb + 8 * g), hi4 = *(const f32x4 *)(p + 32 * kb + 8 * g + 4);
      const float v[8] = {lo4[0] * inv, lo4[1] * inv, lo4[2] * inv, lo4[3] * inv, hi4[0] * inv, hi4[1] * inv, hi4[2] * inv, hi4[3] * inv};
      u32x4 pl[kSplit];
      split_planes8(v, pl);
      frag[(size_t)kb * 128] = pl[0];
      frag[(size_t)kb * 128 + 64] = pl[1];
    }
  }
}

// ---- the batched GEMM of both products: out[cloud][16 mg + .][16 ng + .] = (sum over K blocks of A B) sa[mg] sb[ng] sconst
// A [MG][kblocks] and B [NG][kblocks] fragments of one cloud's workspace block.  A wave owns kAttnMT x kAttnNT tiles and
// reads every fragment it multiplies as one 16-byte load per lane and plane, the next K block's while this one's MFMAs
// issue.  Edge tiles: the group index is clamped for the loads and the tile is not stored.
// APPLY: the second product (no B scales; a kernel of its own name in a profile).
template <bool EX, bool APPLY>
__global__ __launch_bounds__(256) void attn_gemm_kernel(const u32x4 *__restrict__ A, const u32x4 *__restrict__ B, int MG, int NG,
                                                        int kblocks, const float *__restrict__ sa, const float *__restrict__ sb,
                                                        float sconst, long long ws_cloud_bytes, float *__restrict__ out,
                                                        long long out_cloud_floats, int ld) {
  constexpr int MT = kAttnMT, NT = kAttnNT, PL = EX ? 1 : kSplit, FU4 = 64 * PL;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mg0 = (blockIdx.y * 2 + (wave >> 1)) * MT, ng0 = (blockIdx.x * 2 + (wave & 1)) * NT;
  if (mg0 >= MG || ng0 >= NG) return;   // whole waves; the kernel has no barrier
  const long long cb = blockIdx.z * ws_cloud_bytes;
  const u32x4 *ap[MT], *bp[NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
    ap[mi] = (const u32x4 *)((const char *)A + cb) + (size_t)min(mg0 + mi, MG - 1) * kblocks * FU4 + lane;
#pragma unroll
  for (int ni = 0; ni < NT; ++ni)
    bp[ni] = (const u32x4 *)((const char *)B + cb) + (size_t)min(ng0 + ni, NG - 1) * kblocks * FU4 + lane;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 a[2][MT][PL], b[2][NT][PL];
  auto load = [&](int buf, int kb) {
#pragma unroll
    for (int pl = 0; pl < PL; ++pl) {
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) a[buf][mi][pl] = ap[mi][(size_t)kb * FU4 + 64 * pl];
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) b[buf][ni][pl] = bp[ni][(size_t)kb * FU4 + 64 * pl];
    }
  };
  auto mul = [&](int buf) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        if constexpr (EX) {
          const f32x4 af = __builtin_bit_cast(f32x4, a[buf][mi][0]), bf = __builtin_bit_cast(f32x4, b[buf][ni][0]);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], bf[j], acc[mi][ni], 0, 0, 0);
        } else {
          acc[mi][ni] = mfma_split(a[buf][mi], b[buf][ni], acc[mi][ni]);
        }
      }
  };
  // EX: the accumulators are folded into a total every kAttnFoldKb K blocks.  One f32 chain over K = 1024 channels is 256
  // dependent roundings at the magnitude of the finished logit (sigma 32 for unit-normal data): 1.9e-4 on the output at
  // c = 1024, more than four times what a blocked f32 GEMM leaves.  Folded, a chain is 32 steps and c / 128 totals.
  [[maybe_unused]] f32x4 total[EX ? MT : 1][EX ? NT : 1];
  if constexpr (EX) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) total[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto fold = [&]() {
    if constexpr (EX) {
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          total[mi][ni] += acc[mi][ni];
          acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
  };
  // two K blocks per trip, the loads unconditional (index clamped: a branch around a load is waited for at the join)
  const int last = kblocks - 1;
  load(0, 0);
  for (int kb = 0; kb < kblocks; kb += 2) {
    if (EX && kb && kb % kAttnFoldKb == 0) fold();
    load(1, min(kb + 1, last));
    mul(0);
    load(0, min(kb + 2, last));
    if (kb + 1 < kblocks) mul(1);
  }
  if constexpr (EX) {
    fold();
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = total[mi][ni];
  }
  const int g = lane >> 4, col = lane & 15;
  out += blockIdx.z * out_cloud_floats;
  const float *sap = sa ? (const float *)((const char *)sa + cb) : nullptr;
  const float *sbp = !APPLY && sb ? (const float *)((const char *)sb + cb) : nullptr;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    if (mg0 + mi >= MG) break;
    const float fa = sap ? sap[mg0 + mi] : 1.f;
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      if (ng0 + ni >= NG) break;
      const float fb = sbp ? sbp[ng0 + ni] : 1.f;
      float *o = out + (size_t)(16 * (mg0 + mi) + 4 * g) * ld + 16 * (ng0 + ni) + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(size_t)r * ld] = acc[mi][ni][r] * fa * fb * sconst;
    }
  }
}

// ---- row softmax: S [n][n] f32 -> P as the B fragments of the apply product (group = 16 queries, K = keys) ---------------
// A workgroup per 16-query group, a wave per four rows.  A row is read three times (maximum, sum, write): 4 KiB at 1024
// keys, out of the cache after the first.
template <bool EX>
__global__ __launch_bounds__(256) void attn_softmax_kernel(const float *__restrict__ S, int n, u32x4 *__restrict__ P,
                                                           long long ws_cloud_bytes) {
  const int grp = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kblocks = n / (EX ? 16 : 32);
  S = (const float *)((const char *)S + blockIdx.y * ws_cloud_bytes);
  P = (u32x4 *)((char *)P + blockIdx.y * ws_cloud_bytes) + (size_t)grp * kblocks * (EX ? 64 : 128);
  for (int rr = 0; rr < 4; ++rr) {
    const int r = 4 * wave + rr;
    const float *row = S + (size_t)(16 * grp + r) * n;
    float m = -__builtin_inff();
    for (int j4 = lane; j4 < n / 4; j4 += 64) {
      const f32x4 v = *(const f32x4 *)(row + 4 * j4);
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int j4 = lane; j4 < n / 4; j4 += 64) {
      const f32x4 v = *(const f32x4 *)(row + 4 * j4);
      sum += expf(v[0] - m);
      sum += expf(v[1] - m);
      sum += expf(v[2] - m);
      sum += expf(v[3] - m);
    }
    const float inv = 1.0f / wave_sum(sum);
    if constexpr (EX) {
      float *pf = (float *)P;
      for (int j = lane; j < n; j += 64)   // k = j % 16 = 4 (MFMA step) + (lane group)
        pf[((size_t)(j >> 4) * 64 + (j & 3) * 16 + r) * 4 + ((j >> 2) & 3)] = expf(row[j] - m) * inv;
    } else {
      const float f = inv * kPScale;
      for (int t = lane; t < n / 8; t += 64) {
        const f32x4 lo4 = *(const f32x4 *)(row + 8 * t), hi4 = *(const f32x4 *)(row + 8 * t + 4);
        const float v[8] = {expf(lo4[0] - m) * f, expf(lo4[1] - m) * f, expf(lo4[2] - m) * f, expf(lo4[3] - m) * f,
                            expf(hi4[0] - m) * f, expf(hi4[1] - m) * f, expf(hi4[2] - m) * f, expf(hi4[3] - m) * f};
        u32x4 pl[kSplit];
        split_planes8(v, pl);
        u32x4 *d = P + (size_t)(t >> 2) * 128 + (t & 3) * 16 + r;
        d[0] = pl[0];
        d[64] = pl[1];
      }
    }
  }
}

template <bool EX>
int launch_attention(const float *q, const float *k, const float *v, int b, int c, int n, char *ws, float *out, hipStream_t st) {
  const AttnWs w = attn_ws(c, n);
  const int chunk = attn_chunk(b, c, n);
  const int kb_c = EX ? c / 16 : (c + 31) / 32, kb_n = EX ? n / 16 : n / 32, ng = n / 16, cgp = c / 16;
  const dim3 blk(256);
  for (int b0 = 0; b0 < b; b0 += chunk) {
    const int nb = b - b0 < chunk ? b - b0 : chunk;
    const size_t off = (size_t)b0 * c * n;
    hipLaunchKernelGGL(attn_pack_kslow_kernel<EX>, dim3((ng + 3) / 4, nb), blk, 0, st, q + off, c, n, kb_c, (u32x4 *)(ws + w.qf),
                       (float *)(ws + w.sq), w.total);
    hipLaunchKernelGGL(attn_pack_kslow_kernel<EX>, dim3((ng + 3) / 4, nb), blk, 0, st, k + off, c, n, kb_c, (u32x4 *)(ws + w.kf),
                       (float *)(ws + w.sk), w.total);
    hipLaunchKernelGGL(attn_pack_kfast_kernel<EX>, dim3((cgp + 3) / 4, nb), blk, 0, st, v + off, c, n, kb_n, (u32x4 *)(ws + w.vf),
                       (float *)(ws + w.sv), w.total);
    if (hipGetLastError() != hipSuccess) return GLDM_ERR_LAUNCH;
    const int tn = (ng + 2 * kAttnNT - 1) / (2 * kAttnNT);
    // scores: rows = queries, columns = keys, K = channels
    hipLaunchKernelGGL((attn_gemm_kernel<EX, false>), dim3(tn, (ng + 2 * kAttnMT - 1) / (2 * kAttnMT), nb), blk, 0, st,
                       (const u32x4 *)(ws + w.qf), (const u32x4 *)(ws + w.kf), ng, ng, kb_c,
                       EX ? nullptr : (const float *)(ws + w.sq), EX ? nullptr : (const float *)(ws + w.sk), 1.0f, w.total,
                       (float *)(ws + w.s), w.total / 4, n);
    hipLaunchKernelGGL(attn_softmax_kernel<EX>, dim3(ng, nb), blk, 0, st, (const float *)(ws + w.s), n, (u32x4 *)(ws + w.pf),
                       w.total);
    // apply: rows = channels, columns = queries, K = keys
    hipLaunchKernelGGL((attn_gemm_kernel<EX, true>), dim3(tn, (cgp + 2 * kAttnMT - 1) / (2 * kAttnMT), nb), blk, 0, st,
                       (const u32x4 *)(ws + w.vf), (const u32x4 *)(ws + w.pf), cgp, ng, kb_n,
                       EX ? nullptr : (const float *)(ws + w.sv), nullptr, EX ? 1.0f : kPScaleInv, w.total, out + off,
                       (long long)c * n, n);
    if (hipGetLastError() != hipSuccess) return GLDM_ERR_LAUNCH;
  }
  return GLDM_OK;
}

}  // namespace

GLDM_API long long gldm_point_attention_workspace_bytes(int b, int c, int n) {
  if (b <= 0 || !attn_shape_ok(c, n)) return -1;
  return attn_ws(c, n).total * attn_chunk(b, c, n);
}

GLDM_API int gldm_point_attention(const float *q, const float *k, const float *v, int b, int c, int n, int exact_f32,
                                  void *workspace, long long workspace_bytes, float *out, gldm_stream_t stream) {
  if (!q || !k || !v || !out || b <= 0 || c <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (!attn_shape_ok(c, n)) return GLDM_ERR_UNSUPPORTED;
  if (!workspace || (((size_t)workspace | (size_t)q | (size_t)k | (size_t)v | (size_t)out) & 15) || workspace_bytes < gldm_point_attention_workspace_bytes(b, c, n))
    return GLDM_ERR_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return exact_f32 ? launch_attention<true>(q, k, v, b, c, n, (char *)workspace, out, st)
                   : launch_attention<false>(q, k, v, b, c, n, (char *)workspace, out, st);
}
