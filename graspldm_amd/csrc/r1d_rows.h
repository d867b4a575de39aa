// r1d_rows.h -- the f32 / generic phases of the 32-column engines r1d_kernel<32, *> (sample-major columns; their convs are
// tile_gemm.h's 1x1 layers and r1d_gemm.h's conv3_f32): LayerNorm over the channels, LinearAttention of one head pair, and
// the 4-channel ResnetBlock on the VALU of one wave.  Included by resnet1d.hip inside its anonymous namespace, behind
// r1d_gemm.h (R1dGeo, R1dCtx) and r1d_tape.h (kOpInts).

// ----------------------------------------------------------- LayerNorm ----
// dst = LN_channels(src) * g  (or res += LN(src) * g when res != null).  Row slot = wave*kRP + sub
// (kSlots = kWaves * kRP of them), rows slot + kSlots i.
template <int NC, int ITERS>
__device__ __forceinline__ void layer_norm_rows(const R1dCtx &c, const float *src, float *dst, float *res, int C,
                                                int g_off) {
  using GG = R1dGeo<NC>;
  float *red1 = c.lds + GG::kMiscRed1, *red2 = c.lds + GG::kMiscRed2;
  const int n = c.lane & (NC - 1), slot = c.wave * GG::kRP + c.lane / NC;
  const lds_f *s3 = (const lds_f *)src;
  const float *g = c.w + g_off;
  float v[ITERS], gv[ITERS];  // the gains are requested up front: their L2 round trip hides behind the statistics
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float x = s3[swz<NC>(row < C ? row : 0, n)];
    gv[i] = g[row < C ? row : 0];
    v[i] = row < C ? x : 0.f;
    sum += v[i];
  }
  if (GG::kRP == 2) sum = half_sum(sum);
  red1[c.wave * NC + n] = sum;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) tot += red1[q * NC + n];
  const float mean = tot / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float d = row < C ? v[i] - mean : 0.f;
    sq += d * d;
  }
  if (GG::kRP == 2) sq = half_sum(sq);
  red2[c.wave * NC + n] = sq;
  __syncthreads();
  float vt = 0.f;
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) vt += red2[q * NC + n];
  const float rstd = __builtin_amdgcn_rsqf(vt / (float)C + 1e-5f);
  lds_f *d3 = (lds_f *)dst, *r3 = (lds_f *)res;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    if (row < C) {
      const float y = (v[i] - mean) * rstd * gv[i];
      const int a = swz<NC>(row, n);
      if (res) r3[a] = r3[a] + y;
      else d3[a] = y;
    }
  }
  __syncthreads();
}

// One-exchange form for the 64-column engine (lane = column, wave = row slot): every wave reduces its rows to
// (sum, M2 about its own mean), ONE barrier, then the parallel-variance merge of the 8 pairs: two barriers per
// LayerNorm instead of three.
template <int ITERS>
__device__ __forceinline__ void layer_norm_rows_1x(const R1dCtx &c, const float *src, float *dst, float *res, int C,
                                                   int g_off) {
  constexpr int NC = 64;
  using GG = R1dGeo<NC>;
  lds_f *red1 = (lds_f *)(c.lds + GG::kMiscRed1), *red2 = (lds_f *)(c.lds + GG::kMiscRed2);
  const int n = c.lane, slot = c.wave;
  const lds_f *s3 = (const lds_f *)src;
  const float *g = c.w + g_off;
  float v[ITERS], gv[ITERS];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float x = s3[swz<NC>(row < C ? row : 0, n)];
    gv[i] = g[row < C ? row : 0];
    v[i] = row < C ? x : 0.f;
    sum += v[i];
  }
  const int cnt = slot < C ? (C - slot + GG::kSlots - 1) / GG::kSlots : 0;  // rows of this slot (wave uniform)
  const float mloc = sum * __builtin_amdgcn_rcpf((float)(cnt > 0 ? cnt : 1));  // C, cnt: powers of two -> exact
  float m2 = 0.f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    const float d = row < C ? v[i] - mloc : 0.f;
    m2 += d * d;
  }
  red1[slot * NC + n] = sum;
  red2[slot * NC + n] = m2;
  __syncthreads();
  float tot = 0.f, ps[GG::kWaves], pm[GG::kWaves];
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) {
    ps[q] = red1[q * NC + n];
    pm[q] = red2[q * NC + n];
    tot += ps[q];
  }
  const float inv_c = __builtin_amdgcn_rcpf((float)C);
  const float mean = tot * inv_c;
  float vt = 0.f;
#pragma unroll
  for (int q = 0; q < GG::kWaves; ++q) {
    const int cq = q < C ? (C - q + GG::kSlots - 1) / GG::kSlots : 0;  // wave uniform
    const float fq = (float)cq, iq = __builtin_amdgcn_rcpf((float)(cq > 0 ? cq : 1));
    const float dm = ps[q] * iq - mean;
    vt += cq > 0 ? pm[q] + fq * dm * dm : 0.f;
  }
  const float rstd = __builtin_amdgcn_rsqf(vt * inv_c + 1e-5f);
  lds_f *d3 = (lds_f *)dst, *r3 = (lds_f *)res;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int row = slot + GG::kSlots * i;
    if (row < C) {
      const float y = (v[i] - mean) * rstd * gv[i];
      const int a = swz<NC>(row, n);
      if (res) r3[a] = r3[a] + y;
      else d3[a] = y;
    }
  }
  __syncthreads();
}

template <int NC>
__device__ __forceinline__ void layer_norm_pass(const R1dCtx &c, const float *src, float *dst, float *res, int C, int g_off) {
  if (GLDM_SKIP(c, 2)) return;
  C = __builtin_amdgcn_readfirstlane(C);
  if constexpr (NC == 64) {
    const int it1 = (C + R1dGeo<NC>::kSlots - 1) / R1dGeo<NC>::kSlots;
    if (it1 <= 1) layer_norm_rows_1x<1>(c, src, dst, res, C, g_off);
    else if (it1 <= 4) layer_norm_rows_1x<4>(c, src, dst, res, C, g_off);
    else if (it1 <= 8) layer_norm_rows_1x<8>(c, src, dst, res, C, g_off);
    else layer_norm_rows_1x<16>(c, src, dst, res, C, g_off);
    return;
  }
  const int it = (C + R1dGeo<NC>::kSlots - 1) / R1dGeo<NC>::kSlots;
  if (it <= 1) layer_norm_rows<NC, 1>(c, src, dst, res, C, g_off);
  else if (it <= 2) layer_norm_rows<NC, 2>(c, src, dst, res, C, g_off);
  else if (it <= 4) layer_norm_rows<NC, 4>(c, src, dst, res, C, g_off);
  else if (it <= 8) layer_norm_rows<NC, 8>(c, src, dst, res, C, g_off);
  else layer_norm_rows<NC, 16>(c, src, dst, res, C, g_off);
}

// -------------------------------------------------- linear attention -------
// qkv: [192][NC] = q(2 heads x 32) | k | v for one head pair; writes 64 rows of o.
// (Sample-major 32-column engine; the 64-column engine has attention_pair_pm.)
template <int NC, int L>
__device__ __forceinline__ void attention_pair(const R1dCtx &c, float *qkv, float *o_rows) {
  if (GLDM_SKIP(c, 4)) return;
  using GG = R1dGeo<NC>;
  static_assert(NC == 32 && GG::kWaves == 4 && (L == 4 || L == 16), "sample-major engine geometry");
  const lds_f *q3 = (const lds_f *)qkv;
  lds_f *o3 = (lds_f *)o_rows;
  if constexpr (L == 4 && NC == 32 && GG::kWaves == 4) {
    // wave = (head of the pair, 16-column half); lane = (column, part): 8 of the head's 32 channels.  The softmax
    // statistics and the 4 x 4 matrix A = softmax_n(k)^T softmax_d(q) combine over the parts with permlane swaps
    // inside the wave: no LDS exchange and no barrier but the final one.
    const int h2 = c.wave >> 1, nn = 16 * (c.wave & 1) + (c.lane & 15), pt = c.lane >> 4, d0 = 8 * pt, sb = nn & ~3;
    const int qr = h2 * kDimHead + d0, kr = 64 + h2 * kDimHead + d0, vr = 128 + h2 * kDimHead + d0;
    float q[8];
    float qmax = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      q[i] = q3[swz<NC>(qr + i, nn)];
      qmax = fmaxf(qmax, q[i]);
    }
    f32x4 kv[8], vv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kv[i] = *(const lds_f4 *)(q3 + swz<NC>(kr + i, sb));
#pragma unroll
    for (int i = 0; i < 8; ++i) vv[i] = *(const lds_f4 *)(q3 + swz<NC>(vr + i, sb));
    qmax = half_max(row_pair_max(qmax));
    float qsum = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float e = fast_exp(q[i] - qmax);
      qsum += e;
      const float km = fmaxf(fmaxf(kv[i].x, kv[i].y), fmaxf(kv[i].z, kv[i].w));
      const float k0 = fast_exp(kv[i].x - km), k1 = fast_exp(kv[i].y - km), k2 = fast_exp(kv[i].z - km),
                  k3 = fast_exp(kv[i].w - km);
      const float f = e * __builtin_amdgcn_rcpf(k0 + k1 + k2 + k3);
      a0 += k0 * f; a1 += k1 * f; a2 += k2 * f; a3 += k3 * f;
    }
    qsum = half_sum(row_pair_sum(qsum));
    a0 = half_sum(row_pair_sum(a0)); a1 = half_sum(row_pair_sum(a1));
    a2 = half_sum(row_pair_sum(a2)); a3 = half_sum(row_pair_sum(a3));
    const float sc = 0.17677669529663687f * __builtin_amdgcn_rcpf(qsum);  // dim_head ** -0.5 / sum
    a0 *= sc; a1 *= sc; a2 *= sc; a3 *= sc;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      o3[swz<NC>(h2 * kDimHead + d0 + i, nn)] = vv[i].x * a0 + vv[i].y * a1 + vv[i].z * a2 + vv[i].w * a3;
    __syncthreads();
  } else {
    // L = 16 (pose decoder): 2 samples x 16 positions per tile, 4 waves.  Both softmaxes are normalised in place
    // first (keys over a sample's 16 positions: two lanes per (head, channel, sample); queries over the 32 channels,
    // scaled by dim_head^-0.5: four lanes per (head, column)), then a wave per (head, sample) takes
    // A = Kn^T Qn (16 x 16, K = 32) and out = V A (32 x 16, K = 16) as 16 MFMAs: A's accumulator registers are the
    // B operand of the second product as they stand (k-step r = key positions {4 kq + r}).  (The first form had every
    // lane recompute A with 512 exponentials: 30-80 k cycles per op, a third of the whole decode.)
    static_assert(NC == 32, "decoder tile");
    const int t = c.tid;
    lds_f *w3 = (lds_f *)qkv;
    {
      const int item = t >> 1, half = t & 1, h = item >> 6, d = (item >> 1) & 31, sm = item & 1;
      const int row = 64 + h * kDimHead + d, col0 = sm * 16 + 8 * half;
      float k[8];
      float km = -3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        k[j] = w3[swz<NC>(row, col0 + j)];
        km = fmaxf(km, k[j]);
      }
      km = dpp_max<0xB1>(km);  // the other half of the sample's positions: lane ^ 1
      float ks = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        k[j] = fast_exp(k[j] - km);
        ks += k[j];
      }
      ks += dpp_mov<0xB1>(ks);
      const float inv = __builtin_amdgcn_rcpf(ks);
#pragma unroll
      for (int j = 0; j < 8; ++j) w3[swz<NC>(row, col0 + j)] = k[j] * inv;
    }
    {
      const int item = t >> 2, qt = t & 3, h = item >> 5, col = item & 31;
      const int row0 = h * kDimHead + 8 * qt;
      float q[8];
      float qm = -3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q[j] = w3[swz<NC>(row0 + j, col)];
        qm = fmaxf(qm, q[j]);
      }
      qm = dpp_max<0xB1>(qm);
      qm = dpp_max<0x4E>(qm);  // the four channel quarters of a column: one quad
      float qs = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q[j] = fast_exp(q[j] - qm);
        qs += q[j];
      }
      qs += dpp_mov<0xB1>(qs);
      qs += dpp_mov<0x4E>(qs);
      const float sc = 0.17677669529663687f * __builtin_amdgcn_rcpf(qs);  // dim_head ** -0.5 / sum
#pragma unroll
      for (int j = 0; j < 8; ++j) w3[swz<NC>(row0 + j, col)] = q[j] * sc;
    }
    __syncthreads();
    const int h = c.wave >> 1, sm = c.wave & 1, m = c.lane & 15, kq = c.lane >> 4;
    f32x4 am = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // channel d = 4 j + kq
      const float ka = q3[swz<NC>(64 + h * kDimHead + 4 * j + kq, sm * 16 + m)];  // Kn^T[key position m][d]
      const float qb = q3[swz<NC>(h * kDimHead + 4 * j + kq, sm * 16 + m)];       // Qn[d][query position m]
      am = __builtin_amdgcn_mfma_f32_16x16x4f32(ka, qb, am, 0, 0, 0);
    }
    // am: lane (query position m, kq), register r = A[key position 4 kq + r][m]
    f32x4 o0 = f32x4{0.f, 0.f, 0.f, 0.f}, o1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // k-step r: key positions 4 kq + r
      const float v0 = q3[swz<NC>(128 + h * kDimHead + m, sm * 16 + 4 * kq + r)];
      const float v1 = q3[swz<NC>(128 + h * kDimHead + 16 + m, sm * 16 + 4 * kq + r)];
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, am[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, am[r], o1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o3[swz<NC>(h * kDimHead + 4 * kq + r, sm * 16 + m)] = o0[r];
      o3[swz<NC>(h * kDimHead + 16 + 4 * kq + r, sm * 16 + m)] = o1[r];
    }
    __syncthreads();
  }
}

// ResnetBlock of a 4-channel level with 4-position samples (the first level of the latent denoiser) on the
// VALU of ONE wave, in registers: as two MFMA ops it is two padded 16x16 tiles and two long epilogues for
// 48 MACs per output.  lane = (channel pair h, column n): every lane keeps all 4 input channels of its column
// and produces output channels 2h, 2h+1.  Taps come from the neighbouring lanes of the quad (= the sample),
// GroupNorm (one channel per group) is a quad reduction, the two channel pairs meet through a permlane swap.
// Weights are read in their packed MFMA-fragment order: conv W[co][ci][tap] at ((ci * 16 + co) * 4 + tap),
// scale/shift Linear W[row][e] at (((e & 3) * 16 + row) * 4 + (e >> 2)).
template <int NC>
__device__ __forceinline__ void resblock4_valu(const R1dCtx &c, const int (&o)[kOpInts], int E) {
  using GG = R1dGeo<NC>;
  if (c.wave != 0) return;
  const int n = c.lane & 31, h = c.lane >> 5, l = n & 3;
  const bool has_l = l != 0, has_r = l != 3;
  lds_f *X = (lds_f *)(c.lds + GG::kBufX);
  const lds_f *G = (const lds_f *)(c.lds + GG::kMiscG) + (n >> 2) * E;
  const float *w = c.w;
  const int c1_w = o[1], c1_b = o[2], n1_w = o[3], n1_b = o[4], c2_w = o[5], c2_b = o[6], n2_w = o[7], n2_b = o[8],
            ss_w = o[9], ss_b = o[10];
  // ---- every parameter of the block is requested up front (one L2 round trip for all of them)
  f32x4 wss[4][2][2], wc1[4][2], wc2[4][2];
  float bss[2][2], bc1[2], bc2[2], g1[2], b1[2], g2[2], b2[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int co = 2 * h + k;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      wss[kq][k][0] = *reinterpret_cast<const f32x4 *>(w + ss_w + (kq * 16 + co) * 4);      // scale row co
      wss[kq][k][1] = *reinterpret_cast<const f32x4 *>(w + ss_w + (kq * 16 + 4 + co) * 4);  // shift row 4 + co
      wc1[kq][k] = *reinterpret_cast<const f32x4 *>(w + c1_w + (kq * 16 + co) * 4);         // kq = input channel
      wc2[kq][k] = *reinterpret_cast<const f32x4 *>(w + c2_w + (kq * 16 + co) * 4);
    }
    bss[k][0] = w[ss_b + co]; bss[k][1] = w[ss_b + 4 + co];
    bc1[k] = w[c1_b + co]; bc2[k] = w[c2_b + co];
    g1[k] = w[n1_w + co]; b1[k] = w[n1_b + co]; g2[k] = w[n2_w + co]; b2[k] = w[n2_b + co];
  }
  float x[4];
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) x[ci] = X[swz<NC>(ci, n)];
  // ---- scale / shift of my two channels: rows 2h + k (scale, the +1 is in the packed bias) and 4 + 2h + k (shift)
  float sc[2], sh[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    sc[k] = bss[k][0];
    sh[k] = bss[k][1];
  }
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) {
    f32x4 gq = f32x4{0.f, 0.f, 0.f, 0.f};  // G[4 j + kq], j = 0..3: the first 16 entries (E = 16: the whole embedding)
#pragma unroll
    for (int j = 0; j < 4; ++j) gq[j] = 4 * j + kq < E ? G[4 * j + kq] : 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[k] += wss[kq][k][0][j] * gq[j];
        sh[k] += wss[kq][k][1][j] * gq[j];
      }
  }
  // a wider embedding (validate() takes E = 32 at 4 positions): its further 16-entry k-blocks, 256 packed floats each
  for (int kb = 1; kb < (E >> 4); ++kb) {
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) {
      f32x4 gq;
#pragma unroll
      for (int j = 0; j < 4; ++j) gq[j] = G[16 * kb + 4 * j + kq];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const f32x4 ws = *reinterpret_cast<const f32x4 *>(w + ss_w + kb * 256 + (kq * 16 + 2 * h + k) * 4);
        const f32x4 wh = *reinterpret_cast<const f32x4 *>(w + ss_w + kb * 256 + (kq * 16 + 4 + 2 * h + k) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sc[k] += ws[j] * gq[j];
          sh[k] += wh[j] * gq[j];
        }
      }
    }
  }
  auto conv3 = [&](const float (&in)[4], const f32x4 (&wc)[4][2], const float (&bc)[2], float (&out)[2]) {
    float lft[4], rgt[4];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const float a = dpp_mov<0x90>(in[ci]), b = dpp_mov<0xF9>(in[ci]);  // quad_perm [0,0,1,2] / [1,2,3,3]
      lft[ci] = has_l ? a : 0.f;
      rgt[ci] = has_r ? b : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float acc = bc[k];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        acc += wc[ci][k].x * lft[ci];
        acc += wc[ci][k].y * in[ci];
        acc += wc[ci][k].z * rgt[ci];
      }
      out[k] = acc;
    }
  };
  auto gn_act = [&](float (&v)[2], const float (&gw)[2], const float (&gb)[2], bool ss) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float m = group_sum<4>(v[k]) * 0.25f;
      const float d = v[k] - m;
      const float rs = __builtin_amdgcn_rsqf(group_sum<4>(d * d) * 0.25f + 1e-5f);
      float y = d * rs * gw[k] + gb[k];
      if (ss) y = y * sc[k] + sh[k];
      v[k] = silu(y);
    }
  };
  auto gather4 = [&](const float (&mine)[2], float (&all)[4]) {  // channels 0,1 live in half 0, channels 2,3 in half 1
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine[k]), __float_as_uint(mine[k]), false, false);
      all[k] = __uint_as_float(r[0]);      // [lo, lo]: half 0's value in both halves
      all[2 + k] = __uint_as_float(r[1]);  // [hi, hi]
    }
  };
  float y[2], ya[4], z[2];
  conv3(x, wc1, bc1, y);
  gn_act(y, g1, b1, !GLDM_SKIP(c, 16));
  gather4(y, ya);
  conv3(ya, wc2, bc2, z);
  gn_act(z, g2, b2, false);
#pragma unroll
  for (int k = 0; k < 2; ++k) X[swz<NC>(2 * h + k, n)] = x[2 * h + k] + z[k];
}
