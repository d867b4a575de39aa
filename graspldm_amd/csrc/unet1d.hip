// unet1d.hip -- Unet1D (grasp_ldm/models/modules/resnets.py:622-857) as ONE kernel: a workgroup carries a tile of
// `tile_samples` samples through the whole network and through every step of a sampling run.  Between the input row and
// the output row nothing but weights, embeddings and step noise touches global memory: the residual stream, the skip stack
// (two tensors per level) and the stem's output `r` live in LDS as f32 rows [channel][column], column = sample * L + position.
//
// The network is a PROGRAM the packer writes behind the weights (graspldm_amd/unet1d_pack.py): a list of 16-int ops
// (conv / GroupNorm / attention / stem / final) that name their LDS buffers and weight offsets, so the length changes, the
// two-source (never materialised) concatenations and the skip stack are decided once on the host, where the LDS map is
// also bounds-checked (unet1d_pack.check_program); the interpreter below has no network-shape logic of its own.
//
// GEMMs: every conv and 1x1 runs on the matrix pipe with f32 accumulation.  Default: split-f16 (mfma_prims.h: split_planes8
// / mfma_split, weights pre-split on the host as [M/16][K/32][hi|lo][64][8]).  exact_f32: the same walk with
// [M/16][K/32][64][8 f32] fragments on v_mfma_f32_16x16x4_f32 (lane (i, g) holds k = 32 kb + 8 g + j of row / column i for
// both operands, so eight 16x16x4 products cover the block).  K runs over [source][tap][32-channel block], every source
// padded to whole blocks with zero weight columns.
//   stride-2 k=4 conv (Downsample): taps read positions 2p-1 .. 2p+2, zero outside [0, Lin)
//   nearest x2 + k=3 conv (Upsample): taps read x[(p + tap - 1) >> 1], zero outside [0, 2 Lin)
// Norms, softmaxes and the scheduler step are f32 on the VALU; sums over a (sample, group) go through wave_sum (fixed tree).
#include "mfma_prims.h"

namespace {

constexpr int kUThreads = 256, kUWaves = kUThreads / 64;

struct UArgs {
  gldm_unet1d_desc d;
  const float *w, *temb, *cemb, *x_in, *coef, *noise;
  const int32_t *timesteps, *sample_t;
  float *out;
  int spc, n, n_steps, kind, clip;
};

struct UConv {
  int src0, c0, pitch_in, src1, c1, dst, pitch_out, m, mode, taps, lin, lout, w_off, b_off, add_off;
};

template <bool F32>
__device__ __forceinline__ void u_conv(float *lds, const float *__restrict__ w, int S, int wave, int lane, const UConv &o) {
  const int ntn = (S * o.lout + 15) >> 4, ntm = o.m >> 4;
  const int kbs = o.taps * (((o.c0 + 31) >> 5) + (o.c1 > 0 ? ((o.c1 + 31) >> 5) : 0));
  const int g = lane >> 4;
  for (int tile = wave; tile < ntm * ntn; tile += kUWaves) {
    const int mt = tile / ntn, nt = tile - mt * ntn;
    const int col = nt * 16 + (lane & 15);
    const int s = col / o.lout, p = col - s * o.lout;
    const bool valid = col < S * o.lout;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float *wt = w + o.w_off + (size_t)mt * kbs * 512;
    int kb = 0;
    for (int src = 0; src < 2; ++src) {
      const int C = src ? o.c1 : o.c0;
      if (C <= 0) continue;
      const int base = src ? o.src1 : o.src0, nb = (C + 31) >> 5;
      for (int t = 0; t < o.taps; ++t) {
        int pin;
        bool ok = valid;
        if (o.mode == 0) pin = p + t - (o.taps >> 1);
        else if (o.mode == 1) pin = 2 * p + t - 1;
        else {
          const int u = p + t - 1;
          ok = ok && u >= 0 && u < o.lout;
          pin = u >> 1;
        }
        ok = ok && pin >= 0 && pin < o.lin;
        const float *xp = lds + base + s * o.lin + pin;
        for (int b = 0; b < nb; ++b, ++kb) {
          float x[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ch = 32 * b + 8 * g + j;
            x[j] = (ok && ch < C) ? xp[ch * o.pitch_in] : 0.f;
          }
          const float *wf = wt + (size_t)kb * 512;
          if constexpr (F32) {
            const f32x4 a0 = *(const f32x4 *)(wf + lane * 8), a1 = *(const f32x4 *)(wf + lane * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], x[j], acc, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], x[4 + j], acc, 0, 0, 0);
          } else {
            u32x4 a[kSplit], bp[kSplit];
            a[0] = *(const u32x4 *)(wf + lane * 4);
            a[1] = *(const u32x4 *)(wf + 256 + lane * 4);
            // Range: the data sets these operands' magnitude (residual stream, stem output, skips), so a
            // COLUMN whose largest magnitude among the block's 32 channels leaves f16's comfortable range is split as
            // x / s, s a power of two, and s is folded back on the column's accumulators (a lane's four belong to its
            // column).  One s per column, not per wave: when L < 16 the wave's 16 columns span several samples, and a
            // loud sample's s would push its neighbours' planes into f16's subnormals.  The branch is wave uniform (any
            // column out of range); inside it a column with s = 1 still accumulates on the matrix pipe, so every column
            // keeps the bits it has without loud neighbours, and a block with no such column takes the plain path.
            // Written as two unlikely detours around ONE split + product so that the plain path falls straight through
            // (an if / else with a product each made it the taken side of a branch: 0.3 % of case A's time).
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(x[j]));
            m = half_max(row_pair_max(m));   // the column's four lane groups: lanes i, i ^ 16, i ^ 32, i ^ 48
            // range_pow2(m) != 1, on the biased exponent (m >= 0): floor(log2 m) in [-100, -8) or [14, 100]
            const unsigned be = __float_as_uint(m) >> 23;
            const bool any = (__builtin_amdgcn_ballot_w64(be - 27u < 92u) | __builtin_amdgcn_ballot_w64(be - 141u < 87u)) != 0;
            float sc = 1.0f;
            f32x4 cin = acc;
            if (__builtin_expect(any, 0)) {
              sc = range_pow2(m);
              const float inv = pow2_inv(sc);
#pragma unroll
              for (int j = 0; j < 8; ++j) x[j] *= inv;
#pragma unroll
              for (int r = 0; r < 4; ++r) cin[r] = sc != 1.0f ? 0.f : acc[r];
            }
            split_planes8(x, bp);
            const f32x4 part = mfma_split(a, bp, cin);
            if (__builtin_expect(any, 0)) {
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[r] = sc != 1.0f ? acc[r] + part[r] * sc : part[r];
            } else {
              acc = part;
            }
          }
        }
      }
    }
    if (valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mt * 16 + 4 * g + r;
        float v = acc[r];
        if (o.b_off >= 0) v += w[o.b_off + row];
        if (o.add_off >= 0) v += lds[o.add_off + row * o.pitch_out + col];
        lds[o.dst + row * o.pitch_out + col] = v;
      }
    }
  }
}

// GroupNorm (eps 1e-5, two-pass variance) + scale/shift + SiLU (+ residual) : one wave per (sample, group)
__device__ __forceinline__ void u_groupnorm(float *lds, const float *__restrict__ w, int S, int wave, int lane, const int *op,
                                            int o_ss) {
  const int buf = op[1], C = op[2], pitch = op[3], L = op[4], gw = op[5], gb = op[6], use_ss = op[7], add = op[8],
            out = op[9], G = op[10];
  const int cg = C / G, nel = cg * L;
  const float inv = 1.0f / (float)nel;
  for (int u = wave; u < S * G; u += kUWaves) {
    const int s = u / G, grp = u - s * G;
    float sum = 0.f;
    for (int e = lane; e < nel; e += 64) {
      const int ch = grp * cg + e / L, p = e % L;
      sum += lds[buf + ch * pitch + s * L + p];
    }
    const float mean = wave_sum(sum) * inv;
    float sq = 0.f;
    for (int e = lane; e < nel; e += 64) {
      const int ch = grp * cg + e / L, p = e % L;
      const float dlt = lds[buf + ch * pitch + s * L + p] - mean;
      sq += dlt * dlt;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) * inv + 1e-5f);
    for (int e = lane; e < nel; e += 64) {
      const int ch = grp * cg + e / L, p = e % L, at = ch * pitch + s * L + p;
      float v = (lds[buf + at] - mean) * rstd * w[gw + ch] + w[gb + ch];
      if (use_ss) v = v * lds[o_ss + ch * S + s] + lds[o_ss + (C + ch) * S + s];
      v = silu(v);
      if (add >= 0) v += lds[add + at];
      lds[out + at] = v;
    }
  }
}

// Residual(PreNorm(LinearAttention)) (resnets.py:211-235; ln2 >= 0) or Residual(PreNorm(Attention)) (:238-261; ln2 < 0), one
// head at a time: qkv rows of a head (q | k | v, 96 rows) -> softmaxes -> A[s][n][m] -> O = V A^T -> to_out accumulated over heads.
template <bool F32>
__device__ __forceinline__ void u_attention(float *lds, const float *__restrict__ w, int S, int tid, int wave, int lane,
                                            const int *op, const gldm_unet1d_desc &d) {
  const int xb = op[1], C = op[2], pitch = op[3], L = op[4], out = op[5], lnb = op[6], yb = op[7], ln_g = op[8],
            qkv_w = op[9], out_w = op[10], out_b = op[11], ln2 = op[12];
  const int N = S * L;
  const int Q = d.o_qkv, K = Q + 32 * pitch, V = Q + 64 * pitch, O = d.o_o, A = d.o_a;
  const float invc = 1.0f / (float)C;
  for (int col = tid; col < N; col += kUThreads) {   // PreNorm: LayerNorm over channels, gain
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += lds[xb + c * pitch + col];
    const float mean = sum * invc;
    float sq = 0.f;
    for (int c = 0; c < C; ++c) {
      const float dl = lds[xb + c * pitch + col] - mean;
      sq += dl * dl;
    }
    const float rstd = 1.0f / sqrtf(sq * invc + 1e-5f);
    for (int c = 0; c < C; ++c) lds[lnb + c * pitch + col] = (lds[xb + c * pitch + col] - mean) * rstd * w[ln_g + c];
  }
  __syncthreads();
  const int kb_qkv = (C + 31) >> 5, mt_out = C >> 4;
  const float scale = 0.17677669529663687f;   // dim_head ** -0.5
  for (int h = 0; h < kHeads; ++h) {
    UConv cq{lnb, C, pitch, 0, 0, Q, pitch, 96, 0, 1, L, L, qkv_w + h * 6 * kb_qkv * 512, -1, -1};
    u_conv<F32>(lds, w, S, wave, lane, cq);
    __syncthreads();
    if (ln2 >= 0) {
      for (int it = tid; it < N + S * 32; it += kUThreads) {
        if (it < N) {   // q: softmax over the head's 32 channels, times scale
          float m = -INFINITY;
          for (int c = 0; c < 32; ++c) m = fmaxf(m, lds[Q + c * pitch + it]);
          float sum = 0.f;
          for (int c = 0; c < 32; ++c) sum += __expf(lds[Q + c * pitch + it] - m);
          const float f = scale / sum;
          for (int c = 0; c < 32; ++c) lds[Q + c * pitch + it] = __expf(lds[Q + c * pitch + it] - m) * f;
        } else {        // k: softmax over the sample's positions
          const int u = it - N, s = u >> 5, c = u & 31;
          float *kr = lds + K + c * pitch + s * L;
          float m = -INFINITY;
          for (int n = 0; n < L; ++n) m = fmaxf(m, kr[n]);
          float sum = 0.f;
          for (int n = 0; n < L; ++n) sum += __expf(kr[n] - m);
          const float f = 1.0f / sum;
          for (int n = 0; n < L; ++n) kr[n] = __expf(kr[n] - m) * f;
        }
      }
      __syncthreads();
      for (int it = tid; it < N * L; it += kUThreads) {   // A[s][n][m] = sum_d q[d][n] k[d][m]
        const int col = it / L, mm = it - col * L, s = col / L;
        float acc = 0.f;
        for (int c = 0; c < 32; ++c) acc += lds[Q + c * pitch + col] * lds[K + c * pitch + s * L + mm];
        lds[A + it] = acc;
      }
    } else {
      for (int col = tid; col < N; col += kUThreads) {     // A[s][i][j] = softmax_j(scale q_i . k_j)
        const int s = col / L;
        float sim[16];
        float m = -INFINITY;
        for (int j = 0; j < L; ++j) {
          float acc = 0.f;
          for (int c = 0; c < 32; ++c) acc += lds[Q + c * pitch + col] * lds[K + c * pitch + s * L + j];
          sim[j] = acc * scale;
          m = fmaxf(m, sim[j]);
        }
        float sum = 0.f;
        for (int j = 0; j < L; ++j) {
          sim[j] = __expf(sim[j] - m);
          sum += sim[j];
        }
        const float f = 1.0f / sum;
        for (int j = 0; j < L; ++j) lds[A + col * L + j] = sim[j] * f;
      }
    }
    __syncthreads();
    for (int it = tid; it < 32 * N; it += kUThreads) {     // O[e][n] = sum_m v[e][m] A[s][n][m]
      const int e = it / N, col = it - e * N, s = col / L;
      float acc = 0.f;
      for (int mm = 0; mm < L; ++mm) acc += lds[V + e * pitch + s * L + mm] * lds[A + col * L + mm];
      lds[O + e * pitch + col] = acc;
    }
    __syncthreads();
    UConv co{O, 32, pitch, 0, 0, yb, pitch, C, 0, 1, L, L, out_w + h * mt_out * 512, h == 0 ? out_b : -1, h == 0 ? -1 : yb};
    u_conv<F32>(lds, w, S, wave, lane, co);
    __syncthreads();
  }
  for (int col = tid; col < N; col += kUThreads) {
    if (ln2 >= 0) {   // to_out.1: LayerNorm with gain, then the residual
      float sum = 0.f;
      for (int c = 0; c < C; ++c) sum += lds[yb + c * pitch + col];
      const float mean = sum * invc;
      float sq = 0.f;
      for (int c = 0; c < C; ++c) {
        const float dl = lds[yb + c * pitch + col] - mean;
        sq += dl * dl;
      }
      const float rstd = 1.0f / sqrtf(sq * invc + 1e-5f);
      for (int c = 0; c < C; ++c)
        lds[out + c * pitch + col] = (lds[yb + c * pitch + col] - mean) * rstd * w[ln2 + c] + lds[xb + c * pitch + col];
    } else {
      for (int c = 0; c < C; ++c) lds[out + c * pitch + col] = lds[yb + c * pitch + col] + lds[xb + c * pitch + col];
    }
  }
}

// x_{t-1} from (x_t, eps): scheduler_update, the arithmetic of gldm_denoise's step
#include "diffusion_step.h"

template <bool F32>
__global__ __launch_bounds__(kUThreads) void unet1d_kernel(const UArgs a) {
  extern __shared__ float lds[];
  const gldm_unet1d_desc &d = a.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int S = d.tile_samples, L = d.seq_len, E = d.emb_dim, R = d.cond_rows;
  const int first = blockIdx.x * S;
  const float *__restrict__ w = a.w;
  const int *prog = (const int *)(w + d.prog_off);
  for (int i = tid; i < S * L; i += kUThreads) {
    const int gi = first + i / L;
    lds[d.o_lat + i] = gi < a.n ? a.x_in[(size_t)gi * L + i % L] : 0.f;
  }
  for (int step = 0; step < a.n_steps; ++step) {
    if (d.has_emb) {   // EMB[e][s] = sum_r silu(time row + conditioning row r): mlp = Linear(SiLU(.)) summed over the R rows
      for (int i = tid; i < E * 16; i += kUThreads) {
        const int e = i >> 4, s = i & 15;
        float v = 0.f;
        if (s < S) {
          int gi = first + s;
          gi = gi < a.n ? gi : a.n - 1;
          float te = 0.f;
          if (d.time_cond) {
            const int t = a.sample_t ? a.sample_t[gi] : a.timesteps[step];
            te = a.temb[(size_t)t * E + e];
          }
          if (a.cemb) {
            const float *ce = a.cemb + ((size_t)(gi / a.spc) * R) * E + e;
            for (int r = 0; r < R; ++r) v += silu(te + ce[(size_t)r * E]);
          } else {
            v = silu(te);
          }
        }
        lds[d.o_emb + e * GLDM_UNET1D_EMB_PITCH + s] = v;
      }
    }
    __syncthreads();
    for (int i = 0; i < d.n_ops; ++i) {
      const int *op = prog + i * GLDM_UNET1D_OP_INTS;
      const int kind = op[0];
      if (kind == GLDM_UNET1D_OP_CONV) {
        UConv c{op[1], op[2], op[3], op[4], op[5], op[6], op[7], op[8], op[9], op[10], op[11], op[12], op[13], op[14], op[15]};
        u_conv<F32>(lds, w, S, wave, lane, c);
      } else if (kind == GLDM_UNET1D_OP_GN) {
        u_groupnorm(lds, w, S, wave, lane, op, d.o_ss);
      } else if (kind == GLDM_UNET1D_OP_ATT) {
        u_attention<F32>(lds, w, S, tid, wave, lane, op, d);
      } else if (kind == GLDM_UNET1D_OP_STEM) {   // init_conv: Conv1d(1 -> C, k = 7, pad 3) of the latent row
        const int dst = op[1], C = op[2], pitch = op[3], wo = op[4], bo = op[5];
        for (int it = tid; it < C * S * L; it += kUThreads) {
          const int c = it / (S * L), col = it - c * (S * L), s = col / L, p = col - s * L;
          float acc = w[bo + c];
          for (int t = 0; t < 7; ++t) {
            const int q = p + t - 3;
            if (q >= 0 && q < L) acc += w[wo + c * 7 + t] * lds[d.o_lat + s * L + q];
          }
          lds[dst + c * pitch + col] = acc;
        }
      } else if (kind == GLDM_UNET1D_OP_FINAL) {  // final_conv: Conv1d(C -> 1, k = 1)
        const int xb = op[1], C = op[2], pitch = op[3], wo = op[4], bo = op[5];
        for (int col = tid; col < S * L; col += kUThreads) {
          float acc = w[bo];
          for (int c = 0; c < C; ++c) acc += w[wo + c] * lds[xb + c * pitch + col];
          lds[d.o_eps + col] = acc;
        }
      }
      __syncthreads();
    }
    if (a.kind != GLDM_SCHED_NONE) {
      const float *cf = a.coef + (size_t)step * GLDM_SCHED_COEF_STRIDE;
      for (int i = tid; i < S * L; i += kUThreads) {
        const int gi = first + i / L;
        float nz = 0.f;
        if (a.kind == GLDM_SCHED_DDPM && cf[7] != 0.f && a.noise && gi < a.n)
          nz = a.noise[((size_t)step * a.n + gi) * L + i % L];
        lds[d.o_lat + i] = scheduler_update(a.kind, a.clip, cf, lds[d.o_lat + i], lds[d.o_eps + i], nz);
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < S * L; i += kUThreads) {
    const int gi = first + i / L;
    if (gi < a.n) a.out[(size_t)gi * L + i % L] = a.kind == GLDM_SCHED_NONE ? lds[d.o_eps + i] : lds[d.o_lat + i];
  }
}

constexpr int kULdsMaxBytes = 160 * 1024;

}  // namespace

GLDM_API int gldm_unet1d_supported(const gldm_unet1d_desc *d, int seq_len) {
  if (!d) return GLDM_ERR_INVALID_ARG;
  if (d->dim != 16 && d->dim != 32) return GLDM_ERR_UNSUPPORTED;
  if (d->n_levels < 2 || d->n_levels > GLDM_UNET1D_MAX_LEVELS) return GLDM_ERR_UNSUPPORTED;
  if (d->widths[0] != d->dim) return GLDM_ERR_UNSUPPORTED;
  for (int i = 0; i <= d->n_levels; ++i)
    if (d->widths[i] < 16 || d->widths[i] > 256 || d->widths[i] % 16) return GLDM_ERR_UNSUPPORTED;
  if (d->groups != 4 && d->groups != 8) return GLDM_ERR_UNSUPPORTED;
  if (d->emb_dim != 4 * d->dim) return GLDM_ERR_UNSUPPORTED;
  if (d->cond_rows < 0 || d->cond_rows > 4) return GLDM_ERR_UNSUPPORTED;
  if (d->time_cond && d->cond_rows > 1) return GLDM_ERR_UNSUPPORTED;   // resnets.py:816-822 adds the embeddings without tiling
  if (seq_len < 2 || seq_len > 16 || seq_len % (1 << (d->n_levels - 1))) return GLDM_ERR_UNSUPPORTED;
  return GLDM_OK;
}

GLDM_API int gldm_unet1d(const gldm_unet1d_desc *desc, const float *weights, const float *temb, const float *cemb,
                         int samples_per_cond, const float *x_in, int n_samples, int seq_len, const int32_t *timesteps,
                         const int32_t *sample_t, int n_steps, int sched_kind, int clip_sample, const float *sched_coef,
                         const float *step_noise, float *x_out, gldm_stream_t stream) {
  if (!desc) return GLDM_ERR_INVALID_ARG;
  const int st = gldm_unet1d_supported(desc, seq_len);
  if (st != GLDM_OK) return st;
  if (!weights || !x_in || !x_out || n_samples <= 0 || n_steps <= 0 || samples_per_cond <= 0) return GLDM_ERR_INVALID_ARG;
  // the packed program was laid out for one length and one tile size: its LDS map is only valid for them
  if (desc->seq_len != seq_len || desc->tile_samples < 1 || desc->tile_samples > 16 || desc->n_ops <= 0 || desc->prog_off <= 0 ||
      desc->lds_floats <= 0 || (long long)desc->lds_floats * 4 > kULdsMaxBytes)
    return GLDM_ERR_INVALID_ARG;
  if ((desc->cond_rows > 0) != (cemb != nullptr)) return GLDM_ERR_INVALID_ARG;
  if (desc->time_cond && (!temb || (!timesteps && !sample_t))) return GLDM_ERR_INVALID_ARG;
  if (desc->has_emb != ((desc->time_cond || desc->cond_rows > 0) ? 1 : 0)) return GLDM_ERR_INVALID_ARG;
  if (sched_kind != GLDM_SCHED_NONE && sched_kind != GLDM_SCHED_DDIM && sched_kind != GLDM_SCHED_DDPM) return GLDM_ERR_UNSUPPORTED;
  if (sched_kind != GLDM_SCHED_NONE && !sched_coef) return GLDM_ERR_INVALID_ARG;
  if (sched_kind == GLDM_SCHED_NONE && n_steps != 1) return GLDM_ERR_INVALID_ARG;
  if (sched_kind != GLDM_SCHED_NONE && sample_t) return GLDM_ERR_INVALID_ARG;
  UArgs a{};
  a.d = *desc;
  a.w = weights; a.temb = temb; a.cemb = cemb; a.x_in = x_in; a.coef = sched_coef; a.noise = step_noise;
  a.timesteps = timesteps; a.sample_t = sample_t; a.out = x_out;
  a.spc = samples_per_cond; a.n = n_samples; a.n_steps = n_steps; a.kind = sched_kind; a.clip = clip_sample;
  const int bytes = desc->lds_floats * 4;
  const int tiles = (n_samples + desc->tile_samples - 1) / desc->tile_samples;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e;
  if (desc->exact_f32) {
    e = hipFuncSetAttribute((const void *)unet1d_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return GLDM_ERR_LAUNCH;
    hipLaunchKernelGGL(unet1d_kernel<true>, dim3(tiles), dim3(kUThreads), bytes, s, a);
  } else {
    e = hipFuncSetAttribute((const void *)unet1d_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return GLDM_ERR_LAUNCH;
    hipLaunchKernelGGL(unet1d_kernel<false>, dim3(tiles), dim3(kUThreads), bytes, s, a);
  }
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}
