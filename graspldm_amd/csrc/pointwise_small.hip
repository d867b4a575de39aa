// pointwise_small.hip -- the k = 1 convs and Linears that are not the fused MLP launches of pointwise_mlp.hip: layers too
// narrow, too odd-shaped or too few-rowed for those, and the bias + activation pass behind a library GEMM.
//   gldm_pointwise_small   narrow cin (3 .. 64), lane = point, fma chains on the VALU
//   gldm_pointwise_any     any (cin, cout, n), exact f32 products on v_mfma_f32_16x16x4_f32
//   gldm_pointwise_rows    a few output rows (<= 8) over many channels, memory bound
//   gldm_linear_rows       Linear over the point axis, a workgroup per row
//   gldm_bias_act          y = act(y + bias) in place
#include "mfma_prims.h"

namespace {

// y[b, c, :] = act(y[b, c, :] + bias[c]) in place: the epilogue of the k = 1 convs that run as plain
// library GEMMs (one pass instead of a bias pass and an activation pass).
__global__ __launch_bounds__(256) void bias_act_kernel(float *__restrict__ y, const float *__restrict__ bias, int c,
                                                       long long n, int relu) {
  const long long row = blockIdx.y;  // b * c + channel
  const float bv = bias[row % c];
  float *p = y + row * n;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 v = reinterpret_cast<float4 *>(p)[i];
    v.x += bv; v.y += bv; v.z += bv; v.w += bv;
    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    reinterpret_cast<float4 *>(p)[i] = v;
  }
}

// ---- narrow k = 1 convs and the Linear over the point axis (the pieces of the shipped encoder that used to go to
// MIOpen / rocBLAS: SharedMLP 3 -> 48 and 48 -> 96 of the PVConv point branches, shared_mlp.py:6-35, and
// out_layer[1] = Linear(n_points -> latent) over the POINT axis, pc_encoders.py:60-82,104-111).  Too small for the
// matrix pipe (<= 4.6 k MAC per point): lane = point, the point's cin inputs in registers, weights wave-uniform on the
// scalar path, fma chain in k order from the bias.
template <int CIN>
__global__ __launch_bounds__(256) void pointwise_small_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                              const float *__restrict__ bias, int cout, long long n,
                                                              int relu, float *__restrict__ y) {
  const int b = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *xb = x + (size_t)b * CIN * n + i;
  float v[CIN];
#pragma unroll
  for (int ci = 0; ci < CIN; ++ci) v[ci] = xb[(size_t)ci * n];
  float *yb = y + (size_t)b * cout * n + i;
  // eight output channels at a time: eight independent fma chains per lane (one chain per pass left the vector pipe waiting
  // on its own result: 0.106 ms for 48 -> 96 over 256 x 1024 points, three times its instruction count)
  constexpr int kCh = 8;
  int co = 0;
  for (; co + kCh <= cout; co += kCh) {
    const float *wr = w + (size_t)co * CIN;
    float acc[kCh];
#pragma unroll
    for (int k = 0; k < kCh; ++k) acc[k] = bias ? bias[co + k] : 0.f;
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
      for (int k = 0; k < kCh; ++k) acc[k] = fmaf(wr[k * CIN + ci], v[ci], acc[k]);
#pragma unroll
    for (int k = 0; k < kCh; ++k) yb[(size_t)(co + k) * n] = relu ? fmaxf(acc[k], 0.f) : acc[k];
  }
  for (; co < cout; ++co) {
    const float *wr = w + (size_t)co * CIN;
    float acc = bias ? bias[co] : 0.f;
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) acc = fmaf(wr[ci], v[ci], acc);
    yb[(size_t)co * n] = relu ? fmaxf(acc, 0.f) : acc;
  }
}

// ---- any-shape k = 1 conv (SharedMLP / feature-propagation layers outside the fused launches' shape sets) --------------
// y[b, co, i] = act(bias[co] + sum_ci W[co][ci] x[b, ci, i]) for ANY (cin, cout, n), weights as stored by nn.Conv1d
// ([cout][cin], BatchNorm folded by the caller): exact f32 products on v_mfma_f32_16x16x4_f32.  A 256-thread workgroup
// owns a 64-row x 64-point output tile (wave = m-tile, four n-tiles); K is staged 16 channels at a time through LDS with
// bounds masks (W rows padded to 17 words, x rows to 80: both fragment reads conflict free).  Replaces the library GEMM
// (rocBLAS / MIOpen through F.conv1d) + bias / activation pass these layers used to take: PointNet++ / PVCNN2 widths such
// as 384 -> 256 over 128 centres.  Not a speed-of-light kernel (one 16-deep stage per barrier pair); the shipped encoder
// never comes here.
__global__ __launch_bounds__(256) void pointwise_any_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                            const float *__restrict__ bias, int cin, int cout, long long n,
                                                            int relu, float *__restrict__ y) {
  __shared__ float Ws[64 * 17];
  __shared__ float Xs[16 * 80];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
  const long long c0 = (long long)blockIdx.x * 64;
  const int r0 = blockIdx.y * 64, b = blockIdx.z;
  x += (size_t)b * cin * n;
  y += (size_t)b * cout * n;
  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int wr = tid >> 2, wk = (tid & 3) * 4;          // W stage: row, first k of the thread's four
  const int xk = tid >> 4, xc = (tid & 15) * 4;         // x stage: channel, first point of the thread's four
  for (int k0 = 0; k0 < cin; k0 += 16) {
    float wv[4], xv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool okw = r0 + wr < cout && k0 + wk + q < cin;
      wv[q] = okw ? w[(size_t)(r0 + wr) * cin + k0 + wk + q] : 0.f;
      const bool okx = k0 + xk < cin && c0 + xc + q < n;
      xv[q] = okx ? x[(size_t)(k0 + xk) * n + c0 + xc + q] : 0.f;
    }
    __syncthreads();   // the previous stage's readers are done
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Ws[wr * 17 + wk + q] = wv[q];
      Xs[xk * 80 + xc + q] = xv[q];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = Ws[(16 * wave + col) * 17 + 4 * j + kq];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Xs[(4 * j + kq) * 80 + 16 * ni + col], acc[ni], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 16 * wave + 4 * kq + r;
    if (row < cout) {
      const float bv = bias ? bias[row] : 0.f;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const long long i = c0 + 16 * ni + col;
        if (i < n) {
          const float v = acc[ni][r] + bv;
          y[(size_t)row * n + i] = relu ? fmaxf(v, 0.f) : v;
        }
      }
    }
  }
}

// y[row, o] = bias[o] + sum_n W[o, n] x[row, n]: one workgroup per row (rows = batch x channels: a few hundred),
// the row staged in LDS, thread = output feature, four interleaved k-ordered fma chains.
__global__ __launch_bounds__(256) void linear_rows_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                          const float *__restrict__ bias, int n, int nout,
                                                          float *__restrict__ y) {
  extern __shared__ float xs[];
  const int row = blockIdx.x;
  for (int i = threadIdx.x; i < n; i += 256) xs[i] = x[(size_t)row * n + i];
  __syncthreads();
  for (int o = threadIdx.x; o < nout; o += 256) {
    const float *wr = w + (size_t)o * n;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;   // four interleaved chains: shorter dependency and error chains
    for (int i = 0; i < n; i += 4) {
      const float4 wv = *reinterpret_cast<const float4 *>(wr + i);
      a0 = fmaf(wv.x, xs[i], a0);
      a1 = fmaf(wv.y, xs[i + 1], a1);
      a2 = fmaf(wv.z, xs[i + 2], a2);
      a3 = fmaf(wv.w, xs[i + 3], a3);
    }
    y[(size_t)row * nout + o] = ((a0 + a1) + (a2 + a3)) + (bias ? bias[o] : 0.f);
  }
}

// ---- a few output rows of a k = 1 conv over [b, cin, n]: out_layer[0] behind the attention block (768 -> 3) ---------------
// Memory bound (one pass over x): a thread owns four consecutive points, walks the channels with 16-byte loads and keeps
// HO accumulators per point; k-ordered fma chain from the bias.  (The any-shape MFMA kernel pads 3 rows to a 64-row tile.)
template <int HO>
__global__ __launch_bounds__(256) void pointwise_rows_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                             const float *__restrict__ bias, int cin, int n, float *__restrict__ y) {
  const int q = blockIdx.x * 256 + threadIdx.x, nq = n / 4;
  if (q >= nq) return;
  const f32x4 *xp = (const f32x4 *)(x + (size_t)blockIdx.y * cin * n) + q;
  f32x4 acc[HO];
#pragma unroll
  for (int o = 0; o < HO; ++o) {
    const float b0 = bias ? bias[o] : 0.f;
    acc[o] = f32x4{b0, b0, b0, b0};
  }
#pragma unroll 8
  for (int ch = 0; ch < cin; ++ch) {
    const f32x4 v = xp[(size_t)ch * nq];
#pragma unroll
    for (int o = 0; o < HO; ++o) {
      const float wv = w[o * cin + ch];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[o][e] = __builtin_fmaf(wv, v[e], acc[o][e]);
    }
  }
  f32x4 *yp = (f32x4 *)(y + (size_t)blockIdx.y * HO * n) + q;
#pragma unroll
  for (int o = 0; o < HO; ++o) yp[(size_t)o * nq] = acc[o];
}

template <int HO>
int launch_rows(const float *x, const float *w, const float *bias, int b, int cin, int hout, int n, float *y, hipStream_t st) {
  if constexpr (HO > 8) {
    return GLDM_ERR_UNSUPPORTED;
  } else {
    if (hout != HO) return launch_rows<HO + 1>(x, w, bias, b, cin, hout, n, y, st);
    hipLaunchKernelGGL(pointwise_rows_kernel<HO>, dim3((n / 4 + 255) / 256, b), dim3(256), 0, st, x, w, bias, cin, n, y);
    return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
  }
}

}  // namespace

GLDM_API int gldm_pointwise_small(const float *x, const float *w, const float *bias, int b, int cin, int cout, long long n,
                                  int relu, float *y, gldm_stream_t stream) {
  if (!x || !w || !y || b <= 0 || cin <= 0 || cout <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((n + 255) / 256), b);
#define GLDM_PS_CASE(C) \
  if (cin == C) { hipLaunchKernelGGL(pointwise_small_kernel<C>, grid, dim3(256), 0, s, x, w, bias, cout, n, relu, y); \
                  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH; }
  GLDM_PS_CASE(3) GLDM_PS_CASE(6) GLDM_PS_CASE(16) GLDM_PS_CASE(24) GLDM_PS_CASE(32) GLDM_PS_CASE(48) GLDM_PS_CASE(64)
#undef GLDM_PS_CASE
  return GLDM_ERR_UNSUPPORTED;
}

GLDM_API int gldm_pointwise_any(const float *x, const float *w, const float *bias, int b, int cin, int cout, long long n,
                                int relu, float *y, gldm_stream_t stream) {
  if (!x || !w || !y || b <= 0 || cin <= 0 || cout <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  const long long tiles = (n + 63) / 64;
  if (tiles > 0x7fffffffLL || b > 65535 || (cout + 63) / 64 > 65535) return GLDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pointwise_any_kernel, dim3((unsigned)tiles, (cout + 63) / 64, b), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, w, bias, cin, cout, n, relu, y);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_linear_rows(const float *x, const float *w, const float *bias, int rows, int n, int nout, float *y,
                              gldm_stream_t stream) {
  if (!x || !w || !y || rows <= 0 || n <= 0 || nout <= 0) return GLDM_ERR_INVALID_ARG;
  if ((n & 3) || (size_t)n * 4 > 64 * 1024) return GLDM_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(linear_rows_kernel, dim3(rows), dim3(256), (size_t)n * sizeof(float),
                     reinterpret_cast<hipStream_t>(stream), x, w, bias, n, nout, y);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_bias_act(float *y, const float *bias, int b, int c, long long n, int relu, gldm_stream_t stream) {
  if (!y || !bias || b <= 0 || c <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if (n & 3) return GLDM_ERR_UNSUPPORTED;  // rows must stay 16-byte aligned
  const long long n4 = n >> 2;
  const int bx = (int)((n4 + 255) / 256 < 1 ? 1 : ((n4 + 255) / 256 > 64 ? 64 : (n4 + 255) / 256));
  hipLaunchKernelGGL(bias_act_kernel, dim3(bx, b * c), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, bias, c, n,
                     relu);
  return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH;
}

GLDM_API int gldm_pointwise_rows(const float *x, const float *w, const float *bias, int b, int cin, int hout, int n, float *y,
                                 gldm_stream_t stream) {
  if (!x || !w || !y || b <= 0 || cin <= 0 || hout <= 0 || n <= 0) return GLDM_ERR_INVALID_ARG;
  if ((((size_t)x | (size_t)y) & 15)) return GLDM_ERR_INVALID_ARG;
  if (hout > 8 || n % 4 || b > 65535) return GLDM_ERR_UNSUPPORTED;
  return launch_rows<1>(x, w, bias, b, cin, hout, n, y, reinterpret_cast<hipStream_t>(stream));
}
