// diffusion_step.h -- one reverse-diffusion step on one element, shared by the two 1-D engines (resnet1d.hip, unet1d.hip)
// and the noise kernel of pose_ops.hip, so that all of them round identically: the Philox4x32-10 + Box-Muller normals and the
// DDIM / DDPM / DPM-Solver++ updates (no contraction: one rounding per written operation).  Device code only, __forceinline__;
// include it inside the translation unit's anonymous namespace, behind <hip/hip_runtime.h> and gldm.h (all it needs).

// Philox4x32-10 (Salmon et al., SC'11: the counter-based generator of curand / torch's device RNG): the four words of
// (key = seed, counter).  Also the uniforms of mesh_sample.hip.
__device__ __forceinline__ void philox4x32_10(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned (&u)[4]) {
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  u[0] = c0; u[1] = c1; u[2] = c2; u[3] = c3;
}

// Box-Muller on those words: four unit normals per (key, counter).  z[0..3] of counter (latent, position block, step) are
// positions 4 block + 0..3.
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3, float (&z)[4]) {
  unsigned u[4];
  philox4x32_10(seed, c0, c1, c2, c3, u);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float a = ((float)u[2 * h] + 1.0f) * 2.3283064365386963e-10f;   // (0, 1]
    const float ang = (float)u[2 * h + 1] * (6.283185307179586f * 2.3283064365386963e-10f);
    const float rad = sqrtf(-2.0f * __logf(a));
    z[2 * h] = rad * __cosf(ang);
    z[2 * h + 1] = rad * __sinf(ang);
  }
}

#pragma clang fp contract(off)
// DPM-Solver++(2M) step of ElucidatedDiffusion.sample_using_dpmpp (elucidated_diffusion.py:259-313) on one element:
// denoised = c_skip x + c_out net (:134, optional clamp :137); denoised_d = (1 - gamma) denoised + gamma old (:303);
// x' = (sigma_next / sigma) x - expm1(-h) denoised_d (:305).  cf = [c_in, c_skip, c_out, 1 - gamma, gamma,
// sigma_fn(t_next) / sigma_fn(t), expm1(-h), use_old].  Every operation rounds once, in the reference's order.
__device__ __forceinline__ float dpmpp_update(int clamp, const float *cf, float x, float net, float *old) {
  const float a = cf[1] * x;
  const float b = cf[2] * net;
  float den = a + b;
  if (clamp) den = fminf(fmaxf(den, -1.0f), 1.0f);
  float d = den;
  if (cf[7] != 0.f) {
    const float p = cf[3] * den;
    const float q = cf[4] * *old;
    d = p + q;
  }
  *old = den;
  const float u = cf[5] * x;
  const float v = cf[6] * d;
  return u - v;
}

__device__ __forceinline__ float scheduler_update(int kind, int clip, const float *cf, float x, float eps, float noise) {
  float x0 = (x - cf[0] * eps) / cf[1];
  if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  if (kind == GLDM_SCHED_DDIM) {
    const float a = cf[2] * x0;
    const float b = cf[3] * eps;
    return a + b;
  }
  const float a = cf[4] * x0;
  const float b = cf[5] * x;
  float prev = a + b;
  if (cf[7] != 0.f) {
    const float nz = cf[6] * noise;
    prev = prev + nz;
  }
  return prev;
}
#pragma clang fp contract(fast)
