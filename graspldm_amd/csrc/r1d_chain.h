// r1d_chain.h -- the cross-workgroup hand-off of r1d_kernel (resnet1d.hip): a left-over tile's steps are split over a chain of
// persistent workgroups (make_plan), and its latent row travels between them through the workspace.  The ticket / done / epoch
// re-arm of the header is at the end of r1d_kernel.  Included by resnet1d.hip inside its anonymous namespace.

// Step-segment hand-off between workgroups (a tile whose steps are split over a chain of slots).
// The whole state of a tile between two steps is its latent row: NC floats.  Each float travels as ONE
// naturally aligned 8-byte granule {value, tag} written by one write-through (agent-scope) store and
// polled with agent-scope loads: a granule is never torn, so no fence, flag or ordering between
// granules is needed (MI355X_MICROARCH.md, "R2's granule").  tag = (launch epoch, step count) is
// unique per launch and step; the zero-initialised workspace holds tag 0, which no hand-off uses.
struct ChainHdr { unsigned ticket, done, epoch, error; };
constexpr int kChainHdrBytes = 256;
__device__ __forceinline__ unsigned chain_tag(unsigned epoch, int step) { return (epoch << 12) | (unsigned)step; }
__device__ __forceinline__ void chain_give(unsigned long long *g, float v, unsigned tag) {
  __hip_atomic_store(g, ((unsigned long long)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float chain_take(unsigned long long *g, unsigned tag, unsigned *error) {
  unsigned long long x = 0;
  for (int spin = 0; spin < (1 << 22); ++spin) {  // bounded: ~2 s; a healthy wait is a few ms at most
    x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)(x >> 32) == tag) return __uint_as_float((unsigned)x);
    __builtin_amdgcn_s_sleep(16);
  }
  // The wait expired: the tile's latent is lost.  The error word is what the host reads (R1dEngine checks it after
  // every chained launch and raises); the NaN makes every output of this tile NaN whether or not anyone looks.
  __hip_atomic_store(error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_nanf("");
}
