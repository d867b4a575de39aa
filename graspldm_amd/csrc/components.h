// components.h -- the pieces of connected-component labelling that tabletop.hip (gldm_segment_tabletop, pixels) and
// cloud_cluster.hip (gldm_cluster_cloud, unorganised points) share: a lock-free union-find whose parents only decrease, the
// 64-bit ranking key (falling size, rising root) and the selection of the max_labels largest keys by one workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kSelectBlock = 1024;   // threads of the selecting workgroup

// parent[x] <= x for every live x, and parents only decrease: both loops below end on their own data.  A plain (stale) value
// of par[] is still an ancestor; the step that decides is the atomicMin.
__device__ __forceinline__ int uf_find(int *par, int x) {
  int p;
  while ((p = __atomic_load_n(&par[x], __ATOMIC_RELAXED)) != x) x = p;
  return x;
}

__device__ __forceinline__ void uf_union(int *par, int a, int b) {
  for (;;) {
    a = uf_find(par, a);
    b = uf_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(&par[a], b);   // a > b: hang the higher root under the lower
    if (old == a) return;
    a = old;   // a had a parent by now: whatever was cut off by the min is joined again through (old, b)
  }
}

// Falling size, then rising root: the larger key ranks first.
__device__ __forceinline__ unsigned long long seg_key(int size, int root) {
  return ((unsigned long long)(unsigned)size << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)root);
}

// One workgroup of kSelectBlock threads, every thread calls it.  Up to kSelectBlock candidates (the usual case): thread i
// holds key i, its rank is the number of larger keys.  More: round k takes the largest key below the one of round k - 1 and
// the rounds stop when nothing is left.  Keys are distinct (distinct roots).  Entries past the number found are 0 / -1.
// s_key: kSelectBlock entries of LDS; s_best: one.
__device__ __forceinline__ void select_largest(const unsigned long long *__restrict__ cand, int m, int max_labels,
                                               int32_t *__restrict__ num_labels, int32_t *__restrict__ label_size,
                                               int32_t *__restrict__ label_root, unsigned long long *s_key,
                                               unsigned long long *s_best) {
  const int tid = threadIdx.x;
  int found = 0;
  if (m <= kSelectBlock) {
    const unsigned long long mine = tid < m ? cand[tid] : 0ull;
    s_key[tid] = mine;
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < m; ++j) rank += s_key[j] > mine ? 1 : 0;   // LDS broadcast reads
    if (tid < m && rank < max_labels) {
      label_size[rank] = (int32_t)(mine >> 32);
      label_root[rank] = (int32_t)(0xFFFFFFFFu - (unsigned)(mine & 0xFFFFFFFFull));
    }
    found = min(m, max_labels);
  } else {
    unsigned long long prev = ~0ull;   // no key reaches it: size <= 2^24
    for (int k = 0; k < max_labels; ++k) {
      unsigned long long best = 0ull;   // below every key: size >= 1
      for (int i = tid; i < m; i += kSelectBlock) {
        const unsigned long long c = cand[i];
        if (c < prev && c > best) best = c;
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
      }
      if ((tid & 63) == 0) s_key[tid >> 6] = best;
      __syncthreads();
      if (tid == 0) {
        unsigned long long b = 0ull;
        for (int wv = 0; wv < kSelectBlock / 64; ++wv) b = s_key[wv] > b ? s_key[wv] : b;
        *s_best = b;
      }
      __syncthreads();
      best = *s_best;   // uniform
      __syncthreads();
      if (!best) break;
      if (tid == 0) {
        label_size[k] = (int32_t)(best >> 32);
        label_root[k] = (int32_t)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
      }
      found = k + 1;
      prev = best;
    }
  }
  if (tid >= found && tid < max_labels) {   // max_labels <= 64 < kSelectBlock
    label_size[tid] = 0;
    label_root[tid] = -1;
  }
  if (tid == 0) *num_labels = found;
}

}  // namespace
