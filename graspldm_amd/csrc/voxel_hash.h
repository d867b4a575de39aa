// voxel_hash.h -- the per-cloud hash table on an origin-anchored lattice that cloud_downsample.hip (gldm_voxel_downsample)
// and cloud_cluster.hip (gldm_cluster_cloud) share: a cell is three signed 21-bit lattice coordinates packed into one 64-bit
// key; cloud i owns a region of 2 slots per row (load factor <= 1/2); linear probing from a hash of the key; a slot is taken
// by compare-and-swap on its key.  A slot type is any struct whose first member is `unsigned long long key`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr double kCellLimit = 1048576.0;   // 2^20: cells lie in [-2^20, 2^20 - 1]

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// 3 x 21 bits of cell + 2^20 (bit 63 clear, so no key equals kEmptyKey); every cell in [-2^20, 2^20 - 1]
__device__ __forceinline__ unsigned long long cell_key(long long cx, long long cy, long long cz) {
  return ((unsigned long long)(cx + (1 << 20)) << 42) | ((unsigned long long)(cy + (1 << 20)) << 21) |
         (unsigned long long)(cz + (1 << 20));
}

// The slot of `key` in region[0 .. len), taking an empty one if the key has none yet; -1 if the region is full of other keys
// (impossible at 2 slots per row).  The loop ends within `len` probes whatever the table holds.
template <typename S>
__device__ __forceinline__ long long hash_insert(S *region, unsigned len, unsigned long long key) {
  unsigned at = (unsigned)(mix64(key) % len);
  for (unsigned probe = 0; probe < len; ++probe) {
    const unsigned long long seen = atomicCAS(&region[at].key, kEmptyKey, key);
    if (seen == kEmptyKey || seen == key) return (long long)at;
    at = at + 1 == len ? 0 : at + 1;
  }
  return -1;
}

// The slot of `key` in a table that no one inserts into any more (an earlier launch built it); -1 if the key is absent.
template <typename S>
__device__ __forceinline__ long long hash_find(const S *region, unsigned len, unsigned long long key) {
  unsigned at = (unsigned)(mix64(key) % len);
  for (unsigned probe = 0; probe < len; ++probe) {
    const unsigned long long seen = region[at].key;
    if (seen == key) return (long long)at;
    if (seen == kEmptyKey) return -1;
    at = at + 1 == len ? 0 : at + 1;
  }
  return -1;
}

}  // namespace
