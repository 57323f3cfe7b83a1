// la3d_draw.hpp - the device draw of the batched RANSAC fits: "index i of trial t of frame p" under a seed, shared by the scale fit of
// the depth alignment (la3d_align.hip, m = ceil(min_samples * n) indices per trial) and the plane fit (la3d_plane.hip, m = 3), so that
// la3d_align_ransac_subsets exports the rows of both.
#pragma once
#include "la3d_device.hpp"

namespace la3d {

// A keyed bijection of [0, n), so the images of 0..m-1 are m DISTINCT indices without
// any memory.  A balanced Feistel network of four rounds over 2 * half bits (the smallest even width that holds n) permutes
// [0, 4^half); images >= n walk on along their cycle until they are back inside [0, n) - fewer than four steps on average, and
// always finite because the cycle returns to i < n.  Counter-based: the key depends on (seed, p, t) only.  Not NumPy's stream.
__device__ inline unsigned long long ar_mix64(unsigned long long z) {   // the finaliser of splitmix64
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ inline unsigned ar_round(unsigned r, unsigned key) {
  unsigned h = r * 0x9E3779B1u + key;
  h ^= h >> 15; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}
// (i < n: an i outside [0, n) sits on a cycle that need not come back inside)
__device__ inline int ar_subset_index(unsigned long long seed, int p, int t, int n, int i) {
  unsigned long long z = ar_mix64(seed + 0x9E3779B97F4A7C15ull);
  z = ar_mix64(z ^ ((unsigned long long)(unsigned)p * 0xD1342543DE82EF95ull + 0x632BE59BD9B4E019ull));
  z = ar_mix64(z ^ ((unsigned long long)(unsigned)t * 0xDA942042E4DD58B5ull + 0x2545F4914F6CDD1Dull));
  const unsigned long long z2 = ar_mix64(z + 0x9E3779B97F4A7C15ull);
  const unsigned key[4] = {(unsigned)z, (unsigned)(z >> 32), (unsigned)z2, (unsigned)(z2 >> 32)};
  const int bits = n <= 2 ? 1 : 32 - __clz(n - 1);
  const int half = (bits + 1) >> 1;
  const unsigned mask = (1u << half) - 1u;
  unsigned v = (unsigned)i;
  do {
    unsigned l = v >> half, r = v & mask;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned nl = r;
      r = l ^ (ar_round(r, key[k]) & mask);
      l = nl;
    }
    v = (l << half) | r;
  } while (v >= (unsigned)n);
  return (int)v;
}

}  // namespace la3d
