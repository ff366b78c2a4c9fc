// Device helpers shared by the top-K kernels (score.hip, neighbors.hip): the order-preserving
// image of a float, the 64-bit selection key built on it, and the in-LDS bitonic sort.
#pragma once
#include "ncf_common.h"

__device__ __forceinline__ uint32_t fkey(float f) {  // order-preserving float -> uint32
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// in-LDS bitonic sort of n2 (a power of two) keys, descending; the whole block participates
__device__ __forceinline__ void bitonic_desc(unsigned long long* keys, int n2) {
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int j = threadIdx.x; j < n2; j += blockDim.x) {
        const int p = j ^ stride;
        if (p > j) {
          const bool desc = (j & size) == 0;
          const unsigned long long x = keys[j], y = keys[p];
          if ((x < y) == desc) { keys[j] = y; keys[p] = x; }
        }
      }
      __syncthreads();
    }
  }
}

// The same sort of several lists at once: list l of `nlist` is the n2 (a power of two, <= SEG)
// keys at keys + list[l] * SEG, each sorted descending on its own (the last merge of every list
// runs downwards, where one sort of the whole array would alternate).  The whole block
// participates.  A thread takes U compare-exchanges of a stage at a time and issues their loads
// together (the pairs of a stage are disjoint): one at a time (load, compare, store, next) the
// sort is a chain of LDS latencies, which four waves on a CU do not hide.
template <int SEG, int U>
__device__ __forceinline__ void bitonic_stage(unsigned long long* keys, const int* list, int npairs,
                                              int half, int lg, int n2, int size, int stride) {
  for (int t0 = threadIdx.x; t0 < npairs; t0 += blockDim.x * U) {
    unsigned long long x[U], y[U];
    int a[U];
    bool swap[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {   // (unconditional loads: a thread past the end re-reads pair 0)
      const int t = t0 + u * blockDim.x;
      const bool ok = t < npairs;
      const int tt = ok ? t : 0;
      const int r = tt & (half - 1);
      const int j = ((r & ~(stride - 1)) << 1) | (r & (stride - 1));   // (bit `stride` clear)
      a[u] = list[tt >> lg] * SEG + j;
      x[u] = keys[a[u]];
      y[u] = keys[a[u] + stride];
      swap[u] = ok && (x[u] < y[u]) == ((j & size & (n2 - 1)) == 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (swap[u]) {
        keys[a[u]] = y[u];
        keys[a[u] + stride] = x[u];
      }
  }
}

template <int SEG>
__device__ __forceinline__ void bitonic_desc_lists(unsigned long long* keys, const int* list,
                                                   int nlist, int n2) {
  const int half = n2 >> 1;
  if (half < 1) return;            // (lists of one key)
  const int lg = __ffs(half) - 1;
  const int npairs = nlist * half;
  const bool few = npairs <= (int)blockDim.x;   // (a pair per thread: nothing to batch)
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (few) bitonic_stage<SEG, 1>(keys, list, npairs, half, lg, n2, size, stride);
      else bitonic_stage<SEG, 4>(keys, list, npairs, half, lg, n2, size, stride);
      __syncthreads();
    }
  }
}
