// Stage 1 of the batched deterministic reductions (reduce.hip) as device code, and the launch
// arguments of both stages.  k_reduce_batch1 and the fused tail launch k_reduce1_catchup call
// the same reduce1_body, so the summation order of every output exists in exactly one place.
#pragma once
#include "ncf_common.h"

namespace ncf_reduce {
namespace {

constexpr int kPB = 64;          // partials per stage-1 chunk
constexpr int kMaxPerLaunch = 24; // descriptors per launch (kernel-argument size)

struct BatchArgs {
  ncf_reduce_desc d[kMaxPerLaunch];
  int64_t scr[kMaxPerLaunch];        // scratch offset (floats) of multi-chunk descriptors
  uint32_t first[kMaxPerLaunch + 1]; // first block of descriptor i (prefix over blocks)
  int32_t chunks[kMaxPerLaunch];
  int32_t vec[kMaxPerLaunch];        // 16-byte (four-column) lanes
  int32_t count;
};

__device__ __forceinline__ int find_desc(const BatchArgs& a, uint32_t b) {
  int i = 0;
  while (i + 1 < a.count && a.first[i + 1] <= b) ++i;
  return i;
}

__device__ __forceinline__ void store_out(const ncf_reduce_desc& d, int64_t i, float t) {
  float* o = d.out + (i / d.cols) * d.ldo + (i % d.cols);
  const float v = d.scale * t;
  *o = d.accumulate ? *o + v : v;
}

template <typename T> __device__ __forceinline__ T zero();
template <> __device__ __forceinline__ float zero<float>() { return 0.0f; }
template <> __device__ __forceinline__ float4 zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// Stage-1 sum of wave w's partials (rows pb + w, pb + w + 4, ... < pe) at element(s) i: T = float
// (one column per lane) or float4 (four adjacent columns per lane, 16-byte loads: each column's
// additions are the scalar form's, in the same order — the same bits).
// NB: loads in flight per thread in the full-chunk loop (16; 4 in the fused tail launch, which
// must fit 64 registers); the additions and their order do not depend on it.
template <typename T, int NB = 16>
__device__ __forceinline__ T stage1_sum(const float* __restrict__ part, int64_t stride, int64_t i,
                                        int pb, int pe, int w) {
  T a0 = zero<T>(), a1 = zero<T>(), a2 = zero<T>(), a3 = zero<T>();
  int p = pb + w;
  // 16 loads in flight per thread (a full 64-partial chunk in one batch), summed in the order
  // of the loop below (accumulator j % 4 takes partial p + 4j): the same bits, without the
  // four dependent rounds of HBM latency
  for (; p + 60 < pe; p += 64) {
#pragma unroll
    for (int h = 0; h < 16; h += NB) {
      T v[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j)
        v[j] = *(const T*)(part + (int64_t)(p + 4 * (h + j)) * stride + i);
#pragma unroll
      for (int j = 0; j < NB; j += 4) {
        a0 += v[j];
        a1 += v[j + 1];
        a2 += v[j + 2];
        a3 += v[j + 3];
      }
    }
  }
  for (; p + 12 < pe; p += 16) {
    a0 += *(const T*)(part + (int64_t)p * stride + i);
    a1 += *(const T*)(part + (int64_t)(p + 4) * stride + i);
    a2 += *(const T*)(part + (int64_t)(p + 8) * stride + i);
    a3 += *(const T*)(part + (int64_t)(p + 12) * stride + i);
  }
  for (; p < pe; p += 4) a0 += *(const T*)(part + (int64_t)p * stride + i);
  return (a0 + a1) + (a2 + a3);
}

// Stage-1 block `block` of the launch group a (256 threads; red: 4 x 64 float4 of LDS): one
// block per (descriptor, 64 lanes of columns, chunk of <= 64 partials); a descriptor flagged vec
// (a.vec: L, stride and the partial base 16-byte multiples) takes four columns per lane — 256
// per block, 16-byte loads (stage 1 streams the batch's ~76 MB of weight-gradient partial sets
// at C2: the wide loads carry it nearer the HBM rate).
template <int NB = 16>
__device__ __forceinline__ void reduce1_body(const BatchArgs& a, float* __restrict__ scratch,
                                             uint32_t block, float4 (*red)[64]) {
  const int di = find_desc(a, block);
  const ncf_reduce_desc& d = a.d[di];
  const int ch = a.chunks[di];
  const bool vec = a.vec[di] != 0;
  const int vw = vec ? 4 : 1;
  const uint32_t local = block - a.first[di];
  const uint32_t gx = (uint32_t)((d.L + 64 * vw - 1) / (64 * vw));
  const int64_t i = ((int64_t)(local % gx) * 64 + (threadIdx.x & 63)) * vw;
  const int y = (int)(local / gx);
  const int w = threadIdx.x >> 6;
  const int l = threadIdx.x & 63;
  const int pb = ch > 1 ? y * kPB : 0;
  const int pe = ch > 1 ? min(d.P, pb + kPB) : d.P;
  if (vec) {
    float4 s = zero<float4>();
    if (i < d.L) s = stage1_sum<float4, NB>(d.part, d.stride, i, pb, pe, w);
    red[w][l] = s;
    __syncthreads();
    if (w == 0 && i < d.L) {
      const float4 t = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
      if (ch > 1) {
        *(float4*)(scratch + a.scr[di] + (int64_t)y * d.L + i) = t;
      } else {
        store_out(d, i, t.x);
        store_out(d, i + 1, t.y);
        store_out(d, i + 2, t.z);
        store_out(d, i + 3, t.w);
      }
    }
    return;
  }
  float s = 0.0f;
  if (i < d.L) s = stage1_sum<float, NB>(d.part, d.stride, i, pb, pe, w);
  red[w][l].x = s;
  __syncthreads();
  if (w == 0 && i < d.L) {
    const float t = (red[0][l].x + red[1][l].x) + (red[2][l].x + red[3][l].x);
    if (ch > 1) scratch[a.scr[di] + (int64_t)y * d.L + i] = t;
    else store_out(d, i, t);
  }
}

}  // namespace
}  // namespace ncf_reduce
