// The row LayerNorm of the embedding gathers: one table row per group of L = D/4 lanes (one float4
// per lane), moments by xor-shuffle inside the group.  Shared by gather_ln.hip (the forward
// gathers) and hour_bwd.hip (which recomputes the unscaled LN'd item rows in the backward of
// forward_simple(hour)), so both produce the same bits from the same table row.
#pragma once
#include "ncf_common.h"

// Every multiply and add below is its own IEEE operation (no fma contraction): which products the
// backend fuses depends on how the SLP vectoriser packed the float4 lanes, so kernels that hold
// one or two float4 per lane would otherwise round differently.  (The including file repeats
// the pragma for its own code.)
#pragma clang fp contract(off)

namespace {

template <int D>
struct RowLN {
  static constexpr int L = D / 4;
  __device__ __forceinline__ static float4 ln(float4 x, float4 g, float4 b, float eps) {
    float s = group_sum<L>(x.x + x.y + x.z + x.w);
    float mean = s * (1.0f / D);
    float4 c = make_float4(x.x - mean, x.y - mean, x.z - mean, x.w - mean);
    float q = group_sum<L>(c.x * c.x + c.y * c.y + c.z * c.z + c.w * c.w);
    float rstd = 1.0f / sqrtf(q * (1.0f / D) + eps);
    return make_float4(c.x * rstd * g.x + b.x, c.y * rstd * g.y + b.y, c.z * rstd * g.z + b.z,
                       c.w * rstd * g.w + b.w);
  }
};

// Out-of-range ids never touch memory out of bounds: they read row 0 and raise bit 0 of *err.
__device__ __forceinline__ int64_t safe_id(int64_t id, int64_t rows, int* err, bool report) {
  if (id < 0 || id >= rows) {
    if (err && report) atomicOr(err, 1);
    return 0;
  }
  return id;
}

}  // namespace
