// The Adam element update of every table / flat-parameter kernel (adam.hip) and of the fused
// embedding-backward + apply (embedding_bwd.hip): one definition, so every schedule takes the
// same bits.  torch.optim.Adam semantics (src/model/trainer.py:71-75, :285); see adam.hip.
#pragma once
#include <cmath>
#include <type_traits>
#include "ncf_common.h"

namespace ncf_adam {
namespace {

struct AdamScalars {
  float neg_step, w1, b2, c2, inv_bc2_sqrt, eps, wd;   // (wd: see scalars_dw, adam.hip)
  float b1, k1, k2;   // zero-gradient step: beta1, (1-beta1) wd, (1-beta2) wd^2
  float ra, rb;       // zero-gradient step s: inv_bc2_sqrt / neg_step, eps / neg_step
};

// One Adam element update, written as explicit fmas with the hardware square root and
// reciprocal (v_sqrt_f32 / v_rcp_f32, ~1 ulp) and 1/sqrt(1-b2^t) folded on the host:
//   g' = g + wd*p;  m += (1-b1)(g' - m);  v = b2 v + (1-b2) g'^2
//   p += (-lr/(1-b1^t)) * m * 1/(sqrt(v) * 1/sqrt(1-b2^t) + eps)
// 11 VALU ops (2 transcendental) per element-step.  Every kernel that applies a step (dense
// sweep, deferred catch-up, touched-row apply) calls this one function with the same fp32
// scalars, so the deferred schedule reproduces the dense schedule bit for bit; against torch's
// correctly rounded CPU Adam the difference is ~1 ulp of the step (parity tests: abs 1e-6).
__device__ __forceinline__ void adam1(float& p, float& m, float& v, float g, float neg_step,
                                      float inv_bc, const AdamScalars& s) {
  g = __builtin_fmaf(s.wd, p, g);
  m = __builtin_fmaf(s.w1, g - m, m);
  v = __builtin_fmaf(s.c2 * g, g, v * s.b2);
  const float denom = __builtin_fmaf(__builtin_amdgcn_sqrtf(v), inv_bc, s.eps);
  p = __builtin_fmaf(neg_step * m, __builtin_amdgcn_rcpf(denom), p);
}

// The step of an element whose gradient is zero (an untouched table row: weight decay only),
// the same update with the constants folded (9 VALU ops, 2 transcendental, instead of 11):
//   m = b1 m + ((1-b1) wd) p;   v = b2 v + ((1-b2) wd^2) p p
//   p += m / (sqrt(v) ra + rb),   ra = inv_bc2_sqrt / neg_step, rb = eps / neg_step
// Used by every schedule for exactly the untouched elements (the dense sweep for rows without a
// gradient slot, the deferred replay for the zero-gradient steps it owes), so the schedules stay
// bit-identical to each other; against torch's Adam it differs by rounding (~1 ulp of m, v).
__device__ __forceinline__ void adam0(float& p, float& m, float& v, float ra, float rb,
                                      const AdamScalars& s) {
  m = __builtin_fmaf(s.b1, m, s.k1 * p);
  v = __builtin_fmaf(s.k2 * p, p, v * s.b2);
  const float den = __builtin_fmaf(__builtin_amdgcn_sqrtf(v), ra, rb);
  p = __builtin_fmaf(m, __builtin_amdgcn_rcpf(den), p);
}

__device__ __forceinline__ void adam1(float& p, float& m, float& v, float g, const AdamScalars& s) {
  adam1(p, m, v, g, s.neg_step, s.inv_bc2_sqrt, s);
}

__device__ __forceinline__ void adam4(float4& p, float4& m, float4& v, float4 g, float ns,
                                      float bc, const AdamScalars& s) {
  adam1(p.x, m.x, v.x, g.x, ns, bc, s);
  adam1(p.y, m.y, v.y, g.y, ns, bc, s);
  adam1(p.z, m.z, v.z, g.z, ns, bc, s);
  adam1(p.w, m.w, v.w, g.w, ns, bc, s);
}

__device__ __forceinline__ void adam4(float4& p, float4& m, float4& v, float4 g, const AdamScalars& s) {
  adam4(p, m, v, g, s.neg_step, s.inv_bc2_sqrt, s);
}

// ---- decoupled weight decay (torch.optim.AdamW; NCF_ADAM_DECOUPLED) -----------------------
// The decay multiplies the parameter before the Adam term is added (torch: param.mul_(1 - lr wd),
// then addcdiv_) and no wd term enters g, m or v:
//   m += (1-b1)(g - m);  v = b2 v + (1-b2) g^2;  p = fma(ns m, rcp(sqrt(v) ibc + eps), p dk)
// dk = (float)(1 - lr wd) of that step (decay_of), a per-step scalar beside ns / ibc / ra / rb.
__device__ __forceinline__ void adamw1(float& p, float& m, float& v, float g, float neg_step,
                                       float inv_bc, float dk, const AdamScalars& s) {
  m = __builtin_fmaf(s.w1, g - m, m);
  v = __builtin_fmaf(s.c2 * g, g, v * s.b2);
  const float denom = __builtin_fmaf(__builtin_amdgcn_sqrtf(v), inv_bc, s.eps);
  p = __builtin_fmaf(neg_step * m, __builtin_amdgcn_rcpf(denom), p * dk);
}

// The zero-gradient step (8 VALU ops, 2 transcendental): m = b1 m; v = b2 v;
//   p = fma(m, rcp(sqrt(v) ra + rb), p dk)
// A never-touched element (m == v == 0) keeps m == v == 0 and takes p = p dk exactly (0 * rcp(rb)
// is a zero: rb is finite and nonzero, -3e38 at lr == 0).
__device__ __forceinline__ void adamw0(float& p, float& m, float& v, float ra, float rb, float dk,
                                       const AdamScalars& s) {
  m = s.b1 * m;
  v = v * s.b2;
  const float den = __builtin_fmaf(__builtin_amdgcn_sqrtf(v), ra, rb);
  p = __builtin_fmaf(m, __builtin_amdgcn_rcpf(den), p * dk);
}

// The element update of a kernel instantiated for one decay rule (DW: decoupled).  A compile-time
// choice: the coupled instantiations are adam1 / adam0 as they stand (dk unused, no multiply).
template <bool DW>
__device__ __forceinline__ void step1(float& p, float& m, float& v, float g, float ns, float bc,
                                      float dk, const AdamScalars& s) {
  if (DW) adamw1(p, m, v, g, ns, bc, dk, s);
  else adam1(p, m, v, g, ns, bc, s);
}

template <bool DW>
__device__ __forceinline__ void step0(float& p, float& m, float& v, float ra, float rb, float dk,
                                      const AdamScalars& s) {
  if (DW) adamw0(p, m, v, ra, rb, dk, s);
  else adam0(p, m, v, ra, rb, s);
}

template <bool DW>
__device__ __forceinline__ void step4(float4& p, float4& m, float4& v, float4 g, float ns,
                                      float bc, float dk, const AdamScalars& s) {
  step1<DW>(p.x, m.x, v.x, g.x, ns, bc, dk, s);
  step1<DW>(p.y, m.y, v.y, g.y, ns, bc, dk, s);
  step1<DW>(p.z, m.z, v.z, g.z, ns, bc, dk, s);
  step1<DW>(p.w, m.w, v.w, g.w, ns, bc, dk, s);
}

// floats per step of the per-step scalar table a kernel reads: 4 (ncf_adam_step_scalars) or
// NCF_ADAMW_TABLE_STRIDE with the step's decay at index 4 (include/ncf_hip.h)
constexpr int step_stride(bool dw) { return dw ? NCF_ADAMW_TABLE_STRIDE : 4; }

// ---- the row variant of a table kernel -----------------------------------------------------
// What the rows of a table are and how they step: fp32 rows, bf16 rows rounded to nearest even
// or stochastically after every step they take, fp32 rows under decoupled weight decay.  These
// four exist (ncf_table_pair's param_dtype, include/ncf_hip.h); a table kernel is instantiated
// per variant, <int D, Rows V>, and reads the variant's properties from RowTraits<V>.
enum class Rows : int { F32, BF16, BF16_SR, F32_DW };

template <Rows V>
struct RowTraits {
  static constexpr bool BF = V == Rows::BF16 || V == Rows::BF16_SR;   // the parameter is bf16
  static constexpr bool SR = V == Rows::BF16_SR;                       // ... rounded stochastically
  static constexpr bool DW = V == Rows::F32_DW;                        // decoupled weight decay
  static constexpr int TS = step_stride(DW);                           // step table stride
};

// Host dispatch: f(tag) with the compile-time tag (tag() == v) of the one variant among Vs that
// v names; false, and no call, if it names none of them.
//   for_rows<Rows::F32, Rows::BF16>(v, [&](auto V) { hipLaunchKernelGGL((k<D, V()>), ...); });
template <Rows V>
using RowsTag = std::integral_constant<Rows, V>;

template <Rows... Vs, class F>
inline bool for_rows(Rows v, F&& f) {
  return ((v == Vs && (f(RowsTag<Vs>{}), true)) || ...);
}

template <class F>
inline void for_any_rows(Rows v, F&& f) {
  for_rows<Rows::F32, Rows::BF16, Rows::BF16_SR, Rows::F32_DW>(v, f);
}

// The variant n table pairs name, or NCF_ERR_ARG (the error names `who`, the entry point called):
// a param_dtype this build knows (NCF_DTYPE_*; NCF_ADAM_DECOUPLED with fp32 rows only), the same
// in every pair, as round_seed is.
inline int rows_of(const char* who, const ncf_table_pair* p, int n, Rows* out) {
  for (int k = 1; k < n; ++k)
    NCF_CHECK_ARG(p[k].param_dtype == p[0].param_dtype && p[k].round_seed == p[0].round_seed,
                  "%s: param_dtype (the pairs differ)", who);
  switch (p[0].param_dtype) {
    case NCF_DTYPE_F32: *out = Rows::F32; return NCF_OK;
    case NCF_DTYPE_BF16: *out = Rows::BF16; return NCF_OK;
    case NCF_DTYPE_BF16_SR: *out = Rows::BF16_SR; return NCF_OK;
    case NCF_DTYPE_F32 | NCF_ADAM_DECOUPLED: *out = Rows::F32_DW; return NCF_OK;
  }
  ncf_set_error("%s: param_dtype %d", who, (int)p[0].param_dtype);
  return NCF_ERR_ARG;
}

inline float decay_of(double lr, double wd) { return (float)(1.0 - lr * wd); }

inline AdamScalars make_scalars(double lr, double beta1, double beta2, double eps, double wd, double step) {
  AdamScalars s;
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  s.neg_step = (float)(-(lr / bc1));
  s.w1 = (float)(1.0 - beta1);
  s.b2 = (float)beta2;
  s.c2 = (float)(1.0 - beta2);
  s.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  s.eps = (float)eps;
  s.wd = (float)wd;
  s.b1 = (float)beta1;
  s.k1 = (float)((1.0 - beta1) * wd);
  s.k2 = (float)((1.0 - beta2) * wd * wd);
  // zero-gradient form: ns folded into the denominator (lr == 0: a finite huge denominator, the
  // step vanishes instead of 0 * inf)
  const double ns = -(lr / bc1);
  s.ra = ns != 0.0 ? (float)((1.0 / sqrt(bc2)) / ns) : -3.0e38f;
  s.rb = ns != 0.0 ? (float)(eps / ns) : -3.0e38f;
  return s;
}

inline AdamScalars consts_of(double beta1, double beta2, double eps, double wd) {
  AdamScalars s = make_scalars(1.0, beta1, beta2, eps, wd, 1.0);
  s.neg_step = 0.f;
  s.inv_bc2_sqrt = 1.f;
  return s;
}

}  // namespace
}  // namespace ncf_adam
