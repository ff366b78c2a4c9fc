// Multi-head attention core with a key/value length that differs from the query length.
//
// Reference: MultiHeadAttention.forward, src/model/architecture.py:35-57.  It reshapes q, k and v
// each with .view(batch, -1, H, hd), so the key length L_k is free of the query length L_q; its
// second instance, sequence_attention (:210-214), is meant for one query over a user's item
// history (config/config.yaml:202 max_sequence_length: 50).  attention.hip (one lane per query
// row, scores in registers) is the L_q == L_k core of the training step; at L_q = 1 it would run
// groups*H lanes of 64 scores each.  Here:
//
//   one wave64 per (group, head); lane j owns key j (L_k <= 64), lane d owns column d (hd <= 64).
//
// The head's K and V slices [L_k, hd] are staged once per wave in LDS with a row stride of
// hd + 1 dwords: the row-wise read (lane = key, fixed d) walks banks with an odd stride and the
// column-wise read (lane = d, fixed key) walks consecutive banks, so neither conflicts.  A query
// row (and its dO row in the backward) lives one column per lane and reaches the other lanes
// through v_readlane (a wave-uniform operand of the FMA), probabilities the same way.  Every
// wave works on its own LDS slice: there is no workgroup barrier, and a wave past groups*H exits
// before any LDS or global access.
//
// Layout: Q, O, dQ [groups*L_q, D]; K, V, dK, dV [groups*L_k, D]; head h owns columns
// [h*hd, (h+1)*hd).  P (pre-dropout softmax, saved for the backward) and the optional mask
// (bytes, 0 = masked) are [groups, H, L_q, L_k].  Dropout element ((b*H + h)*L_q + i)*L_k + j of
// the ncf_dropout_scale stream: attention.hip's index when L_q == L_k.  A masked score is -inf
// before the softmax (probability exactly 0: the backward needs no mask); a fully masked row is
// NaN, as torch's softmax over all -inf makes it.  The per-score arithmetic (FMA order over d and
// over j) is attention.hip's; the softmax row sum and the backward's sum P dP are wave
// reductions (xor butterflies: a fixed order, bitwise reproducible).
//
// Backward: one launch.  Lane j keeps dK_j and dV_j [hd] in registers and accumulates them over
// the queries i = 0 .. L_q - 1 in ascending order; dS never leaves the wave.  No atomics.
#include "ncf_common.h"

#include <limits.h>

namespace {

// waves per workgroup: the dynamic LDS of a workgroup, NW * 2 * L_k * (hd + 1) dwords, stays
// below 64 KB at L_k = 64 (hd 64: 33,280 B; hd 32: 33,792 B; hd 16: 34,816 B; hd 8: 18,432 B)
template <int HD>
struct XCfg {
  static constexpr int NW = HD >= 64 ? 1 : (HD == 32 ? 2 : 4);
  static constexpr int LDR = HD + 1;   // LDS row stride in dwords
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// the value lane `src` holds (src wave-uniform): an SGPR operand, no LDS round trip
__device__ __forceinline__ float lane_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// rows [0, L) x columns [0, HD) of a head slice (global row stride D) <-> LDS [L][HD + 1]
template <int HD>
__device__ __forceinline__ void stage_in(const float* __restrict__ src, int L, int D, float* dst,
                                         int lane) {
  for (int e = lane; e < L * HD; e += NCF_WAVE) {
    const int j = e / HD, d = e % HD;
    dst[j * XCfg<HD>::LDR + d] = src[(int64_t)j * D + d];
  }
}

template <int HD>
__device__ __forceinline__ void stage_out(const float* src, int L, int D, float* __restrict__ dst,
                                          int lane) {
  for (int e = lane; e < L * HD; e += NCF_WAVE) {
    const int j = e / HD, d = e % HD;
    dst[(int64_t)j * D + d] = src[j * XCfg<HD>::LDR + d];
  }
}

template <int HD>
__global__ __launch_bounds__(XCfg<HD>::NW * NCF_WAVE) void k_attn_x_fwd(
    const float* __restrict__ Q, const float* __restrict__ Kt, const float* __restrict__ V,
    int64_t BH, int Lq, int Lk, int H, float scale, float p_drop, uint64_t seed,
    const ncf_step_clock* clock, const uint8_t* __restrict__ mask, float* __restrict__ P,
    float* __restrict__ O) {
  constexpr int LDR = XCfg<HD>::LDR;
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t bh = (int64_t)blockIdx.x * XCfg<HD>::NW + wv;
  if (bh >= BH) return;
  if (clock) seed += clock->seed;  // per-step stream of a captured step
  const int h = (int)(bh % H);
  const int64_t b = bh / H;
  const int D = H * HD;
  float* Ks = lds + (size_t)wv * 2 * Lk * LDR;
  float* Vs = Ks + Lk * LDR;
  stage_in<HD>(Kt + b * Lk * D + h * HD, Lk, D, Ks, lane);
  stage_in<HD>(V + b * Lk * D + h * HD, Lk, D, Vs, lane);
  wave_lds_sync();
  const bool key = lane < Lk, col = lane < HD;
  const float* krow = Ks + (key ? lane : 0) * LDR;   // lanes past L_k read row 0, use nothing
  const float inv_keep = p_drop > 0.0f ? 1.0f / (1.0f - p_drop) : 1.0f;
  for (int i = 0; i < Lq; ++i) {
    const int64_t row = bh * Lq + i;
    const int64_t qoff = (b * Lq + i) * D + h * HD + lane;
    const float qd = col ? Q[qoff] : 0.0f;
    float acc = 0.0f;
#pragma unroll
    for (int d = 0; d < HD; ++d) acc = fmaf(lane_bcast(qd, d), krow[d], acc);
    float s = -INFINITY;
    if (key) {
      s = acc / scale;
      if (mask && mask[row * Lk + lane] == 0) s = -INFINITY;
    }
    const float mx = wave_max(s);
    float e = 0.0f;
    if (key) e = mx == -INFINITY ? NAN : expf(s - mx);
    const float sum = wave_sum(e);
    float pd = 0.0f;
    if (key) {
      const float pj = e / sum;
      P[row * Lk + lane] = pj;
      pd = p_drop > 0.0f
               ? pj * ncf_dropout_scale(seed, (uint64_t)row * Lk + lane, p_drop, inv_keep)
               : pj;
    }
    float o = 0.0f;
    const float* vcol = Vs + (col ? lane : 0);
    for (int j = 0; j < Lk; ++j) o = fmaf(lane_bcast(pd, j), vcol[j * LDR], o);
    if (col) O[qoff] = o;
  }
}

template <int HD>
__global__ __launch_bounds__(XCfg<HD>::NW * NCF_WAVE) void k_attn_x_bwd(
    const float* __restrict__ Q, const float* __restrict__ Kt, const float* __restrict__ V,
    const float* __restrict__ P, const float* __restrict__ dO, int64_t BH, int Lq, int Lk, int H,
    float scale, float p_drop, uint64_t seed, const ncf_step_clock* clock,
    float* __restrict__ dQ, float* __restrict__ dK, float* __restrict__ dV) {
  constexpr int LDR = XCfg<HD>::LDR;
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t bh = (int64_t)blockIdx.x * XCfg<HD>::NW + wv;
  if (bh >= BH) return;
  if (clock) seed += clock->seed;  // per-step stream of a captured step
  const int h = (int)(bh % H);
  const int64_t b = bh / H;
  const int D = H * HD;
  float* Ks = lds + (size_t)wv * 2 * Lk * LDR;
  float* Vs = Ks + Lk * LDR;
  stage_in<HD>(Kt + b * Lk * D + h * HD, Lk, D, Ks, lane);
  stage_in<HD>(V + b * Lk * D + h * HD, Lk, D, Vs, lane);
  wave_lds_sync();
  const bool key = lane < Lk, col = lane < HD;
  const int jrow = (key ? lane : 0) * LDR;   // lanes past L_k read row 0, use nothing
  const int dcol = col ? lane : 0;
  const float inv_keep = p_drop > 0.0f ? 1.0f / (1.0f - p_drop) : 1.0f;
  float dk[HD], dv[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) { dk[d] = 0.0f; dv[d] = 0.0f; }
  for (int i = 0; i < Lq; ++i) {
    const int64_t row = bh * Lq + i;
    const int64_t qoff = (b * Lq + i) * D + h * HD + lane;
    const float gd = col ? dO[qoff] : 0.0f;
    const float qd = col ? Q[qoff] : 0.0f;
    float dp = 0.0f;
#pragma unroll
    for (int d = 0; d < HD; ++d) dp = fmaf(lane_bcast(gd, d), Vs[jrow + d], dp);
    float pj = 0.0f, keep = 1.0f;
    if (key) {
      pj = P[row * Lk + lane];
      if (p_drop > 0.0f) keep = ncf_dropout_scale(seed, (uint64_t)row * Lk + lane, p_drop, inv_keep);
    }
    dp *= keep;
    const float tsum = wave_sum(key ? pj * dp : 0.0f);
    const float ds = key ? pj * (dp - tsum) : 0.0f;
    const float pd = pj * keep;
    float dq = 0.0f;
    for (int j = 0; j < Lk; ++j) dq = fmaf(lane_bcast(ds, j), Ks[j * LDR + dcol], dq);
    if (col) dQ[qoff] = dq / scale;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      dk[d] = fmaf(ds, lane_bcast(qd, d), dk[d]);
      dv[d] = fmaf(pd, lane_bcast(gd, d), dv[d]);
    }
  }
  // dK, dV rows out through the wave's LDS slice (K and V are no longer needed): coalesced stores
  wave_lds_sync();
  if (key) {
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      Ks[jrow + d] = dk[d] / scale;
      Vs[jrow + d] = dv[d];
    }
  }
  wave_lds_sync();
  stage_out<HD>(Ks, Lk, D, dK + b * Lk * D + h * HD, lane);
  stage_out<HD>(Vs, Lk, D, dV + b * Lk * D + h * HD, lane);
}

template <int HD>
int x_fwd(const float* q, const float* k, const float* v, int64_t BH, int Lq, int Lk, int H,
          float p, uint64_t seed, const ncf_step_clock* clock, const uint8_t* mask, float* P,
          float* O, hipStream_t st) {
  constexpr int NW = XCfg<HD>::NW;
  const size_t lds = (size_t)NW * 2 * Lk * XCfg<HD>::LDR * sizeof(float);
  hipLaunchKernelGGL((k_attn_x_fwd<HD>), dim3(ncf_cdiv(BH, NW)), dim3(NW * NCF_WAVE), lds, st, q, k,
                     v, BH, Lq, Lk, H, sqrtf((float)HD), p, seed, clock, mask, P, O);
  NCF_CHECK_LAUNCH("ncf_attention_x_fwd");
  return NCF_OK;
}

template <int HD>
int x_bwd(const float* q, const float* k, const float* v, const float* P, const float* dO,
          int64_t BH, int Lq, int Lk, int H, float p, uint64_t seed, const ncf_step_clock* clock,
          float* dQ, float* dK, float* dV, hipStream_t st) {
  constexpr int NW = XCfg<HD>::NW;
  const size_t lds = (size_t)NW * 2 * Lk * XCfg<HD>::LDR * sizeof(float);
  hipLaunchKernelGGL((k_attn_x_bwd<HD>), dim3(ncf_cdiv(BH, NW)), dim3(NW * NCF_WAVE), lds, st, q, k,
                     v, P, dO, BH, Lq, Lk, H, sqrtf((float)HD), p, seed, clock, dQ, dK, dV);
  NCF_CHECK_LAUNCH("ncf_attention_x_bwd");
  return NCF_OK;
}

}  // namespace

#define NCF_X_CHECK_SHAPE(name)                                                                   \
  NCF_CHECK_ARG(groups >= 0 && len_q >= 1 && len_q <= 64 && len_k >= 1 && len_k <= 64 &&          \
                    heads >= 1 && dim >= heads && dim % heads == 0 &&                             \
                    groups <= (int64_t)INT_MAX / heads,                                           \
                name ": bad shape (groups=%lld Lq=%lld Lk=%lld H=%lld D=%lld; 1<=Lq,Lk<=64)",     \
                (long long)groups, (long long)len_q, (long long)len_k, (long long)heads,          \
                (long long)dim);                                                                  \
  NCF_CHECK_ARG(dropout_p >= 0.0f && dropout_p < 1.0f, name ": dropout_p out of [0,1)")

extern "C" int ncf_attention_x_fwd(const float* q, const float* k, const float* v, int64_t groups,
                                   int64_t len_q, int64_t len_k, int64_t heads, int64_t dim,
                                   float dropout_p, uint64_t seed, const ncf_step_clock* clock,
                                   const uint8_t* mask, float* probs, float* out, void* stream) {
  NCF_X_CHECK_SHAPE("ncf_attention_x_fwd");
  const int64_t hd = dim / heads;
  NCF_CHECK_ARG(hd == 8 || hd == 16 || hd == 32 || hd == 64,
                "ncf_attention_x_fwd: head dim %lld unsupported (8/16/32/64)", (long long)hd);
  if (groups == 0) return NCF_OK;
  NCF_CHECK_ARG(q && k && v && probs && out, "ncf_attention_x_fwd: NULL buffer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t BH = groups * heads;
  const int Lq = (int)len_q, Lk = (int)len_k, H = (int)heads;
  switch (hd) {
    case 8: return x_fwd<8>(q, k, v, BH, Lq, Lk, H, dropout_p, seed, clock, mask, probs, out, st);
    case 16: return x_fwd<16>(q, k, v, BH, Lq, Lk, H, dropout_p, seed, clock, mask, probs, out, st);
    case 32: return x_fwd<32>(q, k, v, BH, Lq, Lk, H, dropout_p, seed, clock, mask, probs, out, st);
    default: return x_fwd<64>(q, k, v, BH, Lq, Lk, H, dropout_p, seed, clock, mask, probs, out, st);
  }
}

extern "C" int ncf_attention_x_bwd(const float* q, const float* k, const float* v,
                                   const float* probs, const float* grad_out, int64_t groups,
                                   int64_t len_q, int64_t len_k, int64_t heads, int64_t dim,
                                   float dropout_p, uint64_t seed, const ncf_step_clock* clock,
                                   float* grad_q, float* grad_k, float* grad_v, void* stream) {
  NCF_X_CHECK_SHAPE("ncf_attention_x_bwd");
  const int64_t hd = dim / heads;
  NCF_CHECK_ARG(hd == 8 || hd == 16 || hd == 32 || hd == 64,
                "ncf_attention_x_bwd: head dim %lld unsupported (8/16/32/64)", (long long)hd);
  if (groups == 0) return NCF_OK;
  NCF_CHECK_ARG(q && k && v && probs && grad_out && grad_q && grad_k && grad_v,
                "ncf_attention_x_bwd: NULL buffer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t BH = groups * heads;
  const int Lq = (int)len_q, Lk = (int)len_k, H = (int)heads;
  switch (hd) {
    case 8: return x_bwd<8>(q, k, v, probs, grad_out, BH, Lq, Lk, H, dropout_p, seed, clock, grad_q, grad_k, grad_v, st);
    case 16: return x_bwd<16>(q, k, v, probs, grad_out, BH, Lq, Lk, H, dropout_p, seed, clock, grad_q, grad_k, grad_v, st);
    case 32: return x_bwd<32>(q, k, v, probs, grad_out, BH, Lq, Lk, H, dropout_p, seed, clock, grad_q, grad_k, grad_v, st);
    default: return x_bwd<64>(q, k, v, probs, grad_out, BH, Lq, Lk, H, dropout_p, seed, clock, grad_q, grad_k, grad_v, st);
  }
}
