// Backward of forward_simple(user_ids, product_ids, hour) (src/model/architecture.py:409-485):
// what the hour path adds to the training backward.
//
//   te = hour_E[hour]                       (:434, :467)
//   tp = te W_p^T + b_p   (tp = te when temporal_dim == mf_embedding_dim)      (:436-442)
//   s  = 1 + f tp,  f = 0.3;  item rows  y_i (x) s  and  z_i (x) s             (:444, :456)
//
// ncf_item_scale_bwd: the head and the attention backward hand back g_imf, g_xi, the gradients
// w.r.t. the SCALED item rows.  The embedding backward wants them w.r.t. the unscaled LN'd rows
// (g (x) s, in place here) and the scale wants dtp = f (g_imf (x) y_i + g_xi (x) z_i).  y_i, z_i
// are recomputed from the item's two table rows with the gather's own row LayerNorm
// (row_ln_dev.h) — never recovered as (stashed scaled row) / s: s = 0 is an ordinary value
// (tp = -1/f).  Layout as the gather: D/4 lanes per row, one float4 each; out-of-range ids read
// row 0 and raise the flag, exactly as the gather does.
//
// ncf_hour_grad: dHourE[h] = sum over the batch rows of hour h of dte, dte = (tower layer 0's
// input gradient, columns D.., read in place at its leading dimension) (+ an optional second
// addend, the T == D scale gradient).  A two-stage ordered reduction, no float atomics: stage 1,
// one workgroup per NCF_HOUR_CHUNK consecutive batch rows, writes a [24, T] partial; stage 2 sums
// the partials in workgroup order.  Inside a workgroup the chunk's rows are dealt round-robin to
// R = 256 / T thread groups (thread = one column of one group, its own LDS accumulator per hour,
// rows in ascending order), and the R accumulators are summed in group order.  Every addition
// sequence of an output element involves only the rows of that element's hour, in an order fixed
// by (n, T): two runs are bitwise equal, and reordering the rows of one hour among themselves
// leaves every other hour's row bitwise unchanged.  Hours absent from the batch come out as 0.
#include "ncf_common.h"

#pragma clang fp contract(off)

#include "row_ln_dev.h"

// batch rows per stage-1 workgroup (mirrored by ops.HOUR_GRAD_CHUNK; tests/test_hour_bwd_golden.py)
#define NCF_HOUR_CHUNK 128

namespace {

constexpr int kHours = 24;

template <int D>
__global__ __launch_bounds__(256) void k_item_scale_bwd(
    const int64_t* __restrict__ iid, int64_t n, const float* __restrict__ mfI,
    const float* __restrict__ mlpI, int64_t nI, const float* __restrict__ g_mf,
    const float* __restrict__ b_mf, const float* __restrict__ g_mlp,
    const float* __restrict__ b_mlp, float eps, const float* __restrict__ item_scale, float f,
    float* __restrict__ g_imf, float* __restrict__ g_xi, float* __restrict__ dtp, int* err) {
  constexpr int L = D / 4;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = t / L;
  const int sub = (int)(t % L);
  if (row >= n) return;  // whole groups retire together
  const int64_t i = safe_id(iid[row], nI, err, sub == 0);
  const int c = sub * 4;
  const float4 yi = RowLN<D>::ln(ld4(mfI + i * D + c), ld4(g_mf + c), ld4(b_mf + c), eps);
  const float4 zi = RowLN<D>::ln(ld4(mlpI + i * D + c), ld4(g_mlp + c), ld4(b_mlp + c), eps);
  const float4 s4 = ld4(item_scale + row * D + c);
  const float4 m = make_float4(1.0f + f * s4.x, 1.0f + f * s4.y, 1.0f + f * s4.z, 1.0f + f * s4.w);
  const float4 ga = ld4(g_imf + row * D + c), gb = ld4(g_xi + row * D + c);
  st4(dtp + row * D + c, make_float4(f * (ga.x * yi.x + gb.x * zi.x), f * (ga.y * yi.y + gb.y * zi.y),
                                     f * (ga.z * yi.z + gb.z * zi.z), f * (ga.w * yi.w + gb.w * zi.w)));
  st4(g_imf + row * D + c, make_float4(ga.x * m.x, ga.y * m.y, ga.z * m.z, ga.w * m.w));
  st4(g_xi + row * D + c, make_float4(gb.x * m.x, gb.y * m.y, gb.z * m.z, gb.w * m.w));
}

template <int D>
int launch_item_scale_bwd(const int64_t* iid, int64_t n, const float* mfI, const float* mlpI,
                          int64_t nI, const float* g_mf, const float* b_mf, const float* g_mlp,
                          const float* b_mlp, float eps, const float* item_scale, float f,
                          float* g_imf, float* g_xi, float* dtp, int* err, hipStream_t st) {
  const int64_t threads = n * (D / 4);
  hipLaunchKernelGGL(k_item_scale_bwd<D>, dim3(ncf_cdiv(threads, 256)), dim3(256), 0, st, iid, n,
                     mfI, mlpI, nI, g_mf, b_mf, g_mlp, b_mlp, eps, item_scale, f, g_imf, g_xi, dtp,
                     err);
  NCF_CHECK_LAUNCH("ncf_item_scale_bwd");
  return NCF_OK;
}

// te[row] = hour_E[hour[row]] at any temporal width (ncf_gather_rows takes 16 / 32 / 64 / 128 / 256)
__global__ void k_hour_rows(const int64_t* __restrict__ hour, int64_t n,
                            const float* __restrict__ hE, int T, float* __restrict__ out,
                            int* err) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = t / T;
  const int c = (int)(t % T);
  if (row >= n) return;
  const int64_t h = safe_id(hour[row], kHours, err, c == 0);
  out[row * T + c] = hE[h * T + c];
}

// stage 1: part[blockIdx.x][h][c] = sum of the chunk's rows of hour h (see the file comment)
__global__ __launch_bounds__(256) void k_hour_grad_part(
    const int64_t* __restrict__ hour, int64_t n, const float* __restrict__ dte, int64_t ld,
    const float* __restrict__ add, int64_t ld_add, int T, float* __restrict__ part) {
  __shared__ float acc[kHours * 256];          // [R][24][T], R * T <= 256
  const int R = 256 / T;
  const int tid = threadIdx.x;
  const int r = tid / T, c = tid % T;
  const int64_t row0 = (int64_t)blockIdx.x * NCF_HOUR_CHUNK;
  const int rows = (int)min((int64_t)NCF_HOUR_CHUNK, n - row0);
  if (r < R) {
    float* mine = acc + (int64_t)r * kHours * T + c;
    for (int h = 0; h < kHours; ++h) mine[h * T] = 0.0f;
    for (int j = r; j < rows; j += R) {
      const int64_t row = row0 + j;
      const int64_t h = hour[row];
      if (h < 0 || h >= kHours) continue;      // (refused by the forward; never out of bounds)
      float v = dte[row * ld + c];
      if (add) v += add[row * ld_add + c];
      mine[h * T] += v;
    }
  }
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * kHours * T;
  for (int e = tid; e < kHours * T; e += 256) {
    float s = acc[e];
    for (int q = 1; q < R; ++q) s += acc[q * kHours * T + e];
    out[e] = s;
  }
}

// stage 2: out[e] = sum over the workgroups' partials, in workgroup order
__global__ void k_hour_grad_sum(const float* __restrict__ part, int P, int L,
                                float* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= L) return;
  float s = 0.0f;
  for (int p = 0; p < P; ++p) s += part[(int64_t)p * L + e];
  out[e] = s;
}

}  // namespace

extern "C" int ncf_hour_rows(const int64_t* hour, int64_t n, const float* hour_embed, int64_t dim,
                             float* out, int* err_flag, void* stream) {
  NCF_CHECK_ARG(n >= 0 && dim >= 1 && dim <= 256, "ncf_hour_rows: bad size (temporal dim 1..256)");
  if (n == 0) return NCF_OK;
  NCF_CHECK_ARG(hour && hour_embed && out, "ncf_hour_rows: null pointer");
  hipLaunchKernelGGL(k_hour_rows, dim3(ncf_cdiv(n * dim, 256)), dim3(256), 0, (hipStream_t)stream,
                     hour, n, hour_embed, (int)dim, out, err_flag);
  NCF_CHECK_LAUNCH("ncf_hour_rows");
  return NCF_OK;
}

extern "C" int64_t ncf_hour_grad_chunk(void) { return NCF_HOUR_CHUNK; }

extern "C" int64_t ncf_hour_grad_workspace(int64_t n, int64_t dim) {
  if (n < 0 || dim < 1) return 0;
  return (int64_t)ncf_cdiv(n, NCF_HOUR_CHUNK) * kHours * dim;
}

extern "C" int ncf_item_scale_bwd(const int64_t* item_ids, int64_t n, const float* mf_item,
                                  const float* mlp_item, int64_t num_items, int64_t dim,
                                  const float* mf_gamma, const float* mf_beta,
                                  const float* mlp_gamma, const float* mlp_beta, float eps,
                                  const float* item_scale, float scale_factor,
                                  float* grad_mf_item_ln, float* grad_mlp_item_ln,
                                  float* grad_scale, int* err_flag, void* stream) {
  NCF_CHECK_ARG(n >= 0 && num_items >= 1, "ncf_item_scale_bwd: bad size");
  if (n == 0) return NCF_OK;
  NCF_CHECK_ARG(item_ids && mf_item && mlp_item && mf_gamma && mf_beta && mlp_gamma && mlp_beta &&
                    item_scale && grad_mf_item_ln && grad_mlp_item_ln && grad_scale,
                "ncf_item_scale_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
#define NCF_ISB(DD)                                                                              \
  case DD:                                                                                       \
    return launch_item_scale_bwd<DD>(item_ids, n, mf_item, mlp_item, num_items, mf_gamma, mf_beta, \
                                     mlp_gamma, mlp_beta, eps, item_scale, scale_factor,         \
                                     grad_mf_item_ln, grad_mlp_item_ln, grad_scale, err_flag, st);
  switch (dim) {
    NCF_ISB(16)
    NCF_ISB(32)
    NCF_ISB(64)
    NCF_ISB(128)
    default:
      ncf_set_error("ncf_item_scale_bwd: unsupported embedding dim %lld (16/32/64/128)",
                    (long long)dim);
      return NCF_ERR_ARG;
  }
#undef NCF_ISB
}

extern "C" int ncf_hour_grad(const int64_t* hour, int64_t n, const float* dte, int64_t ld,
                             const float* add, int64_t ld_add, int64_t dim, float* grad_hour,
                             float* workspace, int64_t workspace_floats, void* stream) {
  NCF_CHECK_ARG(n >= 0 && dim >= 1 && dim <= 256, "ncf_hour_grad: bad size (temporal dim 1..256)");
  NCF_CHECK_ARG(grad_hour && (n == 0 || (hour && dte && ld >= dim)) && (!add || ld_add >= dim),
                "ncf_hour_grad: null pointer / leading dimension below dim");
  NCF_CHECK_ARG(n <= (int64_t)NCF_HOUR_CHUNK * 0x7fffffff / (kHours * 256),
                "ncf_hour_grad: batch too large");
  if (workspace_floats < ncf_hour_grad_workspace(n, dim) || (n > 0 && !workspace)) {
    ncf_set_error("ncf_hour_grad: workspace too small");
    return NCF_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int P = ncf_cdiv(n, NCF_HOUR_CHUNK), T = (int)dim, L = kHours * T;
  if (P > 0)
    hipLaunchKernelGGL(k_hour_grad_part, dim3(P), dim3(256), 0, st, hour, n, dte, ld, add, ld_add,
                       T, workspace);
  hipLaunchKernelGGL(k_hour_grad_sum, dim3(ncf_cdiv(L, 256)), dim3(256), 0, st, workspace, P, L,
                     grad_hour);
  NCF_CHECK_LAUNCH("ncf_hour_grad");
  return NCF_OK;
}
