// Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, src/model/trainer.py:278-283)
// over gradients that live in several buffers: the compact table rows of a backward (the first
// num_unique rows of each w.G, a count only the device knows) and the flat dense gradient buffer.
//
//   total = || all valid elements ||_2   (or max |x|: norm_kind 1)
//   c     = min(1, max_norm / (total + 1e-6)),  every valid element *= c
//
// Two launches over the same grid, one workgroup per NCF_GRAD_CLIP_CHUNK floats of a segment's
// CAPACITY (rows x dim), so the grid never depends on a device count:
//   1. k_clip_partial: workgroup b sums the squares of the valid elements of its chunk in fp64
//      (thread: its elements in ascending order; wave: xor-butterfly shuffles; workgroup: the four
//      wave sums in wave order) and writes part[b] — exactly 0 for a chunk wholly past the count.
//   2. k_clip_scale: every workgroup adds part[0..P) in the same fixed order (thread t takes
//      t, t + 256, ...; then the butterfly and the wave order of launch 1), so all of them hold
//      the same total and coefficient bit for bit, and scales its own chunk.  Workgroup 0 writes
//      out = {total, c}.
// No atomics, no hand-off between workgroups inside a launch: every addition sequence is fixed by
// (segment capacities, P) alone — not by the grid's dispatch order or XCD placement — so two runs
// give the same bits.  fp64 accumulation (the kernels are memory-bound) leaves the norm at the
// fp32 rounding of an essentially exact sum; the coefficient is rounded to fp32 once and each
// element takes one fp32 multiply.  Rows at and past a segment's device count are never read or
// written (they are uninitialised memory).
#include "ncf_common.h"

#define NCF_GRAD_CLIP_CHUNK 4096

namespace {

constexpr int kChunk = NCF_GRAD_CLIP_CHUNK;
constexpr int kThreads = 256;
constexpr int kPer = kChunk / kThreads;      // floats per thread
static_assert(kPer % 4 == 0, "a thread takes whole float4s");

struct ClipArgs {
  ncf_grad_seg s[NCF_GRAD_CLIP_MAX_SEGS];
  uint32_t first[NCF_GRAD_CLIP_MAX_SEGS + 1];   // first workgroup of segment i
  uint32_t vec;                                  // bit i: segment i takes 16-byte loads / stores
  int32_t count;
};

__device__ __forceinline__ int find_seg(const ClipArgs& a, uint32_t b) {
  int i = 0;
  while (i + 1 < a.count && a.first[i + 1] <= b) ++i;
  return i;
}

// [lo, hi): the valid floats of this workgroup's chunk (empty when the chunk lies past the count)
__device__ __forceinline__ void chunk_range(const ClipArgs& a, int si, uint32_t block, int64_t& lo,
                                            int64_t& hi) {
  const ncf_grad_seg& s = a.s[si];
  int64_t rows = s.rows;
  if (s.rows_dev) rows = min(max((int64_t)*s.rows_dev, (int64_t)0), s.rows);
  lo = (int64_t)(block - a.first[si]) * kChunk;
  hi = min(lo + kChunk, rows * s.dim);
}

// INF: the largest |x| (NaN kept, as torch's max does); else the sum of squares
template <bool INF>
__device__ __forceinline__ double fold(double acc, float x) {
  if constexpr (INF) {
    const double v = (double)fabsf(x);
    return (v > acc || v != v) ? v : acc;
  } else {
    return acc + (double)x * (double)x;
  }
}

template <bool INF>
__device__ __forceinline__ double join(double a, double b) {
  if constexpr (INF) return (b > a || b != b) ? b : a;
  else return a + b;
}

// the workgroup's value from each thread's: butterfly inside a wave (every lane ends with the
// same bits: a + b and b + a are the same fp operation), then the waves in order
template <bool INF>
__device__ __forceinline__ double block_join(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = join<INF>(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int q = 1; q < kThreads / 64; ++q) t = join<INF>(t, red[q]);
  return t;
}

template <bool INF>
__global__ __launch_bounds__(kThreads) void k_clip_partial(const ClipArgs a,
                                                           double* __restrict__ part) {
  __shared__ double red[kThreads / 64];
  const int si = find_seg(a, blockIdx.x);
  int64_t lo, hi;
  chunk_range(a, si, blockIdx.x, lo, hi);
  const float* __restrict__ p = a.s[si].data;
  double acc = 0.0;
  if ((a.vec >> si) & 1u) {        // valid floats and chunk starts are multiples of 4
    float4 v[kPer / 4];
#pragma unroll
    for (int k = 0; k < kPer / 4; ++k) {
      const int64_t i = lo + ((int64_t)k * kThreads + threadIdx.x) * 4;
      v[k] = i < hi ? ld4(p + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < kPer / 4; ++k) {
      acc = fold<INF>(acc, v[k].x);
      acc = fold<INF>(acc, v[k].y);
      acc = fold<INF>(acc, v[k].z);
      acc = fold<INF>(acc, v[k].w);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int64_t i = lo + (int64_t)k * kThreads + threadIdx.x;
      acc = fold<INF>(acc, i < hi ? p[i] : 0.0f);
    }
  }
  const double t = block_join<INF>(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// scale: 0 computes the norm only (one workgroup, out[1] = 1, nothing else written)
template <bool INF>
__global__ __launch_bounds__(kThreads) void k_clip_scale(const ClipArgs a,
                                                         const double* __restrict__ part, int P,
                                                         double max_norm, int scale,
                                                         float* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < P; i += kThreads) acc = join<INF>(acc, part[i]);
  const double t = block_join<INF>(acc, red);
  const float total = (float)(INF ? t : sqrt(t));
  float c = 1.0f;
  if (scale) {
    const double r = max_norm / ((INF ? t : sqrt(t)) + 1e-6);
    c = (float)((r < 1.0 || r != r) ? r : 1.0);      // min(1, r), NaN kept (torch.clamp)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = total;
    out[1] = c;
  }
  if (!scale || c == 1.0f || P == 0) return;          // (x * 1 = x: no store needed)
  const int si = find_seg(a, blockIdx.x);
  int64_t lo, hi;
  chunk_range(a, si, blockIdx.x, lo, hi);
  float* __restrict__ p = a.s[si].data;
  if ((a.vec >> si) & 1u) {
#pragma unroll
    for (int k = 0; k < kPer / 4; ++k) {
      const int64_t i = lo + ((int64_t)k * kThreads + threadIdx.x) * 4;
      if (i < hi) {
        const float4 v = ld4(p + i);
        st4(p + i, make_float4(v.x * c, v.y * c, v.z * c, v.w * c));
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int64_t i = lo + (int64_t)k * kThreads + threadIdx.x;
      if (i < hi) p[i] *= c;
    }
  }
}

// validates the list and fills the launch arguments; returns the number of chunks, or -1
int64_t plan(const ncf_grad_seg* segs, int nsegs, ClipArgs* a, const char* who) {
  if (nsegs < 0 || nsegs > NCF_GRAD_CLIP_MAX_SEGS || (nsegs > 0 && !segs)) {
    ncf_set_error("%s: %d segments (0..%d)", who, nsegs, NCF_GRAD_CLIP_MAX_SEGS);
    return -1;
  }
  int64_t total = 0;
  uint32_t vec = 0;
  for (int i = 0; i < nsegs; ++i) {
    const ncf_grad_seg& s = segs[i];
    if (s.rows < 0 || s.dim < 1 || s.rows > (((int64_t)1 << 40) / s.dim) ||
        (s.rows > 0 && (!s.data || ((uintptr_t)s.data & 3))) || ((uintptr_t)s.rows_dev & 3)) {
      ncf_set_error("%s: segment %d: bad size or pointer", who, i);
      return -1;
    }
    if (a) {
      a->s[i] = s;
      a->first[i] = (uint32_t)total;
    }
    if (s.dim % 4 == 0 && ((uintptr_t)s.data & 15) == 0) vec |= 1u << i;
    total += (s.rows * s.dim + kChunk - 1) / kChunk;
    if (total > 0x3fffffff) {
      ncf_set_error("%s: too many elements", who);
      return -1;
    }
  }
  if (a) {
    for (int i = nsegs; i <= NCF_GRAD_CLIP_MAX_SEGS; ++i) a->first[i] = (uint32_t)total;
    a->vec = vec;
    a->count = nsegs;
  }
  return total;
}

}  // namespace

extern "C" int64_t ncf_grad_clip_chunk(void) { return NCF_GRAD_CLIP_CHUNK; }

extern "C" int64_t ncf_grad_clip_workspace(const ncf_grad_seg* segs, int nsegs) {
  const int64_t P = plan(segs, nsegs, nullptr, "ncf_grad_clip_workspace");
  return P < 0 ? 0 : 8 * (P > 0 ? P : 1);
}

extern "C" int ncf_grad_clip(const ncf_grad_seg* segs, int nsegs, int norm_kind, double max_norm,
                             void* workspace, int64_t workspace_bytes, float* out, void* stream) {
  NCF_CHECK_ARG(norm_kind == 0 || norm_kind == 1, "ncf_grad_clip: norm_kind 0 (2-norm) or 1 (inf)");
  NCF_CHECK_ARG(max_norm > 0.0, "ncf_grad_clip: max_norm must be > 0 (+inf: the norm only)");
  NCF_CHECK_ARG(out && ((uintptr_t)out & 3) == 0, "ncf_grad_clip: null / misaligned out");
  ClipArgs a;
  memset(&a, 0, sizeof a);
  const int64_t P = plan(segs, nsegs, &a, "ncf_grad_clip");
  if (P < 0) return NCF_ERR_ARG;
  if (workspace_bytes < 8 * P || (P > 0 && (!workspace || ((uintptr_t)workspace & 7)))) {
    ncf_set_error("ncf_grad_clip: workspace too small (or not 8-byte aligned)");
    return NCF_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int scale = max_norm < __builtin_inf() ? 1 : 0;
  const unsigned grid2 = scale && P > 0 ? (unsigned)P : 1u;
  if (norm_kind == 0) {
    if (P > 0) hipLaunchKernelGGL(k_clip_partial<false>, dim3((unsigned)P), dim3(kThreads), 0, st, a, part);
    hipLaunchKernelGGL(k_clip_scale<false>, dim3(grid2), dim3(kThreads), 0, st, a, part, (int)P,
                       max_norm, scale, out);
  } else {
    if (P > 0) hipLaunchKernelGGL(k_clip_partial<true>, dim3((unsigned)P), dim3(kThreads), 0, st, a, part);
    hipLaunchKernelGGL(k_clip_scale<true>, dim3(grid2), dim3(kThreads), 0, st, a, part, (int)P,
                       max_norm, scale, out);
  }
  NCF_CHECK_LAUNCH("ncf_grad_clip");
  return NCF_OK;
}
