// Batched deterministic reductions: every deferred gradient reduction of a backward pass in two
// launches (ncf_hip.h, "deferred reductions").
//
// A training step produces ~25 parameter gradients as sums over batch rows (split-K slabs of the
// weight gradients, per-block dgamma/dbeta/dbias partials of the row ops, the head and the
// embedding LayerNorms).  None of them is on the critical path of the backward (only dX is), so
// instead of two small launches each, the list is run at the end of the backward:
//   stage 1: one 256-thread block per (descriptor, 64 outputs, chunk of <= 64 partials); a
//            descriptor with P <= NCF_REDUCE_ONE_STAGE (256) partials finishes here, otherwise
//            each chunk writes its own row of `scratch`;
//   stage 2: sums the chunk rows of the multi-chunk descriptors in chunk order.
// The summation order of every output depends only on (P, chunking) — never on scheduling —
// and is the order of ncf_reduce_parts (ncf_common.h), so a deferred reduction is bit-identical
// to the inline one.
//
// ncf_reduce_batch_catchup is the same two stages with the deferred table Adam's late catch-up
// of the next batch's rows (adam_catchup_dev.h) inside the first stage-1 launch
// (k_reduce1_catchup): the memory-bound reduce blocks and the latency-bound replay chains share
// the CUs on the step's own queue, with no cross-queue event between them.
#include "ncf_common.h"
#include "reduce_dev.h"          // stage 1 and the launch arguments (shared with the fused launch)
#include "adam_catchup_dev.h"

using namespace ncf_reduce;
using namespace ncf_adam;

namespace {

// ncf_reduce_set_vec: 0 one column per lane, 1 four columns per lane (16-byte loads, 16 in
// flight per thread; the default)
int VEC_LANES = 1;
// ncf_reduce_catchup_set_order: which class of blocks of k_reduce1_catchup takes the low block
// indices and so dispatches first (0: the reduce blocks, the default; 1: the catch-up's replay
// chains; 2: the two interleaved).  Measured: DESIGN §15.
int TAIL_ORDER = 0;

__global__ __launch_bounds__(256) void k_reduce_batch1(const BatchArgs a, float* __restrict__ scratch) {
  __shared__ float4 red[4][64];
  reduce1_body(a, scratch, blockIdx.x, red);
}

// Stage 1 of one launch group and the catch-up of both id kinds' listed rows (lock = 0) in one
// 1-D grid: nred reduce blocks (reduce1_body, as k_reduce_batch1) and npairs * ncx catch-up
// blocks (pairs_catchup_body, as k_pairs_catchup's grid (ncx, npairs)).  The two classes touch
// disjoint memory (gradient partials and outputs; table rows, moments and stamps).
// The replay is VALU-bound and wants every wave slot: the kernel is held to 64 registers (8
// waves per SIMD, 8 blocks per CU), which the reduce blocks meet with kTailLoads = 4 loads in
// flight per thread where k_reduce_batch1 keeps 16 (90 registers, 5 waves) — the same additions
// in the same order.  At 90 registers the fused launch took 33 us of the C2 step, at 64 with 8
// loads (28 B of scratch per lane) 28 us, with 4 loads (50 registers at D <= 128, no scratch)
// 27 us; DESIGN §15.
constexpr int kTailLoads = 4;
template <int D, Rows V>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_reduce1_catchup(const BatchArgs a,
                                                         float* __restrict__ scratch, uint32_t nred,
                                                         const PairArgs pa,
                                                         const uint32_t* __restrict__ count,
                                                         int64_t max_n, int32_t target_rel,
                                                         const ncf_step_clock* __restrict__ clock,
                                                         const float* __restrict__ table,
                                                         const AdamScalars s, uint32_t ncx,
                                                         int order) {
  __shared__ float4 red[4][64];
  const uint32_t ncatch = gridDim.x - nred;
  uint32_t b = blockIdx.x;
  bool catchup;
  int k = 0;
  if (order == 2) {
    // interleaved: groups of one catch-up block per kind and one reduce block while both
    // classes last (the listed rows sit in each kind's low blocks), then the longer class
    const uint32_t np = ncatch / ncx, per = np + 1;
    const uint32_t m = min(ncx, nred);
    if (b < m * per) {
      const uint32_t j = b % per;
      catchup = j < np;
      k = (int)j;
      b /= per;
    } else {
      const uint32_t r = b - m * per;
      catchup = ncx > nred;
      k = catchup ? (int)(r % np) : 0;
      b = m + (catchup ? r / np : r);
    }
  } else {
    if (order == 1) {
      catchup = b < ncatch;
      if (!catchup) b -= ncatch;
    } else {
      catchup = b >= nred;
      if (catchup) b -= nred;
    }
    if (catchup) {
      k = (int)(b / ncx);
      b %= ncx;
    }
  }
  if (catchup)
    pairs_catchup_body<D, V>(pa, k, b, count, max_n, target_rel, clock, table, s, 0);
  else
    reduce1_body<kTailLoads>(a, scratch, b, red);
}
// the arguments travel by value in the kernel-argument segment (4 KB)
static_assert(sizeof(BatchArgs) + sizeof(PairArgs) + sizeof(AdamScalars) + 96 <= 4096,
              "k_reduce1_catchup: kernel arguments exceed 4 KB");


// stage 2: one thread per output element (four per thread for a vec descriptor) of the
// multi-chunk descriptors
// k_reduce_parts' order: "wave" w sums rows w, w+4, ... — while four more of its rows remain
// (p + 12 < pe), a group of four into accumulators 0..3; its last (at most three) rows into
// accumulator 0 — then (a0 + a1) + (a2 + a3) per wave and (w0 + w1) + (w2 + w3).
// Every load of a batch of kBatch rows (the float form 64, the float4 form 32: 128 registers) is
// issued before the batch's first add: one round of memory latency per batch where the rolled
// loops above waited for one per group of four rows, per wave (a dozen in series for the 25
// chunk rows of the C2 step's embedding-LayerNorm gradients).  A batch is made of groups of 16
// consecutive rows (row 16 g + 4 k + w: wave w, slot k); rows past pe load row pe - 1 again
// (always valid) and are not added.  Each accumulator takes the same rows in the same
// (ascending) order as before: the same bits.
template <typename T>
__device__ __forceinline__ T stage2_sum(const float* __restrict__ s, int64_t L, int pe) {
  constexpr int kBatch = sizeof(T) == sizeof(float) ? 64 : 32;
  T a[4][4];
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int k = 0; k < 4; ++k) a[w][k] = zero<T>();
  for (int b = 0; b < pe; b += kBatch) {
    T v[kBatch];
#pragma unroll
    for (int g = 0; g < kBatch; g += 16) {
      if (b + g < pe) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          v[g + j] = *(const T*)(s + (int64_t)min(b + g + j, pe - 1) * L);
      }
    }
#pragma unroll
    for (int g = 0; g < kBatch; g += 16) {
      if (b + g < pe) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int w = j & 3, k = j >> 2;
          // wave w's group starting at row b + g + w is a full one iff its last row exists
          const bool full = b + g + w + 12 < pe;
          if (full) a[w][k] += v[g + j];
          else if (b + g + j < pe) a[w][0] += v[g + j];
        }
      }
    }
  }
  T ws[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) ws[w] = (a[w][0] + a[w][1]) + (a[w][2] + a[w][3]);
  return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ __launch_bounds__(256) void k_reduce_batch2(const BatchArgs a,
                                                       const float* __restrict__ scratch) {
  const int di = find_desc(a, blockIdx.x);
  const ncf_reduce_desc& d = a.d[di];
  const bool vec = a.vec[di] != 0;
  const int64_t i = ((int64_t)(blockIdx.x - a.first[di]) * 256 + threadIdx.x) * (vec ? 4 : 1);
  if (i >= d.L) return;
  const float* s = scratch + a.scr[di] + i;
  const int pe = a.chunks[di];
  if (vec) {
    const float4 t = stage2_sum<float4>(s, d.L, pe);
    store_out(d, i, t.x);
    store_out(d, i + 1, t.y);
    store_out(d, i + 2, t.z);
    store_out(d, i + 3, t.w);
    return;
  }
  store_out(d, i, stage2_sum<float>(s, d.L, pe));
}

int chunks_of(int P) { return P > NCF_REDUCE_ONE_STAGE ? (P + kPB - 1) / kPB : 1; }

}  // namespace

extern "C" int64_t ncf_reduce_set_vec(int64_t on) {
  const int was = VEC_LANES;
  if (on >= 0) VEC_LANES = on > 0 ? 1 : 0;
  return was;
}

extern "C" int64_t ncf_reduce_batch_scratch(const ncf_reduce_list* list) {
  if (!list) return 0;
  int64_t f = 0;
  for (int i = 0; i < list->count && i < NCF_REDUCE_LIST_MAX; ++i) {
    const int c = chunks_of(list->d[i].P);
    if (c > 1) f += (int64_t)c * list->d[i].L;
  }
  return f;
}


namespace {

// the catch-up that rides in the first stage-1 launch (ncf_reduce_batch_catchup)
struct Tail {
  PairArgs pa;
  int npairs;
  int64_t dim;
  const uint32_t* count;
  int64_t max_n;
  int32_t target_rel;
  const ncf_step_clock* clock;
  const float* table;
  AdamScalars s;
};

// The widest rows whose decoupled catch-up rides in the fused launch.  The decoupled replay keeps
// more steps in flight per lane (m and v do not depend on p, so the compiler runs their chains
// ahead); held to the fused kernel's 64 registers at D = 256 it spilled 116 B per lane (compiler
// resource report), so that width takes the reduce and the catch-up as two launches: same bits.
constexpr int kDwFusedMaxDim = 128;

// whether rows of width dim and variant v have an instantiation of the fused kernel: asked by
// its launch (fused_d) and by ncf_reduce_batch_catchup, which makes the two launches otherwise
constexpr bool tail_fused(int64_t dim, Rows v) {
  return v != Rows::F32_DW || dim <= kDwFusedMaxDim;
}

template <int D>
int fused_d(const BatchArgs& a1, float* scratch, uint32_t b1, const Tail& t, hipStream_t st) {
  const uint32_t ncx = (uint32_t)ncf_cdiv(t.max_n * Replay<D>::LPR, 256);
  const dim3 grid(b1 + (uint32_t)t.npairs * ncx);
  for_any_rows(t.pa.variant, [&](auto V) {
    if constexpr (tail_fused(D, V()))   // (the others never get here)
      hipLaunchKernelGGL((k_reduce1_catchup<D, V()>), grid, dim3(256), 0, st, a1, scratch, b1,
                         t.pa, t.count, t.max_n, t.target_rel, t.clock, t.table, t.s, ncx,
                         TAIL_ORDER);
  });
  NCF_CHECK_LAUNCH("ncf_reduce_batch_catchup(stage 1 + catch-up)");
  return NCF_OK;
}

int fused_launch(const BatchArgs& a1, float* scratch, uint32_t b1, const Tail& t, hipStream_t st) {
  NCF_DISPATCH_DIM(t.dim, fused_d, a1, scratch, b1, t, st);
}

// Every listed reduction, a launch group of <= kMaxPerLaunch descriptors at a time.  With
// `tail` (max_n > 0, a non-empty list) the first group's stage 1 is the fused launch.
int run_list(const char* who, const ncf_reduce_list* list, float* scratch, int64_t scratch_floats,
             const Tail* tail, hipStream_t st) {
  NCF_CHECK_ARG(list && list->count >= 0 && list->count <= NCF_REDUCE_LIST_MAX, "%s: bad list",
                who);
  if (scratch_floats < ncf_reduce_batch_scratch(list)) {
    ncf_set_error("%s: scratch %lld < %lld floats", who, (long long)scratch_floats,
                  (long long)ncf_reduce_batch_scratch(list));
    return NCF_ERR_WORKSPACE;
  }
  int64_t scr_off = 0;
  for (int base = 0; base < list->count; base += kMaxPerLaunch) {
    BatchArgs a1, a2;
    memset(&a1, 0, sizeof(a1));
    memset(&a2, 0, sizeof(a2));
    uint32_t b1 = 0, b2 = 0;
    for (int j = 0; j < kMaxPerLaunch && base + j < list->count; ++j) {
      const ncf_reduce_desc& d = list->d[base + j];
      NCF_CHECK_ARG(d.part && d.out && d.L >= 0 && d.P >= 1 && d.cols >= 1 && d.stride >= d.L,
                    "%s: bad descriptor %d", who, base + j);
      const int c = chunks_of(d.P);
      const bool vec = VEC_LANES > 0 && d.L % 4 == 0 && d.stride % 4 == 0 &&
                       ((uintptr_t)d.part & 15) == 0 &&
                       (c == 1 || (scr_off % 4 == 0 && ((uintptr_t)scratch & 15) == 0));
      const int vw = vec ? 4 : 1;
      const uint32_t gx = (uint32_t)((d.L + 64 * vw - 1) / (64 * vw));
      a1.d[a1.count] = d;
      a1.vec[a1.count] = vec;
      a1.chunks[a1.count] = c;
      a1.first[a1.count] = b1;
      a1.scr[a1.count] = c > 1 ? scr_off : 0;
      b1 += gx * (uint32_t)c;
      if (c > 1) {
        a2.d[a2.count] = d;
        a2.chunks[a2.count] = c;
        a2.vec[a2.count] = vec;
        a2.first[a2.count] = b2;
        a2.scr[a2.count] = scr_off;
        b2 += (uint32_t)((d.L + 256 * vw - 1) / (256 * vw));
        ++a2.count;
        scr_off += (int64_t)c * d.L;
      }
      ++a1.count;
    }
    a1.first[a1.count] = b1;
    a2.first[a2.count] = b2;
    if (tail && base == 0) {
      const int rc = fused_launch(a1, scratch, b1, *tail, st);
      if (rc != NCF_OK) return rc;
    } else if (b1 > 0) {
      hipLaunchKernelGGL(k_reduce_batch1, dim3(b1), dim3(256), 0, st, a1, scratch);
      NCF_CHECK_LAUNCH("ncf_reduce_batch(stage 1)");
    }
    if (b2 > 0) {
      hipLaunchKernelGGL(k_reduce_batch2, dim3(b2), dim3(256), 0, st, a2, (const float*)scratch);
      NCF_CHECK_LAUNCH("ncf_reduce_batch(stage 2)");
    }
  }
  return NCF_OK;
}

}  // namespace

extern "C" int ncf_reduce_batch(const ncf_reduce_list* list, float* scratch,
                                int64_t scratch_floats, void* stream) {
  return run_list("ncf_reduce_batch", list, scratch, scratch_floats, nullptr, (hipStream_t)stream);
}

extern "C" int64_t ncf_reduce_catchup_set_order(int64_t order) {
  const int was = TAIL_ORDER;
  if (order >= 0) TAIL_ORDER = order > 2 ? 2 : (int)order;
  return was;
}

// ncf_reduce_batch(list, ...) and ncf_adam_pairs_catchup_lock_clock(pairs, ..., lock = 0, ...) on
// one stream, with the catch-up inside the first group's stage-1 launch: the same bits as the
// two calls (the same device bodies; the two touch disjoint memory).
extern "C" int ncf_reduce_batch_catchup(const ncf_reduce_list* list, float* scratch,
                                        int64_t scratch_floats, const ncf_table_pair* pairs,
                                        int npairs, int64_t dim, const uint32_t* count,
                                        int64_t max_n, int32_t target_rel,
                                        const ncf_step_clock* clock, const float* step_table,
                                        double beta1, double beta2, double eps,
                                        double weight_decay, void* stream) {
  NCF_CHECK_ARG(list && list->count >= 0 && list->count <= NCF_REDUCE_LIST_MAX,
                "ncf_reduce_batch_catchup: bad list");
  Tail tail{{}, npairs, dim, count, max_n, target_rel, clock, step_table,
            consts_of(beta1, beta2, eps, weight_decay)};
  const int rc = pair_args("ncf_reduce_batch_catchup", pairs, npairs, &tail.pa);
  if (rc != NCF_OK) return rc;
  NCF_CHECK_ARG(count && clock && step_table, "ncf_reduce_batch_catchup: bad args");
  if (max_n <= 0)
    return run_list("ncf_reduce_batch_catchup", list, scratch, scratch_floats, nullptr,
                    (hipStream_t)stream);
  if (!tail_fused(dim, tail.pa.variant)) {
    const int rc = run_list("ncf_reduce_batch_catchup", list, scratch, scratch_floats, nullptr,
                            (hipStream_t)stream);
    if (rc != NCF_OK) return rc;
    return ncf_adam_pairs_catchup_lock_clock(pairs, npairs, dim, count, max_n, target_rel, 0,
                                             clock, step_table, beta1, beta2, eps, weight_decay,
                                             stream);
  }
  if (list->count == 0)
    return ncf_adam_pairs_catchup_lock_clock(pairs, npairs, dim, count, max_n, target_rel, 0,
                                             clock, step_table, beta1, beta2, eps, weight_decay,
                                             stream);
  return run_list("ncf_reduce_batch_catchup", list, scratch, scratch_floats, &tail,
                  (hipStream_t)stream);
}
