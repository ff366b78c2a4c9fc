// Exact nearest-product search over the exported embeddings: the query the reference's production
// API sends to its Vertex Tree-AH index (src/inference/api.py:63-73: find_neighbors(user
// embedding, k, category_filter); the index: setup_tree_ah_endpoint.py:25-32, cosine distance over
// the L2-normalised "mlp" product vectors of generate_embeddings.py:193-221), answered exactly.
//
// One request is one vector, a batch tens to a few hundred, the catalogue 100K to 5M rows: the
// matrix is read once per block of 32 queries.  The catalogue is cut into slabs; a workgroup
// (kNW waves) scans one slab for one block of up to 32 queries:
//   * the 32 (normalised) query rows are the A operand of v_mfma_f32_32x32x2_f32, in registers
//     (k-permuted: step s uses k = s + (D/2) h for lane half h); a wave multiplies them with one
//     32-item tile per step, staged by the wave itself through its own LDS tile ([32][D+1]:
//     coalesced 16-byte global loads, conflict-free operand reads), the next kPD tiles' loads
//     in flight behind the MFMAs.  fp32 operands and accumulation in a fixed order: a similarity
//     does not depend on the slab plan or the run;
//   * selection in LDS on the 64-bit key fkey(sim) << 32 | (0xFFFFFFFF - position) (the key of
//     k_select / k_merge: similarity desc, then position asc; the order is total, ties need no
//     special case).  Per query: a list of kSeg keys, a count and the running K-th key.  A
//     candidate that passes the filters is appended iff its key is greater than the running
//     K-th key.  A list holds at most kKeep keys when a step begins and a step appends at most
//     kNW * 32 (one per item), so it cannot overflow; lists longer than kKeep after a step are
//     sorted, cut to K, and their K-th key becomes the bar (nn_compact).  The kept SET is a
//     function of the bars only, which change at step boundaries only, so the append order (LDS
//     atomics) does not reach the result;
//   * at the end every list is sorted once more and its first K keys are the slab's partial
//     list, in the layout ncf_score_merge reads.
// Filters (before the key test): the item's category against the query's (CAT instances: the
// categories travel with their tiles), and the one position a query skips.
// A NaN similarity fails the first comparison (sim >= bar) and is never kept.
#include "ncf_common.h"
#include "scan_tile_dev.h"   // the query half, the MFMA chain and the row map (the tiling is its own)
#include "select_dev.h"

namespace {

typedef unsigned long long u64;

constexpr int kNW = 4;      // waves per workgroup: one 32-item tile each per step
constexpr int kQB = 32;     // queries per workgroup (the MFMA's 32 rows)
constexpr int kKeep = 128;  // the largest K; a list longer than this after a step is compacted
constexpr int kSeg = 256;   // keys per list
static_assert(kKeep + kNW * 32 <= kSeg, "a step's appends must fit behind the kept keys");
constexpr int kPD = 2;      // steps of item tiles in flight per wave (register ring)

template <int D>
constexpr size_t nn_tile_bytes() {
  return ((size_t)kNW * 32 * (D + 1) * sizeof(float) + 15) & ~(size_t)15;
}

// Lists with more than `limit` keys: sorted descending (over the power of two that holds the
// longest of them), cut to K, the bar raised to the K-th key of a full list.  The whole block
// enters after a barrier and leaves after one.  act: [kQB] list numbers, then their count and
// the sort size.
__device__ __forceinline__ void nn_compact(u64* keys, uint32_t* cnt, u64* thr, float* thf, int* act,
                                           uint32_t limit, int K, int nq) {
  if (threadIdx.x == 0) {
    int n = 0;
    uint32_t longest = 1;
    for (int q = 0; q < nq; ++q)
      if (cnt[q] > limit) {
        act[n++] = q;
        longest = max(longest, min(cnt[q], (uint32_t)kSeg));
      }
    int n2 = 1;
    while ((uint32_t)n2 < longest) n2 <<= 1;
    act[kQB] = n;
    act[kQB + 1] = n2;
  }
  __syncthreads();
  const int n = act[kQB], n2 = act[kQB + 1];
  for (int e = threadIdx.x; e < n * n2; e += blockDim.x) {
    const int q = act[e / n2], j = e & (n2 - 1);
    if ((uint32_t)j >= cnt[q]) keys[q * kSeg + j] = 0ull;   // (below every real key)
  }
  __syncthreads();
  bitonic_desc_lists<kSeg>(keys, act, n, n2);
  if ((int)threadIdx.x < n) {
    const int q = act[threadIdx.x];
    const uint32_t c = min(cnt[q], (uint32_t)K);
    cnt[q] = c;
    if (c == (uint32_t)K) {
      const u64 t = keys[q * kSeg + K - 1];
      thr[q] = t;
      thf[q] = fkey_inv((uint32_t)(t >> 32));
    }
  }
  __syncthreads();
}

// CAT: a category filter is in use (the items' categories travel with their tiles)
template <int D, bool CAT>
__global__ __launch_bounds__(64 * kNW) void k_nn_scan(
    const float* __restrict__ queries, int64_t n_queries, int normalize,
    const float* __restrict__ vectors, int64_t n_items, const int32_t* __restrict__ item_cat,
    const int32_t* __restrict__ query_cat, const int64_t* __restrict__ query_skip,
    int64_t slab_items, int K, float* __restrict__ part_sim, int64_t* __restrict__ part_item) {
  constexpr int KH = D / 2;        // k per lane half
  constexpr int NV = D / 8;        // float4 per lane to stage a 32 x D tile
  constexpr int R4 = D / 4;        // float4 per row
  constexpr int PITCH = D + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char nn_raw[];
  __shared__ u64 thr[kQB];         // the running K-th key (0: the list is not full yet)
  // its similarity (-inf before; +inf for the rows past the block's queries)
  __shared__ __attribute__((aligned(16))) float thf[kQB];
  __shared__ uint32_t cnt[kQB];
  __shared__ int qcat[kQB], qskip[kQB], act[kQB + 2];
  __shared__ int cs[CAT ? 64 * kNW : 1];   // the categories of each wave's tile
  float* ps = reinterpret_cast<float*>(nn_raw) + (threadIdx.x >> 6) * (32 * PITCH);
  u64* keys = reinterpret_cast<u64*>(nn_raw + nn_tile_bytes<D>());   // [queries of a block][kSeg]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int64_t q0 = (int64_t)blockIdx.y * kQB;
  const int nq = (int)min((int64_t)kQB, n_queries - q0);
  if (tid < kQB) {
    const bool v = tid < nq;
    thr[tid] = 0ull;
    thf[tid] = v ? -INFINITY : INFINITY;
    cnt[tid] = 0u;
    qcat[tid] = (v && query_cat) ? query_cat[q0 + tid] : -1;
    const int64_t sk = (v && query_skip) ? query_skip[q0 + tid] : -1;
    qskip[tid] = (sk >= 0 && sk < n_items) ? (int)sk : -1;
  }
  // this lane's half of query row i (every wave holds all 32 rows), normalised
  float a[KH];
  {
    const bool v = i < nq;
    scan_load_half<KH>(queries + (q0 + (v ? i : 0)) * D + KH * h, a, v);
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < KH; ++k) ss = fmaf(a[k], a[k], ss);
    ss += __shfl_xor(ss, 32, 64);   // (both halves form the same sum)
    if (normalize && ss > 0.0f) {   // a zero row stays zero; a NaN row stays NaN
      const float nrm = sqrtf(ss);
#pragma unroll
      for (int k = 0; k < KH; ++k) a[k] = a[k] / nrm;
    }
  }
  scan_consume<KH>(a);
  const int64_t it0 = (int64_t)blockIdx.x * slab_items;
  const int64_t it1 = min(n_items, it0 + slab_items);
  const int64_t ntiles = it0 < it1 ? (it1 - it0 + 31) / 32 : 0;
  const int64_t nsteps = (ntiles + kNW - 1) / kNW;
  // register ring of kPD staged tiles (and their items' categories): the loads of step s + kPD
  // are issued while step s is multiplied, so a tile's HBM latency has kPD steps to hide behind
  // (one step, ~1 us of MFMAs with four waves on the CU, is shorter than a loaded HBM miss)
  float4 pv[kPD][NV];
  int pc[kPD] = {};
  auto fetch = [&](int64_t t0, float4 (&v)[NV], int& vc) {
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int f = c * 64 + lane;
      const int64_t item = t0 + f / R4;
      const int64_t src = item < it1 ? item : it0;   // clamped, unconditional (it0 < it1 here)
      v[c] = ld4(vectors + src * D + (f % R4) * 4);
    }
    if constexpr (CAT) vc = item_cat[t0 + i < it1 ? t0 + i : it0];
  };
  const bool has_skip = query_skip != nullptr;
  // one step: this wave's tile of step `step` from ring slot (v, vc), which is then refilled
  auto do_step = [&](int64_t step, float4 (&v)[NV], int& vc) {
    const int64_t t0 = it0 + (step * kNW + w) * 32;   // (may lie past it1: no item of it is valid)
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      const int f = c * 64 + lane;
      float* dst = ps + (f / R4) * PITCH + (f % R4) * 4;
      dst[0] = v[c].x; dst[1] = v[c].y; dst[2] = v[c].z; dst[3] = v[c].w;
    }
    // (through LDS like the tile: held in a register across the refill below, the value would
    // be copied at the loop's end, behind a wait for every load in flight)
    if constexpr (CAT) cs[tid] = vc;
    wave_lds_sync();
    // (unconditional: past the slab the addresses are clamped; a branch around the loads would
    // make the compiler wait for every outstanding load, the other ring slots' included, before
    // the next slot is stored)
    fetch(t0 + (int64_t)kPD * kNW * 32, v, vc);
    // acc[r]: query row scan_row(r, h), item t0 + i
    const f32x16 acc = scan_chain<KH>(a, ps + i * PITCH + KH * h);
    const int64_t pos = t0 + i;
    const bool ivalid = pos < it1;
    float th[16];
    uint32_t hm = 0;
    int over = 0;   // this thread saw a list grow past kKeep
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 t = *reinterpret_cast<const float4*>(thf + 8 * c + 4 * h);
      th[4 * c] = t.x; th[4 * c + 1] = t.y; th[4 * c + 2] = t.z; th[4 * c + 3] = t.w;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) hm |= (acc[r] >= th[r] ? 1u : 0u) << r;   // (a NaN: never)
    if (ivalid && hm) {
      const uint32_t low = 0xFFFFFFFFu - (uint32_t)pos;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!((hm >> r) & 1u)) continue;
        const int ql = scan_row(r, h);
        if (ql >= nq) continue;
        if constexpr (CAT) {
          const int qc = qcat[ql];
          if (qc >= 0 && cs[tid] != qc) continue;
        }
        if (has_skip && (int)pos == qskip[ql]) continue;
        const float s = acc[r] + 0.0f;   // (-0 -> +0: one key per value)
        const u64 key = ((u64)fkey(s) << 32) | (u64)low;
        // above the bar's similarity the key is greater whatever the positions; the 64-bit
        // bar is read only at equal similarity
        if (s > th[r] || key > thr[ql]) {
          const uint32_t p = atomicAdd(&cnt[ql], 1u);
          if (p < (uint32_t)kSeg) keys[ql * kSeg + p] = key;
          if (p >= (uint32_t)kKeep) over = 1;
        }
      }
    }
    if (__syncthreads_or(over))   // (uniform; also the step's barrier)
      nn_compact(keys, cnt, thr, thf, act, (uint32_t)kKeep, K, nq);
  };
  if (nsteps > 0) {
#pragma unroll
    for (int d = 0; d < kPD; ++d) fetch(it0 + ((int64_t)d * kNW + w) * 32, pv[d], pc[d]);
  }
  __syncthreads();
  int64_t s0 = 0;
  for (; s0 + kPD <= nsteps; s0 += kPD) {
#pragma unroll
    for (int d = 0; d < kPD; ++d) do_step(s0 + d, pv[d], pc[d]);   // (static ring slots)
  }
#pragma unroll
  for (int d = 0; d + 1 < kPD; ++d)   // the last nsteps % kPD steps
    if (s0 + d < nsteps) do_step(s0 + d, pv[d], pc[d]);
  __syncthreads();
  nn_compact(keys, cnt, thr, thf, act, 0u, K, nq);
  const int64_t n_slabs = gridDim.x;
  for (int e = tid; e < nq * K; e += blockDim.x) {
    const int q = e / K, j = e % K;
    const bool ok = (uint32_t)j < cnt[q];
    const u64 k = ok ? keys[q * kSeg + j] : 0ull;
    const int64_t o = ((q0 + q) * n_slabs + blockIdx.x) * K + j;
    part_sim[o] = ok ? fkey_inv((uint32_t)(k >> 32)) : 0.0f;
    part_item[o] = ok ? (int64_t)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull)) : -1;
  }
}

template <int D, bool CAT>
int nn_launch(const float* queries, int64_t n_queries, int normalize, const float* vectors,
              int64_t n_items, const int32_t* item_cat, const int32_t* query_cat,
              const int64_t* query_skip, int64_t slab_items, int64_t n_slabs, int K,
              float* part_sim, int64_t* part_item, hipStream_t stream) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)k_nn_scan<D, CAT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(nn_tile_bytes<D>() + sizeof(u64) * kQB * kSeg));
    attr = true;
  }
  // lists for the queries a block really holds: a single query leaves room for four
  // workgroups on a CU, a full block takes most of its LDS
  const int64_t nqa = n_queries < kQB ? n_queries : kQB;
  const size_t lds = nn_tile_bytes<D>() + sizeof(u64) * (size_t)nqa * kSeg;
  const dim3 grid((unsigned)n_slabs, (unsigned)((n_queries + kQB - 1) / kQB));
  hipLaunchKernelGGL((k_nn_scan<D, CAT>), grid, dim3(64 * kNW), lds, stream, queries, n_queries,
                     normalize, vectors, n_items, item_cat, query_cat, query_skip, slab_items, K,
                     part_sim, part_item);
  NCF_CHECK_LAUNCH("ncf_nn_scan");
  return NCF_OK;
}

}  // namespace

extern "C" int ncf_nn_scan(const float* queries, int64_t n_queries, int normalize,
                           const float* vectors, int64_t n_items, int64_t dim,
                           const int32_t* item_cat, const int32_t* query_cat,
                           const int64_t* query_skip, int64_t slab_items, int64_t n_slabs, int K,
                           float* part_sim, int64_t* part_item, void* stream) {
  NCF_CHECK_ARG(K >= 1 && K <= kKeep, "ncf_nn_scan: need 1 <= K <= %d", kKeep);
  NCF_CHECK_ARG(dim == 16 || dim == 32 || dim == 64 || dim == 128,
                "ncf_nn_scan: dim must be 16, 32, 64 or 128");
  NCF_CHECK_ARG(slab_items >= 1, "ncf_nn_scan: slab_items must be >= 1");
  NCF_CHECK_ARG(n_queries >= 0 && n_queries <= (int64_t)kQB * 65535,
                "ncf_nn_scan: need 0 <= n_queries <= %d", kQB * 65535);
  NCF_CHECK_ARG(n_items >= 0 && n_items < (1ll << 31), "ncf_nn_scan: need 0 <= n_items < 2^31");
  NCF_CHECK_ARG(n_slabs >= 0 && n_slabs < (1ll << 31) &&
                    n_slabs >= (n_items + slab_items - 1) / slab_items,
                "ncf_nn_scan: n_slabs must cover the catalogue (>= ceil(n_items / slab_items))");
  NCF_CHECK_ARG(!(query_cat && !item_cat), "ncf_nn_scan: query_cat needs item_cat");
  if (n_queries == 0 || n_slabs == 0) return NCF_OK;
  NCF_CHECK_ARG(queries && part_sim && part_item && (vectors || n_items == 0),
                "ncf_nn_scan: null pointer");
  NCF_CHECK_ARG((((uintptr_t)queries | (uintptr_t)vectors) & 15) == 0,
                "ncf_nn_scan: queries and vectors must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
#define NN_CASE(DIM)                                                                          \
  case DIM:                                                                                   \
    return query_cat                                                                          \
               ? nn_launch<DIM, true>(queries, n_queries, normalize, vectors, n_items,       \
                                      item_cat, query_cat, query_skip, slab_items, n_slabs,  \
                                      K, part_sim, part_item, st)                            \
               : nn_launch<DIM, false>(queries, n_queries, normalize, vectors, n_items,      \
                                       nullptr, nullptr, query_skip, slab_items, n_slabs, K, \
                                       part_sim, part_item, st);
  switch (dim) {
    NN_CASE(16)
    NN_CASE(32)
    NN_CASE(64)
    default:
    NN_CASE(128)
  }
#undef NN_CASE
}
