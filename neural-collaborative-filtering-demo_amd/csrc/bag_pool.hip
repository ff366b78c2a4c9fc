// Pooled embedding bags: segmented row gather-sum (forward) and its deterministic backward.
//
// Reference (ethanshenley/Neural-Collaborative-Filtering-Demo): the four tables are torchrec
// EmbeddingBagCollections with PoolingType.SUM (src/model/architecture.py:153-190); torchrec pools
// a bag of any length (nn.EmbeddingBag mode sum / mean, per_sample_weights).  The reference's own
// call sites feed single-id bags (gather_ln.hip); this file is the general bag.
//
// Forward: a bag is owned by a group of L = D/4 lanes holding one float4 each (as a row is in
// gather_ln.hip), so a wave64 pools 64/L bags at a time: one bag per wave at D = 256, four at
// D = 64.  A group walks its bag in position order with kFwdInFlight independent row loads issued
// before the first add; groups grid-stride over the bags.  No LDS, no shuffles, no barriers.
//
// Backward: the dense [rows, D] gradient without float atomics.  ncf_dedup_ids2 (second list
// empty) sorts (id, position) stably and leaves segments (one per unique id) and pieces (a
// segment cut at every sorted position multiple of ncf_seg::PIECE = 16) in the workspace
// (segments.h).  k_bag_pos maps every position to its bag and coefficient (scale_b * w_p).  One
// lane group sums one piece in sorted-position order: the only piece of a segment goes straight
// to its gradient row; of a longer segment the first piece goes to the row, the others to a
// partial row each (the workspace's xp0 rows), and k_bag_combine adds the partial rows to the
// gradient row in piece order.  Every step is a pure function of the input: bitwise reproducible.
//
// Compact destination (NCF_BAG_COMPACT): the same pieces and the same combine with the gradient
// row of segment c at row c of a [U, D] buffer instead of row uniq[c] of the dense one
// (k_bag_pieces / k_bag_combine<D, COMPACT>: a compile-time choice of the destination index, so
// the dense instantiations are the kernels they were).  Nothing is zero-filled; U and the unique
// ids are read from the head of the workspace (include/ncf_hip.h).
#include "segments.h"

// Each multiply and add is its own IEEE operation (no fma contraction), as in gather_ln.hip: the
// sum of a bag is the written order whatever the vectoriser packs, and a bag of one id is the
// bits of ncf_gather_rows.
#pragma clang fp contract(off)

using namespace ncf_seg;

namespace {

// Independent row loads a lane group issues before the adds that consume them.  Interleaved A/B
// at D = 64, 1M-row table, 4 against 8 everywhere (and 8 against 16 in the combine): forward
// 26.5 -> 24.3 us (4,096 bags of 50) and 42.3-44.5 -> 41.8-42.5 us (20,480 bags); forward +
// backward on Zipf ids (one id 27K times) 383 -> 360 us, on uniform ids 439-441 -> 447-451 us.
// So: 8 in the forward, 4 in the piece sums (at most PIECE rows each), 16 in the combine (the
// pass whose length the most frequent id sets).
constexpr int kFwdInFlight = 8;
constexpr int kPieceInFlight = 4;
constexpr int kCombineInFlight = 16;
constexpr int kMaxBlocks = 2048;   // 8 workgroups of 256 per CU; grid-stride beyond

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 f4_scale(float4 a, float s) {
  return make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}

// [lo, hi) of bag b clamped into [0, n_ids]; *bad when the offsets decrease or leave the range
__device__ __forceinline__ void bag_range(const int64_t* __restrict__ offsets, int64_t b,
                                          int64_t n_ids, int64_t* lo, int64_t* hi, bool* bad) {
  int64_t a = offsets[b], e = offsets[b + 1];
  *bad = a < 0 || e > n_ids || e < a;
  a = a < 0 ? 0 : (a > n_ids ? n_ids : a);
  e = e < a ? a : (e > n_ids ? n_ids : e);
  *lo = a;
  *hi = e;
}

template <int D, bool W>
__global__ __launch_bounds__(256) void k_bag_pool_fwd(
    const int64_t* __restrict__ ids, int64_t n_ids, const int64_t* __restrict__ offsets,
    int64_t bags, const float* __restrict__ weights, const float* __restrict__ table, int64_t rows,
    int mean, float* __restrict__ out, int* err) {
  constexpr int L = D / 4, G = 256 / L;   // lanes per bag, bags per workgroup pass
  const int sub = threadIdx.x % L;
  const int c = sub * 4;
  for (int64_t b = (int64_t)blockIdx.x * G + threadIdx.x / L; b < bags;
       b += (int64_t)gridDim.x * G) {
    int64_t lo, hi;
    bool bad;
    bag_range(offsets, b, n_ids, &lo, &hi, &bad);
    bool oor = false;
    float4 acc = f4_zero();
    for (int64_t p = lo; p < hi; p += kFwdInFlight) {
      float4 x[kFwdInFlight];
#pragma unroll
      for (int j = 0; j < kFwdInFlight; ++j) {
        x[j] = f4_zero();
        if (p + j < hi) {
          const int64_t id = ids[p + j];
          if (id < 0 || id >= rows) {
            oor = true;
          } else {
            x[j] = ld4(table + id * D + c);
            if (W) x[j] = f4_scale(x[j], weights[p + j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kFwdInFlight; ++j)
        if (p + j < hi) acc = (p == lo && j == 0) ? x[j] : f4_add(acc, x[j]);
    }
    if (mean && hi > lo) acc = f4_scale(acc, 1.0f / (float)(hi - lo));
    st4(out + b * D + c, acc);
    if (sub == 0 && (oor || bad) && err) atomicOr(err, (oor ? 1 : 0) | (bad ? 2 : 0));
  }
}

// position -> (bag, coefficient); bag = -1 for a position no bag holds or whose id is out of range
template <int Dummy = 0>
__global__ __launch_bounds__(256) void k_bag_pos(const int64_t* __restrict__ ids, int64_t n_ids,
                                                 const int64_t* __restrict__ offsets, int64_t bags,
                                                 const float* __restrict__ weights, int64_t rows,
                                                 int mean, int32_t* __restrict__ pos_bag,
                                                 float* __restrict__ pos_coef) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_ids) return;
  // first bag whose end lies past p (offsets ascending; any other offsets still end in [0, bags])
  int64_t l = 0, r = bags;
  while (l < r) {
    const int64_t m = (l + r) >> 1;
    if (offsets[m + 1] > p) r = m; else l = m + 1;
  }
  int32_t bag = -1;
  float coef = 0.0f;
  const int64_t id = ids[p];
  if (l < bags && id >= 0 && id < rows) {
    int64_t lo, hi;
    bool bad;
    bag_range(offsets, l, n_ids, &lo, &hi, &bad);
    if (p >= lo && p < hi) {
      bag = (int32_t)l;
      coef = weights ? weights[p] : 1.0f;
      if (mean) coef = coef * (1.0f / (float)(hi - lo));
    }
  }
  pos_bag[p] = bag;
  pos_coef[p] = coef;
}

// row of segment c in the gradient buffer: uniq[c] (dense [rows, D]) or c (compact [U, D])
template <bool COMPACT>
__device__ __forceinline__ int64_t dest_row(const int64_t* __restrict__ uniq, uint32_t c) {
  if (COMPACT) return (int64_t)c;
  return uniq[c];
}

// one lane group per piece (<= PIECE sorted positions of one id), summed in sorted-position order
template <int D, bool COMPACT>
__global__ __launch_bounds__(256) void k_bag_pieces(
    const uint32_t* __restrict__ sv, const uint32_t* __restrict__ pstart,
    const uint32_t* __restrict__ pseg, const int64_t* __restrict__ uniq,
    const uint32_t* __restrict__ totals, const int32_t* __restrict__ pos_bag,
    const float* __restrict__ pos_coef, const float* __restrict__ grad_out,
    float* __restrict__ grad_table, float* __restrict__ partial) {
  constexpr int L = D / 4, G = 256 / L;
  const int c4 = (threadIdx.x % L) * 4;
  const int64_t Pn = totals[2];
  for (int64_t p = (int64_t)blockIdx.x * G + threadIdx.x / L; p < Pn;
       p += (int64_t)gridDim.x * G) {
    const uint32_t ps = pseg[p];
    const uint32_t c = ps & ~FIRST_PIECE;
    const int64_t i0 = pstart[p], i1 = pstart[p + 1];
    float4 acc = f4_zero();
    for (int64_t i = i0; i < i1; i += kPieceInFlight) {
      float4 g[kPieceInFlight];
#pragma unroll
      for (int j = 0; j < kPieceInFlight; ++j) {
        g[j] = f4_zero();
        if (i + j < i1) {
          const uint32_t pos = sv[i + j];
          const int32_t b = pos_bag[pos];
          if (b >= 0) g[j] = f4_scale(ld4(grad_out + (int64_t)b * D + c4), pos_coef[pos]);
        }
      }
#pragma unroll
      for (int j = 0; j < kPieceInFlight; ++j)
        if (i + j < i1) acc = f4_add(acc, g[j]);
    }
    if (ps & FIRST_PIECE) st4(grad_table + dest_row<COMPACT>(uniq, c) * D + c4, acc);
    else st4(partial + (p - c - 1) * D + c4, acc);   // non-first pieces before p: p - (c + 1)
  }
}

// segments of more than one piece: gradient row (its first piece) + the partial rows, in order
template <int D, bool COMPACT>
__global__ __launch_bounds__(256) void k_bag_combine(const uint32_t* __restrict__ fpiece,
                                                     const int64_t* __restrict__ uniq,
                                                     const uint32_t* __restrict__ totals,
                                                     const float* __restrict__ partial,
                                                     float* __restrict__ grad_table) {
  constexpr int L = D / 4, G = 256 / L;
  const int c4 = (threadIdx.x % L) * 4;
  const int64_t U = totals[0];
  for (int64_t c = (int64_t)blockIdx.x * G + threadIdx.x / L; c < U;
       c += (int64_t)gridDim.x * G) {
    const int64_t p0 = fpiece[c], p1 = fpiece[c + 1];
    if (p1 - p0 <= 1) continue;
    float* row = grad_table + dest_row<COMPACT>(uniq, (uint32_t)c) * D + c4;
    float4 acc = ld4(row);
    const float* part = partial + (p0 - c) * D + c4;   // partial row of piece p0 + 1
    const int64_t m = p1 - p0 - 1;
    for (int64_t q = 0; q < m; q += kCombineInFlight) {
      float4 g[kCombineInFlight];
#pragma unroll
      for (int j = 0; j < kCombineInFlight; ++j)
        g[j] = q + j < m ? ld4(part + (q + j) * D) : f4_zero();
#pragma unroll
      for (int j = 0; j < kCombineInFlight; ++j)
        if (q + j < m) acc = f4_add(acc, g[j]);
    }
    st4(row, acc);
  }
}

// grad_weights[p] = <grad_out[bag(p)], table[ids[p]]>; 0 where the position contributes nothing
template <int D>
__global__ __launch_bounds__(256) void k_bag_grad_weights(
    const int64_t* __restrict__ ids, int64_t n_ids, const int32_t* __restrict__ pos_bag,
    const float* __restrict__ table, const float* __restrict__ grad_out,
    float* __restrict__ grad_weights) {
  constexpr int L = D / 4;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = t / L;
  const int c4 = (int)(t % L) * 4;
  if (p >= n_ids) return;   // whole groups retire together
  const int32_t b = pos_bag[p];
  float dot = 0.0f;
  if (b >= 0) {   // (uniform in the lane group; pos_bag < 0 covers an id out of range)
    const float4 x = ld4(table + ids[p] * D + c4), g = ld4(grad_out + (int64_t)b * D + c4);
    dot = x.x * g.x + x.y * g.y + x.z * g.z + x.w * g.w;
  }
  dot = group_sum<L>(dot);
  if (c4 == 0) grad_weights[p] = dot;
}

int grid_for(int64_t items, int per_block) {
  int64_t b = (items + per_block - 1) / per_block;
  if (b < 1) b = 1;
  return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}

template <int D>
int launch_bag_fwd(const int64_t* ids, int64_t n_ids, const int64_t* offsets, int64_t bags,
                   const float* weights, const float* table, int64_t rows, int mean, float* out,
                   int* err, hipStream_t st) {
  const dim3 grid(grid_for(bags, 256 / (D / 4)));
  if (weights)
    hipLaunchKernelGGL((k_bag_pool_fwd<D, true>), grid, dim3(256), 0, st, ids, n_ids, offsets,
                       bags, weights, table, rows, mean, out, err);
  else
    hipLaunchKernelGGL((k_bag_pool_fwd<D, false>), grid, dim3(256), 0, st, ids, n_ids, offsets,
                       bags, weights, table, rows, mean, out, err);
  NCF_CHECK_LAUNCH("ncf_bag_pool_fwd");
  return NCF_OK;
}

// workspace: the output block (include/ncf_hip.h: U uint32[2] at NCF_BAG_WS_COUNT_OFFSET, uniq ids
// int64[n + 2] at NCF_BAG_WS_IDS_OFFSET) | the dedup's (segments.h) | pos_bag int32[n] | pos_coef
// f32[n]; one layout and one size for the dense and the compact call
struct BagWS {
  uint32_t* count;
  int64_t* uniq;
  void* dedup;
  int64_t dedup_bytes;
  int32_t* pos_bag;
  float* pos_coef;
};
static_assert(NCF_BAG_WS_COUNT_OFFSET == 0 && NCF_BAG_WS_IDS_OFFSET == 256, "workspace head");
int64_t bag_ws_bytes(int64_t n, int64_t D) {
  return NCF_BAG_WS_IDS_OFFSET + round256(8 * (n + 2)) + round256(ws_bytes(n, D)) +
         2 * round256(4 * (n + 2));
}
BagWS bag_carve(void* base, int64_t n, int64_t D) {
  BagWS w;
  char* p = (char*)base;
  w.count = (uint32_t*)(p + NCF_BAG_WS_COUNT_OFFSET);
  p += NCF_BAG_WS_IDS_OFFSET;
  w.uniq = (int64_t*)p;
  p += round256(8 * (n + 2));
  w.dedup = p;
  w.dedup_bytes = ws_bytes(n, D);
  p += round256(w.dedup_bytes);
  w.pos_bag = (int32_t*)p;
  p += round256(4 * (n + 2));
  w.pos_coef = (float*)p;
  return w;
}

template <int D, bool COMPACT>
int launch_bag_table_grad(const WS& w, const uint32_t* sv, const BagWS& b, int64_t n_ids,
                          const float* grad_out, float* grad_table, hipStream_t st) {
  constexpr int G = 256 / (D / 4);
  hipLaunchKernelGGL((k_bag_pieces<D, COMPACT>), dim3(grid_for(pieces_max(n_ids), G)), dim3(256),
                     0, st, sv, w.pstart0, w.pseg0, b.uniq, w.totals, b.pos_bag, b.pos_coef,
                     grad_out, grad_table, w.xp0);
  NCF_CHECK_LAUNCH("ncf_bag_pool_bwd(pieces)");
  hipLaunchKernelGGL((k_bag_combine<D, COMPACT>), dim3(grid_for(n_ids, G)), dim3(256), 0, st,
                     w.fpiece0, b.uniq, w.totals, w.xp0, grad_table);
  NCF_CHECK_LAUNCH("ncf_bag_pool_bwd(combine)");
  return NCF_OK;
}

template <int D>
int launch_bag_bwd(const int64_t* ids, int64_t n_ids, const BagWS& b, const float* table,
                   const float* grad_out, int64_t rows, float* grad_table, float* grad_weights,
                   bool compact, hipStream_t st) {
  const WS w = carve(b.dedup, n_ids, D);
  uint32_t *k0, *v0, *k1, *v1;
  sorted_bufs(w, sort_passes(rows, 1), &k0, &v0, &k1, &v1);
  if (grad_table) {
    const int rc = compact
        ? launch_bag_table_grad<D, true>(w, v0, b, n_ids, grad_out, grad_table, st)
        : launch_bag_table_grad<D, false>(w, v0, b, n_ids, grad_out, grad_table, st);
    if (rc != NCF_OK) return rc;
  }
  if (grad_weights) {
    hipLaunchKernelGGL((k_bag_grad_weights<D>), dim3(ncf_cdiv(n_ids * (D / 4), 256)), dim3(256), 0,
                       st, ids, n_ids, b.pos_bag, table, grad_out, grad_weights);
    NCF_CHECK_LAUNCH("ncf_bag_pool_bwd(weights)");
  }
  return NCF_OK;
}

#define NCF_BAG_DISPATCH_D(D, FN, ...)                                                       \
  switch (D) {                                                                               \
    case 16: return FN<16>(__VA_ARGS__);                                                     \
    case 32: return FN<32>(__VA_ARGS__);                                                     \
    case 64: return FN<64>(__VA_ARGS__);                                                     \
    case 128: return FN<128>(__VA_ARGS__);                                                   \
    case 256: return FN<256>(__VA_ARGS__);                                                   \
    default: ncf_set_error("unsupported embedding dim %lld (16/32/64/128/256)", (long long)D); \
      return NCF_ERR_ARG;                                                                    \
  }

bool dim_ok(int64_t d) { return d == 16 || d == 32 || d == 64 || d == 128 || d == 256; }

}  // namespace

extern "C" int ncf_bag_pool_fwd(const int64_t* ids, int64_t n_ids, const int64_t* offsets,
                                int64_t bags, const float* weights, const float* table,
                                int64_t rows, int64_t dim, int mode, float* out, int* err_flag,
                                void* stream) {
  NCF_CHECK_ARG(n_ids >= 0 && bags >= 0 && rows >= 0, "ncf_bag_pool_fwd: negative size");
  NCF_CHECK_ARG(mode == 0 || mode == 1, "ncf_bag_pool_fwd: mode must be 0 (sum) or 1 (mean)");
  NCF_CHECK_ARG(dim_ok(dim), "unsupported embedding dim %lld (16/32/64/128/256)", (long long)dim);
  if (bags == 0) return NCF_OK;
  NCF_CHECK_ARG(offsets && out && (n_ids == 0 || (ids && table)),
                "ncf_bag_pool_fwd: null pointer");
  NCF_BAG_DISPATCH_D(dim, launch_bag_fwd, ids, n_ids, offsets, bags, weights, table, rows, mode,
                     out, err_flag, (hipStream_t)stream);
}

extern "C" int64_t ncf_bag_pool_bwd_workspace(int64_t n_ids, int64_t bags, int64_t dim) {
  (void)bags;   // (the position-to-bag map is per id; nothing is kept per bag)
  return bag_ws_bytes(n_ids < 0 ? 0 : n_ids, dim);
}

extern "C" int ncf_bag_pool_bwd(const int64_t* ids, int64_t n_ids, const int64_t* offsets,
                                int64_t bags, const float* weights, const float* table,
                                const float* grad_out, int64_t rows, int64_t dim, int mode,
                                float* grad_table, float* grad_weights, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  NCF_CHECK_ARG(n_ids >= 0 && n_ids < (1ll << 30) && bags >= 0 && bags < (1ll << 31),
                "ncf_bag_pool_bwd: bad n_ids / bags");
  NCF_CHECK_ARG(rows >= 0 && rows <= (1ll << 32), "ncf_bag_pool_bwd: rows must be in [0, 2^32]");
  const bool compact = (mode & NCF_BAG_COMPACT) != 0;
  mode &= ~NCF_BAG_COMPACT;
  NCF_CHECK_ARG(mode == 0 || mode == 1,
                "ncf_bag_pool_bwd: mode must be 0 (sum) or 1 (mean), NCF_BAG_COMPACT the only flag");
  NCF_CHECK_ARG(dim_ok(dim), "unsupported embedding dim %lld (16/32/64/128/256)", (long long)dim);
  NCF_CHECK_ARG(grad_weights == nullptr || (mode == 0 && (table || n_ids == 0)),
                "ncf_bag_pool_bwd: grad_weights is for mode 0 (sum) and needs the table");
  NCF_CHECK_ARG(grad_table || grad_weights, "ncf_bag_pool_bwd: no gradient asked for");
  NCF_CHECK_ARG(!compact || (grad_table && workspace),
                "ncf_bag_pool_bwd: NCF_BAG_COMPACT needs grad_table and the workspace");
  hipStream_t st = (hipStream_t)stream;
  const auto ws_short = [&]() {
    if (workspace_bytes >= bag_ws_bytes(n_ids, dim)) return false;
    ncf_set_error("ncf_bag_pool_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes,
                  (long long)bag_ws_bytes(n_ids, dim));
    return true;
  };
  // dense: the O(rows) zero-fill; compact: nothing but the rows of the unique ids is written
  if (!compact && grad_table && rows > 0 &&
      hipMemsetAsync(grad_table, 0, (size_t)rows * dim * sizeof(float), st) != hipSuccess) {
    ncf_set_error("ncf_bag_pool_bwd: zero-fill of grad_table failed");
    return NCF_ERR_LAUNCH;
  }
  if (n_ids == 0 || rows == 0) {
    if (compact) {   // U = 0 in the output block, nothing else
      if (ws_short()) return NCF_ERR_WORKSPACE;
      if (hipMemsetAsync((char*)workspace + NCF_BAG_WS_COUNT_OFFSET, 0, 2 * sizeof(uint32_t),
                         st) != hipSuccess) {
        ncf_set_error("ncf_bag_pool_bwd: zeroing the unique count failed");
        return NCF_ERR_LAUNCH;
      }
    }
    if (grad_weights && n_ids > 0)
      (void)hipMemsetAsync(grad_weights, 0, (size_t)n_ids * sizeof(float), st);
    return NCF_OK;
  }
  NCF_CHECK_ARG(ids && offsets && (grad_out || bags == 0) && workspace,
                "ncf_bag_pool_bwd: null pointer");
  if (ws_short()) return NCF_ERR_WORKSPACE;
  const BagWS b = bag_carve(workspace, n_ids, dim);
  if (grad_table) {
    // (count[0] = U, count[1] = 0 for the empty second list: the head of the workspace)
    const int rc = ncf_dedup_ids2(ids, n_ids, rows, nullptr, 0, 1, dim, b.uniq, nullptr, nullptr,
                                  nullptr, b.count, b.dedup, b.dedup_bytes, stream);
    if (rc != NCF_OK) return rc;
  }
  hipLaunchKernelGGL(k_bag_pos<>, dim3(ncf_cdiv(n_ids, 256)), dim3(256), 0, st, ids, n_ids,
                     offsets, bags, weights, rows, mode, b.pos_bag, b.pos_coef);
  NCF_CHECK_LAUNCH("ncf_bag_pool_bwd(positions)");
  NCF_BAG_DISPATCH_D(dim, launch_bag_bwd, ids, n_ids, b, table, grad_out, rows, grad_table,
                     grad_weights, compact, st);
}
