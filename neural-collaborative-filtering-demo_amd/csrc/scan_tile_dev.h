// The fp32 MFMA scan tile shared by the scoring kernels (score.hip k_collect, rank.hip k_rank /
// pair_logit, neighbors.hip k_nn_scan): 32 query rows x 32 items per wave on
// v_mfma_f32_32x32x2_f32.  Every fp32 logit these kernels compare comes from the ONE arithmetic
// written here: a chain of D/2 MFMA steps from a zero accumulator, step s at k = s + (D/2) h
// (h: the lane half), and then, where there is a bias, one separate fp32 add.  An f32 MFMA output
// element is the k-ordered fmaf chain of its A row and B column, whatever its place in the tile,
// so the same row and item give the same bits in every kernel built from these pieces.
#pragma once
#include "ncf_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kItemTile = 32;   // items per tile (the MFMA's 32 columns)
constexpr int kScanRows = 256;  // query rows per workgroup of scan_tiles: 8 waves x 32

// the query row (of the wave's 32) whose logit accumulator register r holds in lane half h; the
// item is the lane's column, lane & 31
__host__ __device__ __forceinline__ constexpr int scan_row(int r, int h) {
  return (r & 3) + 8 * (r >> 2) + 4 * h;
}

// The map inverted on the tile's diagonal: the dot product of row i with column i (lanes i and
// i + 32) is in lane half scan_diag_half(i), register scan_diag_reg(i).
__host__ __device__ __forceinline__ constexpr int scan_diag_half(int i) { return (i >> 2) & 1; }
__host__ __device__ __forceinline__ constexpr int scan_diag_reg(int i) { return (i & 3) + 4 * (i >> 3); }
constexpr bool scan_diag_inverts_row() {
  for (int i = 0; i < 32; ++i)
    if (scan_row(scan_diag_reg(i), scan_diag_half(i)) != i) return false;
  return true;
}
static_assert(scan_diag_inverts_row(), "scan_diag_* must invert scan_row");

// This lane's half of an operand row in registers, k-permuted: p points at the row's element
// (D/2) h, so MFMA step s of lane half h multiplies k = s + (D/2) h.  !valid: zeros, nothing read.
template <int KH>
__device__ __forceinline__ void scan_load_half(const float* __restrict__ p, float (&a)[KH],
                                               bool valid = true) {
#pragma unroll
  for (int v = 0; v < KH / 4; ++v) {
    const float4 x = valid ? ld4(p + 4 * v) : make_float4(0.f, 0.f, 0.f, 0.f);
    a[4 * v] = x.x; a[4 * v + 1] = x.y; a[4 * v + 2] = x.z; a[4 * v + 3] = x.w;
  }
}

// Consume the query registers before a tile loop: with their loads still pending at the loop
// header the compiler's wait-count pass puts a vmcnt(0) in front of their first MFMA in EVERY
// iteration, which also drains the next tile's prefetch and exposes its HBM latency (measured:
// the matrix cores idle half the time).
template <int KH>
__device__ __forceinline__ void scan_consume(const float (&a)[KH]) {
#pragma unroll
  for (int k = 0; k < KH; ++k) asm volatile("" ::"v"(a[k]));
}

// The chain: from a zero accumulator, steps s = 0 .. KH - 1 in order, a[s] against b[s] (b: an
// LDS tile row or registers).  acc[r] = the dot product of row scan_row(r, h) and column lane & 31.
template <int KH, typename B>
__device__ __forceinline__ f32x16 scan_chain(const float (&a)[KH], const B& b) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int s = 0; s < KH; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
  return acc;
}

// The workgroup tile loop of k_collect and k_rank: 512 threads (8 waves, each with its 32 query
// rows in `a`) stream the 32-item tiles of [it0, it1) through double-buffered LDS ([32][D + 1]
// pitch: conflict-free, and the tiles' biases) behind a one-tile register prefetch.  One barrier
// per tile: a wave writes a buffer again two tiles on, after the barrier of the tile between,
// which every wave passes only when it has read this one.  The next tile's loads are issued
// behind the barrier (clamped, unconditional addresses), then the chain runs and
// consume(acc, b, item, ivalid) gets the wave's 32 x 32 products, the lane's item (t0 + lane & 31),
// its bias and whether it lies inside the block.  after_barrier() runs right behind the tile's
// barrier, uniformly (k_collect's candidate flush).
template <int D, typename After, typename Consume>
__device__ __forceinline__ void scan_tiles(const float (&a)[D / 2], const float* __restrict__ items,
                                           const float* __restrict__ bias, int64_t it0,
                                           int64_t it1, After&& after_barrier, Consume&& consume) {
  static_assert(D == 64 || D == 128, "the fp32 scan takes 64- or 128-deep rows");
  constexpr int KH = D / 2;      // k per lane half
  constexpr int NV = D / 64;     // float4 per thread to stage a 32 x D tile
  __shared__ float ps[2][kItemTile][D + 1];
  __shared__ float bs[2][kItemTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const int i = lane & 31, h = lane >> 5;
  // staging: 512 threads x NV float4 = one 32 x D tile
  const int sj = tid >> 4, sk = (tid & 15) * 4;
  float4 pv[NV];
  float pb = 0.0f;
  auto fetch = [&](int64_t t0) {
    const int64_t item = t0 + sj;
    const int64_t src = item < it1 ? item : it0;  // clamped, unconditional
#pragma unroll
    for (int c = 0; c < NV; ++c) pv[c] = ld4(items + src * D + sk + 64 * c);
    pb = bias[src];
  };
  // the load of tile t + 1 is issued while tile t is multiplied
  if (it0 < it1) fetch(it0);
  int buf = 0;
  for (int64_t t0 = it0; t0 < it1; t0 += kItemTile) {
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      float* dst = &ps[buf][sj][sk + 64 * c];
      dst[0] = pv[c].x; dst[1] = pv[c].y; dst[2] = pv[c].z; dst[3] = pv[c].w;
    }
    if ((tid & 15) == 0) bs[buf][sj] = pb;
    __syncthreads();
    after_barrier();
    if (t0 + kItemTile < it1) fetch(t0 + kItemTile);
    const f32x16 acc = scan_chain<KH>(a, &ps[buf][i][KH * h]);
    const int64_t item = t0 + i;
    consume(acc, bs[buf][i], item, item < it1);
    buf ^= 1;
  }
}

// The item split of a scan_tiles launch over n_rows rows and n_items items: items per workgroup
// (a multiple of the tile) such that the grid fills the chip (>= ~1024 workgroups, ~2 per CU
// and more) with >= 8 tiles each.  The grid is ceil(n_items / per) x ceil(n_rows / kScanRows).
static inline int64_t scan_items_per_block(int64_t n_rows, int64_t n_items) {
  const int64_t rb = (n_rows + kScanRows - 1) / kScanRows;
  int64_t splits = (1024 + rb - 1) / rb;
  const int64_t max_splits = (n_items + 8 * kItemTile - 1) / (8 * kItemTile);
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  const int64_t per = (n_items + splits - 1) / splits;
  return (per + kItemTile - 1) / kItemTile * kItemTile;
}
