// Exact rank of one held-out item per queried row over the whole catalogue (leave-one-out
// evaluation): place[r] = #{ j not in seen(u_r) : beats(j) }, 0-based, with
//   beats(j) = (s_j > s_h and j != h) or (s_j == s_h and j < h)
// the (score desc, item id asc) order of the top-k pipeline (score.hip) and s the fp32 logit
// q_r . p_j + bias_j of the factorised scorer.  A count: no candidate lists, caps, thresholds or
// re-runs, and an integer result, so the atomics leave it deterministic.
//
// Every logit compared here comes from ONE arithmetic, scan_tile_dev.h's scan_chain (the one
// score.hip's k_collect runs): D/2 v_mfma_f32_32x32x2_f32 from a zero accumulator with MFMA step
// s at k = s + (D/2)h (h: the lane half), then one fp32 add of the bias.  An f32 MFMA output
// element is the k-ordered fmaf chain of its A row and B column, whatever its place in the
// 32 x 32 tile, so the held-out item's logit (ncf_rank_pair_logits: 32 (row, item) pairs per wave on the tile's diagonal), the scan's
// logit of the same item (k_rank) and a seen item's logit (k_seen_correct, diagonal again) are the
// same bits, and two items with bit-identical row and bias tie exactly.  The j != h guard keeps an
// item from beating itself even if that did not hold.
//   1. ncf_rank_pair_logits   target[r] = s of (row r, held[r]);
//   2. ncf_rank_scan          count[r] += #{ j in the block's items : beats(j) } (k_rank: the
//                             tile loop of score.hip's k_collect, scan_tiles, with a count as
//                             its consumer);
//   3. ncf_rank_seen_correct  count[r] -= #{ j in seen(u_r) : beats(j) }, O(seen) work, so the
//                             scan needs no per-item lookup.
#include "ncf_common.h"
#include "scan_tile_dev.h"

namespace {

constexpr int kBadItem = 4;          // err_flag bit: an item id outside the catalogue

// beats(j) as 0 / 1 without a branch (a lower id beats at s >= s_h, a higher one at s > s_h, h
// itself never): the scan evaluates it 16 times per lane and tile, and a branch per row there
// drains the prefetched tile at every s_waitcnt behind it
__device__ __forceinline__ int32_t beats(float s, int32_t j, float sh, int32_t h) {
  return ((int32_t)(j < h) & (int32_t)(s >= sh)) | ((int32_t)(j > h) & (int32_t)(s > sh));
}

// The logit of pair i (i = lane & 31) of a wave's 32 (query row, item) pairs: lane (i, h) passes
// its pair's row and item pointers advanced by (D/2)h.  The 32 x 32 product of the 32 rows and
// the 32 items holds pair i's dot product on its diagonal: column i (lanes i and i + 32), row i,
// so in lane half scan_diag_half(i), register scan_diag_reg(i).
// Returns it (plus b) in that lane, `own` true there; every lane of the wave must call this.
template <int D>
__device__ __forceinline__ float pair_logit(const float* __restrict__ qp,
                                            const float* __restrict__ pp, float b, int i, int h,
                                            bool& own) {
  constexpr int KH = D / 2;
  float x[KH], y[KH];
  scan_load_half<KH>(qp, x);
  scan_load_half<KH>(pp, y);
  const f32x16 acc = scan_chain<KH>(x, y);
  own = h == scan_diag_half(i);
  const int rsel = scan_diag_reg(i);
  float d = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) d = r == rsel ? acc[r] : d;
  return d + b;
}

// ---- 1. pair logits: one wave per 32 pairs
template <int D>
__global__ __launch_bounds__(256) void k_pair_logits(
    const float* __restrict__ q, int64_t n_queries, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ pair_item, int64_t n_pairs, const float* __restrict__ items,
    const float* __restrict__ bias, int64_t n_items, float* __restrict__ out,
    int* __restrict__ err) {
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const int64_t e = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + i;
  const bool valid = e < n_pairs;   // (a wave past the list still runs the MFMAs, on pair 0)
  const int64_t ee = valid ? e : 0;
  int64_t row = rows ? rows[ee] : ee;
  int64_t item = pair_item[ee];
  if (row < 0 || row >= n_queries || item < 0 || item >= n_items) {
    if (err && valid && h == 0) atomicOr(err, kBadItem);
    row = 0;
    item = 0;
  }
  bool own;
  const float s = pair_logit<D>(q + row * D + (D / 2) * h, items + item * D + (D / 2) * h,
                                bias[item], i, h, own);
  if (own && valid) out[e] = s;
}

// ---- 2. the scan.  k_collect's tiling (scan_tile_dev.h scan_tiles): a 512-thread workgroup
// owns 256 queried rows (8 waves x 32), q in registers, 32-item tiles of p and bias through the
// shared tile loop; per tile a wave adds beats() of its 32 x 32 logits into 16 per-lane counters
// (row scan_row(r, h), item = the lane's column).  After the loop the 32 lanes of a half are
// summed and lanes 0..15 of each half add one row's count to count[row].
template <int D>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(D == 64 ? 4 : 2))) void k_rank(
    const float* __restrict__ q, int64_t n_rows, const float* __restrict__ items,
    const float* __restrict__ bias, int64_t n_items, int64_t items_per_block,
    const float* __restrict__ target, const int32_t* __restrict__ held,
    int32_t* __restrict__ count) {
  constexpr int KH = D / 2;      // k per lane half (MFMA step s: k = s + KH h)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int64_t slot0 = (int64_t)blockIdx.y * kScanRows + w * 32;
  const int64_t my_row = slot0 + i < n_rows ? slot0 + i : 0;
  float a[KH];
  scan_load_half<KH>(q + my_row * D + KH * h, a);
  scan_consume<KH>(a);
  // the 16 rows whose logits this lane holds: target logit, held-out id, running count.  A row
  // past n_rows never counts (+inf target, id -1) and is never written.
  float tg[16];
  int32_t hid[16], cnt[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t s = slot0 + scan_row(r, h);
    const bool v = s < n_rows;
    tg[r] = v ? target[s] : INFINITY;
    hid[r] = v ? held[s] : -1;
    cnt[r] = 0;
  }
  const int64_t it0 = (int64_t)blockIdx.x * items_per_block;
  const int64_t it1 = min(n_items, it0 + items_per_block);
  scan_tiles<D>(
      a, items, bias, it0, it1, [] {},
      [&](const f32x16& acc, float b, int64_t item64, bool inside) {
        const int32_t item = (int32_t)item64;
        const int32_t ivalid = inside ? 1 : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) cnt[r] += beats(acc[r] + b, item, tg[r], hid[r]) & ivalid;
      });
  // sum over the 32 lanes of a half (xor offsets < 32 stay inside it); lane i < 16 of half h
  // then owns row scan_row(i, h)
  int32_t mine = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int32_t c = cnt[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    mine = i == r ? c : mine;
  }
  if (i < 16) {
    const int64_t s = slot0 + scan_row(i, h);
    if (s < n_rows && mine != 0) atomicAdd(&count[s], mine);
  }
}

// ---- 3. seen correction: one wave per queried row walks its user's seen items 32 at a time
// (their logits on the diagonal of the row's q against 32 item rows) and takes the ones that
// beat the held-out item off the row's count.  Runs after the scan on the same stream.
template <int D>
__global__ __launch_bounds__(256) void k_seen_correct(
    const float* __restrict__ q, int64_t n_rows, const int32_t* __restrict__ held,
    const float* __restrict__ target, const int64_t* __restrict__ user_ids, int64_t num_users,
    const int64_t* __restrict__ seen_offsets, const int32_t* __restrict__ seen_items,
    const float* __restrict__ items, const float* __restrict__ bias, int64_t n_items,
    int32_t* __restrict__ count, int* __restrict__ err) {
  const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;   // (whole waves)
  const int64_t u = user_ids[row];
  if (u < 0 || u >= num_users) return;   // no list (the queries kernel flags the id)
  const int64_t o0 = seen_offsets[u];
  const int64_t len = seen_offsets[u + 1] - o0;
  const float sh = target[row];
  const int32_t hd = held[row];
  const float* qp = q + row * D + (D / 2) * h;
  int32_t total = 0;
  for (int64_t c0 = 0; c0 < len; c0 += 32) {   // (wave-uniform trip count)
    bool valid = c0 + i < len;
    int64_t item = valid ? seen_items[o0 + c0 + i] : 0;
    if (item < 0 || item >= n_items) {
      if (err && h == 0) atomicOr(err, kBadItem);
      valid = false;
      item = 0;
    }
    bool own;
    const float s = pair_logit<D>(qp, items + item * D + (D / 2) * h, bias[item], i, h, own);
    total += __popcll(__ballot(own && valid && beats(s, (int32_t)item, sh, hd)));
  }
  if (lane == 0 && total != 0) count[row] -= total;
}

}  // namespace

extern "C" int ncf_rank_pair_logits(const float* queries, int64_t n_queries, const int32_t* rows,
                                    const int32_t* pair_items, int64_t n_pairs,
                                    const float* items, const float* item_bias, int64_t n_items,
                                    int64_t dim, float* out, int* err_flag, void* stream) {
  NCF_CHECK_ARG(dim == 64 || dim == 128, "ncf_rank_pair_logits: dim must be 64 or 128");
  NCF_CHECK_ARG(n_pairs >= 0 && n_queries >= 0 && n_items >= 0 && n_items < (1ll << 31),
                "ncf_rank_pair_logits: bad size");
  if (n_pairs == 0) return NCF_OK;
  NCF_CHECK_ARG(n_queries >= 1 && n_items >= 1 && queries && pair_items && items && item_bias && out,
                "ncf_rank_pair_logits: pairs over an empty query or item set, or a null pointer");
  NCF_CHECK_ARG((((uintptr_t)queries | (uintptr_t)items) & 15) == 0,
                "ncf_rank_pair_logits: rows must be 16-B aligned");
  const dim3 grid((unsigned)ncf_cdiv(n_pairs, 128));
  if (dim == 64)
    hipLaunchKernelGGL(k_pair_logits<64>, grid, dim3(256), 0, (hipStream_t)stream, queries,
                       n_queries, rows, pair_items, n_pairs, items, item_bias, n_items, out,
                       err_flag);
  else
    hipLaunchKernelGGL(k_pair_logits<128>, grid, dim3(256), 0, (hipStream_t)stream, queries,
                       n_queries, rows, pair_items, n_pairs, items, item_bias, n_items, out,
                       err_flag);
  NCF_CHECK_LAUNCH("ncf_rank_pair_logits");
  return NCF_OK;
}

extern "C" int ncf_rank_scan(const float* queries, int64_t n_rows, const float* items,
                             const float* item_bias, int64_t n_items, int64_t dim,
                             const float* target, const int32_t* held, int64_t items_per_block,
                             int32_t* count, void* stream) {
  NCF_CHECK_ARG(dim == 64 || dim == 128, "ncf_rank_scan: dim must be 64 or 128");
  NCF_CHECK_ARG(n_rows >= 0 && n_items >= 0 && n_items < (1ll << 31) && items_per_block >= 0 &&
                    items_per_block % kItemTile == 0,
                "ncf_rank_scan: bad size (items_per_block: 0 or a multiple of %d)", kItemTile);
  if (n_rows == 0 || n_items == 0) return NCF_OK;
  NCF_CHECK_ARG(queries && items && item_bias && target && held && count,
                "ncf_rank_scan: null pointer");
  NCF_CHECK_ARG((((uintptr_t)queries | (uintptr_t)items) & 15) == 0,
                "ncf_rank_scan: rows must be 16-B aligned");
  const int64_t per = items_per_block ? items_per_block : scan_items_per_block(n_rows, n_items);
  const int64_t splits = (n_items + per - 1) / per;
  const int64_t rb = (n_rows + kScanRows - 1) / kScanRows;
  NCF_CHECK_ARG(rb < 65536, "ncf_rank_scan: too many rows per call (max %d)", 65535 * 256);
  const dim3 grid((unsigned)splits, (unsigned)rb);
  if (dim == 64)
    hipLaunchKernelGGL(k_rank<64>, grid, dim3(512), 0, (hipStream_t)stream, queries, n_rows, items,
                       item_bias, n_items, per, target, held, count);
  else
    hipLaunchKernelGGL(k_rank<128>, grid, dim3(512), 0, (hipStream_t)stream, queries, n_rows,
                       items, item_bias, n_items, per, target, held, count);
  NCF_CHECK_LAUNCH("ncf_rank_scan");
  return NCF_OK;
}

extern "C" int ncf_rank_seen_correct(const float* queries, int64_t n_rows, const int32_t* held,
                                     const float* target, const int64_t* user_ids,
                                     int64_t num_users, const int64_t* seen_offsets,
                                     const int32_t* seen_items, const float* items,
                                     const float* item_bias, int64_t n_items, int64_t dim,
                                     int32_t* count, int* err_flag, void* stream) {
  NCF_CHECK_ARG(dim == 64 || dim == 128, "ncf_rank_seen_correct: dim must be 64 or 128");
  NCF_CHECK_ARG(n_rows >= 0 && num_users >= 0 && n_items >= 0 && n_items < (1ll << 31),
                "ncf_rank_seen_correct: bad size");
  if (n_rows == 0 || n_items == 0 || num_users == 0) return NCF_OK;
  NCF_CHECK_ARG(queries && held && target && user_ids && seen_offsets && items && item_bias &&
                    count,
                "ncf_rank_seen_correct: null pointer");
  NCF_CHECK_ARG((((uintptr_t)queries | (uintptr_t)items) & 15) == 0,
                "ncf_rank_seen_correct: rows must be 16-B aligned");
  const dim3 grid((unsigned)ncf_cdiv(n_rows, 4));
  if (dim == 64)
    hipLaunchKernelGGL(k_seen_correct<64>, grid, dim3(256), 0, (hipStream_t)stream, queries,
                       n_rows, held, target, user_ids, num_users, seen_offsets, seen_items, items,
                       item_bias, n_items, count, err_flag);
  else
    hipLaunchKernelGGL(k_seen_correct<128>, grid, dim3(256), 0, (hipStream_t)stream, queries,
                       n_rows, held, target, user_ids, num_users, seen_offsets, seen_items, items,
                       item_bias, n_items, count, err_flag);
  NCF_CHECK_LAUNCH("ncf_rank_seen_correct");
  return NCF_OK;
}
