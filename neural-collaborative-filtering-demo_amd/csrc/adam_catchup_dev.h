// The deferred table Adam's catch-up of listed rows, as device code: the replay of the
// zero-gradient steps a row owes (catch_up_row) and the body of the both-kinds catch-up
// (pairs_catchup_body).  One definition for every kernel that replays rows: the catch-up, sweep
// and claim kernels of adam.hip and the fused tail launch of reduce.hip (k_reduce1_catchup) take
// the same arithmetic in the same order, so every schedule gives the same bits.
#pragma once
#include <cstddef>
#include "ncf_common.h"
#include "adam_math.h"

namespace ncf_adam {
namespace {

// ---- deferred dense-exact schedule -------------------------------------------------------
// A row that receives no gradient at step s still takes the step with g = 0 (weight decay only).
// Instead of streaming every untouched row every step, rows carry stamp[row] = the last step
// their (p, m, v) reflect; before a row is READ it is caught up by replaying the missing
// zero-gradient steps s = stamp+1 .. target with that step's scalars (step table, 4 floats per
// step: [4s] = -lr/(1-b1^s), [4s+1] = 1/sqrt(1-b2^s) for the gradient step adam1, [4s+2] / [4s+3]
// = ra / rb for the zero-gradient step adam0), element by element, with the very same adam0
// arithmetic as the dense sweep's untouched rows.
// Results are bit-identical to the dense sweep; the cost moves from HBM traffic to VALU work.
struct TablePtrs {
  float *p0, *m0, *v0, *p1, *m1, *v1;  // two tables sharing the row index space (GMF + MLP)
  const float *G0, *G1;                 // compact gradients (apply only)
};

// Replay layout: lane = column.  One row (of both tables of a pair) per wave when D >= 64
// (EPL = D/64 columns per lane, stride 64), 64/D rows per wave when D < 64.  With one row per
// wave the replay bounds (from, to) are wave-uniform: the step loop is scalar, the per-step
// scalars come through the scalar cache, and no lane idles on another row's longer catch-up.
template <int D>
struct Replay {
  static constexpr int LPR = D < 64 ? D : 64;   // lanes per row
  static constexpr int EPL = D / LPR;           // columns per lane
};

// One owed zero-gradient step of one column, of one table or (PAIR) of both tables of a pair:
// the variant's element update (step0) with the step's scalars ra / rb (/ dk, its decay, under
// decoupled weight decay: one more float per step of the table, RowTraits<V>::TS), then the
// variant's rounding of a bf16 parameter, which is stored (rounded) after every step it takes:
// to nearest even, or stochastically with the step's bits (ncf_sr_*, ncf_common.h): key the
// row's key of this step, ew the element's word (ncf_sr_elem).  Every loop that replays owed
// steps calls this.
template <Rows V, bool PAIR>
__device__ __forceinline__ void owed_step(float& p0, float& m0, float& v0, float& p1, float& m1,
                                          float& v1, float ra, float rb, float dk, uint32_t key,
                                          uint32_t ew, const AdamScalars& s) {
  using R = RowTraits<V>;
  step0<R::DW>(p0, m0, v0, ra, rb, dk, s);
  if (R::BF && !R::SR) p0 = ncf_round_bf16(p0);
  if (PAIR) step0<R::DW>(p1, m1, v1, ra, rb, dk, s);
  if (PAIR && R::BF && !R::SR) p1 = ncf_round_bf16(p1);
  if (R::SR) {
    const uint32_t h = ncf_sr_bits(key, ew);
    p0 = ncf_sr_round0(p0, h);
    if (PAIR) p1 = ncf_sr_round1(p1, h);
  }
}

// The replay of zero-gradient steps from+1 .. to on EPL columns of one (pair of) table row(s).
// With wave-uniform bounds (one row per wave) the per-step scalars are scalar loads; they are
// fetched 8 steps (16 floats) at a time, one chunk AHEAD of the steps that use them, so the
// scalar-load latency hides behind 8 steps of VALU work instead of stalling every step (the
// step table is padded >= 4096 steps past any target, deferred.py _ensure).  Same adam1 calls in
// the same order: results are bit-identical to the step-by-step loop.
// Stochastic rounding: sr_base is the row's ncf_sr_base, wave-uniform like the bounds, so a
// step's key is scalar work; e_lo the low word of the lane's first element.
// Decoupled weight decay: the step's decay travels with ra / rb, a third scalar per owed step
// through the same scalar loads and the same prefetch (NS scalars per step; the coupled form
// keeps its two).
template <int EPL, bool PAIR, Rows V = Rows::F32>
__device__ __forceinline__ void replay_uniform(float* p0, float* m0, float* v0, float* p1,
                                               float* m1, float* v1, int32_t from, int32_t to,
                                               const float* __restrict__ table,
                                               const AdamScalars& s, uint32_t sr_base = 0,
                                               uint32_t e_lo = 0) {
  constexpr bool SR = RowTraits<V>::SR, DW = RowTraits<V>::DW;
  constexpr int C = 8;                 // steps per chunk
  constexpr int TS = RowTraits<V>::TS; // floats per step of the table
  constexpr int NS = DW ? 3 : 2;       // scalars a zero-gradient step reads: ra, rb (, decay)
  int32_t q = from + 1;
  uint32_t ew[EPL];                    // SR: the elements' words, the same at every step
#pragma unroll
  for (int j = 0; j < EPL; ++j) ew[j] = SR ? ncf_sr_elem(e_lo + j * 64) : 0u;
  float sc[NS * C];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    sc[NS * k] = table[TS * (q + k) + 2];
    sc[NS * k + 1] = table[TS * (q + k) + 3];
    if (DW) sc[NS * k + NS - 1] = table[TS * (q + k) + 4];
  }
  while (q + C - 1 <= to) {
    float nx[NS * C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
      nx[NS * k] = table[TS * (q + C + k) + 2];
      nx[NS * k + 1] = table[TS * (q + C + k) + 3];
      if (DW) nx[NS * k + NS - 1] = table[TS * (q + C + k) + 4];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of this chunk's steps
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const uint32_t key = SR ? ncf_sr_key(sr_base, q + k) : 0u;
      const float dk = DW ? sc[NS * k + NS - 1] : 1.f;
#pragma unroll
      for (int j = 0; j < EPL; ++j)
        owed_step<V, PAIR>(p0[j], m0[j], v0[j], p1[j], m1[j], v1[j], sc[NS * k], sc[NS * k + 1],
                           dk, key, ew[j], s);
    }
#pragma unroll
    for (int k = 0; k < NS * C; ++k) sc[k] = nx[k];
    q += C;
  }
#pragma unroll
  for (int k = 0; k < C - 1; ++k) {    // the last to - q + 1 < C steps
    if (q + k > to) break;
    const uint32_t key = SR ? ncf_sr_key(sr_base, q + k) : 0u;
    const float dk = DW ? sc[NS * k + NS - 1] : 1.f;
#pragma unroll
    for (int j = 0; j < EPL; ++j)
      owed_step<V, PAIR>(p0[j], m0[j], v0[j], p1[j], m1[j], v1[j], sc[NS * k], sc[NS * k + 1],
                         dk, key, ew[j], s);
  }
}

// Row `row` (columns sub, sub + LPR, ... of it) from step `from` to step `to`.  Stochastic
// rounding runs under `seed` for the tables of pair `kind` (ncf_sr_*).
template <int D, Rows V = Rows::F32>
__device__ __forceinline__ void catch_up_row(const TablePtrs& t, int64_t row, int sub, int32_t from,
                                             int32_t to, const float* __restrict__ table,
                                             const AdamScalars& s, uint32_t seed = 0,
                                             int kind = 0) {
  constexpr bool BF = RowTraits<V>::BF, SR = RowTraits<V>::SR, DW = RowTraits<V>::DW;
  constexpr int TS = RowTraits<V>::TS;
  constexpr int EPL = Replay<D>::EPL, LPR = Replay<D>::LPR;
  if (Replay<D>::LPR == 64) {   // the whole wave holds this row: make the bounds scalar
    from = __builtin_amdgcn_readfirstlane(from);
    to = __builtin_amdgcn_readfirstlane(to);
  }
  if (from >= to) return;
  const int64_t o = row * D + sub;
  const uint32_t e_lo = (uint32_t)o;
  uint32_t base = 0;
  if (SR) {
    base = ncf_sr_base(seed, kind, (uint32_t)((uint64_t)o >> 32));
    if (Replay<D>::LPR == 64) base = __builtin_amdgcn_readfirstlane(base);
  }
  float p0[EPL], m0[EPL], v0[EPL], p1[EPL], m1[EPL], v1[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j) {
    p0[j] = ldp<BF>(t.p0, o + j * LPR); m0[j] = t.m0[o + j * LPR]; v0[j] = t.v0[o + j * LPR];
  }
  if (t.p1) {
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      p1[j] = ldp<BF>(t.p1, o + j * LPR); m1[j] = t.m1[o + j * LPR]; v1[j] = t.v1[o + j * LPR];
    }
    if (Replay<D>::LPR == 64) {
      replay_uniform<EPL, true, V>(p0, m0, v0, p1, m1, v1, from, to, table, s, base, e_lo);
    } else {
#pragma unroll 2
      for (int32_t q = from + 1; q <= to; ++q) {
        const float ra = table[TS * q + 2], rb = table[TS * q + 3];
        const float dk = DW ? table[TS * q + 4] : 1.f;
        const uint32_t key = SR ? ncf_sr_key(base, q) : 0u;
        // Not owed_step<V, true>: this loop steps both tables before it rounds either, and with
        // owed_step's order (round the first, then step the second) the compiler schedules the
        // nearest-even bf16 form of two kernels differently at D < 64.  Same values either way;
        // the loop keeps its order so that the machine code stays what was measured.
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
          step0<DW>(p0[j], m0[j], v0[j], ra, rb, dk, s);
          step0<DW>(p1[j], m1[j], v1[j], ra, rb, dk, s);
          if (BF && !SR) { p0[j] = ncf_round_bf16(p0[j]); p1[j] = ncf_round_bf16(p1[j]); }
          if (SR) {
            const uint32_t h = ncf_sr_bits(key, ncf_sr_elem(e_lo + j * LPR));
            p0[j] = ncf_sr_round0(p0[j], h);
            p1[j] = ncf_sr_round1(p1[j], h);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      stp<BF>(t.p1, o + j * LPR, p1[j]); t.m1[o + j * LPR] = m1[j]; t.v1[o + j * LPR] = v1[j];
    }
  } else if (Replay<D>::LPR == 64) {
    replay_uniform<EPL, false, V>(p0, m0, v0, p1, m1, v1, from, to, table, s, base, e_lo);
  } else {
#pragma unroll 2
    for (int32_t q = from + 1; q <= to; ++q) {
      const float ra = table[TS * q + 2], rb = table[TS * q + 3];
      const float dk = DW ? table[TS * q + 4] : 1.f;
      const uint32_t key = SR ? ncf_sr_key(base, q) : 0u;
#pragma unroll
      for (int j = 0; j < EPL; ++j)
        owed_step<V, false>(p0[j], m0[j], v0[j], p1[j], m1[j], v1[j], ra, rb, dk, key,
                            SR ? ncf_sr_elem(e_lo + j * LPR) : 0u, s);
    }
  }
#pragma unroll
  for (int j = 0; j < EPL; ++j) {
    stp<BF>(t.p0, o + j * LPR, p0[j]); t.m0[o + j * LPR] = m0[j]; t.v0[o + j * LPR] = v0[j];
  }
}

// ---- both id kinds per launch (k = kind)
struct PairArgs {
  TablePtrs t[2];
  const int64_t* ids[2];
  int32_t* stamp[2];
  int64_t rows[2];
  Rows variant;      // which instantiation the host launches (rows_of); no kernel reads it
  int32_t reserved0;
  uint32_t seed;     // round_seed of the stochastic rounding (ncf_sr_base)
  int32_t reserved1;
};
static_assert(sizeof(PairArgs) == 192 && offsetof(PairArgs, seed) == 184,
              "PairArgs: kernel arguments, the offsets the kernels load from stay put");

// The launch arguments of the n (1 or 2) pairs an entry point was given, or NCF_ERR_ARG: what
// every pairs entry checks of its tables (the variant: rows_of, adam_math.h).
inline int pair_args(const char* who, const ncf_table_pair* p, int n, PairArgs* out) {
  NCF_CHECK_ARG(p && n >= 1 && n <= 2, "%s: bad args", who);
  PairArgs a;
  memset(&a, 0, sizeof(a));
  const int rc = rows_of(who, p, n, &a.variant);
  if (rc != NCF_OK) return rc;
  for (int k = 0; k < n; ++k) {
    a.t[k] = TablePtrs{p[k].p0, p[k].m0, p[k].v0, p[k].p1, p[k].m1, p[k].v1, p[k].g0, p[k].g1};
    a.ids[k] = p[k].row_ids;
    a.stamp[k] = p[k].stamp;
    a.rows[k] = p[k].rows;
  }
  a.seed = (uint32_t)p[0].round_seed;
  *out = a;
  return NCF_OK;
}

// Block bx (of ncf_cdiv(max_n * Replay<D>::LPR, 256), 256 threads) of the catch-up of kind k's
// listed rows ids[k][0 .. count[k]) to clock->t + target_rel.
template <int D, Rows V>
__device__ __forceinline__ void pairs_catchup_body(const PairArgs& a, int k, uint32_t bx,
                                                   const uint32_t* __restrict__ count,
                                                   int64_t max_n, int32_t target_rel,
                                                   const ncf_step_clock* __restrict__ clock,
                                                   const float* __restrict__ table,
                                                   const AdamScalars& s, int lock) {
  constexpr int L = Replay<D>::LPR;   // lanes per row
  const int64_t tt = (int64_t)bx * 256 + threadIdx.x;
  const int64_t c = tt / L;
  const int sub = (int)(tt % L);
  if (c >= max_n || c >= (int64_t)count[k]) return;
  const int32_t target = clock->t + target_rel;
  const int64_t row = a.ids[k][c];
  int32_t* stamp = a.stamp[k];
  const int32_t from = stamp[row];
  catch_up_row<D, V>(a.t[k], row, sub, from, target, table, s, a.seed, k);
  // lock: every listed row is marked in flight (current through target, its gradient step still
  // to come: the step's apply writes the plain stamp back); replays of other rows skip it.  A
  // listed row that is locked already, or ahead of the target, keeps its stamp: it was not
  // brought to the target, and writing target | LOCK over s | LOCK would drop the steps it owes
  if (sub == 0 && (from < target || (lock && from == target)))
    stamp[row] = lock ? (target | NCF_STAMP_LOCK) : target;
}

}  // namespace
}  // namespace ncf_adam

#define NCF_DISPATCH_DIM(D, FN, ...)                                          \
  switch (D) {                                                                \
    case 16: return FN<16>(__VA_ARGS__);                                      \
    case 32: return FN<32>(__VA_ARGS__);                                      \
    case 64: return FN<64>(__VA_ARGS__);                                      \
    case 128: return FN<128>(__VA_ARGS__);                                    \
    case 256: return FN<256>(__VA_ARGS__);                                    \
    default: ncf_set_error("unsupported dim %lld", (long long)D); return NCF_ERR_ARG; \
  }
