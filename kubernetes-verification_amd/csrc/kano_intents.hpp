// kano_intents.hpp -- user-declared allow / deny intents checked against the
// resident bit matrix (kano_intents / kano_intent_pairs, kano_ext.hip).  Read
// from the matrix itself, so it holds for built, updated, edited, loaded,
// path and edge matrices and for row shards alike.
//
// Intent k is a source set S_k, a destination set D_k (bit rows of W words,
// LSB first) and two flag bits.  With the considered pairs
//   C_k = {(i, j) : i in S_k held by this context, j in D_k, i != j unless
//          INTENT_SELF}
// a deny intent's violations are the pairs of C_k with M[i, j] = 1 and an
// allow intent's those with M[i, j] = 0.  Three launches a pass:
//   * k_intent_lists: a wave an intent.  It clears D_k past n and S_k outside
//     the held rows, counts |D_k| and |S_k & D_k| and compacts S_k into an
//     ascending row list (a wave exclusive scan of popcounts per 64 words);
//     it also resets the intent's accumulators, so no fill precedes it.
//   * k_intent_rows: a wave's item is (intent k, a run of rows of list k).
//     The wave sweeps INTENT_RB rows at a time over the W words, 64 words a
//     sweep and one coalesced word a lane; the rows of a sweep share the load
//     of D_k's word.  Per lane it keeps the popcount of x & d and, per row,
//     the first violating column it saw; a ballot per row says whether the
//     row has a violation at all, and only the item's first such row pays a
//     wave min for its column.  Per item, not per row, one lane adds
//     `reachable` and `bad_sources` and folds (i << 32) | j into the intent's
//     witness with an unsigned 64-bit atomicMin.  A run is INTENT_R rows at
//     least and an intent has INTENT_MAX_ITEMS items at most: that bounds the
//     atomics that meet on one intent's three words.
//   * kano_intent_pairs adds k_intent_row_counts (a wave a list row: its
//     violations), an exclusive scan (kano_prims.hpp) and k_intent_emit (a
//     wave a list row again, k_diff_emit's pattern: the order is by
//     construction).
// Blocks hand data to each other only across these launch boundaries.
#pragma once
#include "kano_prims.hpp"

namespace kano {

constexpr int INTENT_R = 16;             // rows of an item at least
constexpr int INTENT_RB = 4;             // rows a wave sweeps together
constexpr int INTENT_MAX_ITEMS = 1024;   // items of one intent at most
constexpr int INTENT_ALLOW = 1;          // flag bit 0: every pair must be reachable
constexpr int INTENT_SELF = 2;           // flag bit 1: the pairs (i, i) are considered
constexpr int INTENT_RES = 5;            // u64 per intent: |D|, |S & D|, reachable, bad sources, witness
constexpr uint32_t INTENT_NO_COL = 0xffffffffu;

// One intent of a pass (host-built); one more entry closes loff and ioff.
struct IntentDesc {
  i64 loff;        // its row list is list[loff .. next loff)
  i64 ioff;        // its items are ioff .. next ioff
  int32_t run;     // rows of one of its items
  int32_t flags;
};

// the violating bits of matrix word x of row `row` against destination word d
// (word index w), and through `reach` the considered bits that are set
__device__ __forceinline__ u64 intent_bits(u64 x, u64 d, bool allow, bool self, i64 w,
                                           int32_t row, u64& reach) {
  u64 r = x & d, v = allow ? d & ~x : r;
  if (!self && (i64)(row >> 6) == w) {
    const u64 keep = ~(1ull << (row & 63));
    r &= keep;
    v &= keep;
  }
  reach = r;
  return v;
}

static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_intent_lists(
    u64* __restrict__ src, u64* __restrict__ dst, i64 W, i64 n, i64 r0, i64 r1,
    const IntentDesc* __restrict__ desc, i64 K, int32_t* __restrict__ list,
    u64* __restrict__ res) {
  const int lane = threadIdx.x & 63;
  const i64 nwaves = (i64)gridDim.x * (TPB / 64);
  for (i64 k = (i64)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); k < K; k += nwaves) {
    u64* s = src + k * W;
    u64* d = dst + k * W;
    const i64 end = desc[k + 1].loff;
    i64 pos = desc[k].loff;
    i64 nd = 0, nsd = 0;
    for (i64 wb = 0; wb < W; wb += 64) {
      const i64 w = wb + lane;
      u64 sv = 0, dv = 0;
      if (w < W) {
        dv = d[w] & valid_mask(w, n);
        sv = s[w] & valid_mask(w, r1) & ~valid_mask(w, r0);
        d[w] = dv;
      }
      nd += __popcll(dv);
      nsd += __popcll(sv & dv);
      int tot;
      i64 p = pos + wave_excl_scan((int)__popcll(sv), tot);
      while (sv) {
        const int b = __ffsll((long long)sv) - 1;
        sv &= sv - 1;
        if (p < end) list[p] = (int32_t)(w * 64 + b);
        ++p;
      }
      pos += tot;
    }
    nd = wave_sum(nd);
    nsd = wave_sum(nsd);
    if (lane == 0) {
      u64* o = res + k * INTENT_RES;
      o[0] = (u64)nd;
      o[1] = (u64)nsd;
      o[2] = 0;
      o[3] = 0;
      o[4] = ~0ull;
    }
  }
}

static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_intent_rows(
    const u64* __restrict__ M, i64 ldM, i64 r0, i64 rl, i64 W, const u64* __restrict__ dst,
    const IntentDesc* __restrict__ desc, i64 K, i64 nitems, const int32_t* __restrict__ list,
    u64* res) {
  const int lane = threadIdx.x & 63;
  // (wave-uniform by construction: lets the item's bookkeeping stay scalar)
  const i64 wave0 = (i64)blockIdx.x * (TPB / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 nwaves = (i64)gridDim.x * (TPB / 64);
  for (i64 item = wave0; item < nitems; item += nwaves) {
    // the last intent whose items start at or before this one (an intent
    // without items shares its offset with the next)
    i64 lo = 0, hi = K;
    while (hi - lo > 1) {
      const i64 mid = (lo + hi) >> 1;
      if (desc[mid].ioff <= item) lo = mid; else hi = mid;
    }
    const i64 k = lo;
    const IntentDesc de = desc[k];
    const i64 cnt = desc[k + 1].loff - de.loff;
    const i64 q0 = (item - de.ioff) * de.run;
    if (q0 >= cnt) continue;
    const i64 q1 = min(cnt, q0 + (i64)de.run);
    const bool allow = de.flags & INTENT_ALLOW, self = de.flags & INTENT_SELF;
    const u64* D = dst + k * W;
    const int32_t* L = list + de.loff;
    u64 best = ~0ull;
    i64 reach = 0;
    int bad = 0;
    for (i64 q = q0; q < q1; q += INTENT_RB) {
      int32_t row[INTENT_RB];
      const u64* p[INTENT_RB];
      uint32_t fc[INTENT_RB];
      bool live[INTENT_RB];
#pragma unroll
      for (int j = 0; j < INTENT_RB; ++j) {
        row[j] = L[min(q + j, q1 - 1)];       // (past the run: its last row again, masked below)
        // (a list entry is a held row by construction; one that is not is read as row 0 and counts nowhere)
        const bool held = (u64)((i64)row[j] - r0) < (u64)rl;
        live[j] = held && q + j < q1;
        p[j] = M + (held ? (i64)row[j] - r0 : 0) * ldM;
        fc[j] = INTENT_NO_COL;
      }
      for (i64 wb = 0; wb < W; wb += 64) {
        const i64 w = wb + lane;
        if (w >= W) continue;
        const u64 d = D[w];
        u64 x[INTENT_RB];
#pragma unroll
        for (int j = 0; j < INTENT_RB; ++j) x[j] = p[j][w];
#pragma unroll
        for (int j = 0; j < INTENT_RB; ++j) {
          u64 r;
          const u64 v = intent_bits(x[j], live[j] ? d : 0ull, allow, self, w, row[j], r);
          reach += __popcll(r);
          if (v && fc[j] == INTENT_NO_COL) fc[j] = (uint32_t)(w * 64 + (__ffsll((long long)v) - 1));
        }
      }
#pragma unroll
      for (int j = 0; j < INTENT_RB; ++j) {
        if (q + j >= q1) break;                                  // wave-uniform
        if (__ballot(fc[j] != INTENT_NO_COL) == 0) continue;     // wave-uniform
        ++bad;
        if (best != ~0ull) continue;          // rows ascend: the first violating row is the item's smallest
        uint32_t c = fc[j];
#pragma unroll
        for (int dlt = 32; dlt >= 1; dlt >>= 1) c = min(c, (uint32_t)__shfl_xor((int)c, dlt, 64));
        best = ((u64)(uint32_t)row[j] << 32) | c;
      }
    }
    reach = wave_sum(reach);
    if (lane == 0) {
      u64* o = res + k * INTENT_RES;
      if (reach) atomicAdd(&o[2], (u64)reach);
      if (bad) atomicAdd(&o[3], (u64)bad);
      if (best != ~0ull) atomicMin(&o[4], best);
    }
  }
}

// cnt[q] = the violations of list row q of one intent (its destination row d)
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_intent_row_counts(
    const u64* __restrict__ M, i64 ldM, i64 r0, i64 rl, i64 W, const u64* __restrict__ d,
    int flags, const int32_t* __restrict__ list, i64 rows, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const bool allow = flags & INTENT_ALLOW, self = flags & INTENT_SELF;
  const i64 nwaves = (i64)gridDim.x * (TPB / 64);
  for (i64 q = (i64)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); q < rows; q += nwaves) {
    const int32_t row = list[q];
    const bool held = (u64)((i64)row - r0) < (u64)rl;            // (always, by construction)
    const u64* p = M + (held ? (i64)row - r0 : 0) * ldM;
    int c = 0;
    for (i64 w = lane; held && w < W; w += 64) {
      u64 r;
      c += __popcll(intent_bits(p[w], d[w], allow, self, w, row, r));
    }
    c = wave_sum(c);
    if (lane == 0) cnt[q] = c;
  }
}

// the violating pairs of one intent as (i, j) int32, ascending by i then j:
// list row q's pairs start at off[q] (k_diff_emit's pattern).  No pair is
// written at or past off[q + 1] or cap.
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_intent_emit(
    const u64* __restrict__ M, i64 ldM, i64 r0, i64 rl, i64 W, const u64* __restrict__ d,
    int flags, const int32_t* __restrict__ list, i64 rows, const i64* __restrict__ off, i64 cap,
    int32_t* __restrict__ pairs) {
  const int lane = threadIdx.x & 63;
  const bool allow = flags & INTENT_ALLOW, self = flags & INTENT_SELF;
  const i64 nwaves = (i64)gridDim.x * (TPB / 64);
  for (i64 q = (i64)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); q < rows; q += nwaves) {
    const i64 beg = off[q], end = min(off[q + 1], cap);
    if (beg >= end) continue;   // (wave-uniform)
    const int32_t row = list[q];
    if ((u64)((i64)row - r0) >= (u64)rl) continue;   // (never, by construction; wave-uniform)
    const u64* p = M + ((i64)row - r0) * ldM;
    i64 pos = beg;
    for (i64 wb = 0; wb < W; wb += 64) {
      const i64 w = wb + lane;
      u64 v = 0, r;
      if (w < W) v = intent_bits(p[w], d[w], allow, self, w, row, r);
      int tot;
      i64 at = pos + wave_excl_scan((int)__popcll(v), tot);
      while (v) {
        const int b = __ffsll((long long)v) - 1;
        v &= v - 1;
        if (at < end) *reinterpret_cast<int2*>(pairs + 2 * at) = make_int2(row, (int)(w * 64 + b));
        ++at;
      }
      pos += tot;
    }
  }
}

}  // namespace kano
