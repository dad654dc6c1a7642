// kano_pairwalk.hpp -- the pair walk: the policies matching a pod pair (i, j),
// read from the resident tables.  With row class c = rcls[i] and column class
// x = ccls[j] (lists mode: ccls null, x = j) they are
//   the build's part   every p of S(c) = slist[soffc[c] .. soffc[c + 1]) whose
//                      bit x is set in AC[p]
//   the added part     every added policy t (engine id P + t) with bit i of
//                      asel[t] and bit j of aalw[t]
// in ascending id order (S(c) is ascending, the added ids follow the build's).
// A pair whose i lies outside [r0, r1) (another shard's row) matches nothing
// here; a build without policies has no classes (rcls null) and only the
// added part.  kano_pair_policies (kano_kernels.hpp), kano_pair_masks
// (kano_ports.hpp) and kano_pair_verdicts / kano_verdict_matrix
// (kano_verdict.hpp) fold these policies; removed ids are the caller's to skip
// (its alive(): the dead flags, or the VD_DEAD keys).  Two forms, chosen per call by the host
// (pair_shape, kano_hip.hip): a lane per pair walking serially, grid-stride
// over the pairs, or a wave per pair with the lanes striding the list.
#pragma once
#include "kano_prims.hpp"

namespace kano {

struct PairTables {
  const int32_t* pairs;  // (i, j) x Q
  i64 Q;
  const int32_t* rcls;   // null: the build had no policies (only the added part)
  const int32_t* ccls;   // null: x = j
  const i64* soffc;
  const int32_t* slist;
  union {                // how a removed id is marked, the family's own:
    const uint8_t* dead;   // P + A flags; null: none removed (pair_policies, pair_masks)
    const uint32_t* key;   // P + A keys, VD_DEAD for a removed id (the verdicts)
  };
  const u64* AC;
  i64 ldC;
  i64 P;
  const u64* asel;
  const u64* aalw;
  i64 W, A;
  i64 r0, r1;
};

// the wave form when a pair walks more than this many policies on average
// (mean |S(c)| + added policies)
constexpr i64 PAIR_WAVE_MIN = 16;

__device__ __forceinline__ bool pair_own(const PairTables& t, i64 i) {
  return i >= t.r0 && i < t.r1;
}

// S(rcls[i]) = slist[s0 .. s0 + s) and j's column class x, for a row held here.
// ccls is not tested: the lists mode (ccls null, x = j) is kano_pair_policies'
// alone and k_pair_lane / k_pair_wave look their lists up themselves; with the
// test the ccls load sat in a branch of its own and was waited for there, not
// together with soffc's (kano_pair_verdicts + 2 %).
__device__ __forceinline__ void pair_list(const PairTables& t, i64 i, i64 j, i64& s0, i64& s,
                                          i64& x) {
  s0 = s = x = 0;
  if (!t.rcls) return;
  const int32_t c = t.rcls[i];
  s0 = t.soffc[c];
  s = t.soffc[c + 1] - s0;
  x = t.ccls[j];
}

__device__ __forceinline__ bool pair_hit_build(const PairTables& t, i64 p, i64 x) {
  return (t.AC[p * t.ldC + (x >> 6)] >> (x & 63)) & 1ull;
}

__device__ __forceinline__ bool pair_hit_added(const PairTables& t, i64 tt, i64 i, i64 j) {
  return ((t.asel[tt * t.W + (i >> 6)] >> (i & 63)) & 1ull) &&
         ((t.aalw[tt * t.W + (j >> 6)] >> (j & 63)) & 1ull);
}

// removed-id flags (P + A of them; null: none removed)
__device__ __forceinline__ bool pair_alive(const uint8_t* dead, i64 p) {
  return !(dead && dead[p]);
}

// the wave form's split: wave gw of the grid's nw takes the contiguous run
// [q0, q1) of the Q pairs (empty for the waves past the last pair)
__device__ __forceinline__ void wave_pair_run(i64 Q, i64& q0, i64& q1) {
  const i64 nw = (i64)gridDim.x * (TPB / 64);
  const i64 gw = (i64)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  const i64 per = (Q + nw - 1) / nw;
  q0 = gw * per;
  q1 = min(Q, q0 + per);
}

// take(p) for the matching policies of (i, j) at positions k0, k0 + step, ..
// of the build's list, then of the added policies (own: this context holds row
// i).  alive(p) is asked before the tables are read (p: i64).  (k0, step) = (0, 1) is
// the serial walk, (lane, 64) a wave's stride.  The first form takes the list
// from a pair_list of the caller's (one lookup for several walks of a pair).
template <class Alive, class Take>
__device__ __forceinline__ void pair_walk(const PairTables& t, i64 i, i64 j, bool own, i64 s0,
                                          i64 s, i64 x, i64 k0, i64 step, Alive alive, Take take) {
  if (!own) return;
  for (i64 k = k0; k < s; k += step) {
    const int32_t p = t.slist[s0 + k];
    if (alive(p) && pair_hit_build(t, p, x)) take(p);
  }
  for (i64 tt = k0; tt < t.A; tt += step) {
    const i64 p = t.P + tt;
    if (alive(p) && pair_hit_added(t, tt, i, j)) take(p);
  }
}

template <class Alive, class Take>
__device__ __forceinline__ void pair_walk(const PairTables& t, i64 i, i64 j, bool own, i64 k0,
                                          i64 step, Alive alive, Take take) {
  i64 s0 = 0, s = 0, x = 0;
  if (own) pair_list(t, i, j, s0, s, x);
  pair_walk(t, i, j, own, s0, s, x, k0, step, alive, take);
}

}  // namespace kano
