// kano_verdict.hpp -- deny rules and priorities over the resident tables (the
// tables kano_pair_policies and kano_policy_subset read; the matrix is not
// touched).  Every alive policy p carries key[p] = rank[p] * 2 + act[p]: rank
// the position of its priority among the distinct alive priorities (0 = the
// smallest number = evaluated first), act 0 allow / 1 deny; a removed id
// carries VD_DEAD (the host folds the context's dead flags into the keys).
// Over the policies matching a pair (i in select_p, j in allow_p):
//   t*(i, j)  = the smallest rank
//   verdict   = none (nothing matches) | deny (a deny policy at t* matches)
//               | allow
//   decider   = the smallest id among the matching policies at t* with the
//               winning action
// The verdict matrix (bit = verdict is allow) is written in four steps:
//   k_verdict_order  every row class's list S(c) copied once per call in
//                    (rank, act, id) order without its dead entries, so the
//                    levels of a class are runs of the copy
//   k_verdict_class  the class-level rows Vc[c]: one walk of the ordered copy
//                    per word, a level resolved at each change of rank
//   k_path_expand16  (kano_path.hpp) the class rows to the member rows
//   k_verdict_rows   only with alive added policies (or without classes):
//                    the rows they select, resolved bit by bit with the walk
//                    of the pair kernels below
#pragma once
#include "kano_pairwalk.hpp"
#include "kano_prims.hpp"

namespace kano {

constexpr uint32_t VD_DEAD = 0xffffffffu;   // the key of a removed id
constexpr uint32_t VD_NONE = 0xffffffffu;   // no rank: above every alive one
constexpr int32_t VD_NOID = 0x7fffffff;

// olist / okey [soffc[c] .. soffc[c] + ocnt[c]) = the alive policies of S(c)
// and their keys, ascending in (key, id); one block per row class
// (grid-stride).  An entry's place is the number of entries below it: the
// list is compared against itself in LDS rounds of TPB, any length.  The
// packed (key, id) words of a list are gathered once into pk (a scratch the
// size of slist; only the block of a class touches its part), so the rounds
// read one word an entry and no key[] gather.  (Within a level the order does
// not matter to k_verdict_class; (key, id) makes the copy deterministic.)
// *deny_classes += 1 for every class with an alive deny policy.
__global__ __launch_bounds__(TPB) void k_verdict_order(i64 U, const i64* __restrict__ soffc,
                                                       const int32_t* __restrict__ slist,
                                                       const uint32_t* __restrict__ key,
                                                       u64* __restrict__ pk,
                                                       int32_t* __restrict__ olist,
                                                       uint32_t* __restrict__ okey,
                                                       int32_t* __restrict__ ocnt,
                                                       unsigned* __restrict__ deny_classes) {
  __shared__ u64 sh[TPB];
  const int t = threadIdx.x;
  for (i64 c = blockIdx.x; c < U; c += gridDim.x) {
    const i64 s0 = soffc[c], s = soffc[c + 1] - s0;
    for (i64 e = t; e < s; e += TPB) {
      const int32_t p = slist[s0 + e];
      pk[s0 + e] = ((u64)key[p] << 32) | (uint32_t)p;
    }
    __syncthreads();                                 // (the block's own global writes)
    int alive = 0, deny = 0;
    for (i64 e0 = 0; e0 < s; e0 += TPB) {            // (block-uniform trip counts)
      const i64 e = e0 + t;
      const u64 mine = e < s ? pk[s0 + e] : ~0ull;
      const int32_t p = (int32_t)(uint32_t)mine;
      const uint32_t kp = (uint32_t)(mine >> 32);
      i64 below = 0;
      for (i64 f0 = 0; f0 < s; f0 += TPB) {
        __syncthreads();
        sh[t] = f0 + t < s ? pk[s0 + f0 + t] : ~0ull;
        __syncthreads();
        const int m = (int)min((i64)TPB, s - f0);
        for (int f = 0; f < m; ++f) below += sh[f] < mine;
      }
      const bool live = e < s && kp != VD_DEAD;      // (dead keys sort last: below < alive count)
      if (live) {
        olist[s0 + below] = p;
        okey[s0 + below] = kp;
      }
      alive += __syncthreads_count(live);
      deny |= __syncthreads_or(live && (kp & 1u));
    }
    if (t == 0) {
      ocnt[c] = alive;
      if (deny) atomicAdd(deny_classes, 1u);
    }
  }
}

// Vc[c][w] over the ldC words of the column classes: the levels of the
// ordered copy resolved with a running decided mask -- per level a = OR of the
// allow policies' AC rows, d = OR of the deny policies', then
//   value |= a & ~d & ~decided,   decided |= a | d.
// A group of wl lanes (the host's: the smallest power of two covering ldC, at
// most TPB) takes a class, lane l of it the words l, l + wl, ..; a block holds
// TPB / wl classes at a time.  One walk of the copy per word: any number of
// levels costs what one level costs, and a long list is a long serial walk of
// its group (the entries' ids and keys are read by position, so only the AC
// word depends on a load).
__global__ __launch_bounds__(TPB) void k_verdict_class(i64 U, const i64* __restrict__ soffc,
                                                       const int32_t* __restrict__ olist,
                                                       const uint32_t* __restrict__ okey,
                                                       const int32_t* __restrict__ ocnt,
                                                       const u64* __restrict__ AC, i64 ldC, int wl,
                                                       u64* __restrict__ Vc) {
  const int t = threadIdx.x, lane = t & (wl - 1), g = t / wl, cpb = TPB / wl;
  for (i64 c = (i64)blockIdx.x * cpb + g; c < U; c += (i64)gridDim.x * cpb) {
    const i64 s0 = soffc[c];
    const int m = ocnt[c];
    for (i64 w = lane; w < ldC; w += wl) {
      u64 value = 0, decided = 0, a = 0, d = 0;
      uint32_t cur = 0;
      for (int k = 0; k < m; ++k) {
        const uint32_t kk = okey[s0 + k];
        const int32_t p = olist[s0 + k];
        if ((kk >> 1) != cur) {                        // the level ends
          value |= a & ~d & ~decided;
          decided |= a | d;
          a = d = 0;
          cur = kk >> 1;
        }
        const u64 x = AC[(i64)p * ldC + w];
        if (kk & 1u) d |= x;
        else a |= x;
      }
      value |= a & ~d & ~decided;
      Vc[c * ldC + w] = value;
    }
  }
}

// ---------------------------------------------------------------------------
// The verdict of one pair: the pair walk (kano_pairwalk.hpp; the dead flags
// are inside the keys) tracking the running (best rank, deny seen at best,
// smallest allow id at best, smallest deny id at best); all of it resets when
// a lower rank matches.  One pair belongs to one lane or one wave: no atomics.
// ---------------------------------------------------------------------------
struct VerdictArgs {
  PairTables t;          // (t.key: the ids' keys)
  uint32_t* out_key;     // Q: best rank * 2 + deny, VD_NONE where nothing matches
  int32_t* out_id;       // Q: the deciding engine id, -1 where nothing matches
};

struct VdState {
  uint32_t best = VD_NONE;
  uint32_t dn = 0;
  int32_t ida = VD_NOID, idd = VD_NOID;
};

__device__ __forceinline__ void vd_take(VdState& s, uint32_t k, int32_t p) {
  const uint32_t r = k >> 1;
  if (r < s.best) {
    s.best = r;
    s.dn = 0;
    s.ida = s.idd = VD_NOID;
  }
  if (r == s.best) {
    if (k & 1u) {
      s.dn = 1;
      s.idd = min(s.idd, p);
    } else {
      s.ida = min(s.ida, p);
    }
  }
}

// the state over the walk's positions k0, k0 + step, .. (own: this context
// holds row i)
__device__ __forceinline__ VdState vd_walk(const VerdictArgs& a, i64 i, i64 j, bool own, i64 k0,
                                           i64 step) {
  VdState s;
  pair_walk(
      a.t, i, j, own, k0, step, [&](i64 p) { return a.t.key[p] != VD_DEAD; },
      [&](i64 p) { vd_take(s, a.t.key[p], (int32_t)p); });
  return s;
}

__device__ __forceinline__ void vd_store(const VerdictArgs& a, i64 q, const VdState& s) {
  const bool none = s.best == VD_NONE;
  a.out_key[q] = none ? VD_NONE : s.best * 2u + s.dn;
  a.out_id[q] = none ? -1 : (s.dn ? s.idd : s.ida);
}

// a lane per pair, S(c) walked serially; grid-stride over the pairs
__global__ __launch_bounds__(TPB) void k_verdict_lane(VerdictArgs a) {
  const i64 stride = (i64)gridDim.x * TPB;
  for (i64 q = (i64)blockIdx.x * TPB + threadIdx.x; q < a.t.Q; q += stride) {
    const i64 i = a.t.pairs[2 * q], j = a.t.pairs[2 * q + 1];
    vd_store(a, q, vd_walk(a, i, j, pair_own(a.t, i), 0, 1));
  }
}

// a wave per pair, the lanes striding S(c) and the added policies, their
// states met by a butterfly (the lower rank wins, equal ranks merge)
__global__ __launch_bounds__(TPB) void k_verdict_wave(VerdictArgs a) {
  const int lane = threadIdx.x & 63;
  i64 q0, q1;
  wave_pair_run(a.t.Q, q0, q1);
  for (i64 q = q0; q < q1; ++q) {                  // wave-uniform
    const i64 i = a.t.pairs[2 * q], j = a.t.pairs[2 * q + 1];
    VdState s = vd_walk(a, i, j, pair_own(a.t, i), lane, 64);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {               // (every lane of the wave arrives)
      VdState u;
      u.best = __shfl_xor(s.best, o, 64);
      u.dn = __shfl_xor(s.dn, o, 64);
      u.ida = __shfl_xor(s.ida, o, 64);
      u.idd = __shfl_xor(s.idd, o, 64);
      if (u.best < s.best) {
        s = u;
      } else if (u.best == s.best) {
        s.dn |= u.dn;
        s.ida = min(s.ida, u.ida);
        s.idd = min(s.idd, u.idd);
      }
    }
    if (lane == 0) vd_store(a, q, s);
  }
}

// Local row rows[blockIdx.x] (a row an alive added policy selects: the class
// row cannot absorb a pod-level set) rewritten bit by bit: lane l of a wave
// walks pair (i, 64 w + l) over the class part and the added policies, the
// ballot is the word.  Every word of the row is written, the bits at
// positions >= n and the words W .. ldM - 1 as zeros.  Exact by construction;
// speed on this path is not a goal.
__global__ __launch_bounds__(TPB) void k_verdict_rows(VerdictArgs a,
                                                      const int32_t* __restrict__ rows, i64 n,
                                                      u64* __restrict__ M, i64 ldM) {
  const i64 r = rows[blockIdx.x], i = a.t.r0 + r;
  const int lane = threadIdx.x & 63;
  for (i64 w = threadIdx.x >> 6; w < ldM; w += TPB / 64) {   // wave-uniform
    const i64 j = w * 64 + lane;
    bool bit = false;
    if (w < a.t.W && j < n) {
      const VdState s = vd_walk(a, i, j, true, 0, 1);
      bit = s.best != VD_NONE && !s.dn;
    }
    const u64 word = __ballot(bit);
    if (lane == 0) M[r * ldM + w] = word;
  }
}

}  // namespace kano
