// kano_k8s_pairs.hpp -- which tier and which rule decide a pod pair under
// k8s.connectivity: kano_k8s_pair_verdicts (DESIGN.md "k8s.connectivity", the
// pair verdicts).  The rule is kano_k8s_conn_tiers' (kano_k8s_tiers.hpp), read
// per pair instead of per class row: for a pair (s, d) the egress direction
// has subject x = s and peer y = d on the egress build, the ingress direction
// x = d and y = s on the ingress build.  Per direction the pair walk
// (kano_pairwalk.hpp; the added part is empty, the codes stand in for the
// removed-id flags) visits every live entry p of S(rcls[x]):
//   isolated |= level(p) == np             (no hit on the allow side needed)
//   p matches the pair iff bit ccls[y] of AC[p] is set
// and keeps three minima of (code, id) as one 64-bit key over the matching
// entries: a below np (the admin tier), m at code np * 4 (a NetworkPolicy
// entry that allows), b above np (the baseline).  Then
//   a allows or denies        -> admin, that action, decider a
//   a passes                  -> passed = a, and on as if no admin rule matched
//   isolated                  -> network: allow by m, else deny (no decider)
//   b                         -> baseline, its action, decider b
//   else                      -> default, allow
// Several actions on one level resolve allow, deny, pass -- the order of the
// codes, so the minimum is kano_k8s_conn_tiers' answer and the decider the
// smallest engine id at the winning code.  Both directions of a pair are
// resolved in one launch and the verdict byte is composed here.  One pair
// belongs to one lane or one wave: no atomics.
#pragma once
#include "kano_k8s_tiers.hpp"
#include "kano_pairwalk.hpp"

namespace kano {

constexpr int K8S_TIER_DEFAULT = 0, K8S_TIER_ADMIN = 1, K8S_TIER_NETWORK = 2, K8S_TIER_BASELINE = 3;
constexpr u64 K8S_NO_ENTRY = ~0ull;   // above every (live code, id) key

// one direction's tables: t.key holds the engine ids' codes, t.rcls is null
// for a side without classes (it resolves to default, allow)
struct K8sPairSide {
  PairTables t;
  uint32_t np;
  int32_t* decider;   // Q, nullable
  int32_t* passed;    // Q, nullable
};

struct K8sPairArgs {
  K8sPairSide side[2];     // egress, ingress
  const int32_t* pairs;    // (src, dst) x Q
  i64 Q;
  int self;                // KANO_K8S_CONN_SELF: s == d is allowed as self traffic
  uint8_t* verdict;        // Q
};

__device__ __forceinline__ u64 k8s_min(u64 x, u64 y) { return x < y ? x : y; }

struct K8sDirState {
  u64 a = K8S_NO_ENTRY, m = K8S_NO_ENTRY, b = K8S_NO_ENTRY;
  bool iso = false;
};

// the state of subject x and peer y over the positions k0, k0 + step, .. of
// the list (s0, s) with y's column class cx, a pair_list of the caller's
__device__ __forceinline__ K8sDirState k8s_dir_walk(const K8sPairSide& d, i64 x, i64 y, i64 s0,
                                                    i64 s, i64 cx, i64 k0, i64 step) {
  K8sDirState st;
  const uint32_t np = d.np;
  pair_walk(
      d.t, x, y, pair_own(d.t, x), s0, s, cx, k0, step,
      [&](i64 p) {
        const uint32_t c = d.t.key[p];
        if (c == TIER_DROPPED) return false;
        st.iso |= (c >> 2) == np;
        return true;
      },
      [&](i64 p) {
        const uint32_t c = d.t.key[p];
        const u64 k = ((u64)c << 32) | (uint32_t)p;
        const uint32_t lv = c >> 2;
        if (lv < np) st.a = k8s_min(st.a, k);
        else if (lv > np) st.b = k8s_min(st.b, k);
        else if (c == np * 4u + TIER_ALLOW) st.m = k8s_min(st.m, k);
      });
  return st;
}

// both directions of (s, d): the two lists are looked up first, so the four
// class loads and then the four offset loads are in flight together before
// either walk waits for its own
__device__ __forceinline__ void k8s_pair_walk(const K8sPairArgs& a, i64 s, i64 d, i64 k0, i64 step,
                                              K8sDirState& eg, K8sDirState& in) {
  i64 e0, es, ex, i0, is, ix;
  pair_list(a.side[0].t, s, d, e0, es, ex);
  pair_list(a.side[1].t, d, s, i0, is, ix);
  eg = k8s_dir_walk(a.side[0], s, d, e0, es, ex, k0, step);
  in = k8s_dir_walk(a.side[1], d, s, i0, is, ix, k0, step);
}

// one direction resolved and its ids stored: tier | deny << 2
__device__ __forceinline__ int k8s_dir_resolve(const K8sPairSide& d, i64 q, const K8sDirState& st) {
  int tier = K8S_TIER_DEFAULT, deny = 0;
  int32_t decider = -1, passed = -1;
  bool done = false;
  if (st.a != K8S_NO_ENTRY) {
    const uint32_t act = (uint32_t)(st.a >> 32) & 3u;
    if (act == TIER_PASS) {
      passed = (int32_t)(uint32_t)st.a;
    } else {
      tier = K8S_TIER_ADMIN, deny = act == TIER_DENY, decider = (int32_t)(uint32_t)st.a;
      done = true;
    }
  }
  if (!done && st.iso) {
    tier = K8S_TIER_NETWORK, deny = st.m == K8S_NO_ENTRY;
    if (!deny) decider = (int32_t)(uint32_t)st.m;
  } else if (!done && st.b != K8S_NO_ENTRY) {
    tier = K8S_TIER_BASELINE, deny = ((uint32_t)(st.b >> 32) & 3u) == TIER_DENY;
    decider = (int32_t)(uint32_t)st.b;
  }
  if (d.decider) d.decider[q] = decider;
  if (d.passed) d.passed[q] = passed;
  return tier | (deny << 2);
}

// verdict[q]: bit 0 allowed, 1 self traffic, 2-3 the egress tier, 4 egress
// denies, 5-6 the ingress tier, 7 ingress denies
__device__ __forceinline__ void k8s_pair_store(const K8sPairArgs& a, i64 q, i64 s, i64 d,
                                               const K8sDirState& eg, const K8sDirState& in) {
  const int e = k8s_dir_resolve(a.side[0], q, eg), i = k8s_dir_resolve(a.side[1], q, in);
  const int self = a.self && s == d;
  const int allowed = self | !((e | i) & 4);
  a.verdict[q] = (uint8_t)(allowed | (self << 1) | (e << 2) | (i << 5));
}

// a lane per pair, both lists walked serially; grid-stride over the pairs
__global__ __launch_bounds__(TPB) void k_k8s_pair_lane(K8sPairArgs a) {
  const i64 stride = (i64)gridDim.x * TPB;
  for (i64 q = (i64)blockIdx.x * TPB + threadIdx.x; q < a.Q; q += stride) {
    const i64 s = a.pairs[2 * q], d = a.pairs[2 * q + 1];
    K8sDirState eg, in;
    k8s_pair_walk(a, s, d, 0, 1, eg, in);
    k8s_pair_store(a, q, s, d, eg, in);
  }
}

__device__ __forceinline__ void k8s_dir_meet(K8sDirState& st) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                 // (every lane of the wave arrives)
    st.a = k8s_min(st.a, __shfl_xor(st.a, o, 64));
    st.m = k8s_min(st.m, __shfl_xor(st.m, o, 64));
    st.b = k8s_min(st.b, __shfl_xor(st.b, o, 64));
  }
  st.iso = __ballot(st.iso) != 0;
}

// a wave per pair, the lanes striding both lists; the three minima and the
// isolated flag of each direction then met across the wave
__global__ __launch_bounds__(TPB) void k_k8s_pair_wave(K8sPairArgs a) {
  const int lane = threadIdx.x & 63;
  i64 q0, q1;
  wave_pair_run(a.Q, q0, q1);
  for (i64 q = q0; q < q1; ++q) {                    // wave-uniform
    const i64 s = a.pairs[2 * q], d = a.pairs[2 * q + 1];
    K8sDirState eg, in;
    k8s_pair_walk(a, s, d, lane, 64, eg, in);
    k8s_dir_meet(eg);
    k8s_dir_meet(in);
    if (lane == 0) k8s_pair_store(a, q, s, d, eg, in);
  }
}

}  // namespace kano
