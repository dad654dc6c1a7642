// AdminNetworkPolicy tiers over the two class-level builds of k8s.connectivity:
// kano_k8s_conn_tiers (DESIGN.md "k8s.connectivity", the tiers).
//
// The host compiles AdminNetworkPolicy, NetworkPolicy and
// BaselineAdminNetworkPolicy rules into the same two builds (kano/k8s.py
// compile_conformant) and gives every engine id a code = level * 4 + action
// (TIER_ALLOW / TIER_DENY / TIER_PASS / TIER_ISOLATE; TIER_DROPPED for an entry
// the query drops).  A level is one rule: the levels below np are the admin
// rules in evaluation order, np is the NetworkPolicy tier (its entries allow,
// or only isolate), the levels above np are the baseline's rules.  Per row
// class c and word w of the column classes, with x(g) the OR of the AC words
// of a run g of equal codes in the (code, id) ordered copy of S(c)
// (k_verdict_order, kano_verdict.hpp; the runs of a level come allow, deny,
// pass):
//   open = ~0, value = passed = 0
//   admin run:   allow: value |= x & open;  pass: passed |= x & open;  open &= ~x
//   rest = open | passed
//   c has an entry at np:  value |= rest & (OR of the allow runs' x at np)
//   else baseline run:     allow: value |= x & rest;  rest &= ~x;  at the end value |= rest
// R[c][w] = value; a class without live entries comes out all ones.  The
// ingress table is then transposed and both are expanded by kano_k8s_conn's
// own kernels (k_k8s_transpose, k_conn_expand, k_conn_rows).
#pragma once
#include "kano_k8s_conn.hpp"
#include "kano_verdict.hpp"

namespace kano {

constexpr uint32_t TIER_ALLOW = 0, TIER_DENY = 1, TIER_PASS = 2, TIER_ISOLATE = 3;
constexpr uint32_t TIER_DROPPED = VD_DEAD;
constexpr uint32_t TIER_MAX_LEVEL = 1u << 30;

// R[c][w] and hasnp[c] (the class has an entry at np: its pods are isolated
// in this direction) for every row class c.  k_verdict_class's shape: a group
// of wl lanes a class, lane l of it the words l, l + wl, ..; one walk of the
// ordered copy per word, any number of levels at the cost of one.  The codes
// and ids are read by position: only the AC word depends on a load.
__global__ __launch_bounds__(TPB) void k_conn_tier_class(i64 U, const i64* __restrict__ soffc,
                                                         const int32_t* __restrict__ olist,
                                                         const uint32_t* __restrict__ okey,
                                                         const int32_t* __restrict__ ocnt,
                                                         uint32_t np, const u64* __restrict__ AC,
                                                         i64 ldC, int wl, u64* __restrict__ R,
                                                         uint8_t* __restrict__ hasnp) {
  const int t = threadIdx.x, lane = t & (wl - 1), g = t / wl, cpb = TPB / wl;
  for (i64 c = (i64)blockIdx.x * cpb + g; c < U; c += (i64)gridDim.x * cpb) {
    const i64 s0 = soffc[c];
    const int m = ocnt[c];
    for (i64 w = lane; w < ldC; w += wl) {
      u64 value = 0, open = ~0ull, passed = 0, allow_np = 0, x = 0;
      bool admin = true, at_np = false;
      // the run x belongs to ends: resolved by its code
      auto resolve = [&](uint32_t code) {
        const uint32_t lv = code >> 2, act = code & 3u;
        if (lv < np) {
          if (act == TIER_ALLOW) value |= x & open;
          if (act == TIER_PASS) passed |= x & open;
          open &= ~x;
          return;
        }
        if (admin) {                                   // the admin tier ends: open is rest
          open |= passed;
          admin = false;
        }
        if (lv == np) {
          at_np = true;
          if (act == TIER_ALLOW) allow_np |= x;
        } else if (!at_np) {
          if (act == TIER_ALLOW) value |= x & open;
          open &= ~x;
        }
      };
      uint32_t cur = m > 0 ? okey[s0] : 0u;
      for (int k = 0; k < m; ++k) {
        const uint32_t code = okey[s0 + k];
        const int32_t p = olist[s0 + k];
        if (code != cur) {
          resolve(cur);
          x = 0;
          cur = code;
        }
        x |= AC[(i64)p * ldC + w];
      }
      if (m > 0) resolve(cur);
      if (admin) open |= passed;
      value |= at_np ? open & allow_np : open;
      R[c * ldC + w] = value;
      if (w == 0) hasnp[c] = (uint8_t)at_np;
    }
  }
}

// iso[i] (nullable) = pod i's row class has an entry at np; *count += those pods
__global__ __launch_bounds__(TPB) void k_conn_tier_isolated(const int32_t* __restrict__ rcls,
                                                            const uint8_t* __restrict__ hasnp,
                                                            i64 n, uint8_t* __restrict__ iso,
                                                            unsigned long long* __restrict__ count) {
  const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
  int v = 0;
  if (i < n) {
    v = hasnp[rcls[i]];
    if (iso) iso[i] = (uint8_t)v;
  }
  const u64 b = __ballot(v);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

}  // namespace kano
