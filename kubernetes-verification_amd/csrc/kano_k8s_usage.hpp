// kano_k8s_usage.hpp -- which rules of a policy set do anything at all under
// k8s.connectivity: kano_k8s_rule_usage (DESIGN.md "k8s.connectivity", the
// rule usage).  Per direction and over every ordered pair (x, y) of pods it
// counts, exactly,
//   decided[p]  the pairs whose decider is entry p   } as kano_k8s_pair_verdicts
//   passed[p]   the pairs whose passed entry is p    } names them per pair
//   tiers[8]    the pairs per (tier, verdict): index tier * 2 + deny
//   sole[g]     the pairs the NetworkPolicy tier allows where every live
//               allowing entry that matches belongs to group g (a group = the
//               entries of one rule): what removing the rule alone would deny
// A pair's answer depends only on (row class of x, column class of y), so the
// counts come from one walk of every class's ordered copy (k_verdict_order:
// ascending (code, id), a total order), 64 column classes a word:
//   m = AC[p][w]:   newly = m & open;  open &= ~m        (first match)
//   admin allow / deny: decided[p] += weight(newly);  pass: passed[p] += .. and
//   the pass mask keeps the bits;  rest = open | pass mask
//   a class with a live entry at np: an allow entry decides m & rest & ~(the
//   bits allowed before it), the remainder of rest is (network, deny); else
//   the baseline entries take first match on rest, the remainder is default
//   weight(bits of word w) = rsize[c] * sum of csize[64 w + b] over the bits
// (csize is 0 past the last column class, which also neutralises the pad bits
// of open = ~0).  sole takes a second walk of the np run: ones / twos masks of
// the groups' ORs say which bits exactly one group matches.
// All counters are 64-bit integer atomics: exact, whatever the arrival order.
// An entry's weights are summed over the class's words -- across the wl lanes
// of its group by shuffles, across waves through LDS when wl > 64 -- before
// the one global atomic, so a call issues at most one atomic per entry of the
// ordered copies (and of the np runs again for sole) plus 8 per block.
// With KANO_K8S_CONN_SELF k_usage_self takes the n diagonal pairs back out: a
// lane per pod, the same first-match walk for the one bit (rcls[x], ccls[x]).
#pragma once
#include "kano_k8s_pairs.hpp"

namespace kano {

using ull = unsigned long long;
constexpr int USAGE_CS_LDS = 12288;   // column classes whose sizes k_usage_class keeps in LDS

// one direction: the ordered copy, the class sizes and the counters
struct K8sUsageSide {
  i64 U;                  // row classes
  const i64* soffc;
  const int32_t* olist;   // k_verdict_order's copy
  const uint32_t* okey;
  const int32_t* ocnt;
  uint32_t np;
  const u64* AC;
  i64 ldC;
  const int32_t* group;   // per engine id, non-decreasing
  const int32_t* rsize;   // U: the pods of a row class
  const int32_t* csize;   // ldC * 64: the pods of a column class, 0 past the last
  ull* decided;           // P
  ull* passed;            // P
  ull* sole;              // groups
  ull* tiers;             // 8
};

// out[cls[i]] += 1 over the pods: the class sizes.  With few classes every pod
// would add to one of a few addresses, so up to USAGE_HIST_LDS bins a block
// counts its pods (grid-stride) in LDS first and adds its nonzero bins once;
// with more bins the adds spread out by themselves and go to memory directly.
constexpr int USAGE_HIST_LDS = 8192;
__global__ __launch_bounds__(TPB) void k_usage_hist(const int32_t* __restrict__ cls, i64 n,
                                                    int32_t* __restrict__ out, i64 bins) {
  __shared__ int32_t sh[USAGE_HIST_LDS];
  const i64 stride = (i64)gridDim.x * TPB;
  if (bins > USAGE_HIST_LDS) {                         // (block-uniform)
    for (i64 i = (i64)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) atomicAdd(&out[cls[i]], 1);
    return;
  }
  for (i64 b = threadIdx.x; b < bins; b += TPB) sh[b] = 0;
  __syncthreads();
  for (i64 i = (i64)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) atomicAdd(&sh[cls[i]], 1);
  __syncthreads();
  for (i64 b = threadIdx.x; b < bins; b += TPB)
    if (sh[b]) atomicAdd(&out[b], sh[b]);
}

// the pods behind the bits of one word (cs = csize + 64 w)
__device__ __forceinline__ u64 usage_weight(u64 bits, const int32_t* cs) {
  u64 s = 0;
  while (bits) {
    s += (u64)cs[__builtin_ctzll(bits)];
    bits &= bits - 1;
  }
  return s;
}

// v summed over the wl lanes of a class's group; every lane of the wave
// (WIDE: of the block) arrives.  !WIDE: wl <= 64, a group lies inside a wave.
// WIDE: a group is wl / 64 whole waves, their sums meet in part[].
template <bool WIDE>
__device__ __forceinline__ u64 usage_group_sum(u64 v, int wl, u64* part) {
  if (!WIDE) {
    if (wl == 1 || __ballot(v != 0) == 0) return v;
    for (int o = wl >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
  if (!__syncthreads_or(v != 0)) return 0;           // (also: part[] is read by now)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const int nw = wl >> 6, w0 = (int)(threadIdx.x / wl) * nw;
  u64 s = 0;
  for (int k = 0; k < nw; ++k) s += part[w0 + k];
  return s;
}

// k_conn_tier_class's shape (a group of wl lanes a class, lane l of it the
// words l, l + wl, ..), walked entry by entry.  The trip counts are made
// wave-uniform (WIDE: block-uniform) so that every lane meets every group sum;
// a lane past its class's list, or past ldC, adds zeros.
template <bool WIDE>
__global__ __launch_bounds__(TPB) void k_usage_class(K8sUsageSide a, int wl) {
  __shared__ ull sh_t[8];
  __shared__ u64 part[TPB / 64];
  __shared__ int32_t sh_cs[USAGE_CS_LDS];
  const int t = threadIdx.x, lane = t & (wl - 1), g = t / wl, cpb = TPB / wl;
  const uint32_t np = a.np;
  const i64 ldC = a.ldC, rounds = (ldC + wl - 1) / wl;
  // the column classes' sizes are read a bit at a time, one dependent load
  // after the other: from LDS where they fit
  const bool staged = ldC * 64 <= USAGE_CS_LDS;
  if (staged)
    for (i64 k = t; k < ldC * 64; k += TPB) sh_cs[k] = a.csize[k];
  if (t < 8) sh_t[t] = 0;
  __syncthreads();
  const int32_t* csize = staged ? sh_cs : a.csize;
  u64 t_def = 0, t_aa = 0, t_ad = 0, t_na = 0, t_nd = 0, t_ba = 0, t_bd = 0;
  for (i64 c0 = (i64)blockIdx.x * cpb; c0 < a.U; c0 += (i64)gridDim.x * cpb) {   // block-uniform
    const i64 c = c0 + g;
    const bool have = c < a.U;
    const i64 s0 = have ? a.soffc[c] : 0;
    const int m = have ? a.ocnt[c] : 0;
    const u64 rs = have ? (u64)a.rsize[c] : 0;
    int mm = m;
    if (WIDE) {
      for (int k = 0; k < cpb; ++k)
        if (c0 + k < a.U) mm = max(mm, a.ocnt[c0 + k]);
    } else {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mm = max(mm, __shfl_xor(mm, o, 64));
    }
    for (i64 r = 0; r < rounds; ++r) {
      const i64 w = lane + r * wl;
      const bool on = have && w < ldC;
      const int32_t* cs = csize + 64 * (on ? w : 0);
      u64 open = ~0ull, pmask = 0, alw = 0, ones = 0, twos = 0, gm = 0;
      int32_t curg = -1;
      bool admin = true, at_np = false;
      for (int k = 0; k < mm; ++k) {
        u64 v = 0;
        ull* dst = nullptr;
        if (k < m) {
          const uint32_t code = a.okey[s0 + k];
          const int32_t p = a.olist[s0 + k];
          const u64 x = on ? a.AC[(i64)p * ldC + w] : 0;
          const uint32_t lv = code >> 2, act = code & 3u;
          if (lv < np) {
            const u64 newly = x & open;
            open &= ~x;
            v = rs * usage_weight(newly, cs);
            if (act == TIER_PASS) {
              pmask |= newly;
              dst = a.passed + p;
            } else {
              dst = a.decided + p;
              (act == TIER_DENY ? t_ad : t_aa) += v;
            }
          } else {
            if (admin) {                               // the admin tier ends: open is rest
              open |= pmask;
              admin = false;
            }
            if (lv == np) {
              at_np = true;
              if (act == TIER_ALLOW) {
                const int32_t gp = a.group[p];
                if (gp != curg) {                      // the group before ends
                  twos |= ones & gm;
                  ones |= gm;
                  gm = 0;
                  curg = gp;
                }
                gm |= x;
                const u64 newly = x & open & ~alw;
                alw |= newly;
                v = rs * usage_weight(newly, cs);
                dst = a.decided + p;
                t_na += v;
              }
            } else if (!at_np) {
              const u64 newly = x & open;
              open &= ~x;
              v = rs * usage_weight(newly, cs);
              dst = a.decided + p;
              (act == TIER_DENY ? t_bd : t_ba) += v;
            }
          }
        }
        v = usage_group_sum<WIDE>(v, wl, part);
        if (lane == 0 && v) atomicAdd(dst, (ull)v);
      }
      if (admin) open |= pmask;
      if (on) (at_np ? t_nd : t_def) += rs * usage_weight(at_np ? open & ~alw : open, cs);
      // sole: the bits of the network tier that exactly one group matches
      const bool again = WIDE ? __syncthreads_or(at_np) != 0 : __ballot(at_np) != 0;
      if (!again) continue;
      twos |= ones & gm;
      ones |= gm;
      const u64 solo = ones & ~twos & open;
      gm = 0;
      curg = -1;
      for (int k = 0; k < mm; ++k) {
        u64 v = 0;
        ull* dst = nullptr;
        if (k < m && at_np && a.okey[s0 + k] == np * 4u + TIER_ALLOW) {
          const int32_t p = a.olist[s0 + k];
          const u64 x = on ? a.AC[(i64)p * ldC + w] : 0;
          const int32_t gp = a.group[p];
          if (gp != curg) {
            gm = 0;
            curg = gp;
          }
          v = rs * usage_weight(x & solo & ~gm, cs);   // each bit once a group
          gm |= x;
          dst = a.sole + gp;
        }
        v = usage_group_sum<WIDE>(v, wl, part);
        if (lane == 0 && v) atomicAdd(dst, (ull)v);
      }
    }
  }
  const u64 tl[8] = {t_def, 0, t_aa, t_ad, t_na, t_nd, t_ba, t_bd};
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (tl[i]) atomicAdd(&sh_t[i], (ull)tl[i]);
  __syncthreads();
  if (t < 8 && sh_t[t]) atomicAdd(a.tiers + t, sh_t[t]);
}

// The diagonal pair (x, x) of every pod taken out of the counts again: the
// walk of k_usage_class for the one bit (rcls[x], ccls[x]), a lane per pod.
__global__ __launch_bounds__(TPB) void k_usage_self(K8sUsageSide a,
                                                    const int32_t* __restrict__ rcls,
                                                    const int32_t* __restrict__ ccls, i64 n) {
  const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
  const bool live = i < n;
  int tier = -1;
  if (live) {
    const int32_t c = rcls[i], j = ccls[i];
    const i64 s0 = a.soffc[c], w = j >> 6;
    const int m = a.ocnt[c];
    const u64 bit = 1ull << (j & 63);
    const uint32_t np = a.np;
    int32_t dec = -1, pas = -1, first = -1, groups = 0, lastg = -1;
    bool open = true, at_np = false;
    int deny = 0;
    tier = K8S_TIER_DEFAULT;
    for (int k = 0; k < m; ++k) {                      // admin, then the np run, then the baseline
      const uint32_t code = a.okey[s0 + k];
      const int32_t p = a.olist[s0 + k];
      const uint32_t lv = code >> 2, act = code & 3u;
      if (lv > np && at_np) break;                     // isolated: the baseline is not read
      if (lv == np) at_np = true;
      if (lv < np ? !open : lv == np && act != TIER_ALLOW) continue;
      if (!(a.AC[(i64)p * a.ldC + w] & bit)) continue;
      if (lv < np) {
        open = false;
        if (act == TIER_PASS) {
          pas = p;
          continue;
        }
        tier = K8S_TIER_ADMIN, deny = act == TIER_DENY, dec = p;
        break;
      }
      if (lv > np) {
        tier = K8S_TIER_BASELINE, deny = act == TIER_DENY, dec = p;
        break;
      }
      if (first < 0) first = p;
      const int32_t gp = a.group[p];
      groups += gp != lastg;
      lastg = gp;
    }
    if (tier == K8S_TIER_DEFAULT && at_np) {
      tier = K8S_TIER_NETWORK, deny = first < 0, dec = first;
      if (groups == 1) atomicAdd(a.sole + lastg, ~0ull);
    }
    if (dec >= 0) atomicAdd(a.decided + dec, ~0ull);
    if (pas >= 0) atomicAdd(a.passed + pas, ~0ull);
    tier = tier * 2 + deny;
  }
  // the tiers by ballot: one atomic a wave and value
  for (int v = 0; v < 8; ++v) {                       // (every lane of the wave arrives)
    const u64 b = __ballot(tier == v);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.tiers + v, (ull)0 - (ull)__popcll(b));
  }
}

}  // namespace kano
