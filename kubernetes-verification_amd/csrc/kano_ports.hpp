// kano_ports.hpp -- port-aware reachability from the resident tables (the
// tables kano_pair_policies reads; the matrix is not touched).
//   subset(S)[i, j]  = 1 iff some alive p in S has i in select_p, j in allow_p
//   pair_masks(i, j) = OR of pmask[p] over the alive p with i in select_p and
//                      j in allow_p (KW words a policy)
// A subset matrix is written in three steps:
//   k_ports_class    the class-level rows McS[c] = OR_{p in S(c), use[p]} AC[p],
//                    once per row class (k_inc_rewrite's first loop runs it
//                    once per member pod)
//   k_path_expand16  (kano_path.hpp, after k_bit_transpose) kano_path's own
//                    last step: a chunk of 16 class rows expanded to pod words
//                    once, in LDS, and streamed to every member row
//   k_ports_rows     only with kept added policies (or without classes): their
//                    pod-level allow sets OR-ed into the rows they select
#pragma once
#include "kano_pairwalk.hpp"
#include "kano_prims.hpp"

namespace kano {

// McS[c][w] = OR of AC[p][w] over the p of S(c) with use[p] (alive and kept),
// one block per row class (grid-stride).  The block is TPB / wl slices of wl
// lanes (wl a power of two <= TPB, the host's: the smallest covering ldC):
// lane t % wl takes word w0 + t % wl, slice t / wl every (TPB / wl)-th policy
// of S(c), so a row of AC is read by consecutive lanes and a class with
// thousands of policies is split over the slices; the slices' words meet in
// LDS.  *kept_classes += 1 for every class with a kept policy.
__global__ __launch_bounds__(TPB) void k_ports_class(i64 U, const i64* __restrict__ soffc,
                                                     const int32_t* __restrict__ slist,
                                                     const uint8_t* __restrict__ use,
                                                     const u64* __restrict__ AC, i64 ldC, int wl,
                                                     u64* __restrict__ McS,
                                                     unsigned* __restrict__ kept_classes) {
  __shared__ u64 red[TPB];
  const int t = threadIdx.x, wlane = t & (wl - 1), slice = t / wl, ns = TPB / wl;
  for (i64 c = blockIdx.x; c < U; c += gridDim.x) {
    const i64 s0 = soffc[c], s1 = soffc[c + 1];
    int any = 0;
    for (i64 w0 = 0; w0 < ldC; w0 += wl) {
      const i64 w = w0 + wlane;
      u64 x = 0;
      for (i64 k = s0 + slice; k < s1; k += ns) {
        const int32_t p = slist[k];
        if (use[p]) {
          any = 1;
          if (w < ldC) x |= AC[(i64)p * ldC + w];
        }
      }
      red[t] = x;
      __syncthreads();
      for (int h = ns >> 1; h > 0; h >>= 1) {
        if (slice < h) red[t] |= red[t + h * wl];
        __syncthreads();
      }
      if (slice == 0 && w < ldC) McS[c * ldC + w] = red[t];
      __syncthreads();
    }
    any = __syncthreads_or(any);
    if (t == 0 && any) atomicAdd(kept_classes, 1u);
  }
}

// The added policies' part of local row r (pod i = r0 + r), 16 bytes a lane:
// M[r] (inplace: as the class rows' expansion wrote it; else zeros -- a build
// without policies has no classes) | aalw[t] of every added policy t with
// use[P + t] that selects i.  aalw's pitch is W; the words W .. ldM - 1 of a
// row stay zero.
__global__ __launch_bounds__(TPB) void k_ports_rows(int inplace, const uint8_t* __restrict__ use,
                                                    i64 P, const u64* __restrict__ asel,
                                                    const u64* __restrict__ aalw, i64 W, i64 A,
                                                    i64 r0, i64 rows, i64 ldM,
                                                    u64* __restrict__ M) {
  const i64 h = ldM / 2;                                  // ldM is a multiple of 16
  const i64 g = (i64)blockIdx.x * TPB + threadIdx.x;
  if (g >= rows * h) return;
  const i64 r = g / h, q = g % h, i = r0 + r;
  u64x2* m = reinterpret_cast<u64x2*>(M + r * ldM) + q;
  u64x2 v = {0ull, 0ull};
  if (inplace) v = *m;
  const i64 w = 2 * q;
  for (i64 t = 0; t < A; ++t) {
    if (!use[P + t] || !((asel[t * W + (i >> 6)] >> (i & 63)) & 1ull)) continue;
    if (w < W) v.x |= aalw[t * W + w];
    if (w + 1 < W) v.y |= aalw[t * W + w + 1];
  }
  *m = v;
}

// ---------------------------------------------------------------------------
// Pair masks: the pair walk (kano_pairwalk.hpp) with out[q * KW + w] = OR of
// pmask[p * KW + w] over the alive matching policies.  The mask words are
// taken PM_CH at a time in registers (one walk for up to 128 slots,
// ceil(KW / PM_CH) walks beyond).  One pair belongs to one lane or one wave:
// no atomics.
// ---------------------------------------------------------------------------
struct PairMaskArgs {
  PairTables t;          // (t.dead: the removed ids' flags)
  const u64* pmask;      // (P + A) x KW
  i64 KW;
  u64* out;              // Q x KW
};
constexpr int PM_CH = 2;

// The mask words of pair q, PM_CH at a time: one list lookup, then a walk per
// chunk over the positions k0, k0 + step, .. (WAVE: a lane's share, the lanes'
// words OR-ed across the wave -- every lane of the wave arrives -- and lane 0
// writing).
template <bool WAVE>
__device__ __forceinline__ void pm_pair(const PairMaskArgs& a, i64 q) {
  const int lane = threadIdx.x & 63;
  const i64 i = a.t.pairs[2 * q], j = a.t.pairs[2 * q + 1];
  const bool own = pair_own(a.t, i);
  i64 s0 = 0, s = 0, x = 0;
  if (own) pair_list(a.t, i, j, s0, s, x);
  for (i64 w0 = 0; w0 < a.KW; w0 += PM_CH) {
    u64 acc[PM_CH];
#pragma unroll
    for (int c = 0; c < PM_CH; ++c) acc[c] = 0;
    pair_walk(
        a.t, i, j, own, s0, s, x, WAVE ? lane : 0, WAVE ? 64 : 1,
        [&](i64 p) { return pair_alive(a.t.dead, p); },
        [&](i64 p) {
#pragma unroll
          for (int c = 0; c < PM_CH; ++c)
            if (w0 + c < a.KW) acc[c] |= a.pmask[p * a.KW + w0 + c];
        });
#pragma unroll
    for (int c = 0; c < PM_CH; ++c) {
      const u64 v = WAVE ? wave_or(acc[c]) : acc[c];
      if ((!WAVE || lane == 0) && w0 + c < a.KW) a.out[q * a.KW + w0 + c] = v;
    }
  }
}

// a lane per pair, S(c) walked serially; grid-stride over the pairs
__global__ __launch_bounds__(TPB) void k_pmask_lane(PairMaskArgs a) {
  const i64 stride = (i64)gridDim.x * TPB;
  for (i64 q = (i64)blockIdx.x * TPB + threadIdx.x; q < a.t.Q; q += stride) pm_pair<false>(a, q);
}

// a wave per pair, the lanes striding S(c) and the added policies
__global__ __launch_bounds__(TPB) void k_pmask_wave(PairMaskArgs a) {
  i64 q0, q1;
  wave_pair_run(a.t.Q, q0, q1);
  for (i64 q = q0; q < q1; ++q) pm_pair<true>(a, q);   // wave-uniform
}

}  // namespace kano
