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
// Pair masks: the walk of k_pair_lane / k_pair_wave (kano_kernels.hpp: the
// same tables, the same ownership rule for row shards, the same dead flags)
// with out[q * KW + w] = OR of pmask[p * KW + w] over pols(i, j) instead of
// a count.  The mask words are taken PM_CH at a time in registers (one walk
// for up to 128 slots, ceil(KW / PM_CH) walks beyond).  One pair belongs to
// one lane or one wave: no atomics.
// ---------------------------------------------------------------------------
struct PairMaskArgs {
  const int32_t* pairs;  // (i, j) x Q
  i64 Q;
  const int32_t* rcls;   // null: the build had no policies (only the added part)
  const int32_t* ccls;
  const i64* soffc;
  const int32_t* slist;
  const uint8_t* dead;   // P + A flags; null: none removed
  const u64* AC;
  i64 ldC;
  i64 P;
  const u64* asel;
  const u64* aalw;
  i64 W, A;
  i64 r0, r1;
  const u64* pmask;      // (P + A) x KW
  i64 KW;
  u64* out;              // Q x KW
};
constexpr int PM_CH = 2;
// the wave form when a pair walks more than this many policies on average
// (mean |S(c)| + added policies: k_pair_wave's threshold, PAIR_WAVE_MIN)
constexpr i64 PMASK_WAVE_MIN = 16;

// a lane per pair, S(c) walked serially; grid-stride over the pairs
__global__ __launch_bounds__(TPB) void k_pmask_lane(PairMaskArgs a) {
  const i64 stride = (i64)gridDim.x * TPB;
  for (i64 q = (i64)blockIdx.x * TPB + threadIdx.x; q < a.Q; q += stride) {
    const i64 i = a.pairs[2 * q], j = a.pairs[2 * q + 1];
    const bool own = i >= a.r0 && i < a.r1;
    i64 s0 = 0, s = 0, x = 0;
    if (own && a.rcls) {
      const int32_t c = a.rcls[i];
      s0 = a.soffc[c];
      s = a.soffc[c + 1] - s0;
      x = a.ccls[j];
    }
    for (i64 w0 = 0; w0 < a.KW; w0 += PM_CH) {
      u64 acc[PM_CH];
#pragma unroll
      for (int c = 0; c < PM_CH; ++c) acc[c] = 0;
      for (i64 k = 0; k < s; ++k) {
        const int32_t p = a.slist[s0 + k];
        if (!(a.dead && a.dead[p]) && ((a.AC[(i64)p * a.ldC + (x >> 6)] >> (x & 63)) & 1ull)) {
#pragma unroll
          for (int c = 0; c < PM_CH; ++c)
            if (w0 + c < a.KW) acc[c] |= a.pmask[(i64)p * a.KW + w0 + c];
        }
      }
      for (i64 t = 0; own && t < a.A; ++t) {
        if (!(a.dead && a.dead[a.P + t]) && ((a.asel[t * a.W + (i >> 6)] >> (i & 63)) & 1ull) &&
            ((a.aalw[t * a.W + (j >> 6)] >> (j & 63)) & 1ull)) {
#pragma unroll
          for (int c = 0; c < PM_CH; ++c)
            if (w0 + c < a.KW) acc[c] |= a.pmask[(a.P + t) * a.KW + w0 + c];
        }
      }
#pragma unroll
      for (int c = 0; c < PM_CH; ++c)
        if (w0 + c < a.KW) a.out[q * a.KW + w0 + c] = acc[c];
    }
  }
}

__device__ __forceinline__ u64 wave_or(u64 x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x |= __shfl_xor(x, o, 64);
  return x;
}

// a wave per pair, the lanes striding S(c) and the added policies, the lanes'
// words OR-ed across the wave; wave gw of nw takes a contiguous run of pairs
__global__ __launch_bounds__(TPB) void k_pmask_wave(PairMaskArgs a) {
  const int lane = threadIdx.x & 63;
  const i64 nw = (i64)gridDim.x * (TPB / 64), gw = (i64)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  const i64 per = (a.Q + nw - 1) / nw;
  const i64 q1 = min(a.Q, (gw + 1) * per);
  for (i64 q = gw * per; q < q1; ++q) {          // wave-uniform
    const i64 i = a.pairs[2 * q], j = a.pairs[2 * q + 1];
    const bool own = i >= a.r0 && i < a.r1;
    i64 s0 = 0, s = 0, x = 0;
    if (own && a.rcls) {
      const int32_t c = a.rcls[i];
      s0 = a.soffc[c];
      s = a.soffc[c + 1] - s0;
      x = a.ccls[j];
    }
    for (i64 w0 = 0; w0 < a.KW; w0 += PM_CH) {
      u64 acc[PM_CH];
#pragma unroll
      for (int c = 0; c < PM_CH; ++c) acc[c] = 0;
      for (i64 k = lane; k < s; k += 64) {
        const int32_t p = a.slist[s0 + k];
        if (!(a.dead && a.dead[p]) && ((a.AC[(i64)p * a.ldC + (x >> 6)] >> (x & 63)) & 1ull)) {
#pragma unroll
          for (int c = 0; c < PM_CH; ++c)
            if (w0 + c < a.KW) acc[c] |= a.pmask[(i64)p * a.KW + w0 + c];
        }
      }
      for (i64 t = lane; own && t < a.A; t += 64) {
        if (!(a.dead && a.dead[a.P + t]) && ((a.asel[t * a.W + (i >> 6)] >> (i & 63)) & 1ull) &&
            ((a.aalw[t * a.W + (j >> 6)] >> (j & 63)) & 1ull)) {
#pragma unroll
          for (int c = 0; c < PM_CH; ++c)
            if (w0 + c < a.KW) acc[c] |= a.pmask[(a.P + t) * a.KW + w0 + c];
        }
      }
#pragma unroll
      for (int c = 0; c < PM_CH; ++c) {
        const u64 v = wave_or(acc[c]);             // (every lane of the wave arrives)
        if (lane == 0 && w0 + c < a.KW) a.out[q * a.KW + w0 + c] = v;
      }
    }
  }
}

}  // namespace kano
