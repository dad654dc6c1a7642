// The Kubernetes reading of NetworkPolicies (networking.k8s.io/v1) over two
// class-level builds: kano_k8s_conn (DESIGN.md "k8s.connectivity").
//
// The host compiles the policies to two kano policy lists (kano/k8s.py
// compile_conformant): the egress build has E[src][dst], the ingress build
// I[dst][src]; an entry selects the policy's pods and allows one peer.  Every
// policy of a type contributes an entry, so a pod is isolated in a direction
// iff its row class's list S(c) of that build is not empty.  With rc / cc the
// row and column classes of the two builds:
//   allowed[s][d] = Re[rc_e(s)][cc_e(d)] & Ti[cc_i(s)][rc_i(d)] | (s == d & SELF)
//   Re[a] = S_e(a) empty ? all ones : OR of AC_e[p] over the kept p of S_e(a)
//   Ri[b] likewise for the ingress build, Ti = Ri transposed (k_k8s_transpose)
// A port query is a keep mask over the entries; isolation reads every entry.
#pragma once
#include "kano_k8s.hpp"

namespace kano {

// R[c][w] for every row class c (grid-stride, one block a class; the shape
// of k_ports_class: TPB / wl slices of wl lanes, the slices' words meeting in
// LDS).  A class without entries is not isolated: all ones.  keep == nullptr
// keeps every entry, and the row is the build's own Mc[c].
__global__ __launch_bounds__(TPB) void k_conn_class(i64 U, const i64* __restrict__ soffc,
                                                    const int32_t* __restrict__ slist,
                                                    const uint8_t* __restrict__ keep,
                                                    const u64* __restrict__ AC,
                                                    const u64* __restrict__ Mc, i64 ldC, int wl,
                                                    u64* __restrict__ R) {
  __shared__ u64 red[TPB];
  const int t = threadIdx.x, wlane = t & (wl - 1), slice = t / wl, ns = TPB / wl;
  for (i64 c = blockIdx.x; c < U; c += gridDim.x) {
    const i64 s0 = soffc[c], s1 = soffc[c + 1];
    if (s1 == s0 || !keep) {                              // block-uniform
      for (i64 w = t; w < ldC; w += TPB) R[c * ldC + w] = s1 == s0 ? ~0ull : Mc[c * ldC + w];
      continue;
    }
    for (i64 w0 = 0; w0 < ldC; w0 += wl) {
      const i64 w = w0 + wlane;
      u64 x = 0;
      for (i64 k = s0 + slice; k < s1; k += ns) {
        const int32_t p = slist[k];
        if (keep[p] && w < ldC) x |= AC[(i64)p * ldC + w];
      }
      red[t] = x;
      __syncthreads();
      for (int h = ns >> 1; h > 0; h >>= 1) {
        if (slice < h) red[t] |= red[t + h * wl];
        __syncthreads();
      }
      if (slice == 0 && w < ldC) R[c * ldC + w] = red[t];
      __syncthreads();
    }
  }
}

// iso[i] (nullable) = pod i's row class has entries; *count += the isolated pods
__global__ __launch_bounds__(TPB) void k_conn_isolated(const int32_t* __restrict__ rcls,
                                                       const i64* __restrict__ soffc, i64 n,
                                                       uint8_t* __restrict__ iso,
                                                       unsigned long long* __restrict__ count) {
  const i64 i = (i64)blockIdx.x * TPB + threadIdx.x;
  int v = 0;
  if (i < n) {
    const i64 c = rcls[i];
    v = soffc[c + 1] > soffc[c];
    if (iso) iso[i] = (uint8_t)v;
  }
  const u64 b = __ballot(v);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// Pod rows from the two class-level tables, k_k8s_expand's shape: a block is
// 16 words (1024 dst pods) x 64 src rows (local row r is pod g0 + r).  The
// 1024 destinations' class ids cc_e(d) and rc_i(d) sit in LDS and then in
// each lane's registers; per src row a lane gathers its pod's bit of
// Re[rc_e(s)] and of Ti[cc_i(s)], ANDs them, a ballot packs 64 pods into a
// word, the lane owning word s >> 6 sets the diagonal bit, and lanes 0-15
// store the row's 16 contiguous words (128 B).  STAGE (the two class rows
// together of <= CONN_STAGE_W words): the block's 64 row pairs are staged in
// LDS first, each table at its own pitch.
// Re == nullptr / Ti == nullptr: that side has no entries and constrains
// nothing (its class ids are not read).  rce == nullptr / cci == nullptr: row
// s is that table's class s -- the streamed form's expansion of one table's
// class rows (the other table absent, no diagonal).
constexpr int CONN_STAGE_W = 2 * K8S_STAGE_W;
template <bool STAGE>
__global__ __launch_bounds__(TPB) void k_conn_expand(const u64* __restrict__ Re, i64 ldE,
                                                     const int32_t* __restrict__ rce,
                                                     const int32_t* __restrict__ cce,
                                                     const u64* __restrict__ Ti, i64 ldT,
                                                     const int32_t* __restrict__ cci,
                                                     const int32_t* __restrict__ rci, int self,
                                                     i64 g0, i64 rows, i64 n, i64 W,
                                                     u64* __restrict__ M, i64 ldM) {
  __shared__ int32_t cid[2 * K8S_XW * 64];
  __shared__ u64 rowbuf[STAGE ? K8S_XR * CONN_STAGE_W : 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const i64 w0 = (i64)blockIdx.x * K8S_XW, r0 = (i64)blockIdx.y * K8S_XR;
  for (int t = threadIdx.x; t < K8S_XW * 64; t += TPB) {
    const i64 j = w0 * 64 + t;
    cid[t] = (j < n && Re) ? cce[j] : 0;
    cid[K8S_XW * 64 + t] = (j < n && Ti) ? rci[j] : 0;
  }
  const i64 r1 = r0 + K8S_XR < rows ? r0 + K8S_XR : rows;
  u64* const bufE = rowbuf;
  u64* const bufT = rowbuf + (STAGE && Re ? K8S_XR * ldE : 0);
  if (STAGE) {
    if (Re)
      for (int t = threadIdx.x; t < K8S_XR * ldE; t += TPB) {
        const i64 rr = t / ldE, w = t % ldE, r = r0 + rr;
        bufE[t] = r < r1 ? Re[(rce ? (i64)rce[g0 + r] : g0 + r) * ldE + w] : 0ull;
      }
    if (Ti)
      for (int t = threadIdx.x; t < K8S_XR * ldT; t += TPB) {
        const i64 rr = t / ldT, w = t % ldT, r = r0 + rr;
        bufT[t] = r < r1 ? Ti[(cci ? (i64)cci[g0 + r] : g0 + r) * ldT + w] : 0ull;
      }
  }
  __syncthreads();
  int ce[K8S_XW], ci[K8S_XW];
#pragma unroll
  for (int k = 0; k < K8S_XW; ++k) {
    ce[k] = cid[k * 64 + lane];
    ci[k] = cid[K8S_XW * 64 + k * 64 + lane];
  }
  // wave wv takes rows r0 + wv, r0 + wv + 4, ...: all 16 words of each
  for (i64 r = r0 + wv; r < r1; r += TPB / 64) {
    const i64 s = g0 + r;
    const u64* er = !Re ? nullptr : STAGE ? bufE + (r - r0) * ldE
                                          : Re + (rce ? (i64)rce[s] : s) * ldE;
    const u64* tr = !Ti ? nullptr : STAGE ? bufT + (r - r0) * ldT
                                          : Ti + (cci ? (i64)cci[s] : s) * ldT;
    u64 mine = 0;
#pragma unroll
    for (int k = 0; k < K8S_XW; ++k) {
      int bit = (w0 + k) * 64 + lane < n;
      if (er) bit &= (int)((er[ce[k] >> 6] >> (ce[k] & 63)) & 1ull);
      if (tr) bit &= (int)((tr[ci[k] >> 6] >> (ci[k] & 63)) & 1ull);
      const u64 b = __ballot(bit);
      if (lane == k) mine = b;
    }
    if (lane < K8S_XW) {
      const i64 w = w0 + lane;
      if (self && w == (s >> 6)) mine |= 1ull << (s & 63);
      if (w < ldM) M[r * ldM + w] = w < W ? mine : 0ull;
    }
  }
}

// The streamed form, k_k8s_rows' shape: both tables' class rows are expanded
// to pod words once (k_conn_expand, one table a launch: XE[a] = Re[a] over
// cc_e(d), XT[x] = Ti[x] over rc_i(d); pad bits and pad words zero), then
// every held row is
//   M[r] = XE[rc_e(s)] & XT[cc_i(s)] | diagonal,   s = g0 + r,
// 16 bytes a lane.  One of XE / XT may be nullptr (a side without entries).
__global__ __launch_bounds__(TPB) void k_conn_rows(const u64* __restrict__ XE,
                                                   const int32_t* __restrict__ rce,
                                                   const u64* __restrict__ XT,
                                                   const int32_t* __restrict__ cci, int self,
                                                   i64 g0, i64 rows, i64 ldM,
                                                   u64* __restrict__ M) {
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const i64 h = ldM / 2;                                  // ldM is a multiple of 16
  const i64 t = (i64)blockIdx.x * TPB + threadIdx.x;
  if (t >= rows * h) return;
  const i64 r = t / h, q = t % h, s = g0 + r;
  u64x2 v;
  if (XE) {
    v = reinterpret_cast<const u64x2*>(XE + (i64)rce[s] * ldM)[q];
    if (XT) v &= reinterpret_cast<const u64x2*>(XT + (i64)cci[s] * ldM)[q];
  } else {
    v = reinterpret_cast<const u64x2*>(XT + (i64)cci[s] * ldM)[q];
  }
  if (self && (s >> 7) == q) {
    if ((s >> 6) & 1) v.y |= 1ull << (s & 63);
    else v.x |= 1ull << (s & 63);
  }
  reinterpret_cast<u64x2*>(M + r * ldM)[q] = v;
}

}  // namespace kano
