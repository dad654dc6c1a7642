// kano_hops.hpp -- shortest paths over the resident bit matrix: a level by
// level breadth-first search for a batch of B sources at once, and the
// canonical witness path of a queried pair (kano_hops / kano_hop_pairs,
// kano_ext.hip).  Read from the matrix itself, so it holds for built,
// updated, edited, loaded, path and edge matrices alike.
//
// With an edge i -> j iff M[i, j] = 1 and L_0 = {s}, V_0 = {} (the source is
// not marked visited: dist(s, s) is the shortest cycle through s),
//   L_k = (OR_{u in L_{k-1}} row(u)) \ V_{k-1},   V_k = V_{k-1} | L_k,
//   dist(s, v) = k iff v in L_k (k >= 1), -1 when v is in no level.
// Per source the device holds dist (n int32), the visited and next bit rows
// (W words each) and the frontier as an index list with its count.  A level
// is two launches:
//   * k_hops_expand: a wave takes (source, chunk of 64 column words, slice
//     of the frontier list), ORs the slice's rows over its chunk in registers
//     and merges into `next` with or_if_new -- the parallelism comes from all
//     three together (one source of C3 has 1,563 words a row: 25 chunks);
//   * k_hops_finish: next & ~visited & valid_mask are the level's new pods:
//     visited takes them, dist = k, and they are compacted into the frontier
//     list of the next level (one atomic per block on the source's count).
// Blocks hand data to each other only across these launch boundaries (the
// atomics on `next` and on the counts are read by the following launch).
// The host reads the B counts after every level and stops when every
// frontier is empty, at max_hops, or -- pair queries -- when every target of
// a source has its distance.
#pragma once
#include "kano_prims.hpp"

namespace kano {

constexpr int HOPS_CW = 64;         // column words of an expand item (one a lane)
constexpr int HOPS_MIN_SLICE = 16;  // frontier rows a wave ORs at least

// The per-batch counters, int32: [count of parity 0 | count of parity 1 |
// targets reached so far], B entries each.  Level k reads the frontier count
// of parity (k - 1) & 1 and writes that of parity k & 1.
__device__ __forceinline__ bool hops_stopped(const int32_t* cnts, const int32_t* ntgt, int B,
                                             int b) {
  return ntgt && cnts[2 * B + b] >= ntgt[b];
}

// dist = -1, visited = next = 0, the frontier {src[b]}, its count 1
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_hops_init(
    int32_t* __restrict__ dist, u64* __restrict__ bits, int32_t* __restrict__ list,
    int32_t* __restrict__ cnts, const int32_t* __restrict__ src, i64 n, i64 W, int B) {
  const i64 stride = (i64)gridDim.x * TPB, t0 = (i64)blockIdx.x * TPB + threadIdx.x;
  for (i64 i = t0; i < (i64)B * n; i += stride) dist[i] = -1;
  for (i64 i = t0; i < 2 * (i64)B * W; i += stride) bits[i] = 0;
  for (i64 b = t0; b < B; b += stride) {
    list[b * n] = src[b];
    cnts[b] = 1;
    cnts[B + b] = 0;
    cnts[2 * B + b] = 0;
  }
}

// next[b] |= OR of the rows of one frontier slice of source b = blockIdx.z
// over the 64 column words of chunk blockIdx.x: a wave an item, the four
// waves of a block take the slices 4 blockIdx.y .. + 3 (no barrier: the
// waves run independently)
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_hops_expand(
    const u64* __restrict__ M, i64 ldM, i64 n, i64 W, const int32_t* __restrict__ list,
    int32_t* __restrict__ cnts, const int32_t* __restrict__ ntgt, int B, int level, int slice,
    u64* next) {
  const int b = blockIdx.z;
  const int32_t cnt = cnts[((level - 1) & 1) * B + b];
  // (the count this level's finish adds to: last read two launches ago)
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) cnts[(level & 1) * B + b] = 0;
  if (cnt <= 0 || hops_stopped(cnts, ntgt, B, b)) return;         // block-uniform
  const i64 k0 = ((i64)blockIdx.y * (TPB / 64) + (threadIdx.x >> 6)) * slice;
  if (k0 >= cnt) return;                                           // wave-uniform
  const i64 k1 = min((i64)cnt, k0 + slice);
  const i64 w = (i64)blockIdx.x * HOPS_CW + (threadIdx.x & 63);
  if (w >= W) return;
  const int32_t* fl = list + (i64)b * n;
  const u64* col = M + w;
  u64 acc = 0;
  i64 k = k0;
  for (; k + 4 <= k1; k += 4) {
    const u64 a0 = col[(i64)fl[k] * ldM], a1 = col[(i64)fl[k + 1] * ldM];
    const u64 a2 = col[(i64)fl[k + 2] * ldM], a3 = col[(i64)fl[k + 3] * ldM];
    acc |= (a0 | a1) | (a2 | a3);
  }
  for (; k < k1; ++k) acc |= col[(i64)fl[k] * ldM];
  if (acc) or_if_new(next + (i64)b * W + w, acc);
}

// The level's new pods of source b = blockIdx.y in the 256 words of chunk
// blockIdx.x: visited |= new, next = 0, dist = level, the pods appended to
// the frontier list (in no particular order), the targets among them counted.
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_hops_finish(
    i64 n, i64 W, u64* __restrict__ visited, u64* __restrict__ next,
    const u64* __restrict__ tmask, int32_t* __restrict__ dist, int32_t* __restrict__ list,
    int32_t* __restrict__ cnts, const int32_t* __restrict__ ntgt, int B, int level) {
  __shared__ int32_t sm[4];
  __shared__ int32_t s_base;
  const int b = blockIdx.y;
  // nothing was expanded for this source: next holds no bit
  if (cnts[((level - 1) & 1) * B + b] <= 0) return;               // block-uniform
  const i64 w = (i64)blockIdx.x * TPB + threadIdx.x;
  u64 nw = 0;
  int32_t hits = 0;
  if (w < W) {
    const i64 at = (i64)b * W + w;
    const u64 nx = next[at];
    if (nx) {
      next[at] = 0;
      const u64 vis = visited[at];
      nw = nx & ~vis & valid_mask(w, n);
      if (nw) {
        visited[at] = vis | nw;
        if (tmask) hits = __popcll(nw & tmask[at]);
      }
    }
  }
  int32_t tot = 0;
  const int32_t pre = block_excl_scan<int32_t>(__popcll(nw), sm, tot);
  if (tot == 0) return;                                            // block-uniform
  if (tmask) {
    const int32_t h = block_sum<int32_t>(hits, sm);
    if (threadIdx.x == 0 && h) atomicAdd(&cnts[2 * B + b], h);
  }
  if (threadIdx.x == 0) s_base = atomicAdd(&cnts[(level & 1) * B + b], tot);
  __syncthreads();
  i64 pos = (i64)b * n + s_base + pre;
  int32_t* d = dist + (i64)b * n;
  while (nw) {
    const int32_t v = (int32_t)(w * 64 + (__ffsll((long long)nw) - 1));
    nw &= nw - 1;
    d[v] = level;
    list[pos++] = v;
  }
}

// out[q] = dist of source slot item.x at pod item.y
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_hops_gather(
    const int32_t* __restrict__ dist, i64 n, const int2* __restrict__ items, i64 nitems,
    int32_t* __restrict__ out) {
  const i64 q = (i64)blockIdx.x * TPB + threadIdx.x;
  if (q >= nitems) return;
  out[q] = dist[(i64)items[q].x * n + items[q].y];
}

// The canonical shortest path of one queried pair a block: t_d = t and, for
// k = d .. 2, t_{k-1} = the smallest u with dist_s[u] = k - 1 and
// M[u, t_k] = 1 -- the threads stride over the pods, test the bit of the
// level's members and min-reduce.  out[off .. off + d] = s, t_1, .., t.
struct HopsWitness {
  int32_t b, t, d, s;
  i64 off;
};
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_hops_witness(
    const u64* __restrict__ M, i64 ldM, i64 n, const int32_t* __restrict__ dist,
    const HopsWitness* __restrict__ items, int32_t* __restrict__ out) {
  __shared__ int32_t sm[TPB / 64];
  const HopsWitness it = items[blockIdx.x];
  const int32_t* ds = dist + (i64)it.b * n;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    out[it.off] = it.s;
    out[it.off + it.d] = it.t;
  }
  int32_t cur = it.t;
  for (int32_t k = it.d; k >= 2; --k) {
    const i64 cw = cur >> 6;
    const int cb = cur & 63;
    int32_t best = INT32_MAX;
    for (i64 u = threadIdx.x; u < n; u += TPB) {
      if (ds[u] == k - 1 && ((M[u * ldM + cw] >> cb) & 1ull)) {
        best = (int32_t)u;      // ascending within a thread: its first is its smallest
        break;
      }
    }
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) best = min(best, __shfl_xor(best, dlt, 64));
    if (lane == 0) sm[wid] = best;
    __syncthreads();
    best = min(min(sm[0], sm[1]), min(sm[2], sm[3]));
    __syncthreads();
    if (best >= n) {            // no predecessor (cannot happen after a finished search)
      if (threadIdx.x == 0)
        for (int32_t j = 1; j < k; ++j) out[it.off + j] = -1;
      return;                   // block-uniform
    }
    cur = best;
    if (threadIdx.x == 0) out[it.off + k - 1] = cur;
  }
}

}  // namespace kano
