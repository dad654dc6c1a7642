// kano_zones.hpp -- the matrix read by columns: the bit transpose of the
// n x n pod matrix into another context (kano_reverse) and the per-row pass
// over a matrix and a second one, typically its reverse (kano_zones;
// kano_ext.hip).  Read from the matrices themselves, so it holds for built,
// updated, edited, loaded, path and edge matrices alike.
//
// k_reverse_tile: a block takes 64 A source rows by B source words.  Lane r
// of a wave loads the B words of row 64 a + r as one contiguous segment
// (8 B bytes, 16-byte loads; the loads of all the wave's row groups go out
// before the first is used), zn_transpose64 turns the 64 x 64 bit block of
// every word across the wave, and lane c stores word (b, a) -- the bits of
// source column 64 b + c in rows 64 a .. 64 a + 63 -- into the LDS tile
// T[64 b + c][a].  After the barrier the A words of every tile row are one
// contiguous segment of a destination row: A / 2 neighbouring lanes store it
// as 16-byte pieces, so one store instruction covers whole 8 A byte
// segments.  The tile's pitch is A + 1 words: odd, so the 16 lanes of
// a ds_write_b64 group (stride one tile row) fall on 16 distinct bank pairs
// of the 32; the read side (rows r, r + 1, .. by 16-byte pieces) is 2-way on
// a quarter of its lanes, far below the memory time of the tile.  Plain loads
// and stores: a row's segment is moved by several instructions of a wave, and
// non-temporal accesses lost the lines between them (2.6 x the time on C3).
//
// k_zone_rows: a wave a row streams A[i] and B[i] 64 words a step (512
// contiguous bytes each).  label[i] = min(i, first common bit), the popcounts
// are wave sums; without the counts the row stops at its first hit, or after
// word i >> 6 (a later common bit cannot lower the label).
#pragma once
#include "kano_prims.hpp"

namespace kano {

// 64 x 64 bit transpose across a wave: lane r holds row r, returns column r
// (kano_kernels.hpp wave_transpose64, the same butterfly: that header's
// kernels belong to kano_hip.hip's translation unit)
__device__ __forceinline__ u64 zn_transpose64(u64 x, int lane) {
  constexpr u64 MS[6] = {0x00000000ffffffffull, 0x0000ffff0000ffffull, 0x00ff00ff00ff00ffull,
                         0x0f0f0f0f0f0f0f0full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int sft = 32 >> k;
    const u64 m = MS[k];
    const u64 y = __shfl_xor(x, sft, 64);
    x = (lane & sft) ? ((x & ~m) | ((y & ~m) >> sft)) : ((x & m) | ((y & m) << sft));
  }
  return x;
}

// D[j][i] = S[i][j] over the tile blockIdx.x = ty * gx + tx: source rows
// 64 A ty .., source words B tx ...  Rows >= n and words >= W read as zero;
// destination rows >= n and words >= W are not written, so the source's tail
// bits go nowhere and the destination's are zeros.  ldS and ldD are even
// (16-byte pieces on both sides).  bits += the set bits stored.
// lane's B words of source row `row` from word c0 on (zeros past n and W)
template <int B>
__device__ __forceinline__ void reverse_load(const u64* __restrict__ S, i64 ldS, i64 row, i64 c0,
                                             i64 n, i64 W, u64 (&x)[B]) {
#pragma unroll
  for (int b = 0; b < B; ++b) x[b] = 0ull;
  if (row >= n) return;
  const u64* p = S + row * ldS + c0;
#pragma unroll
  for (int b = 0; b < B; b += 2) {
    if (c0 + b < W) {                    // (c0 + b even, ldS even: the pair lies in the row)
      const u64x2 v = *reinterpret_cast<const u64x2*>(p + b);
      x[b] = v.x;
      x[b + 1] = c0 + b + 1 < W ? v.y : 0ull;
    }
  }
}

// AHEAD: every load of the wave's row groups is issued before the first
// transpose waits for one; else a row group at a time.
template <int A, int B, bool AHEAD>
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_reverse_tile(
    const u64* __restrict__ S, i64 ldS, u64* __restrict__ D, i64 ldD, i64 n, i64 W, i64 gx,
    unsigned long long* __restrict__ bits) {
  static_assert(A % 2 == 0 && B % 2 == 0 && A % (TPB / 64) == 0, "tile shape");
  constexpr int P = A + 1;               // tile pitch in words
  constexpr int HP = A / 2;              // 16-byte pieces of a tile row
  constexpr int NW = TPB / 64, AW = A / NW;
  __shared__ u64 T[64 * B * P];
  __shared__ i64 sm[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const i64 ty = (i64)blockIdx.x / gx, tx = (i64)blockIdx.x - ty * gx;
  const i64 r0 = ty * 64 * A, c0 = tx * B;
  if constexpr (AHEAD) {
    u64 x[AW][B];
#pragma unroll
    for (int k = 0; k < AW; ++k)
      reverse_load<B>(S, ldS, r0 + 64 * (wv + k * NW) + lane, c0, n, W, x[k]);
#pragma unroll
    for (int k = 0; k < AW; ++k) {
#pragma unroll
      for (int b = 0; b < B; ++b)
        T[(b * 64 + lane) * P + wv + k * NW] = zn_transpose64(x[k][b], lane);
    }
  } else {
#pragma unroll 1
    for (int a = wv; a < A; a += NW) {
      u64 x[B];
      reverse_load<B>(S, ldS, r0 + 64 * a + lane, c0, n, W, x);
#pragma unroll
      for (int b = 0; b < B; ++b) T[(b * 64 + lane) * P + a] = zn_transpose64(x[b], lane);
    }
  }
  __syncthreads();
  const i64 d0 = c0 * 64, wd0 = ty * A;
  i64 cnt = 0;
#pragma unroll 4
  for (int i = threadIdx.x; i < 64 * B * HP; i += TPB) {
    const int r = i / HP, h = i - r * HP;
    const i64 drow = d0 + r, wd = wd0 + 2 * h;
    if (drow < n && wd < W) {
      const u64 lo = T[r * P + 2 * h], hi = T[r * P + 2 * h + 1];
      u64* q = D + drow * ldD + wd;
      if (wd + 1 < W) {
        u64x2 v;
        v.x = lo;
        v.y = hi;
        *reinterpret_cast<u64x2*>(q) = v;
        cnt += __popcll(lo) + __popcll(hi);
      } else {
        *q = lo;
        cnt += __popcll(lo);
      }
    }
  }
  cnt = block_sum<i64>(cnt, sm);
  if (threadIdx.x == 0 && cnt) atomicAdd(bits, (unsigned long long)cnt);
}

// Row i = blockIdx.x * 4 + wave of two whole matrices of the same n:
//   label[i]   = min({i} u {j : A[i,j] = 1 and B[i,j] = 1})
//   fan_out[i] = popcount(A[i]), fan_in[i] = popcount(B[i]), cyclic[i] = A[i,i]
// over the bits below n.  counts == 0: the label alone (fan_out, fan_in and
// cyclic are not touched).
static __global__ __attribute__((unused)) __launch_bounds__(TPB) void k_zone_rows(
    const u64* __restrict__ A, i64 ldA, const u64* __restrict__ Bm, i64 ldB, i64 n, i64 W,
    int counts, int32_t* __restrict__ label, int32_t* __restrict__ fan_out,
    int32_t* __restrict__ fan_in, uint8_t* __restrict__ cyclic) {
  const int lane = threadIdx.x & 63;
  const i64 i = (i64)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (i >= n) return;                                   // wave-uniform
  const u64* a = A + i * ldA;
  const u64* b = Bm + i * ldB;
  const i64 wend = counts ? W : min(W, (i >> 6) + 1);
  i64 lab = i;
  bool found = false;
  int32_t ca = 0, cb = 0;
  for (i64 w0 = 0; w0 < wend; w0 += 64) {
    const i64 w = w0 + lane;
    u64 av = 0ull, bv = 0ull;
    if (w < wend) {
      const u64 vm = valid_mask(w, n);
      av = a[w] & vm;
      bv = b[w] & vm;
    }
    ca += __popcll(av);
    cb += __popcll(bv);
    if (!found) {
      const u64 x = av & bv;
      const u64 hit = __ballot(x != 0ull);
      if (hit) {                                        // wave-uniform
        const int first = __ffsll((long long)hit) - 1;
        const u64 xf = __shfl(x, first, 64);
        lab = min(lab, (w0 + first) * 64 + (__ffsll((long long)xf) - 1));
        found = true;
      }
    }
    if (found && !counts) break;                        // wave-uniform
  }
  if (counts) {
    ca = wave_sum(ca);
    cb = wave_sum(cb);
  }
  if (lane == 0) {
    label[i] = (int32_t)lab;
    if (counts) {
      if (fan_out) fan_out[i] = ca;
      if (fan_in) fan_in[i] = cb;
      if (cyclic) cyclic[i] = (uint8_t)((a[i >> 6] >> (i & 63)) & 1ull);
    }
  }
}

}  // namespace kano
