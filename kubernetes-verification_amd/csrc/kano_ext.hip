// kano_ext.hip -- the extensions of SURVEY.md §8(f) on an engine context
// (include/kano_hip.h): multi-hop reachability (kubesv/kubesv/constraint.py:
// 233-237), the matrix row format (kano_py/kano/model.py:136-139 bitarray
// bytes), incremental policy updates (model.py:125-165 over an updated policy
// list) and kubesv's edge relation (kubesv/kubesv/constraint.py:191-231).
// Shares the context and its helpers with kano_hip.hip (kano_engine.hpp).
#include "kano_engine.hpp"
#include "kano_inc.hpp"
#include "kano_k8s.hpp"
#include "kano_k8s_conn.hpp"
#include "kano_k8s_pairs.hpp"
#include "kano_k8s_tiers.hpp"
#include "kano_k8s_usage.hpp"
#include "kano_path.hpp"
#include "kano_hops.hpp"
#include "kano_intents.hpp"
#include "kano_ports.hpp"
#include "kano_verdict.hpp"
#include "kano_zones.hpp"

using namespace kano_eng;

// ===========================================================================
// Multi-hop reachability (kubesv/kubesv/
// constraint.py:233-237).  See kano_path.hpp for the class-level recurrence.
// ===========================================================================
namespace {

struct PathGeom {
  bool identity = false;   // an edited M: every pod is its own row / column class
  i64 rows = 0;            // row classes (or n)
  i64 Ua = 0;              // column classes (or n)
  i64 KW = 0;              // words of a class-level row holding bits (ceil(Ua / 64))
  i64 ldR = 0;             // pitch of the class-level rows
  const u64* base = nullptr;   // R_1 = Mc (or M)
  const u64* T = nullptr;      // one hop out of a column class (pitch ldR)
};

template <int CW>
int path_or_launch(kano_ctx* ctx, const u64* D, u64* R, u64* Dn, const PathGeom& g) {
  const i64 nch = (g.ldR + 64 * CW - 1) / (64 * CW);
  hipLaunchKernelGGL(k_path_or<CW>, dim3(nblk(g.rows * nch, TPB / 64)), dim3(TPB), 0, ctx->stream,
                     D, R, Dn, g.ldR, g.T, g.ldR, g.rows, g.KW, nch, P_<u64>(ctx->pcnt));
  KLAUNCH();
  return 0;
}

template <int TM, int TN>
int path_mfma_launch(kano_ctx* ctx, const PathMfmaArgs& a, i64 tiles) {
  hipLaunchKernelGGL((k_path_mfma<TM, TN>), dim3(nblk(tiles, TPB / 64)), dim3(TPB), 0, ctx->stream,
                     a);
  KLAUNCH();
  return 0;
}

// this context's rows' part of T (all of T for a full build): T[b] = OR of
// Mc[rc(j)] over the members j of column class b in [r0, r1)
int path_t_local(kano_ctx* src, kano_ctx* ctx, u64* Tout) {
  const i64 n = src->n, Ua = src->cc.U, ldR = src->ldC, KW = (Ua + 63) / 64;
  const u64* base = P_<u64>(src->Mc);
  const i64 nch = (ldR + 255) / 256;
  if (KW <= 4 && Ua <= 65536) {
    // narrow class rows: slices of the column classes' member lists
    KTRY(dalloc(ctx, ctx->pB, sizeof(int32_t) * (Ua + 1)));
    KCHK(hipMemsetAsync(Tout, 0, sizeof(u64) * Ua * ldR, ctx->stream));
    hipLaunchKernelGGL(k_path_t_items, dim3(1), dim3(TPB), 0, ctx->stream,
                       P_<int32_t>(src->cc.moff), Ua, P_<int32_t>(ctx->pB));
    KLAUNCH();
    const i64 nitems = (n + 64 * NT_SLICE - 1) / (64 * NT_SLICE) + Ua;   // upper bound
    hipLaunchKernelGGL(k_path_t_narrow, dim3(nblk(nitems, TPB / 64)), dim3(TPB), 0, ctx->stream,
                       base, ldR, P_<int32_t>(src->rc.cls), P_<int32_t>(src->cc.moff),
                       P_<int32_t>(src->cc.mem), Ua, KW, P_<int32_t>(ctx->pB), nitems, src->r0,
                       src->r1, Tout);
  } else {
    hipLaunchKernelGGL(k_path_t<4>, dim3(nblk(Ua * nch, TPB / 64)), dim3(TPB), 0, ctx->stream,
                       base, ldR, P_<int32_t>(src->rc.cls), P_<int32_t>(src->cc.moff),
                       P_<int32_t>(src->cc.mem), Ua, KW, nch, src->r0, src->r1, Tout);
  }
  KLAUNCH();
  return 0;
}

// ctx's pod rows from class-level rows over src's classes (kano_path's last
// step, kano_policy_subset's write): M[i] bit j = R[rc(i)][cc(j)] for every
// row i that ctx and src hold.  R (rows x ldR words, Ua column classes) is
// bit-transposed into 16-row groups (rt16: ceil(rows / 16) * Ua uint16, the
// caller's), then one block per (group, word range) expands a chunk of the
// class rows and streams it to the member rows (k_path_expand16).  Every word
// of every held row is written, the bits at positions >= n as zeros.
int path_expand_rows(kano_ctx* ctx, kano_ctx* src, const u64* R, i64 ldR, i64 rows, i64 Ua,
                     void* rt16v) {
  const i64 n = src->n, ldM = ctx->ldM;
  const i64 ng = (rows + 15) / 16, RW = (rows + 63) / 64, CWn = (Ua + 63) / 64;
  const i64 CG = (CWn + 15) / 16;
  hipLaunchKernelGGL(k_bit_transpose<true>, dim3(nblk(RW * CG, TPB / 64)), dim3(TPB), 0,
                     ctx->stream, R, ldR, rows, RW, CG, Ua, rt16v, Ua, ng);
  KLAUNCH();
  constexpr int SUB = 2;
  // member slices when the (group, word range) blocks alone cannot fill
  // the chip and the classes are large (broad selectors)
  const i64 gxy = (i64)nblk(ldM, (i64)TPB * SUB) * ng;
  const i64 avg_members = (n + rows - 1) / rows;
  const i64 Z = std::max<i64>(1, std::min<i64>({(2048 + gxy - 1) / gxy, avg_members / 8, 64}));
  const dim3 grid(nblk(ldM, (i64)TPB * SUB), (unsigned)ng, (unsigned)Z);
  const size_t lds = sizeof(uint16_t) * (size_t)Ua;
  const uint16_t* rt16 = reinterpret_cast<const uint16_t*>(rt16v);
  const bool use_lds = lds <= 64 * 1024 && ctx->path_lds;
  const bool staged = avg_members >= 16;
  auto launch = [&](auto kern, size_t shm) {   // (by handle: see launch_marked)
    hipExtLaunchKernelGGL(kern, grid, dim3(TPB), (std::uint32_t)shm, ctx->stream, nullptr,
                          nullptr, 0, rt16, Ua, rows,
                       P_<int32_t>(src->cc.cls), n, P_<int32_t>(src->rc.moff),
                       P_<int32_t>(src->rc.mem), P_<u64>(ctx->M), ldM, src->r0);
  };
  if (use_lds && staged) launch(k_path_expand16<SUB, true, true>, lds);
  else if (use_lds) launch(k_path_expand16<SUB, true, false>, lds);
  else if (staged) launch(k_path_expand16<SUB, false, true>, 0);
  else launch(k_path_expand16<SUB, false, false>, 0);
  KLAUNCH();
  return 0;
}

int path_impl(kano_ctx* src, kano_ctx* ctx, int hops, int mode, int64_t* info, bool t_ready) {
  const i64 n = src->n, W = src->W, ldM = src->ldM;
  PathGeom g;
  g.identity = src->rows_dirty;
  if (g.identity) {
    g.rows = n;
    g.Ua = n;
    g.KW = W;
    g.ldR = ldM;
    g.base = P_<u64>(src->M);
    g.T = P_<u64>(src->M);   // T[b] = M[b]: column class b is pod b
  } else {
    g.rows = src->rc.U;
    g.Ua = src->cc.U;
    g.KW = (g.Ua + 63) / 64;
    g.ldR = src->ldC;
    g.base = P_<u64>(src->Mc);
  }
  const i64 Rw = g.rows * g.ldR;   // words of one class-level matrix
  i64 steps = 0, used = 0, mfma_steps = 0;
  if (n > 0 && W > 0 && hops != 1 && g.rows > 0 && g.Ua > 0) {
    if (!g.identity) {
      if (!t_ready) KTRY(path_t_local(src, ctx, P_<u64>(ctx->pT)));
      g.T = P_<u64>(ctx->pT);
    }
    // R[0] (the identity case writes the destination matrix in place), R[1]
    // for the MFMA's out-of-place steps, two delta buffers
    u64* Rb[2];
    if (g.identity) {
      Rb[0] = P_<u64>(ctx->M);
    } else {
      KTRY(dalloc(ctx, ctx->pR[0], sizeof(u64) * Rw));
      Rb[0] = P_<u64>(ctx->pR[0]);
    }
    KTRY(dalloc(ctx, ctx->pD[0], sizeof(u64) * Rw));
    KTRY(dalloc(ctx, ctx->pD[1], sizeof(u64) * Rw));
    KTRY(dalloc(ctx, ctx->pcnt, sizeof(u64) * PATH_CNT_SLOTS * PATH_CNT_STRIDE));
    // (the MFMA step writes the words its tiles cover: the rest stay zero)
    KCHK(hipMemsetAsync(ctx->pD[0].p, 0, sizeof(u64) * Rw, ctx->stream));
    KCHK(hipMemsetAsync(ctx->pD[1].p, 0, sizeof(u64) * Rw, ctx->stream));
    Rb[1] = nullptr;
    u64* Db[2] = {P_<u64>(ctx->pD[0]), P_<u64>(ctx->pD[1])};
    KCHK(hipMemcpyAsync(Rb[0], g.base, sizeof(u64) * Rw, hipMemcpyDeviceToDevice, ctx->stream));
    // the delta of step 1 is R_1 itself; its size decides the first step
    const u64* D = g.base;
    KCHK(hipMemsetAsync(ctx->pcnt.p, 0, sizeof(u64) * PATH_CNT_SLOTS * PATH_CNT_STRIDE, ctx->stream));
    hipLaunchKernelGGL(k_popcount_words, dim3(std::min<i64>(2048, nblk(Rw))), dim3(TPB), 0,
                       ctx->stream, g.base, Rw, P_<u64>(ctx->pcnt));
    KLAUNCH();
    std::vector<u64> slots(PATH_CNT_SLOTS * PATH_CNT_STRIDE);
    auto read_count = [&](u64& out) -> int {
      KCHK(hipMemcpyAsync(slots.data(), ctx->pcnt.p, sizeof(u64) * slots.size(),
                          hipMemcpyDeviceToHost, ctx->stream));
      KTRY(sync(ctx));
      out = 0;
      for (int k = 0; k < PATH_CNT_SLOTS; ++k) out += slots[(size_t)k * PATH_CNT_STRIDE];
      return 0;
    };
    u64 dbits = 0;
    KTRY(read_count(dbits));
    int ri = 0, di = 0;
    const i64 TMr = 32 * ctx->path_tm;
    const i64 Rpad = (g.rows + 255) / 256 * 256, Upad = (g.Ua + 255) / 256 * 256;
    bool have_b = false;
    const double cells = (double)g.rows * (double)g.Ua;
    for (i64 k = 2; (hops == 0 || k <= hops) && dbits > 0; ++k) {
      bool mf = mode == KANO_PATH_MFMA;
      if (mode == KANO_PATH_AUTO) mf = (double)dbits * 100.0 > ctx->path_dens * cells;
      KCHK(hipMemsetAsync(ctx->pcnt.p, 0, sizeof(u64) * PATH_CNT_SLOTS * PATH_CNT_STRIDE, ctx->stream));
      if (!mf) {
        if (g.ldR <= 128) KTRY(path_or_launch<2>(ctx, D, Rb[ri], Db[di], g));
        else KTRY(path_or_launch<4>(ctx, D, Rb[ri], Db[di], g));
      } else {
        if (!have_b) {   // T bit-transposed: B[kw][c] bit t = T[64 kw + t][c]
          KTRY(dalloc(ctx, ctx->pB, sizeof(u64) * g.KW * Upad));
          // (T rows b = column classes; out row kw = 64 of them, Upad columns)
          const i64 CG = (Upad / 64 + 15) / 16;
          hipLaunchKernelGGL(k_bit_transpose<false>, dim3(nblk(g.KW * CG, TPB / 64)), dim3(TPB),
                             0, ctx->stream, g.T, g.ldR, g.Ua, g.KW, CG, Upad,
                             (void*)P_<u64>(ctx->pB), Upad, (i64)0);
          KLAUNCH();
          have_b = true;
        }
        KTRY(dalloc(ctx, ctx->pA, sizeof(u64) * g.KW * Rpad));
        hipLaunchKernelGGL(k_word_transpose, dim3(nblk(g.KW, 64), (unsigned)(Rpad / 64)),
                           dim3(TPB), 0, ctx->stream, Rb[ri], g.ldR, g.rows, g.KW,
                           P_<u64>(ctx->pA), Rpad, g.KW);
        KLAUNCH();
        if (!Rb[1]) {
          KTRY(dalloc(ctx, ctx->pR[1], sizeof(u64) * Rw));
          Rb[1] = P_<u64>(ctx->pR[1]);
          KCHK(hipMemsetAsync(Rb[1], 0, sizeof(u64) * Rw, ctx->stream));
        }
        PathMfmaArgs a{};
        a.A = P_<u64>(ctx->pA);
        a.B = P_<u64>(ctx->pB);
        a.ldA = Rpad;
        a.ldB = Upad;
        a.KW = g.KW;
        a.base = g.base;
        a.old = Rb[ri];
        a.out = Rb[ri ^ 1];
        a.delta = Db[di];
        a.ldR = g.ldR;
        a.rows = g.rows;
        const int TNc = ctx->path_tn == 4 ? 4 : 2;
        const i64 TMc = ctx->path_tn == 4 ? 64 : TMr;
        a.tiles_n = Upad / (32 * TNc);
        a.cnt = P_<u64>(ctx->pcnt);
        // (2 x 2 waves per block, XCD-grouped block order: 8 * ceil(blocks / 8))
        const i64 blocks = (Rpad / (2 * TMc)) * (a.tiles_n / 2);
        const i64 tiles = (blocks + 7) / 8 * 8 * (TPB / 64);
        if (ctx->path_tn == 4) KTRY((path_mfma_launch<2, 4>(ctx, a, tiles)));
        else if (ctx->path_tm == 1) KTRY((path_mfma_launch<1, 2>(ctx, a, tiles)));
        else if (ctx->path_tm == 4) KTRY((path_mfma_launch<4, 2>(ctx, a, tiles)));
        else KTRY((path_mfma_launch<2, 2>(ctx, a, tiles)));
        ri ^= 1;
        ++mfma_steps;
      }
      KTRY(read_count(dbits));
      D = Db[di];
      di ^= 1;
      ++used;
      if (dbits > 0) ++steps;
    }
    if (g.identity) {
      if (ri != 0)
        KCHK(hipMemcpyAsync(Rb[0], Rb[ri], sizeof(u64) * Rw, hipMemcpyDeviceToDevice,
                            ctx->stream));
    } else {
      KTRY(dalloc(ctx, ctx->pA, sizeof(uint16_t) * ((g.rows + 15) / 16) * g.Ua));
      KTRY(path_expand_rows(ctx, src, Rb[ri], g.ldR, g.rows, g.Ua, ctx->pA.p));
    }
  } else if (n > 0 && W > 0) {
    // one hop (or an empty class set): the matrix itself
    KCHK(hipMemcpyAsync(ctx->M.p, src->M.p, sizeof(u64) * rows_local(src) * ldM,
                        hipMemcpyDeviceToDevice, ctx->stream));
  }
  KTRY(sync(ctx));
  ctx->cols_valid = false;
  ctx->rows_dirty = true;
  if (info) {
    info[0] = steps;
    info[1] = used;
    info[2] = mfma_steps;
    info[3] = g.rows;
    info[4] = g.Ua;
    info[5] = g.identity ? 1 : 0;
  }
  return 0;
}

}  // namespace

extern "C" {

int kano_path(kano_ctx* src, kano_ctx* dst, int hops, int mode, int64_t* info) {
  if (!src || !dst) return -EINVAL;
  if (src == dst) return fail(dst, -EINVAL, "kano_path: the destination must be another context");
  if (hops < 0) return fail(dst, -EINVAL, "kano_path: hops < 0");
  if (mode < KANO_PATH_AUTO || mode > KANO_PATH_MFMA)
    return fail(dst, -EINVAL, "kano_path: unknown mode");
  if (src->device != dst->device) return fail(dst, -EINVAL, "kano_path: contexts on two devices");
  kano_ctx* ctx = dst;
  KCHK(hipSetDevice(dst->device));
  {
    const int rc = ensure_matrix(src);
    if (rc) return fail(dst, rc, "kano_path: source: " + src->err);
  }
  if (src->r0 != 0 || src->r1 != src->n)
    return fail(dst, -ENOTSUP, "kano_path: the source holds a row shard (needs every row)");
  KTRY(ensure_matrix(dst));
  if (dst->n != src->n || dst->r0 != 0 || dst->r1 != dst->n || dst->ldM != src->ldM)
    return fail(dst, -EINVAL, "kano_path: the destination must hold a matrix of the same size");
  {
    const int rc = sync(src);   // the source's matrix and classes are complete
    if (rc) return fail(dst, rc, "kano_path: source: " + src->err);
  }
  KTRY(dalloc(ctx, ctx->pT, sizeof(u64) * std::max<i64>(1, src->cc.U * src->ldC)));
  return path_impl(src, dst, hops, mode, info, false);
}

int kano_path_shard_words(kano_ctx* src, int64_t* words) {
  if (!src || !words) return -EINVAL;
  KTRY(ensure_matrix(src));
  *words = src->rows_dirty ? 0 : src->cc.U * src->ldC;
  return 0;
}

int kano_path_shard(kano_ctx* src, uint64_t* t_dev) {
  if (!src) return -EINVAL;
  kano_ctx* ctx = src;
  KCHK(hipSetDevice(src->device));
  KTRY(ensure_matrix(src));
  if (src->rows_dirty)
    return fail(src, -ENOTSUP, "kano_path_shard: an edited row shard (needs every row)");
  if (src->cc.U * src->ldC > 0) {
    if (!t_dev) return fail(src, -EINVAL, "kano_path_shard: t_dev is NULL");
    KTRY(path_t_local(src, src, reinterpret_cast<u64*>(t_dev)));
  }
  return sync(src);
}

int kano_path_combine(kano_ctx* src, kano_ctx* dst, const uint64_t* gathered_dev, int32_t nranks,
                      int hops, int mode, int64_t* info) {
  if (!src || !dst || src == dst) return -EINVAL;
  kano_ctx* ctx = dst;
  if (hops < 0 || nranks < 1 || mode < KANO_PATH_AUTO || mode > KANO_PATH_MFMA)
    return fail(dst, -EINVAL, "kano_path_combine: bad arguments");
  if (src->device != dst->device) return fail(dst, -EINVAL, "kano_path_combine: two devices");
  KCHK(hipSetDevice(dst->device));
  {
    const int rc = ensure_matrix(src);
    if (rc) return fail(dst, rc, "kano_path_combine: source: " + src->err);
  }
  if (src->rows_dirty) return fail(dst, -ENOTSUP, "kano_path_combine: an edited row shard");
  KTRY(ensure_matrix(dst));
  if (dst->n != src->n || dst->r0 != src->r0 || dst->r1 != src->r1 || dst->ldM != src->ldM)
    return fail(dst, -EINVAL, "kano_path_combine: the destination must hold the same rows");
  {
    const int rc = sync(src);
    if (rc) return fail(dst, rc, "kano_path_combine: source: " + src->err);
  }
  const i64 nw = src->cc.U * src->ldC;
  KTRY(dalloc(ctx, ctx->pT, sizeof(u64) * std::max<i64>(1, nw)));
  if (nw > 0) {
    if (!gathered_dev) return fail(dst, -EINVAL, "kano_path_combine: gathered_dev is NULL");
    hipLaunchKernelGGL(k_or_parts, dim3(std::min<i64>(4096, nblk(nw))), dim3(TPB), 0,
                       ctx->stream, reinterpret_cast<const u64*>(gathered_dev), nranks, nw,
                       P_<u64>(ctx->pT));
    KLAUNCH();
  }
  return path_impl(src, dst, hops, mode, info, true);
}


int kano_export_rows(kano_ctx* ctx, int64_t r0, int64_t nrows, uint8_t* dst) {
  KTRY(ensure_matrix(ctx));
  if (nrows < 0 || r0 < ctx->r0 || r0 + nrows > ctx->r1 || (!dst && nrows > 0))
    return fail(ctx, -EINVAL, "kano_export_rows: rows outside this shard");
  const i64 nb = (ctx->n + 7) / 8;
  if (nrows == 0 || nb == 0) return 0;
  // staged through scratch in chunks of <= 64 MB
  const i64 chunk = std::max<i64>(1, (64ll << 20) / nb);
  KTRY(dalloc(ctx, ctx->scratch_words, (size_t)(std::min(chunk, (i64)nrows) * nb + 16)));
  uint8_t* st = reinterpret_cast<uint8_t*>(ctx->scratch_words.p);
  for (i64 c0 = 0; c0 < nrows; c0 += chunk) {
    const i64 cr = std::min<i64>(chunk, nrows - c0);
    const i64 q = (nb + 3) / 4;
    hipLaunchKernelGGL(k_words_to_bytes, dim3(nblk(cr * q)), dim3(TPB), 0, ctx->stream,
                       P_<u64>(ctx->M) + (r0 - ctx->r0 + c0) * ctx->ldM, ctx->ldM, cr, nb, st);
    KLAUNCH();
    KCHK(hipMemcpyAsync(dst + c0 * nb, st, (size_t)(cr * nb), hipMemcpyDeviceToHost, ctx->stream));
    KTRY(sync(ctx));
  }
  return 0;
}

int kano_import_rows(kano_ctx* ctx, int64_t r0, int64_t nrows, const uint8_t* src) {
  KTRY(ensure_matrix(ctx));
  if (nrows < 0 || r0 < ctx->r0 || r0 + nrows > ctx->r1 || (!src && nrows > 0))
    return fail(ctx, -EINVAL, "kano_import_rows: rows outside this shard");
  const i64 nb = (ctx->n + 7) / 8;
  if (nrows == 0 || nb == 0) return 0;
  const i64 chunk = std::max<i64>(1, (64ll << 20) / nb);
  KTRY(dalloc(ctx, ctx->scratch_words, (size_t)(std::min(chunk, (i64)nrows) * nb + 16)));
  uint8_t* st = reinterpret_cast<uint8_t*>(ctx->scratch_words.p);
  for (i64 c0 = 0; c0 < nrows; c0 += chunk) {
    const i64 cr = std::min<i64>(chunk, nrows - c0);
    KCHK(hipMemcpyAsync(st, src + c0 * nb, (size_t)(cr * nb), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_bytes_to_words, dim3(nblk(cr * ctx->ldM)), dim3(TPB), 0, ctx->stream, st,
                       cr, nb, ctx->n, P_<u64>(ctx->M) + (r0 - ctx->r0 + c0) * ctx->ldM,
                       ctx->ldM);
    KLAUNCH();
    KTRY(sync(ctx));
  }
  ctx->cols_valid = false;
  ctx->rows_dirty = true;
  ctx->user_edited = true;
  return 0;
}


// ---------------------------------------------------------------------------
// Incremental policy updates (kano_inc.hpp)

int kano_add_policies(kano_ctx* ctx, int64_t Pn, int32_t ncols_x, const int32_t* xval,
                      const int64_t* sel_off, const int32_t* sel_col, const int32_t* sel_val,
                      const int64_t* alw_off, const int32_t* alw_col, const int32_t* alw_val,
                      int64_t* first_id) {
  KTRY(ensure_matrix(ctx));
  if (Pn < 0 || ncols_x < 0 || (Pn > 0 && (!sel_off || !alw_off)) ||
      (ncols_x > 0 && !xval && ctx->n > 0))
    return fail(ctx, -EINVAL, "kano_add_policies: bad arguments");
  const i64 n = ctx->n, W = ctx->W;
  if (first_id) *first_id = ctx->P + ctx->inc_A;
  if (Pn == 0) return 0;
  const i64 ns = sel_off[Pn], na = alw_off[Pn];
  const int32_t ncol_all = ctx->ncols + (int32_t)(ctx->inc_xcols + ncols_x);
  for (i64 t = 0; t < ns; ++t)
    if (sel_col[t] < 0 || sel_col[t] >= ncol_all)
      return fail(ctx, -EINVAL, "kano_add_policies: select term column out of range");
  for (i64 t = 0; t < na; ++t)
    if (alw_col[t] < 0 || alw_col[t] >= ncol_all)
      return fail(ctx, -EINVAL, "kano_add_policies: allow term column out of range");
  // the extra columns append to the ones earlier additions brought
  if (ncols_x > 0 && n > 0) {
    const i64 have = ctx->inc_xcols * n, add = (i64)ncols_x * n;
    DBuf grown;
    KTRY(dalloc(ctx, grown, sizeof(int32_t) * (have + add)));
    if (have > 0)
      KCHK(hipMemcpyAsync(grown.p, ctx->xv.p, sizeof(int32_t) * have, hipMemcpyDeviceToDevice,
                          ctx->stream));
    KCHK(hipMemcpyAsync(P_<int32_t>(grown) + have, xval, sizeof(int32_t) * add,
                        hipMemcpyHostToDevice, ctx->stream));
    KTRY(sync(ctx));
    ctx->xv = std::move(grown);
  }
  ctx->inc_xcols += ncols_x;
  if (ncols_x > 0) ctx->cls_valid = false;   // new pod columns: the next build classifies again
  // pod-level sets of the added policies (A x W words each side)
  const i64 A0 = ctx->inc_A, A1 = A0 + Pn;
  if (A1 > ctx->inc_acap) {
    const i64 cap = std::max<i64>(A1, 2 * ctx->inc_acap);
    DBuf s2, a2;
    KTRY(dalloc(ctx, s2, sizeof(u64) * std::max<i64>(1, cap * W)));
    KTRY(dalloc(ctx, a2, sizeof(u64) * std::max<i64>(1, cap * W)));
    if (A0 > 0 && W > 0) {
      KCHK(hipMemcpyAsync(s2.p, ctx->asel.p, sizeof(u64) * A0 * W, hipMemcpyDeviceToDevice,
                          ctx->stream));
      KCHK(hipMemcpyAsync(a2.p, ctx->aalw.p, sizeof(u64) * A0 * W, hipMemcpyDeviceToDevice,
                          ctx->stream));
    }
    KTRY(sync(ctx));
    ctx->asel = std::move(s2);
    ctx->aalw = std::move(a2);
    ctx->inc_acap = cap;
  }
  // the batch's terms: [soff | aoff] (i64) then [scol | sval | acol | aval] (i32)
  const size_t hdr = sizeof(i64) * 2 * (Pn + 1);
  const size_t body = sizeof(int32_t) * 2 * (ns + na);
  std::vector<uint8_t> h(hdr + body + 16);
  std::memcpy(h.data(), sel_off, sizeof(i64) * (Pn + 1));
  std::memcpy(h.data() + sizeof(i64) * (Pn + 1), alw_off, sizeof(i64) * (Pn + 1));
  int32_t* hb = reinterpret_cast<int32_t*>(h.data() + hdr);
  if (ns) std::memcpy(hb, sel_col, sizeof(int32_t) * ns);
  if (ns) std::memcpy(hb + ns, sel_val, sizeof(int32_t) * ns);
  if (na) std::memcpy(hb + 2 * ns, alw_col, sizeof(int32_t) * na);
  if (na) std::memcpy(hb + 2 * ns + na, alw_val, sizeof(int32_t) * na);
  KTRY(dalloc(ctx, ctx->iterm, h.size()));
  KCHK(hipMemcpyAsync(ctx->iterm.p, h.data(), h.size(), hipMemcpyHostToDevice, ctx->stream));
  const i64* d_soff = P_<i64>(ctx->iterm);
  const i64* d_aoff = d_soff + (Pn + 1);
  const int32_t* d_b = reinterpret_cast<const int32_t*>(P_<uint8_t>(ctx->iterm) + hdr);
  u64* sel = P_<u64>(ctx->asel) + A0 * W;
  u64* alw = P_<u64>(ctx->aalw) + A0 * W;
  if (n > 0) {
    hipLaunchKernelGGL(k_inc_eval, dim3(nblk(n), (unsigned)Pn, 2), dim3(TPB), 0, ctx->stream,
                       P_<int32_t>(ctx->pv), n, ctx->ncols, P_<int32_t>(ctx->xv), d_soff, d_b,
                       d_b + ns, d_aoff, d_b + 2 * ns, d_b + 2 * ns + na, W, sel, alw);
    KLAUNCH();
    const i64 rl = rows_local(ctx);
    if (rl > 0)
      hipLaunchKernelGGL(k_inc_or, dim3(nblk(rl)), dim3(TPB), 0, ctx->stream,
                         P_<u64>(ctx->asel), P_<u64>(ctx->aalw), W, A0, Pn, ctx->r0, rl,
                         P_<u64>(ctx->M), ctx->ldM);
    KLAUNCH();
  }
  KTRY(sync(ctx));
  ctx->inc_A = A1;
  ctx->dead.resize((size_t)(ctx->P + A1), 0);
  ctx->cols_valid = false;
  ctx->rows_dirty = true;
  return 0;
}

int kano_remove_policies(kano_ctx* ctx, int64_t count, const int64_t* ids) {
  KTRY(ensure_matrix(ctx));
  if (count < 0 || (count > 0 && !ids)) return fail(ctx, -EINVAL, "kano_remove_policies");
  if (ctx->user_edited)
    return fail(ctx, -EINVAL, "kano_remove_policies: the matrix was edited; rebuild instead");
  const i64 Ptot = ctx->P + ctx->inc_A;
  std::vector<uint8_t> newdead((size_t)std::max<i64>(1, Ptot), 0);
  i64 fresh = 0;
  for (i64 k = 0; k < count; ++k) {
    if (ids[k] < 0 || ids[k] >= Ptot) return fail(ctx, -EINVAL, "kano_remove_policies: bad id");
    if (ctx->dead[ids[k]]) return fail(ctx, -EINVAL, "kano_remove_policies: id already removed");
    if (!newdead[ids[k]]) ++fresh;
    newdead[ids[k]] = 1;
  }
  if (fresh == 0) return 0;
  for (i64 p = 0; p < Ptot; ++p) ctx->dead[p] |= newdead[p];
  const i64 n = ctx->n, W = ctx->W, rl = rows_local(ctx);
  // [newdead | dead] flags, the row list, its count
  KTRY(dalloc(ctx, ctx->idead, 2 * (size_t)std::max<i64>(1, Ptot) + 16));
  KCHK(hipMemcpyAsync(ctx->idead.p, newdead.data(), (size_t)Ptot, hipMemcpyHostToDevice,
                      ctx->stream));
  KCHK(hipMemcpyAsync(P_<uint8_t>(ctx->idead) + Ptot, ctx->dead.data(), (size_t)Ptot,
                      hipMemcpyHostToDevice, ctx->stream));
  KTRY(dalloc(ctx, ctx->irows, sizeof(int32_t) * std::max<i64>(1, rl) + 64));
  u64* cnt = reinterpret_cast<u64*>(P_<int32_t>(ctx->irows) + std::max<i64>(1, rl) + 8);
  cnt = reinterpret_cast<u64*>((reinterpret_cast<uintptr_t>(cnt) + 7) & ~(uintptr_t)7);
  KCHK(hipMemsetAsync(cnt, 0, sizeof(u64), ctx->stream));
  const bool classes = ctx->rc.U > 0 && rl > 0;
  if (rl > 0) {
    hipLaunchKernelGGL(k_inc_mark, dim3(nblk(rl)), dim3(TPB), 0, ctx->stream,
                       classes ? P_<int32_t>(ctx->rc.cls) : (const int32_t*)nullptr,
                       P_<i64>(ctx->soffc), P_<int32_t>(ctx->slist), P_<uint8_t>(ctx->idead),
                       ctx->P, P_<u64>(ctx->asel), W, ctx->inc_A, ctx->r0, rl,
                       P_<int32_t>(ctx->irows), cnt);
    KLAUNCH();
  }
  u64 nrows = 0;
  KCHK(hipMemcpyAsync(&nrows, cnt, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  KTRY(sync(ctx));
  if (nrows > 0) {
    const size_t lds = sizeof(u64) * (size_t)std::max<i64>(1, ctx->ldC);
    if (lds > 64 * 1024) return fail(ctx, -ENOTSUP, "kano_remove_policies: too many column classes");
    hipLaunchKernelGGL(k_inc_rewrite, dim3((unsigned)nrows), dim3(TPB), lds, ctx->stream,
                       P_<int32_t>(ctx->irows),
                       classes ? P_<int32_t>(ctx->rc.cls) : (const int32_t*)nullptr,
                       P_<i64>(ctx->soffc), P_<int32_t>(ctx->slist),
                       P_<uint8_t>(ctx->idead) + Ptot, ctx->P, P_<u64>(ctx->AC), ctx->ldC,
                       P_<int32_t>(ctx->cc.cls), n, P_<u64>(ctx->asel), P_<u64>(ctx->aalw), W,
                       ctx->inc_A, ctx->r0, P_<u64>(ctx->M), ctx->ldM);
    KLAUNCH();
  }
  KTRY(sync(ctx));
  ctx->cols_valid = false;
  ctx->rows_dirty = true;
  return 0;
}

int kano_added_policy_sets(kano_ctx* ctx, int64_t id, uint64_t* sel, uint64_t* allow) {
  KTRY(ensure_matrix(ctx));
  const i64 q = id - ctx->P;
  if (q < 0 || q >= ctx->inc_A) return fail(ctx, -EINVAL, "kano_added_policy_sets: bad id");
  const i64 W = ctx->W;
  if (W == 0) return 0;
  if (sel)
    KCHK(hipMemcpyAsync(sel, P_<u64>(ctx->asel) + q * W, sizeof(u64) * W, hipMemcpyDeviceToHost,
                        ctx->stream));
  if (allow)
    KCHK(hipMemcpyAsync(allow, P_<u64>(ctx->aalw) + q * W, sizeof(u64) * W,
                        hipMemcpyDeviceToHost, ctx->stream));
  return sync(ctx);
}

// kubesv's edge relation (kubesv/kubesv/constraint.py:191-231) from the two
// per-direction kano matrices: see kano_k8s.hpp.
int kano_k8s_edge(kano_ctx* in_t, kano_ctx* eg_t, kano_ctx* dst, int flags, int64_t* info) {
  if (!in_t || !eg_t || !dst) return -EINVAL;
  if (dst == in_t || dst == eg_t)
    return fail(dst, -EINVAL, "kano_k8s_edge: the destination must be another context");
  if (in_t->device != dst->device || eg_t->device != dst->device)
    return fail(dst, -EINVAL, "kano_k8s_edge: contexts on two devices");
  kano_ctx* ctx = dst;
  KCHK(hipSetDevice(dst->device));
  for (kano_ctx* s : {in_t, eg_t}) {
    const int rc = ensure_built(s);
    if (rc) return fail(dst, rc, "kano_k8s_edge: source: " + s->err);
    if (s->lists_mode) return fail(dst, -EINVAL, "kano_k8s_edge: a source holds policy lists");
    if (s->r0 != 0 || s->r1 != s->n)
      return fail(dst, -ENOTSUP, "kano_k8s_edge: a source holds a row shard (needs every row)");
  }
  KTRY(ensure_matrix(dst));
  const i64 n = dst->n, W = dst->W, ldM = dst->ldM, r0 = dst->r0, rl = rows_local(dst);
  if (in_t->n != n || eg_t->n != n || in_t->ldM != ldM || eg_t->ldM != ldM)
    return fail(dst, -EINVAL, "kano_k8s_edge: the three matrices must have the same size");
  const bool classes = !in_t->rows_dirty && !eg_t->rows_dirty && in_t->rc.U > 0 &&
                       eg_t->rc.U > 0 && in_t->cc.U > 0 && eg_t->cc.U > 0 &&
                       !(flags & KANO_K8S_PODS);
  const bool pod_form = !(flags & KANO_K8S_ALL) && !classes;
  if ((flags & KANO_K8S_DST_EG) && (pod_form || dst->rows_dirty || dst->P != eg_t->P))
    return fail(dst, -EINVAL, "kano_k8s_edge: KANO_K8S_DST_EG needs dst = an unedited build "
                              "of the egress policies (class-level form)");
  if (pod_form) {
    if (r0 != 0 || rl != n)
      return fail(dst, -ENOTSUP, "kano_k8s_edge: the pod-level form needs every row");
    for (kano_ctx* s : {in_t, eg_t}) {
      const int rc = ensure_matrix(s);   // (a deferred matrix write runs now)
      if (rc) return fail(dst, rc, "kano_k8s_edge: source: " + s->err);
    }
  }
  for (kano_ctx* s : {in_t, eg_t}) {
    const int rc = sync(s);   // the sources' classes / matrices are complete
    if (rc) return fail(dst, rc, "kano_k8s_edge: source: " + s->err);
  }
  u64* E = P_<u64>(dst->M);
  u64 added = 0;
  const int self = (flags & KANO_K8S_SELF) ? 1 : 0;
  if (rl > 0 && W > 0) {
    if (flags & KANO_K8S_ALL) {
      hipLaunchKernelGGL(k_k8s_ones, dim3(nblk(rl * ldM)), dim3(TPB), 0, ctx->stream, E, ldM, rl,
                         n, W);
      KLAUNCH();
    } else if (classes) {
      // class level (kano_k8s.hpp): B, EgA, Mc_i transposed, Ec, expansion;
      // only Mc and the class ids of the two builds are read
      const i64 Ui = in_t->rc.U, Xi = in_t->cc.U, Ue = eg_t->rc.U, Ye = eg_t->cc.U;
      const i64 ldCe = eg_t->ldC, ldCi = in_t->ldC;
      const i64 KWb = (Ue + 63) / 64, KWa = (Ui + 63) / 64, NWe = (Ye + 63) / 64;
      KTRY(dalloc(ctx, ctx->pA, sizeof(u64) * Ui * KWb));
      KTRY(dalloc(ctx, ctx->pB, sizeof(u64) * Ui * ldCe));
      KTRY(dalloc(ctx, ctx->pT, sizeof(u64) * Xi * KWa));
      KTRY(dalloc(ctx, ctx->pR[0], sizeof(u64) * Xi * ldCe));
      KCHK(hipMemsetAsync(ctx->pA.p, 0, sizeof(u64) * Ui * KWb, ctx->stream));
      hipLaunchKernelGGL(k_k8s_pairs, dim3(nblk(n)), dim3(TPB), 0, ctx->stream,
                         P_<int32_t>(in_t->rc.cls), P_<int32_t>(eg_t->rc.cls), n,
                         P_<u64>(ctx->pA), KWb);
      KLAUNCH();
      const i64 nch = (ldCe + 255) / 256;
      hipLaunchKernelGGL(k_k8s_or_rows<4>, dim3(nblk(Ui * nch, TPB / 64)), dim3(TPB), 0,
                         ctx->stream, P_<u64>(ctx->pA), KWb, KWb, P_<u64>(eg_t->Mc), ldCe, NWe,
                         P_<u64>(ctx->pB), ldCe, Ui, nch);
      KLAUNCH();
      const i64 CGi = ((Xi + 63) / 64 + 15) / 16;
      hipLaunchKernelGGL(k_k8s_transpose, dim3(nblk(KWa * CGi, TPB / 64)), dim3(TPB), 0,
                         ctx->stream, P_<u64>(in_t->Mc), ldCi, Ui, KWa, CGi, Xi,
                         P_<u64>(ctx->pT), KWa);
      KLAUNCH();
      hipLaunchKernelGGL(k_k8s_or_rows<4>, dim3(nblk(Xi * nch, TPB / 64)), dim3(TPB), 0,
                         ctx->stream, P_<u64>(ctx->pT), KWa, KWa, P_<u64>(ctx->pB), ldCe, NWe,
                         P_<u64>(ctx->pR[0]), ldCe, Xi, nch);
      KLAUNCH();
      // class rows of <= K8S_STAGE_W words are staged in LDS by the expansion
      // (launched by handle: see launch_marked)
      auto K8S_EXPAND = ldCe <= K8S_STAGE_W ? k_k8s_expand<true> : k_k8s_expand<false>;
      const int32_t* cci = P_<int32_t>(in_t->cc.cls);
      const int32_t* rce = P_<int32_t>(eg_t->rc.cls);
      const int32_t* cce = P_<int32_t>(eg_t->cc.cls);
      // KANO_K8S_DST_EG: dst already holds the shard's EgT rows (a build of
      // the egress policies), so the self term needs no expansion
      const bool in_place = self && (flags & KANO_K8S_DST_EG);
      const i64 Us = (self && !in_place) ? Ue : 0;
      if (Xi + Us <= std::max<i64>(rl / 2, 1) && ldM % 2 == 0) {
        // expand the class rows once (Ec's Xi rows; for self traffic Mc_e's
        // Ue rows, i.e. EgT by egress row class), then stream them to the
        // shard's pod rows
        KTRY(dalloc(ctx, ctx->pR[1], sizeof(u64) * (Xi + Us) * ldM));
        u64* Xe = P_<u64>(ctx->pR[1]);
        u64* Se = Xe + Xi * ldM;
        hipExtLaunchKernelGGL(K8S_EXPAND, dim3(nblk(ldM, K8S_XW), nblk(Xi, K8S_XR)), dim3(TPB), 0,
                           ctx->stream, nullptr, nullptr, 0, P_<u64>(ctx->pR[0]), ldCe, (const int32_t*)nullptr,
                           (const u64*)nullptr, ldCe, (const int32_t*)nullptr, cce, 0, (i64)0, Xi,
                           n, W, Xe, ldM);
        KLAUNCH();
        if (Us) {
          hipExtLaunchKernelGGL(K8S_EXPAND, dim3(nblk(ldM, K8S_XW), nblk(Ue, K8S_XR)), dim3(TPB),
                              0, ctx->stream, nullptr, nullptr, 0, P_<u64>(eg_t->Mc), ldCe, (const int32_t*)nullptr,
                             (const u64*)nullptr, ldCe, (const int32_t*)nullptr, cce, 0, (i64)0,
                             Ue, n, W, Se, ldM);
          KLAUNCH();
        }
        if (in_place) {
          hipLaunchKernelGGL(k_k8s_or_into, dim3(nblk(rl * (ldM / 2))), dim3(TPB), 0, ctx->stream,
                             Xe, cci, r0, rl, ldM, E);
        } else {
          hipLaunchKernelGGL(k_k8s_rows, dim3(nblk(rl * (ldM / 2))), dim3(TPB), 0, ctx->stream,
                             Xe, cci, Se, rce, self, r0, rl, ldM, E);
        }
        KLAUNCH();
      } else {
        hipExtLaunchKernelGGL(K8S_EXPAND, dim3(nblk(ldM, K8S_XW), nblk(rl, K8S_XR)), dim3(TPB), 0,
                           ctx->stream, nullptr, nullptr, 0, P_<u64>(ctx->pR[0]), ldCe, cci, P_<u64>(eg_t->Mc), ldCe,
                           rce, cce, self, r0, rl, n, W, E, ldM);
        KLAUNCH();
      }
      added = (u64)-1;
    } else {
      // pod level: edge starts as EgT (self ingress traffic: sel = src) or
      // empty, then edge[src] |= OR_{sel in In[src]} EgT[sel], In = InT^T
      if (self)
        KCHK(hipMemcpyAsync(E, eg_t->M.p, sizeof(u64) * n * ldM, hipMemcpyDeviceToDevice,
                            ctx->stream));
      else
        KCHK(hipMemsetAsync(E, 0, sizeof(u64) * n * ldM, ctx->stream));
      KTRY(dalloc(ctx, ctx->pA, sizeof(u64) * n * ldM));
      KTRY(dalloc(ctx, ctx->pB, sizeof(u64) * n * ldM));
      KTRY(dalloc(ctx, ctx->pcnt, sizeof(u64) * PATH_CNT_SLOTS * PATH_CNT_STRIDE));
      KCHK(hipMemsetAsync(ctx->pcnt.p, 0, sizeof(u64) * PATH_CNT_SLOTS * PATH_CNT_STRIDE,
                          ctx->stream));
      const i64 CG = (W + 15) / 16;
      hipLaunchKernelGGL(k_k8s_transpose, dim3(nblk(W * CG, TPB / 64)), dim3(TPB), 0, ctx->stream,
                         P_<u64>(in_t->M), ldM, n, W, CG, n, P_<u64>(ctx->pA), ldM);
      KLAUNCH();
      PathGeom g;
      g.identity = true;
      g.rows = n;
      g.Ua = n;
      g.KW = W;
      g.ldR = ldM;
      g.T = P_<u64>(eg_t->M);
      if (ldM <= 128) KTRY(path_or_launch<2>(ctx, P_<u64>(ctx->pA), E, P_<u64>(ctx->pB), g));
      else KTRY(path_or_launch<4>(ctx, P_<u64>(ctx->pA), E, P_<u64>(ctx->pB), g));
      std::vector<u64> slots(PATH_CNT_SLOTS * PATH_CNT_STRIDE);
      KCHK(hipMemcpyAsync(slots.data(), ctx->pcnt.p, sizeof(u64) * slots.size(),
                          hipMemcpyDeviceToHost, ctx->stream));
      KTRY(sync(ctx));
      for (int k = 0; k < PATH_CNT_SLOTS; ++k) added += slots[(size_t)k * PATH_CNT_STRIDE];
    }
  }
  KTRY(sync(ctx));
  ctx->cols_valid = false;
  ctx->rows_dirty = true;
  if (info) info[0] = (int64_t)added;
  return 0;
}

}  // extern "C"

// ===========================================================================
// matrix_diff: two resident matrices compared in one pass (k_diff_rows /
// k_diff_emit, kano_kernels.hpp; launched through kano_hip.hip's helpers).
// ===========================================================================
namespace {

// kano_path's preamble for two contexts holding the same rows: both matrices
// present, a's pending work complete; the work then runs on b's stream and
// errors are reported on b
int diff_prepare(kano_ctx* a, kano_ctx* b, const char* what) {
  kano_ctx* ctx = b;
  const std::string w(what);
  if (a->device != b->device) return fail(b, -EINVAL, w + ": contexts on two devices");
  KCHK(hipSetDevice(b->device));
  if (a != b) {
    const int rc = ensure_matrix(a);
    if (rc) return fail(b, rc, w + ": first matrix: " + a->err);
  }
  KTRY(ensure_matrix(b));
  if (a->n != b->n) return fail(b, -EINVAL, w + ": the matrices differ in size");
  if (a->r0 != b->r0 || a->r1 != b->r1)
    return fail(b, -EINVAL, w + ": the contexts hold different rows");
  if ((a->ldM | b->ldM) & 1) return fail(b, -ENOTSUP, w + ": odd row pitch");
  if (a != b) {
    const int rc = sync(a);
    if (rc) return fail(b, rc, w + ": first matrix: " + a->err);
  }
  return 0;
}

// diff_buf's layout for `rows` rows: [totals 2 | col_added W | col_removed W]
// u64, then [row_added | row_removed] int32
struct DiffBuf {
  u64* totals;
  u64* col;
  int32_t* row;
  size_t bytes;
};
DiffBuf diff_layout(kano_ctx* b, i64 rows, bool full) {
  DiffBuf d;
  const size_t words = 2 + (full ? 2 * (size_t)b->W : 0);
  d.bytes = sizeof(u64) * words + (full ? sizeof(int32_t) * 2 * (size_t)rows : 0);
  d.totals = P_<u64>(b->diff_buf);
  d.col = d.totals + 2;
  d.row = reinterpret_cast<int32_t*>(d.totals + words);
  return d;
}

// the pass over rows [q0, q0 + rows) of both matrices into b->diff_buf
int diff_pass(kano_ctx* a, kano_ctx* b, i64 q0, i64 rows, bool full, DiffBuf* out) {
  kano_ctx* ctx = b;
  KTRY(dalloc(ctx, b->diff_buf, diff_layout(b, rows, full).bytes));
  const DiffBuf d = diff_layout(b, rows, full);
  KCHK(hipMemsetAsync(b->diff_buf.p, 0, d.bytes, ctx->stream));
  DiffOut o{};
  o.totals = d.totals;
  if (full) {
    o.col_added = d.col;
    o.col_removed = d.col + b->W;
    o.row_added = d.row;
    o.row_removed = d.row + rows;
  }
  KTRY(diff_rows_launch(ctx, P_<u64>(a->M) + (q0 - a->r0) * a->ldM, a->ldM,
                        P_<u64>(b->M) + (q0 - b->r0) * b->ldM, b->ldM, rows, o));
  *out = d;
  return 0;
}

}  // namespace

extern "C" {

int kano_diff(kano_ctx* a, kano_ctx* b, int64_t* totals, int32_t* row_added,
              int32_t* row_removed, uint64_t* col_added, uint64_t* col_removed) {
  if (!a || !b) return -EINVAL;
  kano_ctx* ctx = b;
  if (!totals) return fail(b, -EINVAL, "kano_diff: totals is NULL");
  KTRY(diff_prepare(a, b, "kano_diff"));
  const i64 rl = rows_local(b), W = b->W;
  totals[0] = totals[1] = 0;
  if (rl > 0) {
    if (row_added) std::memset(row_added, 0, sizeof(int32_t) * (size_t)rl);
    if (row_removed) std::memset(row_removed, 0, sizeof(int32_t) * (size_t)rl);
  }
  if (W > 0) {
    if (col_added) std::memset(col_added, 0, sizeof(u64) * (size_t)W);
    if (col_removed) std::memset(col_removed, 0, sizeof(u64) * (size_t)W);
  }
  if (rl <= 0 || W <= 0) return 0;
  const bool full = row_added || row_removed || col_added || col_removed;
  // timing=1: the call's device time (the fill and the kernel, no copy)
  EventPair<> tev;
  if (ctx->stage_timing) KTRY(tev.start(ctx));
  DiffBuf d{};
  KTRY(diff_pass(a, b, b->r0, rl, full, &d));
  KTRY(tev.stop(ctx, &ctx->diff_ms));
  u64 t[2] = {0, 0};
  KCHK(hipMemcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
  if (row_added)
    KCHK(hipMemcpyAsync(row_added, d.row, sizeof(int32_t) * rl, hipMemcpyDeviceToHost,
                        ctx->stream));
  if (row_removed)
    KCHK(hipMemcpyAsync(row_removed, d.row + rl, sizeof(int32_t) * rl, hipMemcpyDeviceToHost,
                        ctx->stream));
  if (col_added)
    KCHK(hipMemcpyAsync(col_added, d.col, sizeof(u64) * W, hipMemcpyDeviceToHost, ctx->stream));
  if (col_removed)
    KCHK(hipMemcpyAsync(col_removed, d.col + W, sizeof(u64) * W, hipMemcpyDeviceToHost,
                        ctx->stream));
  KTRY(sync(ctx));
  totals[0] = (int64_t)t[0];
  totals[1] = (int64_t)t[1];
  return 0;
}

int kano_diff_pairs(kano_ctx* a, kano_ctx* b, int kind, int64_t r0, int64_t nrows,
                    int64_t max_pairs, int64_t* count, int32_t* pairs) {
  if (!a || !b) return -EINVAL;
  kano_ctx* ctx = b;
  if (!count) return fail(b, -EINVAL, "kano_diff_pairs: count is NULL");
  *count = 0;
  if (kind != 0 && kind != 1) return fail(b, -EINVAL, "kano_diff_pairs: unknown kind");
  if (max_pairs < 0) return fail(b, -EINVAL, "kano_diff_pairs: max_pairs < 0");
  KTRY(diff_prepare(a, b, "kano_diff_pairs"));
  if (nrows < 0 || r0 < b->r0 || r0 > b->r1 || nrows > b->r1 - r0)
    return fail(b, -EINVAL, "kano_diff_pairs: rows outside this shard");
  if (nrows == 0 || b->W == 0) return 0;
  // the range recounted: its row counts are the emission's offsets
  DiffBuf d{};
  KTRY(diff_pass(a, b, r0, nrows, true, &d));
  u64 t[2] = {0, 0};
  KCHK(hipMemcpyAsync(t, d.totals, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
  KTRY(sync(ctx));
  const i64 total = (i64)t[kind];
  *count = total;
  if (!pairs || total == 0) return 0;
  if (total > max_pairs)
    return fail(b, -ENOSPC, "kano_diff_pairs: " + std::to_string(total) + " pairs, room for " +
                                std::to_string(max_pairs));
  DBuf off, out;
  KTRY(dalloc(ctx, off, sizeof(i64) * (size_t)(nrows + 1 + 2 * DIFF_SCAN_TILES + 1)));
  KTRY(dalloc(ctx, out, sizeof(int32_t) * 2 * (size_t)total));
  i64* offp = P_<i64>(off);
  KTRY(diff_offsets_launch(ctx, d.row + (kind ? nrows : 0), nrows, offp + nrows + 1, offp));
  KTRY(diff_emit_launch(ctx, P_<u64>(a->M) + (r0 - a->r0) * a->ldM, a->ldM,
                        P_<u64>(b->M) + (r0 - b->r0) * b->ldM, b->ldM, nrows, kind, r0, offp,
                        total, P_<int32_t>(out)));
  KCHK(hipMemcpyAsync(pairs, out.p, sizeof(int32_t) * 2 * (size_t)total, hipMemcpyDeviceToHost,
                      ctx->stream));
  return sync(ctx);
}

int kano_copy_matrix(kano_ctx* src, kano_ctx* dst) {
  if (!src || !dst) return -EINVAL;
  kano_ctx* ctx = dst;
  if (src == dst)
    return fail(dst, -EINVAL, "kano_copy_matrix: the destination must be another context");
  KTRY(diff_prepare(src, dst, "kano_copy_matrix"));
  const i64 rl = rows_local(dst), W = dst->W;
  if (rl > 0 && W > 0) {
    if (src->ldM == dst->ldM)
      KCHK(hipMemcpyAsync(dst->M.p, src->M.p, sizeof(u64) * rl * dst->ldM,
                          hipMemcpyDeviceToDevice, ctx->stream));
    else
      KCHK(hipMemcpy2DAsync(dst->M.p, sizeof(u64) * dst->ldM, src->M.p, sizeof(u64) * src->ldM,
                            sizeof(u64) * W, (size_t)rl, hipMemcpyDeviceToDevice, ctx->stream));
  }
  KTRY(sync(dst));
  dst->cols_valid = false;
  dst->rows_dirty = true;
  dst->user_edited = true;
  return 0;
}

int kano_diff_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->diff_ms;
  return 0;
}

}  // extern "C"

// ===========================================================================
// group_reachability: the matrix's quotient by two pod labellings
// (k_group_masks / k_group_rows, kano_kernels.hpp; launched through
// kano_hip.hip's helpers).
// ===========================================================================
namespace {

constexpr i64 GROUP_MAX_CELLS = 1ll << 27;     // Gs * Gd of one call (1 GiB of counts)
constexpr i64 GROUP_MASK_BUDGET = 1ll << 30;   // bytes of transposed masks of one pass

// the local rows in source-group order and their runs of at most run_len
// rows; the rows left out of counts follow as runs of group -1 when with_out
void group_runs(const int32_t* gs, i64 r0, i64 rl, i64 Gs, bool with_out, i64 run_len,
                std::vector<int32_t>& order, std::vector<GroupRun>& runs) {
  order.clear();
  runs.clear();
  order.reserve((size_t)rl);
  auto key = [&](i64 r) -> i64 { return gs[r0 + r] < 0 ? Gs : gs[r0 + r]; };
  if (Gs <= (1ll << 22)) {   // a counting sort (stable: rows ascending in a group)
    std::vector<i64> pos((size_t)Gs + 2, 0);
    for (i64 r = 0; r < rl; ++r) ++pos[key(r) + 1];
    for (i64 g = 0; g <= Gs; ++g) pos[g + 1] += pos[g];
    order.resize((size_t)rl);
    for (i64 r = 0; r < rl; ++r) order[pos[key(r)]++] = (int32_t)r;
  } else {
    for (i64 r = 0; r < rl; ++r) order.push_back((int32_t)r);
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t x, int32_t y) { return key(x) < key(y); });
  }
  if (!with_out)
    while (!order.empty() && key(order.back()) == Gs) order.pop_back();
  const i64 m = (i64)order.size();
  for (i64 p = 0; p < m;) {
    const i64 k = key(order[p]);
    i64 q = p;
    while (q < m && q - p < run_len && key(order[q]) == k) ++q;
    runs.push_back(GroupRun{k == Gs ? -1 : (int32_t)k, (int32_t)p, (int32_t)(q - p)});
    p = q;
  }
}

}  // namespace

extern "C" {

int kano_group_counts(kano_ctx* ctx, const int32_t* gsrc, int32_t Gs, const int32_t* gdst,
                      int32_t Gd, int64_t* counts, int32_t* row_counts) {
  if (!ctx) return -EINVAL;
  if (!gsrc || !gdst || !counts)
    return fail(ctx, -EINVAL, "kano_group_counts: gsrc, gdst or counts is NULL");
  if (Gs <= 0 || Gd <= 0) return fail(ctx, -EINVAL, "kano_group_counts: Gs and Gd must be > 0");
  if ((i64)Gs * Gd > GROUP_MAX_CELLS)
    return fail(ctx, -ENOTSUP, "kano_group_counts: Gs * Gd = " + std::to_string((i64)Gs * Gd) +
                                   " beyond " + std::to_string(GROUP_MAX_CELLS) +
                                   " (ask for row_counts with fewer source groups)");
  KTRY(ensure_matrix(ctx));
  const i64 n = ctx->n, W = ctx->W, rl = std::max<i64>(0, rows_local(ctx));
  for (i64 i = 0; i < n; ++i)
    if (gsrc[i] >= Gs || gdst[i] >= Gd)
      return fail(ctx, -ERANGE, "kano_group_counts: pod " + std::to_string(i) +
                                    " has a group id at or past its group count");
  const size_t cells = (size_t)Gs * (size_t)Gd, rcells = (size_t)rl * (size_t)Gd;
  std::memset(counts, 0, sizeof(int64_t) * cells);
  if (row_counts && rcells) std::memset(row_counts, 0, sizeof(int32_t) * rcells);
  KTRY(sync(ctx));
  if (n == 0 || W == 0 || rl == 0) return 0;

  // passes of nbp batches of 64 destination groups
  const i64 nb = ((i64)Gd + 63) / 64;
  i64 nbp = std::max<i64>(1, GROUP_MASK_BUDGET / (512 * W));
  nbp = std::min(nbp, std::max<i64>(1, (i64)0x7fffffff / W));
  if (ctx->group_batches > 0) nbp = std::min<i64>(nbp, ctx->group_batches);
  nbp = std::min(nbp, nb);
  std::vector<int32_t> order;
  std::vector<GroupRun> runs;
  group_runs(gsrc, ctx->r0, rl, Gs, row_counts != nullptr,
             group_run_rows(ctx, rl, nbp, row_counts != nullptr), order, runs);
  const i64 nruns = (i64)runs.size();
  if (nruns == 0) return 0;   // every source id negative, no row counts wanted

  // the call's own buffers
  DBuf in, masks, out, rows;
  const size_t b_gd = sizeof(int32_t) * (size_t)n, b_ord = sizeof(int32_t) * order.size(),
               b_run = sizeof(GroupRun) * runs.size();
  KTRY(dalloc(ctx, in, b_gd + b_ord + b_run));
  KTRY(dalloc(ctx, masks, sizeof(u64) * 64 * (size_t)nbp * (size_t)W));
  KTRY(dalloc(ctx, out, sizeof(u64) * cells));
  if (row_counts) KTRY(dalloc(ctx, rows, sizeof(int32_t) * rcells));
  char* ip = static_cast<char*>(in.p);
  KCHK(hipMemcpyAsync(ip, gdst, b_gd, hipMemcpyHostToDevice, ctx->stream));
  KCHK(hipMemcpyAsync(ip + b_gd, order.data(), b_ord, hipMemcpyHostToDevice, ctx->stream));
  KCHK(hipMemcpyAsync(ip + b_gd + b_ord, runs.data(), b_run, hipMemcpyHostToDevice,
                      ctx->stream));
  // timing=1: the call's device time (the fills and the kernels, no copy)
  EventPair<> tev;
  if (ctx->stage_timing) KTRY(tev.start(ctx));
  KCHK(hipMemsetAsync(out.p, 0, sizeof(u64) * cells, ctx->stream));
  if (row_counts) KCHK(hipMemsetAsync(rows.p, 0, sizeof(int32_t) * rcells, ctx->stream));
  const int32_t* gd_d = reinterpret_cast<const int32_t*>(ip);
  const int32_t* ord_d = reinterpret_cast<const int32_t*>(ip + b_gd);
  const GroupRun* run_d = reinterpret_cast<const GroupRun*>(ip + b_gd + b_ord);
  for (i64 b0 = 0; b0 < nb; b0 += nbp) {
    const i64 k = std::min(nbp, nb - b0);
    KTRY(group_masks_launch(ctx, gd_d, b0, k, P_<u64>(masks)));
    KTRY(group_rows_launch(ctx, P_<u64>(masks), b0, k, ord_d, run_d, nruns, Gd, P_<u64>(out),
                           row_counts ? P_<int32_t>(rows) : nullptr));
  }
  KTRY(tev.stop(ctx, &ctx->group_ms));
  KCHK(hipMemcpyAsync(counts, out.p, sizeof(u64) * cells, hipMemcpyDeviceToHost, ctx->stream));
  if (row_counts)
    KCHK(hipMemcpyAsync(row_counts, rows.p, sizeof(int32_t) * rcells, hipMemcpyDeviceToHost,
                        ctx->stream));
  return sync(ctx);
}

int kano_group_counts_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->group_ms;
  return 0;
}

}  // extern "C"

// ===========================================================================
// hop_distance / path_witness: breadth-first search over the resident matrix
// (k_hops_*, kano_hops.hpp), a batch of sources at once.
// ===========================================================================
namespace {

constexpr i64 HOPS_MAX_CELLS = 1ll << 28;     // S * n of one kano_hops call (1 GiB of dist)
constexpr i64 HOPS_BUDGET = 1ll << 30;        // bytes of per-source device state of one batch
constexpr i64 HOPS_MAX_BATCH = 64;            // sources of one batch at most
constexpr i64 HOPS_TARGET_WAVES = 16384;      // expand items (waves) a level aims at

// what a call accumulates over its batches (kano_hops' info)
struct HopsStats {
  i64 levels = 0, rows_ored = 0, batches = 0, reached = 0;
};

// the call's own buffers: per source dist and the frontier list (n int32
// each), visited | next | target mask (W words each); the batch's sources,
// counters and target counts; the counters' page-locked landing buffer
struct HopsBufs {
  DBuf dist, list, bits, small, items, gath, nodes;
  Pinned<int32_t> pin;
  EventPair<> ev;   // timing=1: a batch's bracket
  i64 B = 0;
};

// the shared preamble: arguments, the matrix present and complete, every row held
int hops_prepare(kano_ctx* ctx, const char* what, int32_t max_hops) {
  const std::string w(what);
  if (max_hops < 0) return fail(ctx, -EINVAL, w + ": max_hops < 0");
  KTRY(ensure_matrix(ctx));
  if (ctx->r0 != 0 || ctx->r1 != ctx->n)
    return fail(ctx, -EINVAL, w + ": the context holds rows [" + std::to_string(ctx->r0) + ", " +
                                  std::to_string(ctx->r1) + ") of " + std::to_string(ctx->n) +
                                  ": a search needs every row");
  return sync(ctx);
}

int hops_alloc(kano_ctx* ctx, HopsBufs& h, i64 nsrc, bool targets) {
  const i64 n = ctx->n, W = ctx->W;
  const i64 per = 8 * n + 24 * W + 64;
  h.B = std::max<i64>(1, std::min<i64>({HOPS_MAX_BATCH, HOPS_BUDGET / per, nsrc}));
  KTRY(dalloc(ctx, h.dist, sizeof(int32_t) * (size_t)(h.B * n)));
  KTRY(dalloc(ctx, h.list, sizeof(int32_t) * (size_t)(h.B * n)));
  KTRY(dalloc(ctx, h.bits, sizeof(u64) * (size_t)((targets ? 3 : 2) * h.B * W)));
  KTRY(dalloc(ctx, h.small, sizeof(int32_t) * (size_t)(5 * h.B)));
  KCHK(h.pin.alloc(sizeof(int32_t) * (size_t)(3 * h.B), hipHostMallocDefault));
  if (ctx->stage_timing)
    for (hipEvent_t& e : h.ev.e) KCHK(hipEventCreate(&e));
  return 0;
}

// One batch: the searches of B sources (src, host) level by level.  tmask /
// ntgt (host; both or neither): per source its targets' bit row and their
// number -- a source stops once all of them have a distance.  On return the
// batch's dist arrays are resident in h.dist and the stream is idle; the
// timing events stay open for the caller's kernels (hops_batch_end).
int hops_batch(kano_ctx* ctx, HopsBufs& h, i64 B, const int32_t* src, int32_t max_hops,
               const u64* tmask, const int32_t* ntgt, HopsStats& st) {
  const i64 n = ctx->n, W = ctx->W;
  int32_t* small = P_<int32_t>(h.small);
  int32_t* src_d = small;
  int32_t* cnts_d = small + h.B;          // 3 B entries, laid out for this batch's B
  int32_t* ntgt_d = small + 4 * h.B;
  u64* visited = P_<u64>(h.bits);
  u64* next = visited + B * W;
  u64* tmask_d = tmask ? next + B * W : nullptr;
  KCHK(hipMemcpyAsync(src_d, src, sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx->stream));
  if (tmask) {
    KCHK(hipMemcpyAsync(ntgt_d, ntgt, sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx->stream));
    KCHK(hipMemcpyAsync(tmask_d, tmask, sizeof(u64) * B * W, hipMemcpyHostToDevice, ctx->stream));
  }
  if (h.ev[0]) KCHK(hipEventRecord(h.ev[0], ctx->stream));
  const i64 cells = std::max(B * n, 2 * B * W);
  hipLaunchKernelGGL(k_hops_init, dim3(std::min<i64>(4096, nblk(cells))), dim3(TPB), 0,
                     ctx->stream, P_<int32_t>(h.dist), visited, P_<int32_t>(h.list), cnts_d, src_d,
                     n, W, (int)B);
  KLAUNCH();
  std::vector<int32_t> cnt((size_t)B, 1);
  std::vector<char> live((size_t)B, 1);
  const i64 nch = (W + HOPS_CW - 1) / HOPS_CW;
  for (i64 k = 1; max_hops == 0 || k <= max_hops; ++k) {
    i64 nlive = 0, maxcnt = 0, sum = 0;
    for (i64 b = 0; b < B; ++b)
      if (live[b]) {
        ++nlive;
        maxcnt = std::max<i64>(maxcnt, cnt[b]);
        sum += cnt[b];
      }
    if (nlive == 0) break;
    if (k > 0x7fffffff) return fail(ctx, -ENOTSUP, "kano_hops: level count overflow");
    st.rows_ored += sum;
    // slices of the frontier: enough waves to fill the device, each OR-ing
    // at least HOPS_MIN_SLICE rows before its atomics
    const i64 slice = std::max<i64>(HOPS_MIN_SLICE,
                                    (maxcnt * nch * nlive + HOPS_TARGET_WAVES - 1) /
                                        HOPS_TARGET_WAVES);
    const i64 nsl = nblk((maxcnt + slice - 1) / slice, TPB / 64);
    hipLaunchKernelGGL(k_hops_expand, dim3((unsigned)nch, (unsigned)nsl, (unsigned)B), dim3(TPB),
                       0, ctx->stream, P_<u64>(ctx->M), ctx->ldM, n, W, P_<int32_t>(h.list),
                       cnts_d, tmask ? ntgt_d : (const int32_t*)nullptr, (int)B, (int)k,
                       (int)slice, next);
    KLAUNCH();
    hipLaunchKernelGGL(k_hops_finish, dim3((unsigned)nblk(W), (unsigned)B), dim3(TPB), 0,
                       ctx->stream, n, W, visited, next, (const u64*)tmask_d, P_<int32_t>(h.dist),
                       P_<int32_t>(h.list), cnts_d, tmask ? ntgt_d : (const int32_t*)nullptr,
                       (int)B, (int)k);
    KLAUNCH();
    KCHK(hipMemcpyAsync(h.pin, cnts_d, sizeof(int32_t) * 3 * B, hipMemcpyDeviceToHost,
                        ctx->stream));
    KTRY(sync(ctx));
    const int32_t* now = h.pin + (k & 1) * B;
    const int32_t* hit = h.pin + 2 * B;
    for (i64 b = 0; b < B; ++b) {
      if (!live[b]) continue;
      cnt[b] = now[b];
      if (cnt[b] > 0) {
        st.reached += cnt[b];
        st.levels = std::max(st.levels, k);
      }
      live[b] = cnt[b] > 0 && !(ntgt && hit[b] >= ntgt[b]);
    }
  }
  st.batches += 1;
  return 0;
}

// closes the batch's timing (after the caller's gather / witness kernels):
// hops_ms holds the batches that ended, also where a later one fails
int hops_batch_end(kano_ctx* ctx, HopsBufs& h) {
  float ms = 0.f;
  KTRY(h.ev.stop(ctx, &ms));
  ctx->hops_ms += ms;
  return 0;
}

}  // namespace

extern "C" {

int kano_hops(kano_ctx* ctx, int64_t S, const int32_t* sources, int32_t max_hops, int32_t* dist,
              int64_t* info) {
  if (!ctx) return -EINVAL;
  if (S < 0 || (S > 0 && (!sources || !dist)))
    return fail(ctx, -EINVAL, "kano_hops: S < 0, or sources or dist is NULL");
  KTRY(hops_prepare(ctx, "kano_hops", max_hops));
  const i64 n = ctx->n;
  for (i64 k = 0; k < S; ++k)
    if (sources[k] < 0 || sources[k] >= n)
      return fail(ctx, -ERANGE, "kano_hops: source " + std::to_string(sources[k]) +
                                    " outside [0, " + std::to_string(n) + ")");
  if (n > 0 && S > HOPS_MAX_CELLS / n)
    return fail(ctx, -ENOTSUP, "kano_hops: S * n = " + std::to_string(S * n) + " beyond " +
                                   std::to_string(HOPS_MAX_CELLS) + " (ask in slices)");
  if (info) std::memset(info, 0, sizeof(int64_t) * 4);
  ctx->hops_ms = 0.f;
  if (n == 0 || S == 0) return 0;
  HopsBufs h;
  HopsStats st;
  KTRY(hops_alloc(ctx, h, S, false));
  for (i64 s0 = 0; s0 < S; s0 += h.B) {
    const i64 B = std::min(h.B, S - s0);
    KTRY(hops_batch(ctx, h, B, sources + s0, max_hops, nullptr, nullptr, st));
    KTRY(hops_batch_end(ctx, h));
    KCHK(hipMemcpyAsync(dist + s0 * n, h.dist.p, sizeof(int32_t) * (size_t)(B * n),
                        hipMemcpyDeviceToHost, ctx->stream));
    KTRY(sync(ctx));
  }
  if (info) {
    info[0] = st.levels;
    info[1] = st.rows_ored;
    info[2] = st.batches;
    info[3] = st.reached;
  }
  return 0;
}

int kano_hop_pairs(kano_ctx* ctx, int64_t Q, const int32_t* pairs, int32_t max_hops, int mode,
                   int32_t* dist, int64_t* total) {
  if (!ctx) return -EINVAL;
  if (total) *total = 0;
  ctx->hop_total = -1;
  ctx->hop_nodes.clear();
  if (Q < 0 || (Q > 0 && (!pairs || !dist)))
    return fail(ctx, -EINVAL, "kano_hop_pairs: Q < 0, or pairs or dist is NULL");
  if (mode != 0 && mode != 1) return fail(ctx, -EINVAL, "kano_hop_pairs: unknown mode");
  KTRY(hops_prepare(ctx, "kano_hop_pairs", max_hops));
  const i64 n = ctx->n, W = ctx->W;
  for (i64 q = 0; q < 2 * Q; ++q)
    if (pairs[q] < 0 || pairs[q] >= n)
      return fail(ctx, -ERANGE, "kano_hop_pairs: pod " + std::to_string(pairs[q]) +
                                    " outside [0, " + std::to_string(n) + ")");
  ctx->hops_ms = 0.f;
  if (Q == 0 || n == 0) {
    if (mode == 1) ctx->hop_total = 0;   // no paths, and a fetch of none is valid
    return 0;
  }

  // the pairs by source: one search per distinct source, whatever its targets
  std::vector<i64> order((size_t)Q);
  for (i64 q = 0; q < Q; ++q) order[q] = q;
  std::stable_sort(order.begin(), order.end(),
                   [&](i64 x, i64 y) { return pairs[2 * x] < pairs[2 * y]; });
  std::vector<int32_t> srcs;          // distinct, ascending
  std::vector<i64> first;             // srcs[k]'s pairs are order[first[k] .. first[k + 1])
  for (i64 p = 0; p < Q; ++p)
    if (p == 0 || pairs[2 * order[p]] != srcs.back()) {
      srcs.push_back(pairs[2 * order[p]]);
      first.push_back(p);
    }
  first.push_back(Q);
  const i64 S = (i64)srcs.size();

  std::vector<int32_t> sorted_nodes;  // the paths in `order`'s order
  std::vector<int32_t> dsort((size_t)Q);
  HopsBufs h;   // (after the host arrays its copies land in: freed, and waited for, first)
  HopsStats st;
  KTRY(hops_alloc(ctx, h, S, true));
  std::vector<u64> tmask((size_t)(h.B * W));
  std::vector<int32_t> ntgt((size_t)h.B);
  std::vector<int2> items;
  std::vector<HopsWitness> wit;
  for (i64 s0 = 0; s0 < S; s0 += h.B) {
    const i64 B = std::min(h.B, S - s0);
    const i64 p0 = first[s0], p1 = first[s0 + B], np = p1 - p0;
    std::fill(tmask.begin(), tmask.begin() + B * W, 0ull);
    items.resize((size_t)np);
    for (i64 b = 0; b < B; ++b) {
      int32_t distinct = 0;
      for (i64 p = first[s0 + b]; p < first[s0 + b + 1]; ++p) {
        const int32_t t = pairs[2 * order[p] + 1];
        u64& word = tmask[(size_t)(b * W + (t >> 6))];
        if (!(word >> (t & 63) & 1ull)) ++distinct;
        word |= 1ull << (t & 63);
        items[(size_t)(p - p0)] = make_int2((int)b, t);
      }
      ntgt[b] = distinct;
    }
    KTRY(dalloc(ctx, h.items, sizeof(int2) * (size_t)np));
    KTRY(dalloc(ctx, h.gath, sizeof(int32_t) * (size_t)np));
    KTRY(hops_batch(ctx, h, B, srcs.data() + s0, max_hops, tmask.data(), ntgt.data(), st));
    KCHK(hipMemcpyAsync(h.items.p, items.data(), sizeof(int2) * (size_t)np,
                        hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_hops_gather, dim3(nblk(np)), dim3(TPB), 0, ctx->stream,
                       P_<int32_t>(h.dist), n, P_<int2>(h.items), np, P_<int32_t>(h.gath));
    KLAUNCH();
    KCHK(hipMemcpyAsync(dsort.data() + p0, h.gath.p, sizeof(int32_t) * (size_t)np,
                        hipMemcpyDeviceToHost, ctx->stream));
    KTRY(sync(ctx));
    if (mode == 1) {
      // the witnesses while the batch's dist arrays are resident
      wit.clear();
      i64 off = 0;
      for (i64 p = p0; p < p1; ++p) {
        const int32_t d = dsort[p];
        if (d < 1) continue;
        wit.push_back(HopsWitness{items[(size_t)(p - p0)].x, items[(size_t)(p - p0)].y, d,
                                  pairs[2 * order[p]], off});
        off += (i64)d + 1;
      }
      if (!wit.empty()) {
        if (wit.size() > (size_t)0x7fffffff)
          return fail(ctx, -ENOTSUP, "kano_hop_pairs: too many paths in one batch");
        KTRY(dalloc(ctx, h.items, sizeof(HopsWitness) * wit.size()));
        KTRY(dalloc(ctx, h.nodes, sizeof(int32_t) * (size_t)off));
        KCHK(hipMemcpyAsync(h.items.p, wit.data(), sizeof(HopsWitness) * wit.size(),
                            hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_hops_witness, dim3((unsigned)wit.size()), dim3(TPB), 0, ctx->stream,
                           P_<u64>(ctx->M), ctx->ldM, n, P_<int32_t>(h.dist),
                           P_<HopsWitness>(h.items), P_<int32_t>(h.nodes));
        KLAUNCH();
        KTRY(hops_batch_end(ctx, h));
        const size_t at = sorted_nodes.size();
        sorted_nodes.resize(at + (size_t)off);
        KCHK(hipMemcpyAsync(sorted_nodes.data() + at, h.nodes.p, sizeof(int32_t) * (size_t)off,
                            hipMemcpyDeviceToHost, ctx->stream));
        KTRY(sync(ctx));
      } else {
        KTRY(hops_batch_end(ctx, h));
      }
    } else {
      KTRY(hops_batch_end(ctx, h));
    }
  }
  for (i64 p = 0; p < Q; ++p) dist[order[p]] = dsort[p];
  if (mode == 1) {
    // pair q's path at the prefix sum of dist + 1 over the pairs before it
    std::vector<i64> offq((size_t)Q + 1, 0);
    for (i64 q = 0; q < Q; ++q) offq[q + 1] = offq[q] + (dist[q] >= 1 ? (i64)dist[q] + 1 : 0);
    ctx->hop_nodes.assign((size_t)offq[Q], 0);
    i64 at = 0;
    for (i64 p = 0; p < Q; ++p) {
      const i64 q = order[p], len = offq[q + 1] - offq[q];
      if (len) std::memcpy(ctx->hop_nodes.data() + offq[q], sorted_nodes.data() + at,
                           sizeof(int32_t) * (size_t)len);
      at += len;
    }
    ctx->hop_total = offq[Q];
    if (total) *total = offq[Q];
  }
  return 0;
}

int kano_hop_pairs_fetch(kano_ctx* ctx, int32_t* nodes) {
  if (!ctx) return -EINVAL;
  if (ctx->hop_total < 0)
    return fail(ctx, -EINVAL, "kano_hop_pairs_fetch: no paths (call kano_hop_pairs with mode 1)");
  if (ctx->hop_total > 0) {
    if (!nodes) return fail(ctx, -EINVAL, "kano_hop_pairs_fetch: nodes is NULL");
    std::memcpy(nodes, ctx->hop_nodes.data(), sizeof(int32_t) * (size_t)ctx->hop_total);
  }
  return 0;
}

int kano_hops_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->hops_ms;
  return 0;
}

}  // extern "C"

// ===========================================================================
// check_intents: user-declared allow / deny intents against the resident
// matrix (k_intent_*, kano_intents.hpp), every intent of a call at once.
// ===========================================================================
namespace {

constexpr i64 INTENT_MAX_WORDS = 1ll << 27;       // K * W of one call (1 GiB a side)
constexpr i64 INTENT_MAX_ROW_WORDS = 1ll << 38;   // sum of |S_k| * W of one call (2 TiB of reads)
constexpr i64 INTENT_LIST_BUDGET = 1ll << 30;     // bytes of source row lists of one pass

// the set bits of s (W words) among the rows [r0, r1)
i64 intent_held_count(const u64* s, i64 r0, i64 r1) {
  i64 c = 0;
  for (i64 w = r0 >> 6; w <= (r1 - 1) >> 6; ++w) {
    u64 v = s[w];
    if (w == r0 >> 6) v &= ~0ull << (r0 & 63);
    if (w == (r1 - 1) >> 6 && (r1 & 63)) v &= (1ull << (r1 & 63)) - 1ull;
    c += __builtin_popcountll(v);
  }
  return c;
}

// intent descriptors for counts ns[0 .. K): rows of an item, item and list offsets
void intent_descs(const i64* ns, const int32_t* flags, i64 K, std::vector<IntentDesc>& d) {
  d.resize((size_t)K + 1);
  i64 loff = 0, ioff = 0;
  for (i64 k = 0; k < K; ++k) {
    i64 run = std::max<i64>(INTENT_R, (ns[k] + INTENT_MAX_ITEMS - 1) / INTENT_MAX_ITEMS);
    run = (run + INTENT_RB - 1) / INTENT_RB * INTENT_RB;
    d[k] = IntentDesc{loff, ioff, (int32_t)run, flags[k]};
    loff += ns[k];
    ioff += (ns[k] + run - 1) / run;
  }
  d[K] = IntentDesc{loff, ioff, 0, 0};
}

unsigned intent_grid(const kano_ctx* ctx, i64 waves) {
  const i64 cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  return (unsigned)std::max<i64>(1, std::min<i64>(nblk(waves, TPB / 64), cus * 8));
}

}  // namespace

extern "C" {

int kano_intents(kano_ctx* ctx, int64_t K, const uint64_t* src, const uint64_t* dst,
                 const int32_t* flags, int64_t* out, int32_t* witness) {
  if (!ctx) return -EINVAL;
  if (K < 0) return fail(ctx, -EINVAL, "kano_intents: K < 0");
  if (K > 0 && (!src || !dst || !flags || !out || !witness))
    return fail(ctx, -EINVAL, "kano_intents: src, dst, flags, out or witness is NULL");
  KTRY(ensure_matrix(ctx));
  const i64 n = ctx->n, W = ctx->W, r0 = ctx->r0, r1 = ctx->r1;
  const i64 rl = std::max<i64>(0, rows_local(ctx));
  if (W > 0 && K > INTENT_MAX_WORDS / W)
    return fail(ctx, -ENOTSUP, "kano_intents: K * W = " + std::to_string(K) + " * " +
                                   std::to_string(W) + " words beyond " +
                                   std::to_string(INTENT_MAX_WORDS) + " (ask in slices of K)");
  for (i64 k = 0; k < K; ++k)
    if (flags[k] & ~(INTENT_ALLOW | INTENT_SELF))
      return fail(ctx, -EINVAL, "kano_intents: intent " + std::to_string(k) +
                                    " has unknown flag bits");
  const bool empty = K == 0 || n == 0 || W == 0 || rl == 0;
  // the held sources of every intent: the row reads of the call, known before
  // anything is launched
  const u64* S = reinterpret_cast<const u64*>(src);
  std::vector<i64> ns((size_t)K, 0);
  i64 rows_total = 0;
  if (!empty)
    for (i64 k = 0; k < K; ++k) {
      ns[k] = intent_held_count(S + k * W, r0, r1);
      rows_total += ns[k];
    }
  if (!empty && rows_total > INTENT_MAX_ROW_WORDS / W)
    return fail(ctx, -ENOTSUP, "kano_intents: " + std::to_string(rows_total) +
                                   " source rows of " + std::to_string(W) + " words beyond " +
                                   std::to_string(INTENT_MAX_ROW_WORDS) +
                                   " row words in one call (narrow the selectors or split the call)");
  for (i64 k = 0; k < K; ++k) {
    std::memset(out + 6 * k, 0, sizeof(int64_t) * 6);
    witness[2 * k] = witness[2 * k + 1] = -1;
  }
  ctx->intents_ms = 0.f;
  KTRY(sync(ctx));
  if (empty) return 0;

  // passes over the intents: the row lists of one pass within the budget
  std::vector<i64> pass{0};
  {
    const i64 cap = INTENT_LIST_BUDGET / (i64)sizeof(int32_t);
    i64 rows = 0;
    for (i64 k = 0; k < K; ++k) {
      if (rows > 0 && rows + ns[k] > cap) {
        pass.push_back(k);
        rows = 0;
      }
      rows += ns[k];
    }
    pass.push_back(K);
  }
  const i64 npass = (i64)pass.size() - 1;
  std::vector<IntentDesc> descs, one;
  std::vector<i64> dbase((size_t)npass);
  i64 max_rows = 0;
  for (i64 p = 0; p < npass; ++p) {
    const i64 k0 = pass[p], Kp = pass[p + 1] - k0;
    intent_descs(ns.data() + k0, flags + k0, Kp, one);
    dbase[p] = (i64)descs.size();
    descs.insert(descs.end(), one.begin(), one.end());
    max_rows = std::max(max_rows, one[Kp].loff);
  }

  // the call's own buffers
  std::vector<u64> hres((size_t)K * INTENT_RES);
  DBuf sd, list, dd, res;
  const size_t b_set = sizeof(u64) * (size_t)K * (size_t)W;
  KTRY(dalloc(ctx, sd, 2 * b_set));
  KTRY(dalloc(ctx, list, sizeof(int32_t) * (size_t)max_rows));
  KTRY(dalloc(ctx, dd, sizeof(IntentDesc) * descs.size()));
  KTRY(dalloc(ctx, res, sizeof(u64) * hres.size()));
  u64* src_d = P_<u64>(sd);
  u64* dst_d = src_d + (size_t)K * (size_t)W;
  KCHK(hipMemcpyAsync(src_d, src, b_set, hipMemcpyHostToDevice, ctx->stream));
  KCHK(hipMemcpyAsync(dst_d, dst, b_set, hipMemcpyHostToDevice, ctx->stream));
  KCHK(hipMemcpyAsync(dd.p, descs.data(), sizeof(IntentDesc) * descs.size(),
                      hipMemcpyHostToDevice, ctx->stream));
  // timing=1: the call's device time (the kernels, no copy)
  EventPair<> tev;
  if (ctx->stage_timing) KTRY(tev.start(ctx));
  for (i64 p = 0; p < npass; ++p) {
    const i64 k0 = pass[p], Kp = pass[p + 1] - k0;
    const IntentDesc* de = P_<IntentDesc>(dd) + dbase[p];
    const i64 nitems = descs[(size_t)(dbase[p] + Kp)].ioff;
    u64* rp = P_<u64>(res) + k0 * INTENT_RES;
    hipLaunchKernelGGL(k_intent_lists, dim3(intent_grid(ctx, Kp)), dim3(TPB), 0, ctx->stream,
                       src_d + k0 * W, dst_d + k0 * W, W, n, r0, r1, de, Kp,
                       P_<int32_t>(list), rp);
    KLAUNCH();
    if (nitems == 0) continue;
    hipLaunchKernelGGL(k_intent_rows, dim3(intent_grid(ctx, nitems)), dim3(TPB), 0, ctx->stream,
                       P_<u64>(ctx->M), ctx->ldM, r0, rl, W, (const u64*)(dst_d + k0 * W), de, Kp,
                       nitems, (const int32_t*)P_<int32_t>(list), rp);
    KLAUNCH();
  }
  KTRY(tev.stop(ctx, &ctx->intents_ms));
  KCHK(hipMemcpyAsync(hres.data(), res.p, sizeof(u64) * hres.size(), hipMemcpyDeviceToHost,
                      ctx->stream));
  KTRY(sync(ctx));
  for (i64 k = 0; k < K; ++k) {
    const u64* h = hres.data() + k * INTENT_RES;
    int64_t* o = out + 6 * k;
    const i64 nd = (i64)h[0], reach = (i64)h[2];
    const i64 pairs = ns[k] * nd - ((flags[k] & INTENT_SELF) ? 0 : (i64)h[1]);
    o[0] = ns[k];
    o[1] = nd;
    o[2] = pairs;
    o[3] = reach;
    o[4] = (flags[k] & INTENT_ALLOW) ? pairs - reach : reach;
    o[5] = (i64)h[3];
    if (h[4] != ~0ull) {
      witness[2 * k] = (int32_t)(h[4] >> 32);
      witness[2 * k + 1] = (int32_t)(h[4] & 0xffffffffull);
    }
  }
  return 0;
}

int kano_intent_pairs(kano_ctx* ctx, const uint64_t* src, const uint64_t* dst, int32_t flags,
                      int64_t limit, int64_t* count, int32_t* pairs) {
  if (!ctx) return -EINVAL;
  if (!count) return fail(ctx, -EINVAL, "kano_intent_pairs: count is NULL");
  *count = 0;
  if (!src || !dst) return fail(ctx, -EINVAL, "kano_intent_pairs: src or dst is NULL");
  if (flags & ~(INTENT_ALLOW | INTENT_SELF))
    return fail(ctx, -EINVAL, "kano_intent_pairs: unknown flag bits");
  if (limit < 0) return fail(ctx, -EINVAL, "kano_intent_pairs: limit < 0");
  KTRY(ensure_matrix(ctx));
  KTRY(sync(ctx));
  const i64 n = ctx->n, W = ctx->W, r0 = ctx->r0, r1 = ctx->r1;
  const i64 rl = rows_local(ctx);
  if (n == 0 || W == 0 || rl <= 0) return 0;
  const i64 ns = intent_held_count(reinterpret_cast<const u64*>(src), r0, r1);
  if (ns == 0) return 0;
  if (ns > (i64)DIFF_SCAN_TILES * SCAN_TILE)
    return fail(ctx, -ENOTSUP, "kano_intent_pairs: more than " +
                                   std::to_string((i64)DIFF_SCAN_TILES * SCAN_TILE) +
                                   " source rows in one call");
  std::vector<IntentDesc> desc;
  intent_descs(&ns, &flags, 1, desc);
  DBuf sd, list, dd, res, cnt, off, outb;
  KTRY(dalloc(ctx, sd, sizeof(u64) * 2 * (size_t)W));
  KTRY(dalloc(ctx, list, sizeof(int32_t) * (size_t)ns));
  KTRY(dalloc(ctx, dd, sizeof(IntentDesc) * 2));
  KTRY(dalloc(ctx, res, sizeof(u64) * INTENT_RES));
  KTRY(dalloc(ctx, cnt, sizeof(int32_t) * (size_t)ns));
  KTRY(dalloc(ctx, off, sizeof(i64) * (size_t)(ns + 1 + 2 * DIFF_SCAN_TILES + 1)));
  u64* src_d = P_<u64>(sd);
  u64* dst_d = src_d + W;
  KCHK(hipMemcpyAsync(src_d, src, sizeof(u64) * W, hipMemcpyHostToDevice, ctx->stream));
  KCHK(hipMemcpyAsync(dst_d, dst, sizeof(u64) * W, hipMemcpyHostToDevice, ctx->stream));
  KCHK(hipMemcpyAsync(dd.p, desc.data(), sizeof(IntentDesc) * 2, hipMemcpyHostToDevice,
                      ctx->stream));
  hipLaunchKernelGGL(k_intent_lists, dim3(1), dim3(TPB), 0, ctx->stream, src_d, dst_d, W, n, r0,
                     r1, (const IntentDesc*)P_<IntentDesc>(dd), (i64)1, P_<int32_t>(list),
                     P_<u64>(res));
  KLAUNCH();
  // pass one: the violations of every source row, then their offsets
  hipLaunchKernelGGL(k_intent_row_counts, dim3(intent_grid(ctx, ns)), dim3(TPB), 0, ctx->stream,
                     P_<u64>(ctx->M), ctx->ldM, r0, rl, W, (const u64*)dst_d, (int)flags,
                     (const int32_t*)P_<int32_t>(list), ns, P_<int32_t>(cnt));
  KLAUNCH();
  i64* offp = P_<i64>(off);
  KTRY(diff_offsets_launch(ctx, P_<int32_t>(cnt), ns, offp + ns + 1, offp));
  i64 total = 0;
  KCHK(hipMemcpyAsync(&total, offp + ns, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
  KTRY(sync(ctx));
  *count = total;
  if (!pairs || total == 0) return 0;
  if (total > limit)
    return fail(ctx, -ENOSPC, "kano_intent_pairs: " + std::to_string(total) +
                                  " pairs, room for " + std::to_string(limit));
  // pass two: the pairs in order
  KTRY(dalloc(ctx, outb, sizeof(int32_t) * 2 * (size_t)total));
  hipLaunchKernelGGL(k_intent_emit, dim3(intent_grid(ctx, ns)), dim3(TPB), 0, ctx->stream,
                     P_<u64>(ctx->M), ctx->ldM, r0, rl, W, (const u64*)dst_d, (int)flags,
                     (const int32_t*)P_<int32_t>(list), ns, (const i64*)offp, total,
                     P_<int32_t>(outb));
  KLAUNCH();
  KCHK(hipMemcpyAsync(pairs, outb.p, sizeof(int32_t) * 2 * (size_t)total, hipMemcpyDeviceToHost,
                      ctx->stream));
  return sync(ctx);
}

int kano_intents_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->intents_ms;
  return 0;
}

}  // extern "C"

// ===========================================================================
// The derived matrices (port_matrix's kano_policy_subset, kano_verdict_matrix):
// the held rows of dst written from src's resident tables.  The matrix of the
// source is not read and nothing of the source is written.  Class-level rows
// first (k_ports_class / k_verdict_class), expanded to the member rows by
// kano_path's last step (path_expand_rows), then the added policies' rows.
// ===========================================================================
namespace {

const char* const NO_POLICIES =
    ": the matrix has no policies (an empty, copied, loaded, path or edge matrix holds rows only)";

struct Geometry {
  i64 P, A;                 // the source's build and added policies
  i64 n, W, ldM, r0, rl;    // the destination's rows (the source's, checked)
  i64 U, Ua, ldC;           // the source's row and column classes
  bool classes;             // the build's part exists
};

// The arguments checked (missing: what of the call's own arrays is NULL, or
// null), both contexts ready, the source's classes complete; g filled.
int derived_begin(kano_ctx* src, kano_ctx* dst, const char* what, i64 nids, const char* missing,
                  Geometry& g) {
  if (!src || !dst) return -EINVAL;
  const std::string w(what);
  if (src == dst) return fail(dst, -EINVAL, w + ": the destination must be another context");
  if (src->device != dst->device) return fail(dst, -EINVAL, w + ": contexts on two devices");
  kano_ctx* ctx = dst;
  KCHK(hipSetDevice(dst->device));
  int rc = ensure_built(src);
  if (rc) return fail(dst, rc, w + ": source: " + src->err);
  if (src->lists_mode)
    return fail(dst, -EINVAL, w + ": the source holds policy lists, not a matrix");
  g.P = src->P;
  g.A = src->inc_A;
  if (g.P == 0 && g.A == 0) return fail(dst, -EINVAL, w + NO_POLICIES);
  if (nids != g.P + g.A)
    return fail(dst, -EINVAL, w + ": nids = " + std::to_string(nids) + ", the source has " +
                                  std::to_string(g.P + g.A) + " engine ids");
  if (missing) return fail(dst, -EINVAL, w + ": " + missing);
  KTRY(ensure_matrix(dst));
  if (dst->n != src->n || dst->r0 != src->r0 || dst->r1 != src->r1 || dst->ldM != src->ldM)
    return fail(dst, -EINVAL,
                w + ": the destination must hold the same rows of a matrix of the same size");
  rc = sync(src);   // the source's classes are complete
  if (rc) return fail(dst, rc, w + ": source: " + src->err);
  g.n = dst->n, g.W = dst->W, g.ldM = dst->ldM, g.r0 = dst->r0, g.rl = rows_local(dst);
  g.U = src->rc.U, g.Ua = src->cc.U, g.ldC = src->ldC;
  g.classes = g.P > 0 && g.U > 0 && g.Ua > 0;
  if (g.classes && (g.U + 15) / 16 > 65535)   // (path_expand_rows' grid)
    return fail(dst, -ENOTSUP, w + ": more than 1,048,560 row classes");
  return 0;
}

// the class kernels' shape: wl lanes a class row (the smallest power of two
// covering ldC, at most TPB) and at most cap blocks (8 per CU)
void derived_shape(const kano_ctx* ctx, i64 ldC, int* wl, i64* cap) {
  *wl = 1;
  while (*wl < TPB && *wl < ldC) *wl <<= 1;
  *cap = (ctx->num_cus > 0 ? ctx->num_cus : 256) * (i64)8;
}

// the tail of a call that began to write dst's rows, however it ends: the rows
// are new, the column results stale
struct RowsEdited {
  kano_ctx* dst;
  ~RowsEdited() {
    dst->cols_valid = false;
    dst->rows_dirty = true;
    dst->user_edited = true;
  }
};

// The keys of the engine ids (kano_verdict.hpp: rank * 2 + action, VD_DEAD
// for a removed id) from the raw priorities: the rank is the position among
// the distinct priorities of the alive ids, ascending; levels[rank] gives the
// priority back.  tally = [alive allow, alive deny].
int verdict_keys(kano_ctx* src, kano_ctx* ctx, const char* what, i64 nids, const int32_t* prio,
                 const uint8_t* action, std::vector<uint32_t>& key, std::vector<int32_t>& levels,
                 i64 tally[2]) {
  for (i64 p = 0; p < nids; ++p)
    if (action[p] > 1)
      return fail(ctx, -EINVAL, std::string(what) + ": action " + std::to_string(p) + " is " +
                                    std::to_string((int)action[p]) + " (0 allow, 1 deny)");
  levels.clear();
  for (i64 p = 0; p < nids; ++p)
    if (!src->dead[p]) levels.push_back(prio[p]);
  std::sort(levels.begin(), levels.end());
  levels.erase(std::unique(levels.begin(), levels.end()), levels.end());
  key.assign((size_t)nids, kano::VD_DEAD);
  tally[0] = tally[1] = 0;
  for (i64 p = 0; p < nids; ++p) {
    if (src->dead[p]) continue;
    const uint32_t rank =
        (uint32_t)(std::lower_bound(levels.begin(), levels.end(), prio[p]) - levels.begin());
    key[p] = rank * 2u + action[p];
    ++tally[action[p]];
  }
  return 0;
}

}  // namespace

extern "C" {

// port_matrix: the matrix of a subset of the policies (k_ports_*, kano_ports.hpp)
int kano_policy_subset(kano_ctx* src, kano_ctx* dst, int64_t nids, const uint8_t* keep,
                       int64_t* info) {
  Geometry g;
  KTRY(derived_begin(src, dst, "kano_policy_subset", nids, keep ? nullptr : "keep is NULL", g));
  kano_ctx* ctx = dst;
  // use[p]: alive and kept
  std::vector<uint8_t> use((size_t)nids);
  i64 kept_build = 0, kept_added = 0;
  for (i64 p = 0; p < nids; ++p) {
    use[p] = keep[p] && !src->dead[p];
    (p < g.P ? kept_build : kept_added) += use[p];
  }
  src->subset_ms = dst->subset_ms = 0.f;
  unsigned kept_classes = 0;
  if (g.n > 0 && g.rl > 0) {
    RowsEdited edited{dst};
    DBuf used, mcs, rt16, cnt;
    KTRY(dalloc(ctx, used, (size_t)nids));
    KTRY(dalloc(ctx, cnt, sizeof(unsigned)));
    KCHK(hipMemcpyAsync(used.p, use.data(), (size_t)nids, hipMemcpyHostToDevice, ctx->stream));
    if (g.classes) {
      KTRY(dalloc(ctx, mcs, sizeof(u64) * (size_t)(g.U * g.ldC)));
      KTRY(dalloc(ctx, rt16, sizeof(uint16_t) * (size_t)(((g.U + 15) / 16) * g.Ua)));
    }
    EventPair<> tev;
    if (src->stage_timing || dst->stage_timing) KTRY(tev.start(ctx));
    KCHK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned), ctx->stream));
    const uint8_t* use_d = P_<uint8_t>(used);
    if (g.classes) {
      int wl;
      i64 cap;
      derived_shape(ctx, g.ldC, &wl, &cap);
      hipLaunchKernelGGL(k_ports_class, dim3((unsigned)std::min<i64>(g.U, cap)), dim3(TPB), 0,
                         ctx->stream, g.U, (const i64*)P_<i64>(src->soffc),
                         (const int32_t*)P_<int32_t>(src->slist), use_d,
                         (const u64*)P_<u64>(src->AC), g.ldC, wl, P_<u64>(mcs),
                         P_<unsigned>(cnt));
      KLAUNCH();
      // the class rows to the member rows: every word of every held row
      KTRY(path_expand_rows(ctx, src, P_<u64>(mcs), g.ldC, g.U, g.Ua, rt16.p));
    }
    // the added policies OR-ed in; without classes the rows start as zeros
    if (!g.classes || kept_added > 0) {
      hipLaunchKernelGGL(k_ports_rows, dim3(nblk(g.rl * (g.ldM / 2))), dim3(TPB), 0, ctx->stream,
                         g.classes ? 1 : 0, use_d, g.P, (const u64*)P_<u64>(src->asel),
                         (const u64*)P_<u64>(src->aalw), g.W, kept_added > 0 ? g.A : 0, g.r0,
                         g.rl, g.ldM, P_<u64>(dst->M));
      KLAUNCH();
    }
    KTRY(tev.stop(ctx, &dst->subset_ms));
    src->subset_ms = dst->subset_ms;
    KCHK(hipMemcpyAsync(&kept_classes, cnt.p, sizeof(unsigned), hipMemcpyDeviceToHost,
                        ctx->stream));
    KTRY(sync(ctx));
  }
  if (info) {
    info[0] = kept_build;
    info[1] = kept_added;
    info[2] = (int64_t)kept_classes;
  }
  return 0;
}

// pair_ports: the pairs' port masks (k_pmask_*, kano_ports.hpp)
int kano_pair_masks(kano_ctx* ctx, int64_t Q, const int32_t* pairs, int64_t nids, int32_t KW,
                    const uint64_t* pmask, uint64_t* out) {
  KTRY(ensure_built(ctx));
  if (ctx->lists_mode)
    return fail(ctx, -EINVAL, "kano_pair_masks: the context holds policy lists, not a matrix");
  const i64 P = ctx->P, A = ctx->inc_A;
  if (P == 0 && A == 0) return fail(ctx, -EINVAL, std::string("kano_pair_masks") + NO_POLICIES);
  if (Q < 0 || KW <= 0) return fail(ctx, -EINVAL, "kano_pair_masks: Q < 0 or KW <= 0");
  if (nids != P + A)
    return fail(ctx, -EINVAL, "kano_pair_masks: nids = " + std::to_string(nids) + ", the context has " +
                                  std::to_string(P + A) + " engine ids");
  if (!pmask || (Q > 0 && (!pairs || !out)))
    return fail(ctx, -EINVAL, "kano_pair_masks: pairs, pmask or out is NULL");
  KTRY(pairs_check(ctx, "kano_pair_masks", Q, pairs, ctx->n, ctx->n));
  ctx->pmask_ms = 0.f;
  if (Q == 0) return 0;
  const size_t b_out = sizeof(u64) * (size_t)Q * (size_t)KW;
  if (rows_local(ctx) <= 0) {
    std::memset(out, 0, b_out);
    return 0;
  }
  const bool any_dead = std::find(ctx->dead.begin(), ctx->dead.end(), 1) != ctx->dead.end();
  DBuf pr, pm, dd, od;
  const size_t b_pm = sizeof(u64) * (size_t)nids * (size_t)KW;
  KTRY(dalloc(ctx, pr, sizeof(int32_t) * 2 * (size_t)Q));
  KTRY(dalloc(ctx, pm, b_pm));
  KTRY(dalloc(ctx, od, b_out));
  if (any_dead) KTRY(dalloc(ctx, dd, (size_t)nids));
  KCHK(hipMemcpyAsync(pr.p, pairs, sizeof(int32_t) * 2 * (size_t)Q, hipMemcpyHostToDevice,
                      ctx->stream));
  KCHK(hipMemcpyAsync(pm.p, pmask, b_pm, hipMemcpyHostToDevice, ctx->stream));
  if (any_dead)
    KCHK(hipMemcpyAsync(dd.p, ctx->dead.data(), (size_t)nids, hipMemcpyHostToDevice,
                        ctx->stream));
  PairMaskArgs a{};
  KTRY(pair_tables(ctx, "kano_pair_masks", P_<int32_t>(pr), Q, a.t));
  a.t.dead = any_dead ? P_<uint8_t>(dd) : nullptr;
  a.pmask = P_<u64>(pm);
  a.KW = KW;
  a.out = P_<u64>(od);
  bool wave;
  unsigned grid;
  pair_shape(ctx, a.t, ctx->pmask_form, ctx->pmask_grid, Q, &wave, &grid);
  EventPair<> tev;
  if (ctx->stage_timing) KTRY(tev.start(ctx));
  if (wave) hipLaunchKernelGGL(k_pmask_wave, dim3(grid), dim3(TPB), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_pmask_lane, dim3(grid), dim3(TPB), 0, ctx->stream, a);
  KLAUNCH();
  KTRY(tev.stop(ctx, &ctx->pmask_ms));
  KCHK(hipMemcpyAsync(out, od.p, b_out, hipMemcpyDeviceToHost, ctx->stream));
  return sync(ctx);
}

int kano_policy_subset_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->subset_ms;
  return 0;
}

int kano_pair_masks_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->pmask_ms;
  return 0;
}

// verdict_matrix: deny rules and priorities (k_verdict_*, kano_verdict.hpp;
// the rows of the added policies are marked by k_inc_mark)
int kano_verdict_matrix(kano_ctx* src, kano_ctx* dst, int64_t nids, const int32_t* prio,
                        const uint8_t* action, int64_t* info) {
  Geometry g;
  KTRY(derived_begin(src, dst, "kano_verdict_matrix", nids,
                     prio && action ? nullptr : "prio or action is NULL", g));
  kano_ctx* ctx = dst;
  std::vector<uint32_t> key;
  std::vector<int32_t> levels;
  i64 tally[2];
  KTRY(verdict_keys(src, dst, "kano_verdict_matrix", nids, prio, action, key, levels, tally));
  // aflag[P + t]: added policy t is alive (k_inc_mark's flags; the build's stay 0)
  std::vector<uint8_t> aflag((size_t)nids, 0);
  i64 alive_added = 0;
  for (i64 t = 0; t < g.A; ++t) alive_added += aflag[g.P + t] = !src->dead[g.P + t];
  src->verdict_ms = dst->verdict_ms = 0.f;
  unsigned deny_classes = 0;
  if (g.n > 0 && g.rl > 0) {
    RowsEdited edited{dst};
    DBuf keyd, flagd, cnt, pk, olist, okey, ocnt, vc, rt16, mrows;
    KTRY(dalloc(ctx, keyd, sizeof(uint32_t) * (size_t)nids));
    KTRY(dalloc(ctx, cnt, 2 * sizeof(u64)));   // [0]: the marked rows, [1]: the deny classes
    KCHK(hipMemcpyAsync(keyd.p, key.data(), sizeof(uint32_t) * (size_t)nids, hipMemcpyHostToDevice,
                        ctx->stream));
    if (g.classes) {
      const size_t nnz = (size_t)std::max<i64>(1, src->nnz_sel);
      KTRY(dalloc(ctx, pk, sizeof(u64) * nnz));
      KTRY(dalloc(ctx, olist, sizeof(int32_t) * nnz));
      KTRY(dalloc(ctx, okey, sizeof(uint32_t) * nnz));
      KTRY(dalloc(ctx, ocnt, sizeof(int32_t) * (size_t)g.U));
      KTRY(dalloc(ctx, vc, sizeof(u64) * (size_t)(g.U * g.ldC)));
      KTRY(dalloc(ctx, rt16, sizeof(uint16_t) * (size_t)(((g.U + 15) / 16) * g.Ua)));
    }
    if (alive_added > 0) {
      KTRY(dalloc(ctx, flagd, (size_t)nids));
      KTRY(dalloc(ctx, mrows, sizeof(int32_t) * (size_t)g.rl));
      KCHK(hipMemcpyAsync(flagd.p, aflag.data(), (size_t)nids, hipMemcpyHostToDevice, ctx->stream));
    }
    EventPair<> tev;
    if (src->stage_timing || dst->stage_timing) KTRY(tev.start(ctx));
    KCHK(hipMemsetAsync(cnt.p, 0, 2 * sizeof(u64), ctx->stream));
    const uint32_t* key_d = P_<uint32_t>(keyd);
    if (g.classes) {
      int wl;
      i64 cap;
      derived_shape(ctx, g.ldC, &wl, &cap);
      hipLaunchKernelGGL(k_verdict_order, dim3((unsigned)std::min<i64>(g.U, cap)), dim3(TPB), 0,
                         ctx->stream, g.U, (const i64*)P_<i64>(src->soffc),
                         (const int32_t*)P_<int32_t>(src->slist), key_d, P_<u64>(pk),
                         P_<int32_t>(olist), P_<uint32_t>(okey), P_<int32_t>(ocnt),
                         reinterpret_cast<unsigned*>(P_<u64>(cnt) + 1));
      KLAUNCH();
      const i64 cpb = TPB / wl;
      hipLaunchKernelGGL(k_verdict_class, dim3((unsigned)std::min<i64>((g.U + cpb - 1) / cpb, cap)),
                         dim3(TPB), 0, ctx->stream, g.U, (const i64*)P_<i64>(src->soffc),
                         (const int32_t*)P_<int32_t>(olist), (const uint32_t*)P_<uint32_t>(okey),
                         (const int32_t*)P_<int32_t>(ocnt), (const u64*)P_<u64>(src->AC), g.ldC,
                         wl, P_<u64>(vc));
      KLAUNCH();
      // the class rows to the member rows: every word of every held row
      KTRY(path_expand_rows(ctx, src, P_<u64>(vc), g.ldC, g.U, g.Ua, rt16.p));
    } else {
      // a build without policies has no classes: the rows start as zeros
      KCHK(hipMemsetAsync(dst->M.p, 0, sizeof(u64) * (size_t)(g.rl * g.ldM), ctx->stream));
    }
    if (alive_added > 0) {
      // the rows an alive added policy selects, resolved bit by bit
      hipLaunchKernelGGL(k_inc_mark, dim3(nblk(g.rl)), dim3(TPB), 0, ctx->stream,
                         (const int32_t*)nullptr, (const i64*)nullptr, (const int32_t*)nullptr,
                         (const uint8_t*)P_<uint8_t>(flagd), g.P, (const u64*)P_<u64>(src->asel),
                         g.W, g.A, g.r0, g.rl, P_<int32_t>(mrows), P_<u64>(cnt));
      KLAUNCH();
      u64 nrows = 0;
      KCHK(hipMemcpyAsync(&nrows, cnt.p, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
      KTRY(sync(ctx));
      if (nrows > (u64)g.rl)
        return fail(ctx, -EIO, "kano_verdict_matrix: row count out of range");
      if (nrows > 0) {
        VerdictArgs a{};
        const int rc = pair_tables(src, "kano_verdict_matrix", nullptr, 0, a.t);
        if (rc) return fail(dst, rc, src->err);
        if (!g.classes) a.t.rcls = nullptr;
        a.t.key = key_d;
        hipLaunchKernelGGL(k_verdict_rows, dim3((unsigned)nrows), dim3(TPB), 0, ctx->stream, a,
                           (const int32_t*)P_<int32_t>(mrows), g.n, P_<u64>(dst->M), g.ldM);
        KLAUNCH();
      }
    }
    KTRY(tev.stop(ctx, &dst->verdict_ms));
    src->verdict_ms = dst->verdict_ms;
    KCHK(hipMemcpyAsync(&deny_classes, P_<u64>(cnt) + 1, sizeof(unsigned), hipMemcpyDeviceToHost,
                        ctx->stream));
    KTRY(sync(ctx));
  }
  if (info) {
    info[0] = tally[0];
    info[1] = tally[1];
    info[2] = (int64_t)levels.size();
    info[3] = (int64_t)deny_classes;
  }
  return 0;
}

// pair_verdicts: the pairs' verdicts and deciders (k_verdict_lane / k_verdict_wave)
int kano_pair_verdicts(kano_ctx* ctx, int64_t Q, const int32_t* pairs, int64_t nids,
                       const int32_t* prio, const uint8_t* action, uint8_t* verdict,
                       int32_t* decided_prio, int32_t* decider, int64_t* counts) {
  KTRY(ensure_built(ctx));
  if (ctx->lists_mode)
    return fail(ctx, -EINVAL, "kano_pair_verdicts: the context holds policy lists, not a matrix");
  const i64 P = ctx->P, A = ctx->inc_A;
  if (P == 0 && A == 0) return fail(ctx, -EINVAL, std::string("kano_pair_verdicts") + NO_POLICIES);
  if (Q < 0) return fail(ctx, -EINVAL, "kano_pair_verdicts: Q < 0");
  if (nids != P + A)
    return fail(ctx, -EINVAL, "kano_pair_verdicts: nids = " + std::to_string(nids) +
                                  ", the context has " + std::to_string(P + A) + " engine ids");
  if (!prio || !action || (Q > 0 && (!pairs || !verdict)))
    return fail(ctx, -EINVAL, "kano_pair_verdicts: pairs, prio, action or verdict is NULL");
  std::vector<uint32_t> key;
  std::vector<int32_t> levels;
  i64 tally[2];
  KTRY(verdict_keys(ctx, ctx, "kano_pair_verdicts", nids, prio, action, key, levels, tally));
  KTRY(pairs_check(ctx, "kano_pair_verdicts", Q, pairs, ctx->n, ctx->n));
  ctx->pverdict_ms = 0.f;
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  if (Q == 0) return 0;
  if (rows_local(ctx) <= 0) {
    std::memset(verdict, 0, (size_t)Q);
    if (decided_prio) std::memset(decided_prio, 0, sizeof(int32_t) * (size_t)Q);
    if (decider) std::fill(decider, decider + Q, -1);
    return 0;
  }
  std::vector<uint32_t> hkey((size_t)Q);
  std::vector<int32_t> hid((size_t)Q);
  DBuf pr, kd, ok, oi;
  KTRY(dalloc(ctx, pr, sizeof(int32_t) * 2 * (size_t)Q));
  KTRY(dalloc(ctx, kd, sizeof(uint32_t) * (size_t)nids));
  KTRY(dalloc(ctx, ok, sizeof(uint32_t) * (size_t)Q));
  KTRY(dalloc(ctx, oi, sizeof(int32_t) * (size_t)Q));
  KCHK(hipMemcpyAsync(pr.p, pairs, sizeof(int32_t) * 2 * (size_t)Q, hipMemcpyHostToDevice,
                      ctx->stream));
  KCHK(hipMemcpyAsync(kd.p, key.data(), sizeof(uint32_t) * (size_t)nids, hipMemcpyHostToDevice,
                      ctx->stream));
  VerdictArgs a{};
  KTRY(pair_tables(ctx, "kano_pair_verdicts", P_<int32_t>(pr), Q, a.t));
  a.t.key = P_<uint32_t>(kd);
  a.out_key = P_<uint32_t>(ok);
  a.out_id = P_<int32_t>(oi);
  bool wave;
  unsigned grid;
  pair_shape(ctx, a.t, ctx->verdict_form, ctx->verdict_grid, Q, &wave, &grid);
  EventPair<> tev;
  if (ctx->stage_timing) KTRY(tev.start(ctx));
  if (wave) hipLaunchKernelGGL(k_verdict_wave, dim3(grid), dim3(TPB), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_verdict_lane, dim3(grid), dim3(TPB), 0, ctx->stream, a);
  KLAUNCH();
  KTRY(tev.stop(ctx, &ctx->pverdict_ms));
  KCHK(hipMemcpyAsync(hkey.data(), ok.p, sizeof(uint32_t) * (size_t)Q, hipMemcpyDeviceToHost,
                      ctx->stream));
  KCHK(hipMemcpyAsync(hid.data(), oi.p, sizeof(int32_t) * (size_t)Q, hipMemcpyDeviceToHost,
                      ctx->stream));
  KTRY(sync(ctx));
  // the keys back to verdicts and raw priorities; a pair whose i this context
  // does not hold matched nothing and adds to no count
  for (i64 q = 0; q < Q; ++q) {
    const bool own = pairs[2 * q] >= ctx->r0 && pairs[2 * q] < ctx->r1;
    const bool hit = hkey[q] != VD_NONE;
    const int v = !hit ? 0 : (hkey[q] & 1u) ? 2 : 1;
    verdict[q] = (uint8_t)v;
    if (decided_prio) decided_prio[q] = hit ? levels[hkey[q] >> 1] : 0;
    if (decider) decider[q] = hit ? hid[q] : -1;
    if (counts && own) ++counts[v];
  }
  return 0;
}

int kano_verdict_matrix_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->verdict_ms;
  return 0;
}

int kano_pair_verdicts_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->pverdict_ms;
  return 0;
}

}  // extern "C"

// ===========================================================================
// k8s.connectivity: the Kubernetes reading of NetworkPolicies from an egress
// and an ingress class-level build (k_conn_*, kano_k8s_conn.hpp).  Only the
// sources' class tables are read (soffc / slist, AC, Mc, the pods' class ids);
// their matrices are neither read nor written.
// ===========================================================================
namespace {

// a source: a full, unedited class-level build.  Errors go to err_ctx.
int conn_source(kano_ctx* s, kano_ctx* err_ctx, const char* what) {
  const std::string w(what);
  const int rc = ensure_built(s);
  if (rc) return s == err_ctx ? rc : fail(err_ctx, rc, w + ": source: " + s->err);
  if (s->lists_mode) return fail(err_ctx, -ENOTSUP, w + ": a source holds policy lists");
  if (s->r0 != 0 || s->r1 != s->n)
    return fail(err_ctx, -ENOTSUP, w + ": a source holds a row shard (needs every row)");
  if (s->inc_A > 0 || std::find(s->dead.begin(), s->dead.end(), 1) != s->dead.end())
    return fail(err_ctx, -ENOTSUP, w + ": a source holds added or removed policies");
  if (s->rows_dirty || s->user_edited)
    return fail(err_ctx, -ENOTSUP, w + ": a source holds edited rows");
  return 0;
}

// without policies a build has no classes: that direction constrains nothing
bool conn_classes(const kano_ctx* s) { return s->P > 0 && s->rc.U > 0 && s->cc.U > 0; }

// The write of dst's held rows from the two class-level tables Re (egress) and
// Ri (ingress; transposed here), shared by kano_k8s_conn and
// kano_k8s_conn_tiers: alloc takes the call's buffers (before the timed
// stretch) and picks the form, launch enqueues the transpose and the rows.
struct ConnWrite {
  DBuf ti, xr;
  bool stream = false;

  int alloc(kano_ctx* eg, kano_ctx* in, kano_ctx* dst, int flags, bool hasE, bool hasI) {
    kano_ctx* ctx = dst;
    const i64 Ue = eg->rc.U, Ui = in->rc.U, Xi = in->cc.U, KWi = (Ui + 63) / 64;
    const i64 rl = rows_local(dst);
    if (hasI) KTRY(dalloc(ctx, ti, sizeof(u64) * (size_t)(Xi * KWi)));
    // the streamed form when the class rows are few beside the held rows (as
    // kano_k8s_edge picks it), or as the flags force
    const i64 Us = (hasE ? Ue : 0) + (hasI ? Xi : 0);
    // (its class-row expansions' grids hold at most 65535 * 64 class rows a
    // table: beyond that the direct form, whatever the flags say)
    const i64 xmax = (i64)65535 * K8S_XR;
    stream = Us > 0 && !(flags & KANO_K8S_CONN_DIRECT) && (!hasE || Ue <= xmax) &&
             (!hasI || Xi <= xmax) &&
             ((flags & KANO_K8S_CONN_STREAM) || Us <= std::max<i64>(rl / 2, 1));
    if (stream) KTRY(dalloc(ctx, xr, sizeof(u64) * (size_t)(Us * dst->ldM)));
    return 0;
  }

  int launch(kano_ctx* eg, kano_ctx* in, kano_ctx* dst, int flags, bool hasE, bool hasI,
             const u64* re, const u64* ri) {
    kano_ctx* ctx = dst;
    const i64 n = dst->n, W = dst->W, ldM = dst->ldM, r0 = dst->r0, rl = rows_local(dst);
    const i64 Ue = eg->rc.U, ldCe = eg->ldC, Ui = in->rc.U, Xi = in->cc.U, ldCi = in->ldC;
    const i64 KWi = (Ui + 63) / 64;
    if (hasI) {
      const i64 CGi = ((Xi + 63) / 64 + 15) / 16;
      hipLaunchKernelGGL(k_k8s_transpose, dim3(nblk(KWi * CGi, TPB / 64)), dim3(TPB), 0,
                         ctx->stream, ri, ldCi, Ui, KWi, CGi, Xi, P_<u64>(ti), KWi);
      KLAUNCH();
    }
    const int self = (flags & KANO_K8S_CONN_SELF) ? 1 : 0;
    const int32_t* rce = P_<int32_t>(eg->rc.cls);
    const int32_t* cce = P_<int32_t>(eg->cc.cls);
    const int32_t* cci = P_<int32_t>(in->cc.cls);
    const int32_t* rci = P_<int32_t>(in->rc.cls);
    if (stream) {
      // the class rows of both tables expanded to pod words once (row r is
      // class r, the other table absent, no diagonal), then streamed to the
      // held rows (kernels picked through a pointer are launched by handle:
      // see launch_marked)
      u64* XE = hasE ? P_<u64>(xr) : nullptr;
      u64* XT = hasI ? P_<u64>(xr) + (hasE ? Ue : 0) * ldM : nullptr;
      const int32_t* const none = nullptr;
      if (hasE) {
        auto CONN_EXPAND = ldCe <= CONN_STAGE_W ? k_conn_expand<true> : k_conn_expand<false>;
        hipExtLaunchKernelGGL(CONN_EXPAND, dim3(nblk(ldM, K8S_XW), nblk(Ue, K8S_XR)), dim3(TPB), 0,
                              ctx->stream, nullptr, nullptr, 0, re, ldCe, none, cce,
                              (const u64*)nullptr, (i64)0, none, none, 0, (i64)0, Ue, n, W, XE,
                              ldM);
        KLAUNCH();
      }
      if (hasI) {
        auto CONN_EXPAND = KWi <= CONN_STAGE_W ? k_conn_expand<true> : k_conn_expand<false>;
        hipExtLaunchKernelGGL(CONN_EXPAND, dim3(nblk(ldM, K8S_XW), nblk(Xi, K8S_XR)), dim3(TPB), 0,
                              ctx->stream, nullptr, nullptr, 0, (const u64*)nullptr, (i64)0, none,
                              none, (const u64*)P_<u64>(ti), KWi, none, rci, 0, (i64)0, Xi, n, W,
                              XT, ldM);
        KLAUNCH();
      }
      hipLaunchKernelGGL(k_conn_rows, dim3(nblk(rl * (ldM / 2))), dim3(TPB), 0, ctx->stream,
                         (const u64*)XE, rce, (const u64*)XT, cci, self, r0, rl, ldM,
                         P_<u64>(dst->M));
      KLAUNCH();
    } else {
      // class rows of <= CONN_STAGE_W words together are staged in LDS by the expansion
      const bool stage = (hasE ? ldCe : 0) + (hasI ? KWi : 0) <= CONN_STAGE_W;
      auto CONN_EXPAND = stage ? k_conn_expand<true> : k_conn_expand<false>;
      hipExtLaunchKernelGGL(CONN_EXPAND, dim3(nblk(ldM, K8S_XW), nblk(rl, K8S_XR)), dim3(TPB), 0,
                            ctx->stream, nullptr, nullptr, 0, hasE ? re : nullptr, ldCe, rce, cce,
                            (const u64*)(hasI ? P_<u64>(ti) : nullptr), KWi, cci, rci, self, r0,
                            rl, n, W, P_<u64>(dst->M), ldM);
      KLAUNCH();
    }
    return 0;
  }
};

// one value per engine id of each source
int conn_nids(const kano_ctx* eg, const kano_ctx* in, kano_ctx* err_ctx, const char* what,
              i64 nids_e, i64 nids_i) {
  if (nids_e != eg->P || nids_i != in->P)
    return fail(err_ctx, -EINVAL, std::string(what) + ": nids = " + std::to_string(nids_e) +
                                      " / " + std::to_string(nids_i) + ", the sources have " +
                                      std::to_string(eg->P) + " / " + std::to_string(in->P) +
                                      " engine ids");
  return 0;
}

// the sources' classes are complete
int conn_sync(kano_ctx* eg, kano_ctx* in, kano_ctx* err_ctx, const char* what) {
  for (kano_ctx* s : {eg, in}) {
    const int rc = sync(s);
    if (rc) return s == err_ctx ? rc : fail(err_ctx, rc, std::string(what) + ": source: " + s->err);
  }
  return 0;
}

// The shared preamble of kano_k8s_conn and kano_k8s_conn_tiers: the three
// contexts checked and ready, the sources' classes complete.  Errors on dst.
int conn_begin(kano_ctx* eg, kano_ctx* in, kano_ctx* dst, const char* what, i64 nids_e,
               i64 nids_i) {
  if (!eg || !in || !dst) return -EINVAL;
  const std::string w(what);
  if (dst == eg || dst == in)
    return fail(dst, -EINVAL, w + ": the destination must be another context");
  if (eg->device != dst->device || in->device != dst->device)
    return fail(dst, -EINVAL, w + ": contexts on two devices");
  kano_ctx* ctx = dst;
  KCHK(hipSetDevice(dst->device));
  KTRY(conn_source(eg, dst, what));
  KTRY(conn_source(in, dst, what));
  KTRY(ensure_matrix(dst));
  const i64 n = dst->n, rl = rows_local(dst);
  if (eg->n != n || in->n != n)
    return fail(dst, -EINVAL, w + ": the three contexts must hold the same pods");
  KTRY(conn_nids(eg, in, dst, what, nids_e, nids_i));
  if ((rl + K8S_XR - 1) / K8S_XR > 65535)   // (k_conn_expand's grid)
    return fail(dst, -ENOTSUP, w + ": more than 4,194,240 rows in one context");
  return conn_sync(eg, in, dst, what);
}

// The codes of kano_k8s_conn_tiers and kano_k8s_pair_verdicts checked ([0]
// egress, [1] ingress); live[side] = the codes that are not dropped.
int tier_codes_check(kano_ctx* err_ctx, const char* what, const i64 nids[2],
                     const uint32_t* const code[2], const uint32_t np[2], i64 live[2]) {
  const char* const side_name[2] = {"egress", "ingress"};
  live[0] = live[1] = 0;
  for (int side = 0; side < 2; ++side) {
    const std::string w = std::string(what) + ": " + side_name[side] + " ";
    if (nids[side] > 0 && !code[side]) return fail(err_ctx, -EINVAL, w + "codes are NULL");
    if (np[side] >= TIER_MAX_LEVEL)
      return fail(err_ctx, -EINVAL, w + "np_level is 2^30 or more");
    for (i64 p = 0; p < nids[side]; ++p) {
      const uint32_t c = code[side][p];
      if (c == TIER_DROPPED) continue;
      const uint32_t lv = c >> 2, act = c & 3u;
      const char* bad = act == TIER_PASS && lv >= np[side]      ? "passes at or above np_level"
                        : act == TIER_ISOLATE && lv != np[side] ? "only isolates off np_level"
                        : act == TIER_DENY && lv == np[side]    ? "denies at np_level"
                                                                : nullptr;
      if (bad)
        return fail(err_ctx, -EINVAL, w + "code " + std::to_string(p) + " (level " +
                                          std::to_string(lv) + ") " + bad);
      ++live[side];
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int kano_k8s_conn(kano_ctx* eg, kano_ctx* in, kano_ctx* dst, int flags, int64_t nids_e,
                  const uint8_t* keep_e, int64_t nids_i, const uint8_t* keep_i, int64_t* info) {
  KTRY(conn_begin(eg, in, dst, "kano_k8s_conn", nids_e, nids_i));
  kano_ctx* ctx = dst;
  const i64 n = dst->n, rl = rows_local(dst);
  const bool hasE = conn_classes(eg), hasI = conn_classes(in);
  i64 kept[2] = {0, 0};
  for (i64 p = 0; p < nids_e; ++p) kept[0] += keep_e ? keep_e[p] != 0 : 1;
  for (i64 p = 0; p < nids_i; ++p) kept[1] += keep_i ? keep_i[p] != 0 : 1;
  unsigned long long iso[2] = {0, 0};
  dst->conn_ms = 0.f;
  if (n > 0 && rl > 0) {
    RowsEdited edited{dst};
    DBuf ke, ki, re, ri, cnt;
    ConnWrite wr;
    const i64 Ue = eg->rc.U, ldCe = eg->ldC, Ui = in->rc.U, ldCi = in->ldC;
    KTRY(dalloc(ctx, cnt, sizeof(unsigned long long) * 2));
    if (hasE) {
      KTRY(dalloc(ctx, re, sizeof(u64) * (size_t)(Ue * ldCe)));
      if (keep_e) {
        KTRY(dalloc(ctx, ke, (size_t)nids_e));
        KCHK(hipMemcpyAsync(ke.p, keep_e, (size_t)nids_e, hipMemcpyHostToDevice, ctx->stream));
      }
    }
    if (hasI) {
      KTRY(dalloc(ctx, ri, sizeof(u64) * (size_t)(Ui * ldCi)));
      if (keep_i) {
        KTRY(dalloc(ctx, ki, (size_t)nids_i));
        KCHK(hipMemcpyAsync(ki.p, keep_i, (size_t)nids_i, hipMemcpyHostToDevice, ctx->stream));
      }
    }
    KTRY(wr.alloc(eg, in, dst, flags, hasE, hasI));
    EventPair<> tev;
    if (dst->stage_timing) KTRY(tev.start(ctx));
    KCHK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * 2, ctx->stream));
    int k = 0;
    for (kano_ctx* s : {eg, in}) {
      const int side = k++;
      if (!(side ? hasI : hasE)) continue;
      int wl;
      i64 cap;
      derived_shape(ctx, s->ldC, &wl, &cap);
      hipLaunchKernelGGL(k_conn_class, dim3((unsigned)std::min<i64>(s->rc.U, cap)), dim3(TPB), 0,
                         ctx->stream, s->rc.U, (const i64*)P_<i64>(s->soffc),
                         (const int32_t*)P_<int32_t>(s->slist),
                         (const uint8_t*)(side ? ki.p : ke.p), (const u64*)P_<u64>(s->AC),
                         (const u64*)P_<u64>(s->Mc), s->ldC, wl, P_<u64>(side ? ri : re));
      KLAUNCH();
      if (!info) continue;   // the isolated pods are counted for info only
      hipLaunchKernelGGL(k_conn_isolated, dim3(nblk(n)), dim3(TPB), 0, ctx->stream,
                         (const int32_t*)P_<int32_t>(s->rc.cls), (const i64*)P_<i64>(s->soffc), n,
                         (uint8_t*)nullptr, P_<unsigned long long>(cnt) + side);
      KLAUNCH();
    }
    KTRY(wr.launch(eg, in, dst, flags, hasE, hasI, hasE ? P_<u64>(re) : nullptr,
                   hasI ? P_<u64>(ri) : nullptr));
    KTRY(tev.stop(ctx, &dst->conn_ms));
    KCHK(hipMemcpyAsync(iso, cnt.p, sizeof(iso), hipMemcpyDeviceToHost, ctx->stream));
    KTRY(sync(ctx));
  }
  if (info) {
    info[0] = (int64_t)iso[0];
    info[1] = (int64_t)iso[1];
    info[2] = kept[0];
    info[3] = kept[1];
  }
  return 0;
}

int kano_k8s_isolated(kano_ctx* ctx, uint8_t* out) {
  if (!ctx) return -EINVAL;
  KCHK(hipSetDevice(ctx->device));
  KTRY(conn_source(ctx, ctx, "kano_k8s_isolated"));
  if (!out) return fail(ctx, -EINVAL, "kano_k8s_isolated: out is NULL");
  const i64 n = ctx->n;
  if (n == 0) return 0;
  if (!conn_classes(ctx)) {
    std::memset(out, 0, (size_t)n);
    return 0;
  }
  DBuf flag, cnt;
  KTRY(dalloc(ctx, flag, (size_t)n));
  KTRY(dalloc(ctx, cnt, sizeof(unsigned long long)));
  KCHK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_conn_isolated, dim3(nblk(n)), dim3(TPB), 0, ctx->stream,
                     (const int32_t*)P_<int32_t>(ctx->rc.cls), (const i64*)P_<i64>(ctx->soffc),
                     n, P_<uint8_t>(flag), P_<unsigned long long>(cnt));
  KLAUNCH();
  KCHK(hipMemcpyAsync(out, flag.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  return sync(ctx);
}

// The tiers (k_conn_tier_*, kano_k8s_tiers.hpp): the class-level rows come
// from the codes' ordered copy instead of a keep mask; the write is
// kano_k8s_conn's own.
int kano_k8s_conn_tiers(kano_ctx* eg, kano_ctx* in, kano_ctx* dst, int flags, int64_t nids_e,
                        const uint32_t* code_e, uint32_t np_level_e, int64_t nids_i,
                        const uint32_t* code_i, uint32_t np_level_i, uint8_t* iso_e,
                        uint8_t* iso_i, int64_t* info) {
  const char* const what = "kano_k8s_conn_tiers";
  KTRY(conn_begin(eg, in, dst, what, nids_e, nids_i));
  kano_ctx* ctx = dst;
  const i64 n = dst->n, rl = rows_local(dst);
  kano_ctx* const src[2] = {eg, in};
  const uint32_t* const code[2] = {code_e, code_i};
  const uint32_t np[2] = {np_level_e, np_level_i};
  const i64 nids[2] = {nids_e, nids_i};
  uint8_t* const iso_out[2] = {iso_e, iso_i};
  i64 live[2];
  KTRY(tier_codes_check(dst, what, nids, code, np, live));
  const bool has[2] = {conn_classes(eg), conn_classes(in)};
  unsigned long long cnt_h[2] = {0, 0};
  dst->conn_ms = 0.f;
  // a side without classes isolates nobody (also where nothing is launched)
  for (int side = 0; side < 2; ++side)
    if (iso_out[side] && n > 0) std::memset(iso_out[side], 0, (size_t)n);
  if (n > 0) {
    RowsEdited edited{dst};
    DBuf key[2], pk[2], olist[2], okey[2], ocnt[2], hasnp[2], r[2], flag[2], cnt;
    ConnWrite wr;
    // cnt: the isolated pods of the two sides, then k_verdict_order's scratch word
    KTRY(dalloc(ctx, cnt, sizeof(unsigned long long) * 3));
    for (int side = 0; side < 2; ++side) {
      if (!has[side]) continue;
      kano_ctx* s = src[side];
      const size_t nnz = (size_t)std::max<i64>(1, s->nnz_sel);
      KTRY(dalloc(ctx, key[side], sizeof(uint32_t) * (size_t)nids[side]));
      KTRY(dalloc(ctx, pk[side], sizeof(u64) * nnz));
      KTRY(dalloc(ctx, olist[side], sizeof(int32_t) * nnz));
      KTRY(dalloc(ctx, okey[side], sizeof(uint32_t) * nnz));
      KTRY(dalloc(ctx, ocnt[side], sizeof(int32_t) * (size_t)s->rc.U));
      KTRY(dalloc(ctx, hasnp[side], (size_t)s->rc.U));
      KTRY(dalloc(ctx, r[side], sizeof(u64) * (size_t)(s->rc.U * s->ldC)));
      if (iso_out[side]) KTRY(dalloc(ctx, flag[side], (size_t)n));
      KCHK(hipMemcpyAsync(key[side].p, code[side], sizeof(uint32_t) * (size_t)nids[side],
                          hipMemcpyHostToDevice, ctx->stream));
    }
    // (a shard without rows still answers the isolation flags and counts)
    if (rl > 0) KTRY(wr.alloc(eg, in, dst, flags, has[0], has[1]));
    EventPair<> tev;
    if (dst->stage_timing) KTRY(tev.start(ctx));
    KCHK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * 3, ctx->stream));
    for (int side = 0; side < 2; ++side) {
      if (!has[side]) continue;
      kano_ctx* s = src[side];
      int wl;
      i64 cap;
      derived_shape(ctx, s->ldC, &wl, &cap);
      hipLaunchKernelGGL(k_verdict_order, dim3((unsigned)std::min<i64>(s->rc.U, cap)), dim3(TPB), 0,
                         ctx->stream, s->rc.U, (const i64*)P_<i64>(s->soffc),
                         (const int32_t*)P_<int32_t>(s->slist),
                         (const uint32_t*)P_<uint32_t>(key[side]), P_<u64>(pk[side]),
                         P_<int32_t>(olist[side]), P_<uint32_t>(okey[side]),
                         P_<int32_t>(ocnt[side]),
                         reinterpret_cast<unsigned*>(P_<unsigned long long>(cnt) + 2));
      KLAUNCH();
      const i64 cpb = TPB / wl;
      hipLaunchKernelGGL(k_conn_tier_class,
                         dim3((unsigned)std::min<i64>((s->rc.U + cpb - 1) / cpb, cap)), dim3(TPB),
                         0, ctx->stream, s->rc.U, (const i64*)P_<i64>(s->soffc),
                         (const int32_t*)P_<int32_t>(olist[side]),
                         (const uint32_t*)P_<uint32_t>(okey[side]),
                         (const int32_t*)P_<int32_t>(ocnt[side]), np[side],
                         (const u64*)P_<u64>(s->AC), s->ldC, wl, P_<u64>(r[side]),
                         P_<uint8_t>(hasnp[side]));
      KLAUNCH();
      if (!info && !iso_out[side]) continue;
      hipLaunchKernelGGL(k_conn_tier_isolated, dim3(nblk(n)), dim3(TPB), 0, ctx->stream,
                         (const int32_t*)P_<int32_t>(s->rc.cls),
                         (const uint8_t*)P_<uint8_t>(hasnp[side]), n,
                         iso_out[side] ? P_<uint8_t>(flag[side]) : (uint8_t*)nullptr,
                         P_<unsigned long long>(cnt) + side);
      KLAUNCH();
    }
    if (rl > 0)
      KTRY(wr.launch(eg, in, dst, flags, has[0], has[1], has[0] ? P_<u64>(r[0]) : nullptr,
                     has[1] ? P_<u64>(r[1]) : nullptr));
    KTRY(tev.stop(ctx, &dst->conn_ms));
    for (int side = 0; side < 2; ++side)
      if (has[side] && iso_out[side])
        KCHK(hipMemcpyAsync(iso_out[side], flag[side].p, (size_t)n, hipMemcpyDeviceToHost,
                            ctx->stream));
    KCHK(hipMemcpyAsync(cnt_h, cnt.p, sizeof(cnt_h), hipMemcpyDeviceToHost, ctx->stream));
    KTRY(sync(ctx));
  }
  if (info) {
    info[0] = (int64_t)cnt_h[0];
    info[1] = (int64_t)cnt_h[1];
    info[2] = live[0];
    info[3] = live[1];
  }
  return 0;
}

int kano_k8s_conn_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->conn_ms;
  return 0;
}

// K8sConnectivity.pair_verdicts: which tier and rule decide each pair, both
// directions in one launch (k_k8s_pair_lane / k_k8s_pair_wave,
// kano_k8s_pairs.hpp).  Sources and codes are checked as kano_k8s_conn_tiers
// checks them; the work runs on eg's stream and errors are reported on eg.
int kano_k8s_pair_verdicts(kano_ctx* eg, kano_ctx* in, int flags, int64_t Q, const int32_t* pairs,
                           int64_t nids_e, const uint32_t* code_e, uint32_t np_level_e,
                           int64_t nids_i, const uint32_t* code_i, uint32_t np_level_i,
                           uint8_t* verdict, int32_t* decider_e, int32_t* passed_e,
                           int32_t* decider_i, int32_t* passed_i, int64_t* counts) {
  const char* const what = "kano_k8s_pair_verdicts";
  if (!eg || !in) return -EINVAL;
  const std::string w(what);
  kano_ctx* ctx = eg;
  if (eg->device != in->device) return fail(eg, -EINVAL, w + ": contexts on two devices");
  KCHK(hipSetDevice(eg->device));
  KTRY(conn_source(eg, eg, what));
  KTRY(conn_source(in, eg, what));
  const i64 n = eg->n;
  if (in->n != n) return fail(eg, -EINVAL, w + ": the two contexts must hold the same pods");
  KTRY(conn_nids(eg, in, eg, what, nids_e, nids_i));
  if (Q < 0) return fail(eg, -EINVAL, w + ": Q < 0");
  if (Q > 0 && (!pairs || !verdict)) return fail(eg, -EINVAL, w + ": pairs or verdict is NULL");
  kano_ctx* const src[2] = {eg, in};
  const uint32_t* const code[2] = {code_e, code_i};
  const uint32_t np[2] = {np_level_e, np_level_i};
  const i64 nids[2] = {nids_e, nids_i};
  int32_t* const dec_out[2] = {decider_e, decider_i};
  int32_t* const pas_out[2] = {passed_e, passed_i};
  i64 live[2];
  KTRY(tier_codes_check(eg, what, nids, code, np, live));
  KTRY(pairs_check(eg, what, Q, pairs, n, n));
  KTRY(conn_sync(eg, in, eg, what));
  eg->kpair_ms = 0.f;
  if (counts) std::fill(counts, counts + 18, (int64_t)0);
  if (Q == 0 || n == 0) return 0;
  const bool has[2] = {conn_classes(eg), conn_classes(in)};
  const size_t b_ids = sizeof(int32_t) * (size_t)Q;
  DBuf pr, vd, key[2], dec[2], pas[2];
  KTRY(dalloc(ctx, pr, 2 * b_ids));
  KTRY(dalloc(ctx, vd, (size_t)Q));
  KCHK(hipMemcpyAsync(pr.p, pairs, 2 * b_ids, hipMemcpyHostToDevice, ctx->stream));
  K8sPairArgs a{};
  a.pairs = P_<int32_t>(pr);
  a.Q = Q;
  a.self = (flags & KANO_K8S_CONN_SELF) ? 1 : 0;
  a.verdict = P_<uint8_t>(vd);
  i64 walk = 0;
  for (int side = 0; side < 2; ++side) {
    kano_ctx* s = src[side];
    K8sPairSide& d = a.side[side];
    const int rc = pair_tables(s, what, a.pairs, Q, d.t);
    if (rc) return s == eg ? rc : fail(eg, rc, s->err);
    d.np = np[side];
    if (dec_out[side]) KTRY(dalloc(ctx, dec[side], b_ids));
    if (pas_out[side]) KTRY(dalloc(ctx, pas[side], b_ids));
    d.decider = dec_out[side] ? P_<int32_t>(dec[side]) : nullptr;
    d.passed = pas_out[side] ? P_<int32_t>(pas[side]) : nullptr;
    // a side without classes constrains nothing: no list is walked
    if (!has[side]) {
      d.t.rcls = nullptr;
      continue;
    }
    KTRY(dalloc(ctx, key[side], sizeof(uint32_t) * (size_t)nids[side]));
    KCHK(hipMemcpyAsync(key[side].p, code[side], sizeof(uint32_t) * (size_t)nids[side],
                        hipMemcpyHostToDevice, ctx->stream));
    d.t.key = P_<uint32_t>(key[side]);
    walk += pair_mean_walk(s, d.t);
  }
  bool wave;
  unsigned grid;
  pair_shape(eg, walk, eg->kpair_form, eg->kpair_grid, Q, &wave, &grid);
  EventPair<> tev;
  if (eg->stage_timing) KTRY(tev.start(ctx));
  if (wave) hipLaunchKernelGGL(k_k8s_pair_wave, dim3(grid), dim3(TPB), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_k8s_pair_lane, dim3(grid), dim3(TPB), 0, ctx->stream, a);
  KLAUNCH();
  KTRY(tev.stop(ctx, &eg->kpair_ms));
  KCHK(hipMemcpyAsync(verdict, vd.p, (size_t)Q, hipMemcpyDeviceToHost, ctx->stream));
  for (int side = 0; side < 2; ++side) {
    if (dec_out[side])
      KCHK(hipMemcpyAsync(dec_out[side], dec[side].p, b_ids, hipMemcpyDeviceToHost, ctx->stream));
    if (pas_out[side])
      KCHK(hipMemcpyAsync(pas_out[side], pas[side].p, b_ids, hipMemcpyDeviceToHost, ctx->stream));
  }
  KTRY(sync(ctx));
  if (counts)
    for (i64 q = 0; q < Q; ++q) {
      const unsigned v = verdict[q];
      counts[0] += v & 1u;
      counts[1] += (v >> 1) & 1u;
      ++counts[2 + ((v >> 2) & 3u) * 2 + ((v >> 4) & 1u)];
      ++counts[10 + ((v >> 5) & 3u) * 2 + ((v >> 7) & 1u)];
    }
  return 0;
}

int kano_k8s_pair_verdicts_time(kano_ctx* eg, float* ms) {
  if (!eg || !ms) return -EINVAL;
  *ms = eg->kpair_ms;
  return 0;
}

// K8sConnectivity.rule_usage: per entry the pairs it decides and passes, per
// rule the pairs only it allows, over all n * n pairs from one walk of every
// class list (k_usage_class, kano_k8s_usage.hpp).  Sources and codes are
// checked as kano_k8s_pair_verdicts checks them; the work runs on eg's stream
// and errors are reported on eg.
int kano_k8s_rule_usage(kano_ctx* eg, kano_ctx* in, int flags, int64_t nids_e,
                        const uint32_t* code_e, uint32_t np_level_e, const int32_t* group_e,
                        int64_t nids_i, const uint32_t* code_i, uint32_t np_level_i,
                        const int32_t* group_i, int64_t* decided_e, int64_t* passed_e,
                        int64_t* sole_e, int64_t* decided_i, int64_t* passed_i, int64_t* sole_i,
                        int64_t* tiers) {
  const char* const what = "kano_k8s_rule_usage";
  if (!eg || !in) return -EINVAL;
  const std::string w(what);
  kano_ctx* ctx = eg;
  if (eg->device != in->device) return fail(eg, -EINVAL, w + ": contexts on two devices");
  KCHK(hipSetDevice(eg->device));
  KTRY(conn_source(eg, eg, what));
  KTRY(conn_source(in, eg, what));
  const i64 n = eg->n;
  if (in->n != n) return fail(eg, -EINVAL, w + ": the two contexts must hold the same pods");
  KTRY(conn_nids(eg, in, eg, what, nids_e, nids_i));
  kano_ctx* const src[2] = {eg, in};
  const uint32_t* const code[2] = {code_e, code_i};
  const uint32_t np[2] = {np_level_e, np_level_i};
  const i64 nids[2] = {nids_e, nids_i};
  const int32_t* const group_in[2] = {group_e, group_i};
  int64_t* const dec_out[2] = {decided_e, decided_i};
  int64_t* const pas_out[2] = {passed_e, passed_i};
  int64_t* const sole_out[2] = {sole_e, sole_i};
  i64 live[2];
  KTRY(tier_codes_check(eg, what, nids, code, np, live));
  // the groups: non-decreasing in the id, from 0 on (NULL: every id its own)
  std::vector<int32_t> group[2];
  i64 ngroups[2];
  for (int side = 0; side < 2; ++side) {
    group[side].resize((size_t)nids[side]);
    for (i64 p = 0; p < nids[side]; ++p) {
      const int32_t g = group_in[side] ? group_in[side][p] : (int32_t)p;
      if (g < (p ? group[side][p - 1] : 0))
        return fail(eg, -EINVAL, w + ": " + (side ? "ingress" : "egress") + " group " +
                                     std::to_string(p) + " is " + std::to_string(g) +
                                     ": groups must be non-decreasing, from 0 on");
      group[side][p] = g;
    }
    ngroups[side] = nids[side] ? (i64)group[side].back() + 1 : 0;
  }
  KTRY(conn_sync(eg, in, eg, what));
  eg->kusage_ms = 0.f;
  for (int side = 0; side < 2; ++side) {
    if (dec_out[side]) std::fill(dec_out[side], dec_out[side] + nids[side], (int64_t)0);
    if (pas_out[side]) std::fill(pas_out[side], pas_out[side] + nids[side], (int64_t)0);
    if (sole_out[side]) std::fill(sole_out[side], sole_out[side] + ngroups[side], (int64_t)0);
  }
  if (tiers) std::fill(tiers, tiers + 16, (int64_t)0);
  if (n == 0) return 0;
  const int self = (flags & KANO_K8S_CONN_SELF) ? 1 : 0;
  const bool has[2] = {conn_classes(eg), conn_classes(in)};
  DBuf key[2], pk[2], olist[2], okey[2], ocnt[2], grp[2], size[2], cnt[2], scratch;
  K8sUsageSide a[2];
  size_t ncnt[2] = {0, 0}, nsize[2] = {0, 0};
  KTRY(dalloc(ctx, scratch, sizeof(unsigned)));       // k_verdict_order's count, not read
  for (int side = 0; side < 2; ++side) {
    if (!has[side]) continue;
    kano_ctx* s = src[side];
    const size_t nnz = (size_t)std::max<i64>(1, s->nnz_sel), P = (size_t)nids[side];
    KTRY(dalloc(ctx, key[side], sizeof(uint32_t) * P));
    KTRY(dalloc(ctx, pk[side], sizeof(u64) * nnz));
    KTRY(dalloc(ctx, olist[side], sizeof(int32_t) * nnz));
    KTRY(dalloc(ctx, okey[side], sizeof(uint32_t) * nnz));
    KTRY(dalloc(ctx, ocnt[side], sizeof(int32_t) * (size_t)s->rc.U));
    KTRY(dalloc(ctx, grp[side], sizeof(int32_t) * P));
    // size: the row classes' pods, then the column classes' (ldC * 64, the pad zero)
    nsize[side] = (size_t)s->rc.U + (size_t)s->ldC * 64;
    KTRY(dalloc(ctx, size[side], sizeof(int32_t) * nsize[side]));
    // cnt: decided, passed, sole, tiers
    ncnt[side] = 2 * P + (size_t)ngroups[side] + 8;
    KTRY(dalloc(ctx, cnt[side], sizeof(ull) * ncnt[side]));
    KCHK(hipMemcpyAsync(key[side].p, code[side], sizeof(uint32_t) * P, hipMemcpyHostToDevice,
                        ctx->stream));
    KCHK(hipMemcpyAsync(grp[side].p, group[side].data(), sizeof(int32_t) * P,
                        hipMemcpyHostToDevice, ctx->stream));
    K8sUsageSide& d = a[side];
    d.U = s->rc.U;
    d.soffc = P_<i64>(s->soffc);
    d.olist = P_<int32_t>(olist[side]);
    d.okey = P_<uint32_t>(okey[side]);
    d.ocnt = P_<int32_t>(ocnt[side]);
    d.np = np[side];
    d.AC = P_<u64>(s->AC);
    d.ldC = s->ldC;
    d.group = P_<int32_t>(grp[side]);
    d.rsize = P_<int32_t>(size[side]);
    d.csize = d.rsize + s->rc.U;
    d.decided = P_<ull>(cnt[side]);
    d.passed = d.decided + P;
    d.sole = d.passed + P;
    d.tiers = d.sole + ngroups[side];
  }
  EventPair<> tev;
  if (eg->stage_timing) KTRY(tev.start(ctx));
  for (int side = 0; side < 2; ++side) {
    if (!has[side]) continue;
    kano_ctx* s = src[side];
    const int32_t* rcls = P_<int32_t>(s->rc.cls);
    const int32_t* ccls = P_<int32_t>(s->cc.cls);
    KCHK(hipMemsetAsync(size[side].p, 0, sizeof(int32_t) * nsize[side], ctx->stream));
    KCHK(hipMemsetAsync(cnt[side].p, 0, sizeof(ull) * ncnt[side], ctx->stream));
    int32_t* rsize = P_<int32_t>(size[side]);
    int wl;
    i64 cap;
    derived_shape(ctx, s->ldC, &wl, &cap);
    // (a block counts 8 pods a lane or more before it adds its bins)
    const dim3 hgrid((unsigned)std::min<i64>(nblk(n, (i64)TPB * 8), cap));
    hipLaunchKernelGGL(k_usage_hist, hgrid, dim3(TPB), 0, ctx->stream, rcls, n, rsize, s->rc.U);
    KLAUNCH();
    hipLaunchKernelGGL(k_usage_hist, hgrid, dim3(TPB), 0, ctx->stream, ccls, n, rsize + s->rc.U,
                       s->ldC * 64);
    KLAUNCH();
    hipLaunchKernelGGL(k_verdict_order, dim3((unsigned)std::min<i64>(s->rc.U, cap)), dim3(TPB), 0,
                       ctx->stream, s->rc.U, (const i64*)P_<i64>(s->soffc),
                       (const int32_t*)P_<int32_t>(s->slist),
                       (const uint32_t*)P_<uint32_t>(key[side]), P_<u64>(pk[side]),
                       P_<int32_t>(olist[side]), P_<uint32_t>(okey[side]), P_<int32_t>(ocnt[side]),
                       P_<unsigned>(scratch));
    KLAUNCH();
    if (eg->kusage_grid > 0) cap = std::min<i64>(cap, eg->kusage_grid);
    const i64 cpb = TPB / wl;
    const dim3 grid((unsigned)std::min<i64>((s->rc.U + cpb - 1) / cpb, cap));
    if (wl > 64) hipLaunchKernelGGL(k_usage_class<true>, grid, dim3(TPB), 0, ctx->stream, a[side], wl);
    else hipLaunchKernelGGL(k_usage_class<false>, grid, dim3(TPB), 0, ctx->stream, a[side], wl);
    KLAUNCH();
    if (!self) continue;
    hipLaunchKernelGGL(k_usage_self, dim3(nblk(n)), dim3(TPB), 0, ctx->stream, a[side], rcls, ccls,
                       n);
    KLAUNCH();
  }
  KTRY(tev.stop(ctx, &eg->kusage_ms));
  std::vector<ull> host[2];
  for (int side = 0; side < 2; ++side) {
    if (!has[side]) continue;
    host[side].resize(ncnt[side]);
    KCHK(hipMemcpyAsync(host[side].data(), cnt[side].p, sizeof(ull) * ncnt[side],
                        hipMemcpyDeviceToHost, ctx->stream));
  }
  KTRY(sync(ctx));
  for (int side = 0; side < 2; ++side) {
    if (!has[side]) {   // no class constrains anything: the whole domain is (default, allow)
      if (tiers) tiers[side * 8] = n * n - (self ? n : 0);
      continue;
    }
    const ull* h = host[side].data();
    const i64 P = nids[side], G = ngroups[side];
    if (dec_out[side]) std::copy(h, h + P, dec_out[side]);
    if (pas_out[side]) std::copy(h + P, h + 2 * P, pas_out[side]);
    if (sole_out[side]) std::copy(h + 2 * P, h + 2 * P + G, sole_out[side]);
    if (tiers) std::copy(h + 2 * P + G, h + 2 * P + G + 8, tiers + side * 8);
  }
  return 0;
}

int kano_k8s_rule_usage_time(kano_ctx* eg, float* ms) {
  if (!eg || !ms) return -EINVAL;
  *ms = eg->kusage_ms;
  return 0;
}

}  // extern "C"

// ===========================================================================
// reverse_matrix / reach_zones: the matrix read by columns (k_reverse_tile)
// and the per-row pass over a matrix and its reverse (k_zone_rows;
// kano_zones.hpp).
// ===========================================================================
namespace {

// the shared preamble of two whole matrices of the same n on one device:
// both present, `other`'s pending work complete; the work then runs on ctx's
// stream and errors are reported on ctx
int zones_prepare(kano_ctx* other, kano_ctx* ctx, const char* what) {
  for (const kano_ctx* c : {other, ctx})
    if (c->r0 != 0 || c->r1 != c->n)
      return fail(ctx, -EINVAL, std::string(what) + ": a context holds rows [" +
                                    std::to_string(c->r0) + ", " + std::to_string(c->r1) +
                                    ") of " + std::to_string(c->n) + ": it needs every row");
  KTRY(diff_prepare(other, ctx, what));
  return sync(ctx);
}

template <int A, int B, bool AHEAD>
int reverse_launch(kano_ctx* ctx, const u64* S, i64 ldS, u64* D, i64 ldD, i64 n, i64 W,
                   unsigned long long* bits, i64* tiles) {
  const i64 gx = (W + B - 1) / B, gy = (n + 64 * A - 1) / (64 * A);
  if (gx * gy > 0x7fffffff)
    return fail(ctx, -ENOTSUP, "kano_reverse: " + std::to_string(gx * gy) + " tiles in one launch");
  hipLaunchKernelGGL((k_reverse_tile<A, B, AHEAD>), dim3((unsigned)(gx * gy)), dim3(TPB), 0, ctx->stream,
                     S, ldS, D, ldD, n, W, gx, bits);
  KLAUNCH();
  *tiles = gx * gy;
  return 0;
}

}  // namespace

extern "C" {

int kano_reverse(kano_ctx* src, kano_ctx* dst, int64_t* info) {
  if (!src || !dst) return -EINVAL;
  kano_ctx* ctx = dst;
  if (info) info[0] = info[1] = 0;
  if (src == dst)
    return fail(dst, -EINVAL, "kano_reverse: the destination must be another context");
  KTRY(zones_prepare(src, dst, "kano_reverse"));
  dst->reverse_ms = 0.f;
  const i64 n = dst->n, W = dst->W;
  if (n == 0 || W == 0) return 0;
  unsigned long long bits = 0;
  i64 tiles = 0;
  RowsEdited edited{dst};
  DBuf cnt;
  KTRY(dalloc(ctx, cnt, sizeof(unsigned long long)));
  // timing=1: the call's device time (the fill and the kernel, no copy)
  EventPair<> tev;
  if (dst->stage_timing) KTRY(tev.start(ctx));
  KCHK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), ctx->stream));
  const u64* S = P_<u64>(src->M);
  u64* D = P_<u64>(dst->M);
  unsigned long long* c = P_<unsigned long long>(cnt);
  if (dst->reverse_tile == 1)        // (the forms measured against the default: DESIGN.md)
    KTRY((reverse_launch<8, 8, false>(ctx, S, src->ldM, D, dst->ldM, n, W, c, &tiles)));
  else if (dst->reverse_tile == 2)
    KTRY((reverse_launch<16, 8, true>(ctx, S, src->ldM, D, dst->ldM, n, W, c, &tiles)));
  else
    KTRY((reverse_launch<8, 8, true>(ctx, S, src->ldM, D, dst->ldM, n, W, c, &tiles)));
  KTRY(tev.stop(ctx, &dst->reverse_ms));
  KCHK(hipMemcpyAsync(&bits, cnt.p, sizeof(bits), hipMemcpyDeviceToHost, ctx->stream));
  KTRY(sync(ctx));
  if (info) {
    info[0] = (int64_t)bits;
    info[1] = tiles;
  }
  return 0;
}

int kano_reverse_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->reverse_ms;
  return 0;
}

int kano_zones(kano_ctx* a, kano_ctx* b, int32_t* label, int32_t* fan_out, int32_t* fan_in,
               uint8_t* cyclic, int64_t* info) {
  if (!a || !b) return -EINVAL;
  kano_ctx* ctx = a;
  if (info) info[0] = info[1] = 0;
  if (!label) return fail(a, -EINVAL, "kano_zones: label is NULL");
  KTRY(zones_prepare(b, a, "kano_zones"));
  a->zones_ms = 0.f;
  const i64 n = a->n, W = a->W;
  if (n == 0 || W == 0) return 0;
  const bool counts = fan_out || fan_in || cyclic;
  // the call's own buffer: [label | fan_out | fan_in] int32, then cyclic
  DBuf out;
  KTRY(dalloc(ctx, out, sizeof(int32_t) * 3 * (size_t)n + (size_t)n));
  int32_t* lab = P_<int32_t>(out);
  uint8_t* cyc = reinterpret_cast<uint8_t*>(lab + 3 * n);
  // timing=1: the call's device time (the kernel, no copy)
  EventPair<> tev;
  if (a->stage_timing) KTRY(tev.start(ctx));
  hipLaunchKernelGGL(k_zone_rows, dim3(nblk(n, TPB / 64)), dim3(TPB), 0, ctx->stream,
                     (const u64*)P_<u64>(a->M), a->ldM, (const u64*)P_<u64>(b->M), b->ldM, n, W,
                     counts ? 1 : 0, lab, lab + n, lab + 2 * n, cyc);
  KLAUNCH();
  KTRY(tev.stop(ctx, &a->zones_ms));
  const size_t nb = sizeof(int32_t) * (size_t)n;
  KCHK(hipMemcpyAsync(label, lab, nb, hipMemcpyDeviceToHost, ctx->stream));
  if (fan_out) KCHK(hipMemcpyAsync(fan_out, lab + n, nb, hipMemcpyDeviceToHost, ctx->stream));
  if (fan_in) KCHK(hipMemcpyAsync(fan_in, lab + 2 * n, nb, hipMemcpyDeviceToHost, ctx->stream));
  if (cyclic) KCHK(hipMemcpyAsync(cyclic, cyc, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  KTRY(sync(ctx));
  if (info) {
    std::vector<int32_t> s(label, label + n);
    std::sort(s.begin(), s.end());
    info[0] = (int64_t)(std::unique(s.begin(), s.end()) - s.begin());
    for (i64 i = 0; i < n; ++i) info[1] += label[i] != (int32_t)i;
  }
  return 0;
}

int kano_zones_time(kano_ctx* ctx, float* ms) {
  if (!ctx || !ms) return -EINVAL;
  *ms = ctx->zones_ms;
  return 0;
}

}  // extern "C"
