/*
 * kano_hip.h -- C ABI of libkano_hip.so, the MI355X (gfx950) engine behind the
 * drop-in `kano` Python API (reference: qiyueyao/Kubernetes-verification,
 * kano_py/).  Every entry point names the reference operation it replaces.
 *
 * Conventions
 *   - return 0 on success, a negative errno-style code on failure; the message
 *     is kept in the context and returned by kano_last_error().
 *   - all pointers are HOST pointers (caller-owned) unless the name ends in
 *     _dev, in which case they are device pointers on the context's device.
 *   - device memory is owned by the context; one context = one build of the
 *     reachability matrix (or one row shard of it) on one GPU.
 *   - bit order: LSB-first inside little-endian uint64 words: bit j of a bit
 *     row lives in word j >> 6, bit j & 63.  The Python layer converts to the
 *     reference's bitarray (big-endian bytes) where the API exposes bitarrays.
 *   - not re-entrant per context; work is issued on the context's stream
 *     (kano_set_stream) and every call that returns host data synchronises it.
 *
 * Interned inputs (built by the Python host layer, kano/_intern.py):
 *   pod_val[c * n + i]  value id of label column c on pod i; -1 = pod i lacks
 *                       the key (value ids are equality classes of Python ==).
 *   sel_off/sel_col/sel_val   CSR, per policy, of the WORKING-SELECTOR terms
 *   alw_off/alw_col/alw_val   CSR, per policy, of the WORKING-ALLOW terms
 *                       (ingress/egress side swap already applied,
 *                       kano_py/kano/model.py:82-93; terms whose key no pod
 *                       carries already dropped, model.py:142-147; a rule value
 *                       no pod carries is -2 and matches nothing).
 */
#ifndef KANO_HIP_H
#define KANO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kano_ctx kano_ctx;

/* Build paths for kano_build(). */
#define KANO_PATH_AUTO    0   /* per-class choice by estimated cost          */
#define KANO_PATH_BITWISE 1   /* LDS scatter / bitwise OR of allow rows      */
#define KANO_PATH_MFMA    2   /* heavy classes by the MFMA contraction       */

/* kano_info() slots */
#define KANO_INFO_N        0
#define KANO_INFO_W        1
#define KANO_INFO_P        2
#define KANO_INFO_U        3   /* row classes (pods with equal selector keys) */
#define KANO_INFO_NNZ_SEL  4   /* sum over classes of |S(c)|                  */
#define KANO_INFO_NNZ_ALW  5   /* sum over policies of |allow_p|              */
#define KANO_INFO_HEAVY    6   /* classes built by the heavy (dense) path     */
#define KANO_INFO_ROW0     7
#define KANO_INFO_ROW1     8
#define KANO_INFO_MAXSEL   9   /* max over classes of |S(c)|                  */
#define KANO_INFO_UA      10   /* column classes (pods with equal allow keys) */
#define KANO_INFO_HEAVY_PATH 11 /* 0 none, 1 bitwise OR, 2 MFMA (fp4)         */
#define KANO_INFO_WORK_ITEMS 12 /* (class, member chunk) items of the list-based row kernel */
#define KANO_INFO_ROWS_KERNEL 13 /* the last matrix write: 2 k_rows, 3 k_rows_prep + k_rows_w
                                    (wide rows), 4 k_ptrans + k_heavy_rows_t (every class
                                    heavy, k_rows not launched), 5 the same then k_rows,
                                    6 the same then k_rows_w; 0 none yet */
#define KANO_INFO_ROWS_CUS 14   /* CUs the last matrix write's stream may use  */
#define KANO_INFO_HEAVY_SEL 15  /* sum of |S(c)| over the heavy classes       */
#define KANO_INFO_HEAVY_KERNEL 16 /* 0 none, 1 k_heavy_mc_or, 2 k_heavy_mc_mfma (split K), 3 k_heavy_gemm */
#define KANO_INFO_CLS_REUSED 17 /* builds on this context that reused the kept pod
                                  classification (see kano_set_policies)        */
#define KANO_INFO_MATCH_FORM 18 /* how the current policies are matched to the pod
                                  classes: bit 0 the select side takes the dense
                                  evaluation (more than 64 distinct slot sets),
                                  bit 1 the allow side; a clear bit: the hash join */
#define KANO_INFO_NSLOTS   19

/* Lifetime.  No reference counterpart: the reference keeps its state in
 * Python objects (kano_py/kano/model.py:167-169 ReachabilityMatrix.__init__). */
int  kano_create(int device, kano_ctx** out);
/* kano_create for builds the caller waits for (the drop-in build_matrix): no
 * CU-masked write stream (~15 ms of the 23 ms creation); a kano_verify step
 * on it still overlaps its matrix write with the next call, on every CU */
int  kano_create_lean(int device, kano_ctx** out);
void kano_destroy(kano_ctx* ctx);
const char* kano_last_error(const kano_ctx* ctx);
int  kano_set_stream(kano_ctx* ctx, void* hip_stream);   /* NULL = own stream */

/* Inputs.  Replace the key-presence bitsets of build_matrix
 * (kano_py/kano/model.py:128-133) and the per-policy selector dicts it reads
 * through Policy.working_selector / working_allow (model.py:82-93, 142-147). */
/* The pod classification (both sides' classes, member lists and
 * representative values) depends only on the pod label table, each side's key
 * columns (which label columns the policy terms name, not their values) and
 * the row shard.  A successful build keeps it and later builds on the context
 * reuse it (counted in KANO_INFO_CLS_REUSED).  It is classified again after:
 * kano_set_pods, kano_set_expressions, a kano_add_policies that brings pod
 * columns, a kano_set_shard with another range, a kano_set_policies whose
 * terms name a different set of label columns on either side (an equal set
 * keeps it), kano_shadow_lists and its kin, and any failed build. */
int kano_set_pods(kano_ctx* ctx, int64_t n, int32_t ncols, const int32_t* pod_val);
int kano_set_policies(kano_ctx* ctx, int64_t P,
                      const int64_t* sel_off, const int32_t* sel_col, const int32_t* sel_val,
                      const int64_t* alw_off, const int32_t* alw_col, const int32_t* alw_val);
/* Row shard [row_begin, row_end) of M owned by this context (multi-GPU row
 * partition); default = all rows. */
int kano_set_shard(kano_ctx* ctx, int64_t row_begin, int64_t row_end);

/* ReachabilityMatrix.build_matrix (kano_py/kano/model.py:125-165): row classes
 * (pods with equal working-selector key values) and column classes (equal
 * working-allow key values), selector evaluation on both, the per-policy
 * allowed pods and the matrix rows M[i] = OR_{p in S(i)} allow_p. */
int kano_build(kano_ctx* ctx, int path);
int kano_info(kano_ctx* ctx, int64_t* out /* KANO_INFO_NSLOTS */);

/* all_reachable / all_isolated (kano_py/kano/algorithm.py:4-17): column AND
 * and column OR of this shard's rows, W = ceil(n/64) words each. */
int kano_col_checks(kano_ctx* ctx, uint64_t* col_and, uint64_t* col_or);
/* Same, unpacked to one byte per column into device memory laid out as
 * [or(n) | cross(n) | nand(n)] so that ranks can combine with a MAX all-reduce
 * (RCCL has no bitwise reduction).  cross is filled only when a gid array was
 * passed to kano_crosscheck_dev. */
int kano_col_flags_dev(kano_ctx* ctx, uint8_t* flags_dev);

/* user_crosscheck (kano_py/kano/algorithm.py:20-42): bit j set iff some row i
 * of this shard has M[i,j] and gid[i] != gid[j]; gid = interned
 * container.getValueOrDefault(label, "") (algorithm.py:23,38), all n pods. */
int kano_crosscheck(kano_ctx* ctx, const int32_t* gid, uint64_t* cross);
int kano_crosscheck_dev(kano_ctx* ctx, const int32_t* gid, uint8_t* flags_dev);

/* Matrix access: getrow / getcol / __getitem__ / __setitem__
 * (kano_py/kano/model.py:171-184); system_isolation reads a row
 * (algorithm.py:45-55).  Rows are global indices inside this shard. */
int kano_get_rows(kano_ctx* ctx, int64_t r0, int64_t nrows, uint64_t* dst);
/* Overwrite rows (assignment to ReachabilityMatrix.matrix rows / the
 * ReachabilityMatrix(container_size, matrix) constructor, model.py:167-169). */
int kano_put_rows(kano_ctx* ctx, int64_t r0, int64_t nrows, const uint64_t* src);
/* Per-row 64-bit digests of rows [r0, r0 + nrows) (no reference counterpart:
 * a full-size matrix does not fit the host; the tests compare digests of
 * two builds of the same rows, e.g. bitwise vs MFMA, sharded vs unsharded).
 * digest = sum_k mix64(row[k] ^ k * 0xD6E8FEB86659FD93) mod 2^64 over the W
 * words, mix64 the splitmix64 finaliser. */
int kano_rows_digest(kano_ctx* ctx, int64_t r0, int64_t nrows, uint64_t* out);
int kano_get_col(kano_ctx* ctx, int64_t j, uint64_t* dst /* ceil(rows/64) */);
int kano_get_bit(kano_ctx* ctx, int64_t i, int64_t j, int* value);
int kano_set_bit(kano_ctx* ctx, int64_t i, int64_t j, int value);

/* Policy.working_select_set / working_allow_set (model.py:119-121, 156):
 * the n-bit sets of policy p (on a row shard, select bits exist for the
 * shard's pods only; the others read 0). */
int kano_get_policy_sets(kano_ctx* ctx, int64_t p, uint64_t* sel, uint64_t* allow);
/* Container.select_policies (model.py:158-161): row class of every pod and the
 * class-level ascending policy lists, CSR over classes (row classes cover the
 * shard's pods; cls is -1 outside the shard). */
int kano_get_classes(kano_ctx* ctx, int32_t* cls /* n */);
int kano_get_select_csr(kano_ctx* ctx, int64_t* off /* U+1 */, int32_t* pol /* nnz_sel */);
/* Container.allow_policies (model.py:162-163) and the allow sets as pod
 * lists (grouped by column class, not sorted), CSR over policies. */
int kano_get_allow_csr(kano_ctx* ctx, int64_t* off /* P+1 */, int32_t* pods /* nnz_alw */);

/* policy_shadow (kano_py/kano/algorithm.py:58-80): emits, for this shard's
 * pods in ascending order, every ordered pair (j,k) of policies selecting the
 * pod with j != k and allow_k a subset of allow_j.  kano_shadow computes and
 * returns the pair count; kano_shadow_fetch copies 2*count int32. */
int kano_shadow(kano_ctx* ctx, int64_t* count);
int kano_shadow_fetch(kano_ctx* ctx, int32_t* pairs);

/* policy_shadow over explicit inputs: n_lists per-container policy lists
 * (CSR soff/slist, the values of Container.select_policies, possibly
 * accumulated over several builds, quirk Q5) and the P allow sets as bit rows
 * of nbits bits (Policy.working_allow_set).  The context holds no matrix
 * afterwards; fetch the pairs with kano_shadow_fetch. */
int kano_shadow_lists(kano_ctx* ctx, int64_t n_lists, int64_t nbits, int64_t P,
                      const int64_t* soff, const int32_t* slist, const uint64_t* allow_rows,
                      int64_t* count);

/* policy_conflict (kano_py/kano/algorithm.py:83-100) raises AttributeError
 * as soon as any container has two selecting policies: *raises = 1 iff some
 * pod of this shard has |S(i)| >= 2. */
int kano_conflict(kano_ctx* ctx, int* raises);

/* The working policy_conflict (the check algorithm.py:83-100 was written to
 * be): emits, for this shard's pods in ascending order,
 * every ordered pair (j,k) of policies selecting the pod, in list order,
 * with j != k by value and allow_j and allow_k sharing no pod.  Duplicates are
 * kept (one entry per pod, quirk Q4); the relation is symmetric, so both
 * orders appear; an empty allow set conflicts with every other policy.
 * mode 0 computes the pairs (fetch 2*count int32 with kano_conflict_fetch),
 * mode 1 only counts (no flags, no compaction; kano_conflict_fetch then
 * returns -EINVAL, as it does before any kano_conflict_pairs).  class_pairs
 * (nullable): the pairs at row-class level, the length kano_conflict_classes
 * writes.  The pairs and their total are the call's own: kano_shadow_fetch
 * after an interleaved kano_conflict_pairs still returns the shadow pairs,
 * and the other way round.  A pairs buffer that cannot be allocated returns
 * -ENOMEM (kano_last_error) and leaves the context usable.  kano_conflict
 * above is unchanged: it reproduces the reference's raise. */
int kano_conflict_pairs(kano_ctx* ctx, int mode, int64_t* count, int64_t* class_pairs);
int kano_conflict_fetch(kano_ctx* ctx, int32_t* pairs /* 2*count */);
/* The same over explicit inputs (the arguments of kano_shadow_lists; an id
 * outside [0, P) returns -ERANGE).  The context holds no matrix afterwards. */
int kano_conflict_lists(kano_ctx* ctx, int64_t n_lists, int64_t nbits, int64_t P,
                        const int64_t* soff, const int32_t* slist, const uint64_t* allow_rows,
                        int mode, int64_t* count);
/* Class level: row class c's conflicting (j,k) are pairs[2*off[c] ..
 * 2*off[c+1]) (off[U] = class_pairs of kano_conflict_pairs) and members[c]
 * pods of this shard share them.  Runs the tests itself; any of the three
 * outputs may be NULL. */
int kano_conflict_classes(kano_ctx* ctx, int64_t* off /* U+1 */, int32_t* pairs,
                          int32_t* members /* U */);

/* policy_impact / policy_redundant: what removing one policy changes.  With
 * cover(i,j) = #{p : i in select_p, j in allow_p} over the working sets,
 *   impact[p] = #{(i,j) : i in select_p, j in allow_p, cover(i,j) == 1},
 * the pod pairs that lose reachability when p alone is removed (the bits in
 * which the matrix differs after removing p), counted over this context's
 * rows r0..r1: the impacts of row shards add up, their flags OR.  p is
 * redundant iff impact[p] == 0 (an empty select or allow set; a policy
 * covered by the union of others; each of two identical policies).
 * mode 0: impact[P] (required), essential[P] (nullable; 1 = not redundant)
 * and *n_redundant (nullable).  mode 1: the flags and the count only, impact
 * may be NULL.  Any other mode returns -EINVAL.  Exact integers.  The device
 * buffers are the call's own: kano_shadow_fetch / kano_conflict_fetch after
 * it return their own results, a call between pipelined kano_verify steps
 * leaves the next step unchanged, and a failed allocation returns -ENOMEM
 * and leaves the context usable. */
int kano_policy_impact(kano_ctx* ctx, int mode, int64_t* impact /* P, NULL in mode 1 */,
                       uint8_t* essential /* P, nullable */, int64_t* n_redundant);
/* The same over explicit inputs (the arguments of kano_shadow_lists): list c
 * is one container's selecting policies, allow_rows[p] the pods p allows.
 * Unlike the shadow and conflict entry points this one needs the ids within
 * one list distinct: a repeated id returns -EINVAL, an id outside [0, P)
 * -ERANGE.  The context holds no matrix afterwards. */
int kano_policy_impact_lists(kano_ctx* ctx, int64_t n_lists, int64_t nbits, int64_t P,
                             const int64_t* soff, const int32_t* slist,
                             const uint64_t* allow_rows, int mode,
                             int64_t* impact, uint8_t* essential, int64_t* n_redundant);

/* pair_policies: which policies allow a given pod pair.  Over the working
 * sets of the matrix's current policies (the build's that are not removed,
 * plus the added ones that are not removed),
 *   pols(i,j)  = the ascending engine ids p with i in select_p, j in allow_p,
 *   cover(i,j) = the length of pols(i,j)
 * for Q query pairs (i,j) = pairs[2q], pairs[2q+1], in any order, duplicates
 * allowed.  A policy appears at most once per pair.  The query speaks about
 * the policies, not about bits edited with kano_set_bit / kano_put_rows: on
 * an unedited matrix cover(i,j) > 0 iff M[i,j] = 1.  Unlike
 * kano_policy_impact it accepts a context after kano_add_policies /
 * kano_remove_policies (the added policies carry the ids P, P+1, ... that
 * kano_add_policies returned; removed ids never appear).
 * mode 0: cover[Q] (nullable), off[Q+1] (nullable; pair q's ids are
 * pol[off[q] .. off[q+1]) of kano_pair_policies_fetch), hist[P + added]
 * (nullable; hist[p] = the queried pairs p allows) and *total = off[Q] =
 * sum of cover (nullable).  mode 1: cover, hist and *total only, no lists on
 * the device and off untouched; kano_pair_policies_fetch then returns
 * -EINVAL, as it does before any call.  Any other mode returns -EINVAL; Q < 0
 * or NULL pairs with Q > 0 -EINVAL; an index outside [0, n) -ERANGE; Q = 0 is
 * valid.  A context whose matrix has no policies (an empty, copied, loaded,
 * path or edge matrix) returns -EINVAL.  On a row shard a pair whose i lies
 * outside r0..r1 gets cover 0 and no ids and adds nothing to hist, so the
 * covers and histograms of row shards add up and every list comes from the
 * shard holding i.  Exact integers.  The device buffers are the call's own:
 * the shadow, conflict and impact fetches after it return their own results,
 * a call between pipelined kano_verify steps leaves the next step unchanged,
 * and a failed allocation returns -ENOMEM and leaves the context usable. */
int kano_pair_policies(kano_ctx* ctx, int64_t Q, const int32_t* pairs /* 2*Q */, int mode,
                       int32_t* cover /* Q, nullable */, int64_t* off /* Q+1, nullable */,
                       int64_t* hist /* P_total, nullable */, int64_t* total);
int kano_pair_policies_fetch(kano_ctx* ctx, int32_t* pol /* total */);
/* The same over explicit inputs (the arguments of kano_shadow_lists): a pair
 * is (list index, bit index).  An id repeated within one list counts once; an
 * id outside [0, P) returns -ERANGE.  The context holds no matrix afterwards. */
int kano_pair_policies_lists(kano_ctx* ctx, int64_t n_lists, int64_t nbits, int64_t P,
                             const int64_t* soff, const int32_t* slist,
                             const uint64_t* allow_rows, int64_t Q, const int32_t* pairs,
                             int mode, int32_t* cover, int64_t* off, int64_t* hist,
                             int64_t* total);
/* KANO_TUNE timing=1: the last call's device time (the fill, the count pass,
 * the offsets' scan and the emit pass; no copies). */
int kano_pair_policies_time(kano_ctx* ctx, float* ms);

/* port_matrix / pair_ports: port-aware reachability.  Both read the tables
 * kano_pair_policies reads, over the same policies (the build's that are not
 * removed plus the added ones that are not removed), and index them by engine
 * id: 0 .. P-1 the build's, then the added ones; nids = P + added, and the
 * entries of removed ids are ignored.  The engine knows no ports: the caller
 * says which policies to keep (keep) or which bits each policy carries
 * (pmask); kano/ports.py builds both from Policy.protocol.
 * kano_policy_subset: dst's rows := the matrix of the kept policies,
 *   subset[i,j] = 1 iff some alive p with keep[p] != 0 has i in select_p and
 *   j in allow_p,
 * for the rows r0..r1 both contexts hold.  dst is a matrix context of the same
 * n, device and rows as src (kano_set_shard with the same range on an empty
 * build); every word of every held row of dst is written (a pod no kept
 * policy selects gets a zero row, bits at positions >= n are zero) and dst
 * then reads as an edited matrix, like kano_path's destination.  The rows of
 * row shards concatenate.  info (nullable) = [kept alive build policies, kept
 * alive added policies, row classes of src with at least one kept policy].
 * kano_pair_masks: out[q*KW + w] = OR of pmask[p*KW + w] over pols(i,j) of
 * pair q (kano_pair_policies' pols), 0 iff cover(i,j) = 0; pairs in any
 * order, duplicates allowed.  On a row shard a pair whose i lies outside
 * r0..r1 gets a zero mask, so the masks of row shards OR together.
 * -EINVAL: a NULL argument (pairs and out may be NULL with Q == 0, info
 * always), src == dst, contexts of different n, device or rows, nids != P +
 * added, KW <= 0, Q < 0, a context holding policy lists, a context whose
 * matrix has no policies (as kano_pair_policies); -ERANGE: a pair index
 * outside [0, n); -ENOTSUP: kano_policy_subset over more than 1,048,560 row
 * classes; -ENOMEM (with a message): a device buffer could not be allocated.
 * kano_policy_subset reports its errors on dst.  Q == 0, n == 0
 * or no held rows give empty or zero results and launch nothing.  Exact bits.
 * The device buffers are the call's own (the flags, the class-level rows
 * U * ldC words and their bit-transposed 16-row groups; the pairs, the masks
 * and the result), freed on return: src's matrix (never read), its class
 * tables and every stored check result (column words, crosscheck words,
 * shadow, conflict and pair_policies lists, impact) are unchanged, a call
 * between pipelined kano_verify steps leaves the next step's results
 * unchanged, and the context stays usable after every error. */
int kano_policy_subset(kano_ctx* src, kano_ctx* dst, int64_t nids,
                       const uint8_t* keep /* nids */,
                       int64_t* info /* 3, nullable */);
int kano_pair_masks(kano_ctx* ctx, int64_t Q, const int32_t* pairs /* 2*Q */,
                    int64_t nids, int32_t KW, const uint64_t* pmask /* nids*KW */,
                    uint64_t* out /* Q*KW */);
/* KANO_TUNE timing=1: the last call's device time in ms (the fills and the
 * kernels, no copies; kano_policy_subset's on src and on dst alike), else 0. */
int kano_policy_subset_time(kano_ctx* ctx, float* ms);
int kano_pair_masks_time(kano_ctx* ctx, float* ms);

/* verdict_matrix / pair_verdicts: deny rules and priorities (the tiers of
 * AdminNetworkPolicy, Calico and Cilium policy sets).  Both read the tables
 * kano_pair_policies reads, over the same policies and the same engine ids as
 * kano_policy_subset (nids = P + added; the entries of removed ids are
 * ignored).  Every policy p carries action[p] (0 allow, 1 deny) and an integer
 * prio[p]: a smaller number is evaluated first, any int32 value is valid, and
 * the C side ranks the raw values.  p matches (i, j) iff i in select_p and j
 * in allow_p (source -> destination, the direction swap already applied).
 *   t*(i,j)  = the smallest prio[p] over the matching policies
 *   verdict  = none  if nothing matches (unreachable: kano's reading),
 *              deny  if some deny policy with prio == t* matches (within one
 *                    priority deny wins),
 *              allow otherwise
 *   decider  = the smallest engine id among the matching policies with
 *              prio == t* and the winning action.
 * All-allow with any priorities gives the built matrix; one priority for all
 * gives subset(allows) & ~subset(denies).  Pass, the order of rules within a
 * policy and bits edited by hand do not enter.
 * kano_verdict_matrix: dst's rows := (verdict == allow), for the rows r0..r1
 * both contexts hold; dst as kano_policy_subset's (same n, device and rows;
 * every word of every held row is written; it then reads as an edited matrix;
 * the rows of row shards concatenate).  Any number of distinct priorities.
 * info (nullable) = [alive allow policies, alive deny policies, distinct
 * priorities of the alive policies, row classes of src with an alive deny
 * policy (a row shard classifies the rows it holds: its count is over those
 * classes, and the counts of shards do not add up to the whole build's)].
 * kano_pair_verdicts: verdict[q] = 0 none / 1 allow / 2 deny; decided_prio[q]
 * (nullable) = t*, 0 where none; decider[q] (nullable) = the engine id, -1
 * where none; counts (nullable) = [none, allow, deny] over the pairs whose i
 * this context holds.  Pairs in any order, duplicates allowed.  On a row
 * shard a pair whose i lies outside r0..r1 gets verdict 0 and decider -1 and
 * adds to no count, so the verdicts of row shards combine by maximum and the
 * counts add.
 * -EINVAL: a NULL argument (pairs and verdict may be NULL with Q == 0;
 * decided_prio, decider, counts and info always), src == dst, contexts of
 * different n, device or rows, nids != P + added, an action byte > 1, Q < 0,
 * a context holding policy lists, a context whose matrix has no policies (as
 * kano_pair_policies); -ERANGE: a pair index outside [0, n); -ENOTSUP:
 * kano_verdict_matrix over more than 1,048,560 row classes; -ENOMEM (with a
 * message): a device buffer could not be allocated.  kano_verdict_matrix
 * reports its errors on dst.  Q == 0, n == 0 or no held rows give empty or
 * zero results and launch nothing.  Exact bits and integers.
 * The device buffers are the call's own (the keys, the rank-ordered copy of
 * the class lists, the class-level rows and their bit-transposed groups, the
 * marked rows; the pairs and the results), freed on return: src's matrix
 * (never read), its class tables and every stored check result are unchanged,
 * a call between pipelined kano_verify steps leaves the next step's results
 * unchanged, and the context stays usable after every error. */
int kano_verdict_matrix(kano_ctx* src, kano_ctx* dst, int64_t nids,
                        const int32_t* prio /* nids */,
                        const uint8_t* action /* nids: 0 allow, 1 deny */,
                        int64_t* info /* 4, nullable */);
int kano_pair_verdicts(kano_ctx* ctx, int64_t Q, const int32_t* pairs /* 2*Q */,
                       int64_t nids, const int32_t* prio, const uint8_t* action,
                       uint8_t* verdict /* Q */, int32_t* decided_prio /* Q, nullable */,
                       int32_t* decider /* Q, nullable */,
                       int64_t* counts /* 3, nullable */);
/* KANO_TUNE timing=1: the last call's device time in ms (the fills and the
 * kernels, no copies; kano_verdict_matrix's on src and on dst alike), else 0.
 * KANO_TUNE pvf=1/2 forces kano_pair_verdicts' lane / wave form, pvgrid=K caps
 * its grid. */
int kano_verdict_matrix_time(kano_ctx* ctx, float* ms);
int kano_pair_verdicts_time(kano_ctx* ctx, float* ms);

/* matrix_diff: what a change adds and removes.  a and b hold matrices of the
 * same n on the same device over the same rows r0..r1 (built, loaded, path or
 * edge matrices alike); for i in [r0, r1), j in [0, n):
 *   added(i,j) = B[i,j] and not A[i,j],   removed(i,j) = A[i,j] and not B[i,j].
 * Bits at positions >= n of a row's last word (kano_put_rows copies them
 * unmasked) belong to neither matrix.  One pass over both matrices on b's
 * stream, after a's pending work; errors are reported on b.  Exact integers.
 * totals[2] = the added and removed bits; row_added / row_removed (rows_local
 * int32 each) the counts per local row; col_added / col_removed (W words
 * each, tail-masked) bit j set when column j gained / lost at least one
 * source.  Any of the four arrays may be NULL; with all four NULL only the
 * totals are computed.  a == b gives an empty diff; n == 0 or no local rows
 * gives zeros.  -EINVAL: a NULL context or totals, two devices, different n,
 * different rows.  Neither matrix, nor any class table or check result of
 * either context, changes; both contexts stay usable after an error.  The
 * totals of row shards add up, their row counts concatenate, their column
 * words OR. */
int kano_diff(kano_ctx* a, kano_ctx* b, int64_t* totals /* 2: added, removed */,
              int32_t* row_added, int32_t* row_removed,    /* rows_local each, or NULL */
              uint64_t* col_added, uint64_t* col_removed); /* W words each, or NULL */
/* The pairs of one kind (0 added, 1 removed) in rows [r0, r0 + nrows) of this
 * shard, as (i, j) int32 with global indices, ascending by i and then j.
 * Self-contained: the call recounts its row range.  *count is always set (0
 * on an argument error); pairs NULL asks for the count alone.  With pairs
 * given and count > max_pairs the call returns -ENOSPC and writes no pair.
 * -EINVAL as kano_diff, and for a kind outside {0, 1}, a row range outside
 * the shard, a NULL count or max_pairs < 0; -ENOTSUP past 4,194,304 rows in
 * one call (split the range). */
int kano_diff_pairs(kano_ctx* a, kano_ctx* b, int kind /* 0 added, 1 removed */,
                    int64_t r0, int64_t nrows, int64_t max_pairs,
                    int64_t* count, int32_t* pairs /* 2*count, or NULL: count only */);
/* dst's rows := src's rows, device to device (dst: a matrix of the same n and
 * rows, e.g. a context with no policies).  dst is then an edited matrix, as
 * after kano_import_rows.  src == dst returns -EINVAL. */
int kano_copy_matrix(kano_ctx* src, kano_ctx* dst);
/* The last kano_diff's device time on this (its second) context, fill and
 * kernel without the copies, in ms; recorded under KANO_TUNE=timing=1, else 0. */
int kano_diff_time(kano_ctx* ctx, float* ms);

/* group_reachability: the matrix's quotient by two pod labellings.  gsrc[i] is
 * the source group of pod i and gdst[j] the destination group of pod j, both
 * int32 over all n pods (the same labelling or two different ones); for the
 * rows r0..r1 this context holds,
 *   counts[g][h]     = #{(i, j) : r0 <= i < r1, 0 <= j < n, M[i,j] = 1,
 *                        gsrc[i] = g, gdst[j] = h}        (int64, Gs x Gd, row-major)
 *   row_counts[i][h] = #{j : M[i,j] = 1, gdst[j] = h}    (int32, rows_local x Gd)
 * A negative id leaves that pod out: a row with gsrc[i] < 0 adds to no counts
 * entry (its row_counts are still computed), a column with gdst[j] < 0 is
 * counted nowhere.  Bits at positions >= n of a row's last word (kano_put_rows
 * copies them unmasked) belong to no group.  Exact integers.  row_counts may
 * be NULL.  Works on every matrix a context holds (built, edited, updated,
 * loaded, path, edge, row shard): the matrix is present (as for
 * kano_get_rows), pending work is waited for, and the passes over the
 * resident rows run on the context's stream in device buffers that are the
 * call's own.  n == 0 or no local rows gives zeros.  The counts of row shards
 * add up, their row_counts concatenate.
 * -EINVAL: a NULL context, gsrc, gdst or counts, Gs <= 0 or Gd <= 0;
 * -ERANGE: an id >= its group count (both arrays are scanned on the host);
 * -ENOTSUP: Gs * Gd > 134,217,728 (2^27 cells, 1 GiB of counts: ask for
 * row_counts with fewer source groups instead); -ENOMEM (with a message): a
 * device buffer could not be allocated -- the masks (at most 1 GiB a pass),
 * Gs * Gd * 8 bytes, rows_local * Gd * 4 bytes.  The context stays usable
 * after every error.  The matrix, the class tables and every stored check
 * result (column words, crosscheck words, shadow and conflict pairs, impact)
 * are unchanged; a call between pipelined kano_verify steps leaves the next
 * step's results unchanged. */
int kano_group_counts(kano_ctx* ctx, const int32_t* gsrc /* n */, int32_t Gs,
                      const int32_t* gdst /* n */, int32_t Gd,
                      int64_t* counts /* Gs*Gd, row-major */,
                      int32_t* row_counts /* rows_local*Gd, or NULL */);
/* The last kano_group_counts' device time, fills and kernels without the
 * copies, in ms; recorded under KANO_TUNE=timing=1, else 0. */
int kano_group_counts_time(kano_ctx* ctx, float* ms);

/* hop_distance / path_witness: shortest paths over the matrix, read as a graph
 * with an edge i -> j iff M[i,j] = 1.  For a source s,
 *   dist(s, t) = the least k >= 1 such that a walk of k edges leads from s to
 *                t, -1 if there is none (or none within max_hops; 0 = no bound)
 * -- k starts at 1, as the closure's "paths of any length >= 1": dist(s, s) is
 * 1 with a self-loop, else the shortest cycle through s, else -1.  With
 * L_0 = {s}, V_0 = {} and L_k = (OR of row(u), u in L_{k-1}) \ V_{k-1},
 * V_k = V_{k-1} | L_k: dist(s, v) = k iff v in L_k.  So
 * kano_path(hops = k)[s,t] = 1 iff 1 <= dist(s,t) <= k, and the closure's bit
 * iff dist(s,t) >= 1.  Bits at positions >= n of a row's last word
 * (kano_put_rows copies them unmasked) are no edges.
 * The canonical shortest path of a pair with d = dist(s, t) >= 1 is
 * [s, t_1, .., t_{d-1}, t] with t_d = t and t_{k-1} = the smallest u in
 * L_{k-1} with M[u, t_k] = 1: d + 1 nodes, every step an edge, unique.
 * Works on every whole matrix a context holds (built, edited, updated,
 * loaded, path, edge): the matrix is present and pending work waited for, as
 * for kano_group_counts; a breadth-first search runs level by level for a
 * batch of up to 64 sources at once, in device buffers that are the call's own
 * (the matrix and every stored result are unchanged).  The host reads the
 * batch's frontier sizes after every level: one round trip a level, so a
 * chain-shaped graph of depth d costs d of them.  Exact integers.
 * kano_hops: dist[k * n + v] = dist(sources[k], v) for S sources (duplicates
 * allowed); info[4] (nullable) = the levels run (the largest finite distance
 * found), the rows OR-ed (frontier pods over all levels and sources), the
 * batches, the pods reached (entries of dist that are >= 1).
 * kano_hop_pairs: dist[q] = dist(pairs[2q], pairs[2q+1]) for Q pairs in any
 * order, duplicates allowed; one search per distinct source, which stops once
 * all of that source's targets have a distance.  mode 0: distances alone;
 * mode 1: also the canonical paths -- pair q's path has dist[q] + 1 nodes (0
 * when dist[q] < 0) at the prefix sum of those lengths over the pairs before
 * it, *total (nullable) = their sum; kano_hop_pairs_fetch copies the nodes
 * out (-EINVAL after mode 0, after an error and before any call).
 * -EINVAL: a NULL context or array, S / Q < 0, max_hops < 0, an unknown mode,
 * a context holding only a row shard (the search needs every row);
 * -ERANGE: a source or target outside [0, n); -ENOTSUP: S * n > 268,435,456
 * (2^28 distances: ask in slices); -ENOMEM (with a message): a device buffer
 * could not be allocated.  n = 0, S = 0 or Q = 0 give empty results and launch
 * nothing.  The context stays usable after every error. */
int kano_hops(kano_ctx* ctx, int64_t S, const int32_t* sources, int32_t max_hops,
              int32_t* dist /* S*n */, int64_t* info /* 4, or NULL */);
int kano_hop_pairs(kano_ctx* ctx, int64_t Q, const int32_t* pairs /* 2*Q */, int32_t max_hops,
                   int mode /* 0 distances, 1 + paths */, int32_t* dist /* Q */,
                   int64_t* total /* path nodes, or NULL */);
int kano_hop_pairs_fetch(kano_ctx* ctx, int32_t* nodes /* total */);
/* The last kano_hops / kano_hop_pairs' device time in ms, summed over its
 * batches: from a batch's first fill to its last kernel, the waits for the
 * host's per-level reads included, the result copies not; recorded under
 * KANO_TUNE=timing=1, else 0. */
int kano_hops_time(kano_ctx* ctx, float* ms);

/* reverse_matrix / reach_zones: the matrix read by columns, and the pods that
 * can all reach each other.
 * kano_reverse: dst[j][i] = src[i][j] for i, j < n, the bit transpose of the
 * whole matrix on the device.  Bits at positions >= n of a source row's last
 * word (kano_put_rows copies them unmasked) are no edges; every destination
 * row's tail bits are written as zero.  dst is a context of the same n on the
 * same device holding every row (e.g. a context with no policies); afterwards
 * it is an edited matrix, as after kano_copy_matrix, that every query and
 * check of this header reads: row t of it is the set of pods that reach t.
 * src is only read (its matrix, class tables and stored check results are
 * unchanged); its pending work is waited for first, as for kano_hops /
 * kano_group_counts, and a call between pipelined kano_verify steps leaves
 * the next step's results unchanged.  A block moves a tile of 512 source rows
 * by 8 source words through LDS, whole 64-byte segments on both sides.
 * info[2] (nullable) = the bits set in the result, the tiles launched.
 * kano_zones: for two whole matrices A (a) and B (b) of the same n on one
 * device (a == b allowed), over the bits below n,
 *   label[i]   = min({i} u {j : A[i,j] = 1 and B[i,j] = 1})
 *   fan_out[i] = popcount(A[i]), fan_in[i] = popcount(B[i]), cyclic[i] = A[i,i]
 *   info[2] (nullable) = the distinct labels, the pods with label[i] != i.
 * With A the transitive closure of M (kano_path, hops = 0) and B its reverse,
 * label[i] is the smallest member of i's strongly connected component,
 * fan_out / fan_in the pods i eventually reaches / that eventually reach i,
 * and cyclic whether i lies on a cycle.  fan_out, fan_in and cyclic may be
 * NULL; with all three NULL a row stops at its first common bit.  Exact
 * integers.  Both matrices are only read; pending work of both is waited for.
 * -EINVAL: a NULL context, src == dst (kano_reverse), a NULL label, matrices
 * of different n, contexts on two devices, either context holding only a row
 * shard; -ENOMEM (with a message): a device buffer could not be allocated.
 * Errors are reported on dst (kano_reverse) and on a (kano_zones).  n == 0
 * returns 0 before any launch.  Both contexts stay usable after every error. */
int kano_reverse(kano_ctx* src, kano_ctx* dst, int64_t* info /* 2, or NULL */);
int kano_zones(kano_ctx* a, kano_ctx* b, int32_t* label /* n */,
               int32_t* fan_out /* n, or NULL */, int32_t* fan_in /* n, or NULL */,
               uint8_t* cyclic /* n, or NULL */, int64_t* info /* 2, or NULL */);
/* The last kano_reverse's device time on its destination (fill and kernel) and
 * the last kano_zones' on its first context (the kernel), without the copies,
 * in ms; recorded under KANO_TUNE=timing=1, else 0. */
int kano_reverse_time(kano_ctx* ctx, float* ms);
int kano_zones_time(kano_ctx* ctx, float* ms);

/* check_intents: what the cluster is supposed to do, checked against the
 * matrix.  Intent k is a source set src[k] and a destination set dst[k] (W
 * words each, bit j of a set in word j >> 6 at position j & 63, the sets free
 * to overlap each other and those of other intents) and flags[k]: bit 0 set
 * = an allow intent (every source must reach every destination), clear = a
 * deny intent (no source may reach a destination); bit 1 set = the pairs
 * (i, i) are considered too.  With S = the pods of src[k] among the rows
 * r0..r1 this context holds, D = the pods of dst[k] and
 *   C = {(i, j) : i in S, j in D, and i != j unless bit 1 is set},
 * out[6k ..] (int64) =
 *   n_src = |S|, n_dst = |D|, pairs = |C|,
 *   reachable   = #{(i, j) in C : M[i,j] = 1},
 *   violations  = reachable for a deny intent, pairs - reachable for an allow
 *                 intent,
 *   bad_sources = #{i in S : some (i, j) in C is a violation},
 * and witness[2k ..] (int32) = the violating (i, j) smallest by i, then j, or
 * (-1, -1) without one.  Set bits at positions >= n, and bits at positions
 * >= n of a row's last word (kano_put_rows copies them unmasked), are nobody.
 * Exact integers.  Works on every matrix a context holds (built, edited,
 * updated, loaded, path, edge, row shard): the matrix is present (as for
 * kano_get_rows), pending work is waited for, and the passes over the
 * resident rows run on the context's stream in device buffers that are the
 * call's own: both set arrays, the sources' row lists (at most 1 GiB a pass
 * over the intents) and 40 bytes an intent.  The call reads 8 * W bytes of
 * the matrix per source of every intent: 8 * W * (sum of n_src) in all, a row
 * that several intents share once for each.  K == 0, n == 0 or no local rows
 * give zeros and (-1, -1) and launch nothing.  Over row shards every field
 * but n_dst adds up, and the witness is the smallest of the shards'.
 * kano_intent_pairs: one intent's violations as (i, j) int32 pairs with
 * global indices, ascending by i and then j.  Self-contained: the call counts
 * first.  *count is always set (0 on an argument error); pairs NULL asks for
 * the count alone.  With pairs given and count > limit the call returns
 * -ENOSPC and writes no pair.
 * -EINVAL: a NULL context or array (kano_intents: with K > 0), K < 0,
 * limit < 0, a NULL count, flag bits other than 0 and 1;
 * -ENOTSUP: K * W > 134,217,728 words (2^27, 1 GiB a side: ask in slices of
 * K); the sum over the intents of n_src * W > 274,877,906,944 row words (2^38,
 * 2 TiB of reads -- a guard against occupying the device for minutes by
 * accident, known on the host before anything is launched: narrow the
 * selectors or split the call); kano_intent_pairs past 4,194,304 source rows;
 * -ENOMEM (with a message): a device buffer could not be allocated.  No error
 * writes a result.  The context stays usable after every error.  The matrix,
 * the class tables and every stored check result (column words, crosscheck
 * words, shadow and conflict pairs, impact) are unchanged; a call between
 * pipelined kano_verify steps leaves the next step's results unchanged. */
int kano_intents(kano_ctx* ctx, int64_t K, const uint64_t* src /* K*W */,
                 const uint64_t* dst /* K*W */,
                 const int32_t* flags /* K: bit 0 = allow kind, bit 1 = keep self pairs */,
                 int64_t* out /* K*6: n_src, n_dst, pairs, reachable, violations, bad_sources */,
                 int32_t* witness /* K*2 */);
int kano_intent_pairs(kano_ctx* ctx, const uint64_t* src /* W */, const uint64_t* dst /* W */,
                      int32_t flags, int64_t limit, int64_t* count,
                      int32_t* pairs /* 2*limit, or NULL: count only */);
/* The last kano_intents' device time, its kernels without the copies, in ms;
 * recorded under KANO_TUNE=timing=1, else 0. */
int kano_intents_time(kano_ctx* ctx, float* ms);

/* The whole verification pass in one call (the sequence kano_py's
 * sample/example.py and tests/test_basic.py run: build_matrix, then
 * all_reachable, all_isolated, user_crosscheck, system_isolation and
 * policy_shadow) with three host syncs in total.  Results are the
 * reference's return values: ascending pod-index lists, concatenated in idx
 * (capacity 4*n) with counts[4] =
 *   [all_reachable (algorithm.py:4-9), all_isolated (:12-17),
 *    user_crosscheck for the group ids gid (:20-42; 0 when gid is NULL;
 *    ngroups > 0 declares every gid < ngroups, checked on the device, so the
 *    host does not scan gid; ngroups <= 0 scans it; gid NULL with ngroups ==
 *    KANO_STORED_GROUPS uses the groups stored by kano_set_groups),
 *    system_isolation(sys_row) (:45-55; -1 when sys_row is not in this shard)].
 * On a row shard the column lists cover only this shard's rows (combine
 * with kano_col_flags_dev / kano_crosscheck_dev across shards instead).
 * When shadow_count is non-NULL, policy_shadow runs too (kano_shadow) and
 * the pairs are copied to shadow_pairs if count <= shadow_cap (otherwise
 * fetch them with kano_shadow_fetch).  shadow_cap < 0 asks for the count
 * only: every subset test still runs, the pairs are not emitted (broad
 * selectors give ~1e11 of them; kano_shadow_fetch then fails).
 * Completion: the call returns once idx, counts and the pairs are in host
 * memory.  The matrix write (model.py:158-160) may still be running on the
 * context's stream then (KANO_TUNE=async=0 waits for it): every later call
 * on the context is ordered after it, and every entry point other than
 * kano_verify / kano_verify_shard / kano_verify_combine / kano_verify_gather /
 * kano_info waits for it first, so no
 * caller can observe an unfinished matrix. */
int kano_verify(kano_ctx* ctx, int path, const int32_t* gid, int32_t ngroups, int64_t sys_row,
                int32_t* idx, int64_t* counts, int32_t* shadow_pairs, int64_t shadow_cap,
                int64_t* shadow_count);

/* Pipelined verification (no reference counterpart: a serving loop that
 * re-runs build_matrix + the checks on the resident inputs, as the benchmark
 * does).  With on != 0, a kano_verify / kano_verify_gather that completes
 * asynchronously also queues the NEXT call's prologue -- the build's fills
 * and classification up to the member lists, which read only the uploaded
 * tables -- on the context stream behind a gate kernel that polls a
 * page-locked word; the next kano_verify / kano_verify_gather opens the gate
 * on entry (nothing runs before the call that asks for it), so the host's
 * issue of those launches leaves the step's critical path.  Every other entry
 * point, and kano_set_pipeline(ctx, 0), opens the gate, waits and puts the
 * context back as the last call left it.  A device-wide synchronisation
 * outside the engine (hipDeviceSynchronize, torch.cuda.synchronize) while a
 * prologue is queued waits for the gate's timeout (200 ms): call
 * kano_settle first.  Default off. */
int kano_set_pipeline(kano_ctx* ctx, int on);

/* The context's queued work finished: a primed prologue's gate opened (the
 * prologue runs and is put back), an asynchronously completing matrix write
 * waited for.  Afterwards no engine work is pending on the device. */
int kano_settle(kano_ctx* ctx);

/* The pipelined calls' gates (kano_set_pipeline): how long each held the
 * engine stream -- from the end of the previous call's last engine-stream
 * kernel to the next call's bell, i.e. that stream's idle time at the step
 * boundary, timed on the device's wall clock without a profiler.  Over the
 * last min(64, gates since the last reset) gates; settles first.  reset != 0
 * starts a new window. */
int kano_gate_timing(kano_ctx* ctx, int reset, int64_t* gates, double* mean_us,
                     double* max_us);

/* kano_verify for one row shard of a multi-GPU build, in two
 * halves around the ranks' exchange step.
 *   kano_verify_shard: the build of this shard's rows and every check up to
 *     the column words, written to words_dev (DEVICE memory, 3*W uint64:
 *     [column OR | cross | column NAND] over this shard's rows; cross is 0
 *     without groups).  Asynchronous on the context stream.
 *   (the caller gathers the nranks word sets rank-major into one device
 *     buffer on the same stream, e.g. an RCCL all-gather over xGMI)
 *   kano_verify_combine: OR of the gathered sets -- all_isolated[j] = no
 *     shard reaches j (algorithm.py:12-17), all_reachable[j] = no shard
 *     misses j (:4-9), user_crosscheck[j] = some shard crosses (:27-42) --
 *     then the same outputs as kano_verify: the three global lists, this
 *     shard's system_isolation row (-1 when sys_row is elsewhere), and this
 *     shard's policy_shadow pairs (rank order = the reference's order).
 * with_shadow: 0 no policy_shadow, 1 the pairs, 2 the pair count only (then
 * kano_verify_combine takes shadow_cap < 0). */
int kano_verify_shard(kano_ctx* ctx, int path, const int32_t* gid, int32_t ngroups,
                      int64_t sys_row, int with_shadow, uint64_t* words_dev);
int kano_verify_combine(kano_ctx* ctx, const uint64_t* gathered_dev, int32_t nranks,
                        int32_t* idx, int64_t* counts, int32_t* shadow_pairs, int64_t shadow_cap,
                        int64_t* shadow_count);

/* kano_verify_shard, the exchange and kano_verify_combine in ONE call, the
 * exchange being an RCCL all-gather issued by the engine itself on the
 * context stream: comm is the caller's ncclComm_t (e.g. torch's
 * ProcessGroupNCCL._comm_ptr()) over nranks ranks, this context's rank
 * among them being the comm's own.  No host code runs between the shard's
 * checks and the combine (the caller's per-collective overhead is gone).
 * The RCCL symbols are resolved at the first call from the process (the
 * library that created comm, e.g. torch's bundled librccl), else
 * librccl.so; without them the call fails (-ENOSYS) and nothing runs.
 * comm NULL emulates rank 0 of nranks on this device (a timing diagnostic,
 * bench.py --rank-of: the all-gather becomes a device copy into rank 0's
 * slot, the other ranks' words stay zero, so the lists are partial).
 * Outputs as kano_verify_combine; with_shadow as kano_verify_shard. */
int kano_verify_gather(kano_ctx* ctx, int path, const int32_t* gid, int32_t ngroups,
                       int64_t sys_row, int with_shadow, void* comm, int32_t nranks,
                       int32_t* idx, int64_t* counts, int32_t* shadow_pairs, int64_t shadow_cap,
                       int64_t* shadow_count);

/* The checks of kano_verify_shard over the matrix rows AS THEY STAND --
 * after kano_add_policies / kano_remove_policies (or edits), which
 * kano_verify, a rebuild from the tables, would undo: this shard's
 * [OR | cross | NAND] column words to words_dev (3*W u64), the system row
 * kept if owned.  Gather the ranks' words and finish with
 * kano_verify_combine (shadow_count NULL); one rank: nranks = 1 with its own
 * words.  Column checks of algorithm.py:4-42 and system_isolation (:45-55)
 * on an incrementally updated, row-sharded matrix. */
int kano_checks_shard(kano_ctx* ctx, const int32_t* gid, int32_t ngroups, int64_t sys_row,
                      uint64_t* words_dev);

/* user_hashmap (algorithm.py:20-24) as resident input: the group id of
 * every pod uploaded once (like the label tables), for kano_verify with
 * gid = NULL, ngroups = KANO_STORED_GROUPS.  ngroups <= 0: max(gid) + 1. */
#define KANO_STORED_GROUPS (-1)
int kano_set_groups(kano_ctx* ctx, const int32_t* gid, int32_t ngroups);

/* Timing of the last kano_build / kano_shadow stages on the context stream
 * (HIP events), milliseconds: [classes, allow, select + plan, rows stage,
 * shadow, build total, k_rows kernel alone, policy_impact].  Slots 0-5 are
 * recorded only when the context was created with KANO_TUNE=timing=1 (each
 * event costs host time on the launch path); slot 6 always; slot 7, the last
 * kano_policy_impact's fill and kernel without the copy, also under timing=1. */
int kano_stage_times(kano_ctx* ctx, float* ms /* 8 */);

/* k_rows launch times (the matrix write of model.py:158-160; HIP events on
 * its stream) accumulated over the launches since the last reset: out[4] =
 * [sum ms, launches, min ms, max ms]; reset != 0 zeroes the sums after
 * reading.  Waits for the context's work first (a benchmark reads it after
 * its timed region, kano_verify's own launches stay asynchronous). */
int kano_rows_timing(kano_ctx* ctx, double* out /* 4 */, int reset);

/* The heavy classes' MFMA contraction (k_heavy_gemm_f4 / k_heavy_mc_mfma on
 * the block-scaled fp4 MFMA, 0/1 operands; the dense path of build_matrix,
 * model.py:158-160 as Sel x Allow thresholded > 0) timed per build (HIP
 * events around its launches on the context stream): out[4] = [sum ms,
 * builds timed, sum of algorithmic ops (2 x heavy row classes x policies x
 * column classes per build), the last build's ops];
 * reset != 0 zeroes the sums after reading. */
int kano_mfma_timing(kano_ctx* ctx, double* out /* 4 */, int reset);

/* Multi-hop reachability, replacing kubesv's
 * `path` relation (kubesv/kubesv/constraint.py:233-237: path :- edge;
 * path :- edge o edge) with kano's matrix as `edge`.  Writes into dst's matrix
 *   hops = 2: P = M | M.M  (the kubesv rule),
 *   hops = k >= 1: pairs joined by a path of at most k edges,
 *   hops = 0: the transitive closure M+ (paths of any length >= 1),
 * computed from src's build at class level (row / column classes; identity
 * classes after an edit of src's matrix).  dst is a context of the same n
 * holding a matrix (e.g. a build with no policies); afterwards it is an
 * edited matrix that every query and check of this header reads.  src must
 * hold every row (no row shard).  mode: KANO_PATH_AUTO picks per step
 * between the semi-naive bit-packed OR (sparse delta) and the fp4 MFMA
 * contraction (dense); KANO_PATH_BITWISE / KANO_PATH_MFMA force one.
 * info (nullable, 6 slots): [composition steps that added pairs, steps run,
 * steps on the MFMA, row classes, column classes, identity classes]. */
int kano_path(kano_ctx* src, kano_ctx* dst, int hops, int mode, int64_t* info);

/* kano_path on one row shard of a multi-GPU build, in two
 * halves around one exchange: T, the one-hop table over column classes, is
 * an OR over all rows, everything else is per row.
 *   kano_path_shard_words: words of T (0 for an edited shard: unsupported).
 *   kano_path_shard: this shard's part of T into t_dev (DEVICE memory).
 *   (the caller gathers the ranks' parts rank-major into one device buffer,
 *   e.g. an RCCL all-gather over xGMI)
 *   kano_path_combine: OR of the parts, then this shard's rows of the path
 *   matrix into dst (a matrix context over the same rows). */
int kano_path_shard_words(kano_ctx* src, int64_t* words);
int kano_path_shard(kano_ctx* src, uint64_t* t_dev);
int kano_path_combine(kano_ctx* src, kano_ctx* dst, const uint64_t* gathered_dev, int32_t nranks,
                      int hops, int mode, int64_t* info);

/* The on-disk / tooling row format: rows of M as
 * kano_py holds them, bitarray bytes in bitarray's default big-endian bit
 * order (kano_py/kano/model.py:136-139,158-160; bitarray.tobytes(): bit j of
 * a row is bit 7 - (j & 7) of byte j >> 3, pad bits zero), ceil(n / 8) bytes
 * per row, rows [r0, r0 + nrows) of this shard.  kano_import_rows writes such
 * rows back (an edit of M, like kano_put_rows; pad bits are cleared). */
int kano_export_rows(kano_ctx* ctx, int64_t r0, int64_t nrows, uint8_t* dst);
int kano_import_rows(kano_ctx* ctx, int64_t r0, int64_t nrows, const uint8_t* src);

/* Incremental policy updates.  The matrix after
 * the update equals ReachabilityMatrix.build_matrix over the updated policy
 * list (kano_py/kano/model.py:125-165); only rows the changed policies select
 * are written.  Policy ids are stable: the build's 0..P-1, then added ones in
 * order (first_id returns the batch's first).  kano_add_policies takes the
 * new policies' working terms as kano_set_policies does; term columns
 * >= the build's ncols index ncols_x extra pod columns (xval[c*n + i], the
 * batch's new keys / custom matchers, appended to earlier batches' extras).
 * kano_remove_policies marks ids removed and rewrites the rows they selected
 * from the alive policies (-EINVAL after an explicit edit of M).  Afterwards
 * the matrix reads as an edited one; kano_build / kano_verify rebuild from
 * the uploaded tables and drop the updates.  kano_added_policy_sets returns
 * an added policy's working_select_set / working_allow_set (model.py:119-121). */
int kano_add_policies(kano_ctx* ctx, int64_t Pn, int32_t ncols_x, const int32_t* xval,
                      const int64_t* sel_off, const int32_t* sel_col, const int32_t* sel_val,
                      const int64_t* alw_off, const int32_t* alw_col, const int32_t* alw_val,
                      int64_t* first_id);
int kano_remove_policies(kano_ctx* ctx, int64_t count, const int64_t* ids);
int kano_added_policy_sets(kano_ctx* ctx, int64_t id, uint64_t* sel, uint64_t* allow);

/* Kubernetes matchExpressions requirements (an
 * extension of kano_py's equality selectors; semantics of the requirements
 * kubesv adapts, kubesv/kubesv/model.py:127-160).  Appends E pod columns
 * ncols .. ncols+E-1 computed on the device: 1 where pod i meets requirement
 * e, else 0 -- op 0 In (the key's value id listed in vals[off[e]..off[e+1]),
 * sorted), 1 NotIn (absent or not listed), 2 Exists, 3 DoesNotExist; col[e]
 * is the key's column (-1: no pod carries it).  Policies then use the term
 * (ncols + e, 1).  Call after kano_set_pods, before kano_set_policies. */
int kano_set_expressions(kano_ctx* ctx, int32_t E, const int32_t* col, const int32_t* op,
                         const int64_t* off, const int32_t* vals);

/* kubesv's edge relation (kubesv/kubesv/
 * constraint.py:191-231, which replaces kano's M with a K8s reading of the
 * policies: namespaces, namespaceSelector, per-direction rules).  in_t and
 * eg_t hold full n x n builds, in_t[sel][src] = ingress_traffic(src, sel) and
 * eg_t[sel][dst] = egress_traffic(dst, sel) (one kano policy per (policy,
 * peer), built by the host from the K8s objects); dst (an n x n context, e.g.
 * kano_create + kano_set_pods with no policies) receives
 *   edge[src][dst] = OR_sel in_t[sel][src] AND eg_t[sel][dst]
 *                    | eg_t[src][dst]          if flags & KANO_K8S_SELF
 * (check_self_ingress_traffic: ingress_traffic(sel, sel)), or every pair if
 * flags & KANO_K8S_ALL (check_select_by_no_policy with a pod selected by no
 * policy: that pod receives from and sends to everyone).  dst then reads as
 * an edited matrix (every check, kano_path for kubesv's path relation).
 * dst may hold a row shard [r0, r1) (kano_set_shard): only its rows are
 * written (class-level form; the sources are full builds, typically made
 * with kano_build_classes so their own matrices are never written).
 * Two forms: class level when both sources are unedited builds (edge[src]
 * [dst] = Ec[cc_i(src)][cc_e(dst)] | Mc_e[rc_e(src)][cc_e(dst)], Ec from two
 * OR-products over the builds' classes, then one expansion to pods), else --
 * or with KANO_K8S_PODS -- pod level (InT transposed, one OR-product).
 * info (nullable): [0] the bits the pod-level product added beyond the self
 * term (-1 for the class-level form). */
#define KANO_K8S_SELF 1
#define KANO_K8S_ALL  2
#define KANO_K8S_PODS 4
/* KANO_K8S_DST_EG: dst is itself a build of eg_t's tables over its row range
 * (kano_build writes EgT's rows, the self term), and the product is OR-ed
 * into it in place -- no expansion of the egress classes. */
#define KANO_K8S_DST_EG 8
int kano_k8s_edge(kano_ctx* in_t, kano_ctx* eg_t, kano_ctx* dst, int flags, int64_t* info);

/* k8s.connectivity: the reading of NetworkPolicies a cluster enforces
 * (networking.k8s.io/v1), from two class-level builds the host compiles
 * (kano/k8s.py compile_conformant): eg holds E[src][dst] (an entry selects an
 * Egress-typed policy's pods and allows one peer of one rule), in holds
 * I[dst][src] likewise for Ingress.  Every policy of a type contributes an
 * entry, so a pod is isolated in a direction iff some entry of that build
 * selects it.  dst's rows :=
 *   allowed[s][d] = (s == d and flags & KANO_K8S_CONN_SELF)
 *                 | (!isoE[s] | E'[s][d]) & (!isoI[d] | I'[d][s])
 * with E' / I' over the kept entries only (keep_e / keep_i: one flag per
 * engine id, NULL keeps all -- a port query keeps the entries whose rule
 * counts on that port); isolation always reads every entry.
 * eg and in are full, unedited builds (kano_build_classes: their matrices are
 * neither read nor written); only their class tables are read.  A source
 * without policies has no classes and constrains nothing: that side is all
 * ones.  dst is a matrix context of the same n and device (an empty build),
 * optionally a row shard (kano_set_shard): every word of every held row is
 * written, bits at positions >= n and the words W .. ldM - 1 are zero, and
 * dst then reads as an edited matrix, like kano_policy_subset's destination.
 * The rows of row shards concatenate.
 * info (nullable) = [egress-isolated pods, ingress-isolated pods, kept egress
 * entries, kept ingress entries]; the first two are counted by the run (two
 * small launches, left out with info NULL) and stay 0 when nothing is
 * launched.
 * kano_k8s_isolated: out[i] = 1 iff some policy of ctx's build selects pod i
 * (the row class's list is not empty), computed on the device, one copy.
 * -EINVAL: a NULL context (or out), dst equal to a source, contexts of
 * different devices or n, nids_e / nids_i other than the sources' P;
 * -ENOTSUP: a source holding a row shard, policy lists, added or removed
 * policies or edited rows, more than 4,194,240 held rows; -ENOMEM (with a
 * message): a device buffer could not be allocated.  kano_k8s_conn reports its
 * errors on dst; the contexts stay usable after every error.  n == 0 or no
 * held rows launch nothing.  The device buffers are the call's own (the keep
 * flags, the class-level rows Re, Ri and Ri transposed), freed on return; the
 * sources' tables and stored results are unchanged.  Exact bits.
 * Two forms write the same bits: direct (every held row gathered from the two
 * class-level tables) and streamed (both tables' class rows expanded to pod
 * words once, then M[s] = XE[rc_e(s)] & XT[cc_i(s)]; taken when the class rows
 * number at most half the held rows, as kano_k8s_edge takes its own).
 * KANO_K8S_CONN_DIRECT / KANO_K8S_CONN_STREAM force one (a table of more than
 * 4,194,240 class rows is never streamed, whatever the flag). */
#define KANO_K8S_CONN_SELF 1
#define KANO_K8S_CONN_DIRECT 2
#define KANO_K8S_CONN_STREAM 4
int kano_k8s_conn(kano_ctx* eg, kano_ctx* in, kano_ctx* dst, int flags,
                  int64_t nids_e, const uint8_t* keep_e /* nids_e, nullable: all */,
                  int64_t nids_i, const uint8_t* keep_i /* nids_i, nullable: all */,
                  int64_t* info /* 4, nullable */);
int kano_k8s_isolated(kano_ctx* ctx, uint8_t* out /* n */);
/* k8s.connectivity with AdminNetworkPolicy tiers (policy.networking.k8s.io/
 * v1alpha1: Allow / Deny / Pass above the NetworkPolicies, the
 * BaselineAdminNetworkPolicy below them).  The host compiles the rules of all
 * three kinds into the same two builds (an entry selects a rule's subject and
 * allows one peer) and gives every engine id a code = level * 4 + action:
 * action 0 allow, 1 deny, 2 pass, 3 isolates only; 0xffffffff: the entry is
 * dropped (its rule does not count on the queried port).  A level is one rule:
 * the levels below np_level are the admin rules in evaluation order, np_level
 * is the NetworkPolicy tier (action 0, or 3 for an entry that selects without
 * allowing: a policy without rules, or a rule the port drops), the levels above
 * it the baseline's rules in order.  Per direction (egress: subject x = src,
 * peer y = dst, build eg; ingress: x = dst, y = src, build in) over the live
 * entries selecting x and allowing y:
 *   the lowest admin level decides -- allow, deny -- or passes; where none
 *   matches or it passes: x selected by some live entry at np_level (isolated)
 *   ? some allow entry at np_level matches : the lowest baseline level
 *   decides, and where none matches the pair is allowed.
 * (Several actions on one level resolve allow, deny, pass in that order.)
 *   allowed[s][d] = (s == d and flags & KANO_K8S_CONN_SELF) | eg(s, d) & in(d, s)
 * Sources, destination, flags, forms, limits and error reporting as for
 * kano_k8s_conn; additionally -EINVAL for NULL codes with nids > 0, an
 * np_level of 2^30 or more (so no level reaches 2^30) and a live code that
 * passes at or above np_level, only isolates off np_level or denies at
 * np_level.  iso_e / iso_i (nullable, n bytes each): 1 iff the pod is selected
 * by a live entry at np_level (some NetworkPolicy of that type selects it);
 * zeros for a side without classes.  info (nullable) = [egress-isolated pods,
 * ingress-isolated pods, live egress codes, live ingress codes]; the first two
 * stay 0 when nothing is launched (n == 0).  A destination holding no rows
 * still gets the flags and counts.  The device buffers (codes, ordered copies,
 * class-level rows, flags) are the call's own, freed on return.  Exact bits. */
int kano_k8s_conn_tiers(kano_ctx* eg, kano_ctx* in, kano_ctx* dst, int flags,
                        int64_t nids_e, const uint32_t* code_e /* nids_e */, uint32_t np_level_e,
                        int64_t nids_i, const uint32_t* code_i /* nids_i */, uint32_t np_level_i,
                        uint8_t* iso_e /* n, nullable */, uint8_t* iso_i /* n, nullable */,
                        int64_t* info /* 4, nullable */);
/* KANO_TUNE timing=1: the last kano_k8s_conn's or kano_k8s_conn_tiers' device
 * time in ms on its destination (the fills and the kernels, no copies), else 0. */
int kano_k8s_conn_time(kano_ctx* ctx, float* ms);
/* K8sConnectivity.pair_verdicts: for each of Q pod pairs (src, dst), which tier
 * and which entry decide it under the rule of kano_k8s_conn_tiers above, per
 * direction (egress: subject src, peer dst, build eg; ingress: subject dst,
 * peer src, build in), from the same two builds and codes (a cluster without
 * admin or baseline rules: np_level 0 and the codes 0 / 3).  Over the live
 * entries selecting the subject and allowing the peer, ordered by (code, id):
 * the first below np_level decides (tier admin) unless it passes -- then it
 * is the passed entry; else a subject selected by a live entry at np_level
 * (isolated; no allowing peer needed) is decided in tier network: allow by the
 * first entry of code np_level * 4, else deny without a decider; else the first
 * entry above np_level decides (tier baseline); else tier default, allow.  A
 * decider is therefore the smallest engine id at the winning code.
 *   verdict[q]: bit 0 allowed, bit 1 self traffic (src == dst and flags &
 *   KANO_K8S_CONN_SELF), bits 2-3 the egress tier (0 default, 1 admin, 2 network,
 *   3 baseline), bit 4 egress denies, bits 5-6 the ingress tier, bit 7 ingress
 *   denies; allowed = self | !(bit 4 | bit 7).
 * decider_* / passed_* (nullable, Q each): engine ids of the respective build,
 * -1 where there is none.  counts (nullable, 18) = [allowed, self, then per
 * egress tier 0..3 its (allow, deny) pairs, then the same 8 for ingress].
 * Pairs in any order, duplicates allowed; only flags & KANO_K8S_CONN_SELF is
 * read.  A side without policies has no classes: (default, allow).
 * -EINVAL: a NULL context, pairs or verdict (Q > 0) or codes (nids > 0), Q < 0,
 * contexts of two devices or different n, nids other than the sources' P, an
 * np_level of 2^30 or more, a live code illegal for its level (as above);
 * -ERANGE: a pair index outside [0, n); -ENOTSUP: a source holding a row
 * shard, policy lists, added or removed policies or edited rows; -ENOMEM (with
 * a message): a device buffer could not be allocated.  Errors are reported on
 * eg; both contexts stay usable after every error.  Q == 0 or n == 0 launch
 * nothing.  The device buffers (pairs, codes, results) are the call's own,
 * freed on return; the sources' tables and stored results are unchanged.
 * Two forms give the same answers: a lane per pair, or a wave per pair (taken
 * when the two builds' mean lists together exceed 16 entries); KANO_TUNE
 * kpf=1 / 2 forces lane / wave, kpgrid=K caps the grid at K blocks. */
int kano_k8s_pair_verdicts(kano_ctx* eg, kano_ctx* in, int flags /* KANO_K8S_CONN_SELF */,
                           int64_t Q, const int32_t* pairs /* 2*Q: src, dst */,
                           int64_t nids_e, const uint32_t* code_e, uint32_t np_level_e,
                           int64_t nids_i, const uint32_t* code_i, uint32_t np_level_i,
                           uint8_t* verdict /* Q */,
                           int32_t* decider_e, int32_t* passed_e, /* Q each, nullable */
                           int32_t* decider_i, int32_t* passed_i,
                           int64_t* counts /* 18, nullable */);
/* KANO_TUNE timing=1: the last kano_k8s_pair_verdicts' device time in ms on
 * eg (the kernel, no copies), else 0. */
int kano_k8s_pair_verdicts_time(kano_ctx* eg, float* ms);
/* K8sConnectivity.rule_usage: which entries of the two builds do anything at
 * all, counted exactly over every ordered pair (x, y) of [0, n)^2 and per
 * direction (subject x, peer y: egress x = src on eg, ingress x = dst on in).
 * With flags & KANO_K8S_CONN_SELF the n pairs x == y are left out of every
 * count (self traffic is allowed before any rule is read); without it they are
 * resolved like any other pair.  tier, deny, decider and passed of a pair are
 * kano_k8s_pair_verdicts' above, unchanged.  Per direction:
 *   decided[id]  the pairs whose decider is entry id
 *   passed[id]   the pairs whose passed entry is id
 *   sole[g]      the pairs of tier network that are allowed where every live
 *                entry of code np_level * 4 that selects x and allows y belongs
 *                to group g
 *   tiers        per tier 0..3 its (allow, deny) pairs, 8 values; egress first.
 *                They sum to n * n, or n * n - n with the self flag.
 * group_* (nullable, nids each): an int32 per engine id, non-decreasing in the
 * id and from 0 on (the entries of one rule are contiguous); NULL: every id
 * its own group.  sole_* holds last group + 1 values.
 * decided == 0 and passed == 0: the entry is dead -- removing it changes no
 * verdict of this query.  For a group at np_level, sole == 0 says removing its
 * entries alone changes no verdict, and removal denies exactly sole pairs of
 * that direction; sole[g] <= the sum of decided over g.
 * A side without policies has no classes: its arrays are zero and the whole
 * domain is (default, allow).  n == 0 launches nothing and returns zeros.
 * The answer depends only on (row class of x, column class of y): one walk of
 * every class's ordered list resolves 64 column classes a word and weights the
 * newly decided bits by the class sizes, so the cost is that of
 * kano_k8s_conn_tiers' class step, not of n * n pair walks.  The counters are
 * 64-bit integer atomics: exact and independent of the order of arrival.
 * Errors as kano_k8s_pair_verdicts (source state, nids, codes; reported on eg,
 * both contexts stay usable); -EINVAL also for groups that decrease or start
 * below 0.  The device buffers are the call's own, freed on return; the
 * sources' tables and stored results are unchanged.  KANO_TUNE kugrid=K caps
 * the class kernel's grid at K blocks. */
int kano_k8s_rule_usage(kano_ctx* eg, kano_ctx* in, int flags /* KANO_K8S_CONN_SELF */,
                        int64_t nids_e, const uint32_t* code_e, uint32_t np_level_e,
                        const int32_t* group_e /* nids_e, nullable */,
                        int64_t nids_i, const uint32_t* code_i, uint32_t np_level_i,
                        const int32_t* group_i /* nids_i, nullable */,
                        int64_t* decided_e, int64_t* passed_e, /* nids_e each, nullable */
                        int64_t* sole_e /* groups of egress, nullable */,
                        int64_t* decided_i, int64_t* passed_i, int64_t* sole_i,
                        int64_t* tiers /* 16: egress 8, ingress 8; nullable */);
/* KANO_TUNE timing=1: the last kano_k8s_rule_usage's device time in ms on eg
 * (the fills and the kernels, no copies), else 0. */
int kano_k8s_rule_usage_time(kano_ctx* eg, float* ms);

/* kano_build without the matrix write (model.py:125-165 up to the class-level
 * matrix Mc, the lists and the column checks): M is written on first use
 * (kano_get_rows, kano_path, ...).  For sources of kano_k8s_edge, which reads
 * only Mc and the classes. */
int kano_build_classes(kano_ctx* ctx, int path);

/* Host time of kano_verify (no reference counterpart; diagnostics for the
 * benchmark, always recorded: a few clock reads per call), microseconds:
 * out[20] = [calls, front sum, back sum, size-wait sum, gap between calls sum,
 *            front max, back max, size-wait max, call max,
 *            size wait 1 max, size wait 2 max, size wait 3 max,
 *            back's parts max: lists + matrix-write launch, policy_shadow's
 *            emission launches, wait for the tail's copies, list copy issue,
 *            pair copy issue, event records, 0, 0];
 * "front" is the build and checks up to the column words, "back" the result
 * lists, the matrix write's launch and the wait for the host results.
 * reset != 0 zeroes them after reading. */
int kano_host_times(kano_ctx* ctx, double* out /* 20 */, int reset);

/* One process over G devices (SURVEY.md §8(b) kano_init(ngpu), §8(e) row
 * sharding; no reference counterpart: kano_py is single-process).  The group
 * owns G member contexts, member r on device devices[r] (NULL: r) with its
 * own streams, each driven by its own persistent host thread (started with
 * the group): a group call hands every member its part and returns when all
 * are done, so the members' uploads, builds and host syncs overlap.  The
 * column checks exchange the members' [OR | cross | NAND] words: ncclAllGather
 * over xGMI (communicators from ncclCommInitAll; mode 1) when the devices are
 * distinct or the flag KANO_GROUP_RCCL asks for it (also for one member),
 * device-to-device copies (mode 2) when members share a device or
 * KANO_GROUP_COPY (flag or environment variable) asks for them; every member
 * ORs the gathered words on its device.  An RCCL exchange that should run and
 * cannot (librccl missing, ncclCommInitAll failing) fails the create: there is
 * no silent fall back to copies.  kano_group_last_error(NULL) says why the
 * last create on this thread failed.
 *   kano_group_upload: kano_set_pods (+ kano_set_expressions when E > 0) +
 *     kano_set_policies on every member, member r's rows [bounds[2r],
 *     bounds[2r+1]) (kano_set_shard) -- the inputs of ReachabilityMatrix.
 *     build_matrix (kano_py/kano/model.py:125-165), all members at once.
 *   kano_group_build: kano_build on every member at once (the whole matrix).
 *   kano_group_set_groups: kano_set_groups on every member (user_hashmap's
 *     groups, algorithm.py:20-24); kano_group_verify / _checks then take
 *     gid = NULL, ngroups = KANO_STORED_GROUPS.  gid holds n entries (n of
 *     kano_group_upload), as for kano_set_groups: the members read all n.
 *   kano_group_verify: kano_verify over the whole matrix -- the three
 *     column lists (all_reachable, all_isolated, user_crosscheck) of every
 *     row, system_isolation(sys_row) from the row's owner, policy_shadow's
 *     pairs concatenated in rank order (= the reference's container order);
 *     arguments as kano_verify_shard / kano_verify_combine (with_shadow 0 /
 *     1 pairs / 2 count only).  One hand-off: every member's shard step, the
 *     exchange between two barriers of the member threads, every combine.
 *   kano_group_checks: the same checks over the members' matrices as they
 *     stand (kano_checks_shard), no policy_shadow.
 *   kano_group_add_policies / kano_group_remove_policies: kano_add_policies /
 *     kano_remove_policies on every member's rows (§8(f) rank 4); the
 *     members' new policy ids agree (first_id).
 *   kano_group_path: kubesv's path relation (kubesv/kubesv/constraint.py:
 *     233-237) of src's row-sharded matrix into dst (a group over the same
 *     devices and row bounds holding an n x n matrix): every member's part of
 *     the one-hop table (kano_path_shard), one exchange (the transport
 *     above), every member's rows (kano_path_combine); info as kano_path.
 *   kano_group_exchange_timing: enable >= 0 switches timing of the verify
 *     exchange (two events on member 0's stream) on / off; out (may be NULL)
 *     = [exchanges timed, total ms, max ms]; reset != 0 zeroes them.
 * kano_group_info: out[0] = G, out[1] = exchange mode. */
typedef struct kano_group kano_group;
#define KANO_GROUP_LEAN 1   /* lean members (kano_create_lean) */
#define KANO_GROUP_RCCL 2   /* the RCCL exchange even for one member; an error if it fails */
#define KANO_GROUP_COPY 4   /* device copies even over distinct devices */
int  kano_group_create(int ngpu, const int* devices, kano_group** out);
/* the same with lean members (kano_create_lean): for the drop-in build_matrix */
int  kano_group_create_lean(int ngpu, const int* devices, kano_group** out);
int  kano_group_create_ex(int ngpu, const int* devices, int flags /* KANO_GROUP_* */,
                          kano_group** out);
void kano_group_destroy(kano_group* g);
const char* kano_group_last_error(const kano_group* g);
int  kano_group_info(kano_group* g, int32_t* out /* 2 */);
int  kano_group_member(kano_group* g, int r, kano_ctx** ctx);
int  kano_group_upload(kano_group* g, int64_t n, int32_t ncols, const int32_t* pod_val,
                       int32_t E, const int32_t* ecol, const int32_t* eop, const int64_t* eoff,
                       const int32_t* evals, int64_t P, const int64_t* sel_off,
                       const int32_t* sel_col, const int32_t* sel_val, const int64_t* alw_off,
                       const int32_t* alw_col, const int32_t* alw_val,
                       const int64_t* bounds /* 2 G */);
int  kano_group_build(kano_group* g, int path);
int  kano_group_set_groups(kano_group* g, const int32_t* gid, int32_t ngroups);
int  kano_group_verify(kano_group* g, int path, const int32_t* gid, int32_t ngroups,
                       int64_t sys_row, int with_shadow, int32_t* idx, int64_t* counts,
                       int32_t* shadow_pairs, int64_t shadow_cap, int64_t* shadow_count);
int  kano_group_checks(kano_group* g, const int32_t* gid, int32_t ngroups, int64_t sys_row,
                       int32_t* idx, int64_t* counts);
int  kano_group_add_policies(kano_group* g, int64_t Pn, int32_t ncols_x, const int32_t* xval,
                             const int64_t* sel_off, const int32_t* sel_col,
                             const int32_t* sel_val, const int64_t* alw_off,
                             const int32_t* alw_col, const int32_t* alw_val, int64_t* first_id);
int  kano_group_remove_policies(kano_group* g, int64_t count, const int64_t* ids);
int  kano_group_path(kano_group* src, kano_group* dst, int hops, int mode, int64_t* info /* 6 */);
int  kano_group_exchange_timing(kano_group* g, int enable, double* out /* 3 */, int reset);

/* Page-locked host buffers for fast device-to-host result copies. */
int  kano_host_alloc(size_t bytes, void** out);
void kano_host_free(void* p);

/* The device memory the engine's buffers hold in this process, every context
 * and every call in progress together: the bytes and the number of buffers
 * (either may be NULL).  A destroyed context and a returned call hold none. */
int  kano_device_bytes(int64_t* bytes, int64_t* buffers);

#ifdef __cplusplus
}
#endif
#endif /* KANO_HIP_H */
