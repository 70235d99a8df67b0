/*
 * matfact_hip.h -- C ABI of the MI355X (gfx950) backend for the matrix-factorisation hot path of
 * vladstojna/recommender-system.  Plain C: pointers and sizes only, callable from the reference's C
 * `main` (or from cgo/ctypes/JNI) with no C++ or torch types in any signature.
 *
 * The reference has no plugin API; the seam a maintainer would cut is the pair of calls its main makes
 * (matFact.c:124 and :127).  Each entry point below names the reference interface it replaces.
 *
 *   LEVEL 1 -- host-buffer drop-ins (what the reference's main would call)
 *     mf_backend_factorize   replaces  matrix_factorization()           matFact.c:29-59 (iteration loop)
 *     mf_backend_recommend   replaces  mat2d_prod() + print_output()    mat2d.c:100-113, matFact.c:10-27
 *     mf_backend_run         both, factors stay in HBM between the two  matFact.c:124-127
 *
 *   LEVEL 2 -- resident shard plan (one per GPU / per rank; what the MPI variant's per-rank state is)
 *     mf_plan_*              replaces  the per-rank body of matrix_factorization()  matFact-mpi.c:155-214
 *                            and compute_reduce_output()                            matFact-mpi.c:51-103
 *
 * Conventions: the caller owns every host buffer; the backend owns device memory for the duration of a
 * level-1 call or the lifetime of a plan.  Every function returns MF_OK (0) or a negative mf_status and
 * never calls exit() (the reference's die(), util.c:7-10, stays in the caller).  The library is HIP-only:
 * there is no CPU fallback -- with no usable GPU every compute entry returns MF_ERR_NO_DEVICE.
 */
#ifndef MATFACT_HIP_H
#define MATFACT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MATFACT_HIP_ABI_VERSION 5   /* 2: mf_shard.users_ext, seeded user sweep, scored recommend (2-D tiles)
                                       3: mf_backend_multi_last_timing, MF_MULTI_REDUCE=peer|rccl; the reserved
                                          MF_PLAN_RELAXED_ORDER flag is gone (never implemented: an atomic sum is
                                          order-nondeterministic and slower than the owner-computes gather)
                                       4: mf_shard.items_pitch / users_pitch, mf_backend_row_pitch, mf_plan_row_pitch
                                       5: mf_backend_multi_last_counters (one host thread per shard enqueues its
                                          iterations; MF_MULTI_THREADS=0 keeps the single enqueueing thread);
                                          additive since: top-N recommendations (MF_TOPN_MAX, mf_plan_recommend_topn,
                                          mf_plan_recommend_topn_info, mf_backend_recommend_topn, mf_backend_run_topn);
                                          loss (mf_plan_loss, mf_plan_set_heldout, mf_plan_iterate_monitored,
                                          mf_backend_loss, mf_backend_loss_total);
                                          ranks of the held-out entries (mf_plan_rank_heldout, mf_plan_rank_heldout_info,
                                          mf_backend_rank_metrics);
                                          similar items (mf_plan_similar_items, mf_plan_similar_items_info,
                                          mf_backend_similar_items);
                                          L2 regularisation (mf_plan_set_regularization, mf_plan_get_regularization,
                                          mf_plan_penalty, mf_backend_run_reg);
                                          frozen factor columns and biases (mf_plan_set_frozen_columns,
                                          mf_plan_get_frozen_columns, mf_backend_bias_mean, mf_backend_bias_pack,
                                          mf_backend_bias_unpack, mf_backend_run_biased);
                                          heavy-ball momentum (mf_plan_set_momentum, mf_plan_get_momentum,
                                          mf_plan_upload_previous, mf_plan_download_previous, mf_backend_run_momentum);
                                          per-entry confidence weights (mf_plan_create_weighted, mf_plan_weight_total,
                                          mf_backend_run_weighted);
                                          box-constrained factors (mf_bounds, mf_plan_set_bounds, mf_plan_get_bounds,
                                          mf_plan_project, mf_plan_bounds_active, mf_backend_run_bounded);
                                          adaptive step sizes (mf_adaptive, mf_plan_set_adaptive, mf_plan_get_adaptive,
                                          mf_plan_reset_adaptive, mf_plan_adaptive_finish,
                                          mf_plan_download_adaptive_state, mf_plan_upload_adaptive_state,
                                          mf_backend_run_adaptive) */

/* == non_zero_entry, datatypes.h:10-15: the (user, item, rating) triple, 16 bytes, array-of-structs */
typedef struct mf_entry {
	int32_t row;
	int32_t col;
	double value;
} mf_entry;

/* The parsed `.in` header plus the entries (matFact.c:79-105; dataset_info datatypes.h:17-27). */
typedef struct mf_problem {
	int32_t users;          /* rows of A, rows of L                 */
	int32_t items;          /* columns of A, rows of R (R is kept transposed, matFact.c:117) */
	int32_t features;       /* K                                    */
	int32_t iters;
	double alpha;
	int64_t nnz;            /* the reference holds this in an int   */
	const mf_entry *entries; /* file order; the reference's inputs are (row, col)-sorted and the
	                            recommendation mask (print_output's cursor) relies on it */
} mf_problem;

typedef enum mf_status {
	MF_OK = 0,
	MF_ERR_ARGUMENT = -1,     /* NULL pointer, negative size, index out of range                    */
	MF_ERR_NO_DEVICE = -2,    /* no HIP device / device index out of range                          */
	MF_ERR_HIP = -3,          /* a HIP runtime call failed; mf_backend_last_hip_error() has its text */
	MF_ERR_NO_MEMORY = -4,    /* host or device allocation failed                                   */
	MF_ERR_UNSUPPORTED = -5,  /* shape outside what the kernels are built for (e.g. K too large)    */
	MF_ERR_STATE = -6         /* plan used before factors were uploaded, etc.                       */
} mf_status;

const char *mf_backend_strerror(int status);
const char *mf_backend_last_hip_error(void);
int mf_backend_abi_version(void);
int mf_backend_device_count(void);            /* >= 0, or a negative mf_status */

/* ------------------------------------------------------------------------------------------ LEVEL 1 */

/* L (users x K) and R (items x K), row-major fp64, are updated in place by `iters` iterations. */
int mf_backend_factorize(const mf_problem *p, double *L, double *R, int device);

/* best[i] = arg max_j (L R^T)[i][j] over the items user i has NOT rated (strict '>', ascending j, so the
 * lowest index wins ties); -1 when user i rated every item (the reference then prints no line). */
int mf_backend_recommend(const mf_problem *p, const double *L, const double *R, int32_t *best, int device);

/* factorize + recommend with the factors resident in HBM in between; L/R receive the final factors
 * (either may be NULL if the caller does not want them back). */
int mf_backend_run(const mf_problem *p, double *L, double *R, int32_t *best, int device);

/* The same when only the recommendation list is wanted -- what the reference's main prints (matFact.c:127):
 * the initial factors go in, nothing but best[] comes back (no device-to-host copy of L and R). */
int mf_backend_run_top1(const mf_problem *p, const double *L0, const double *R0, int32_t *best, int device);

/* Top-N recommendations (an extension: the reference prints one item per user).  items and scores are user_count x n,
 * row-major; 1 <= n <= MF_TOPN_MAX.  Row i is T_i = print_output's rule applied n times, each pick removed from the set
 * of unrated items: empty set -> -1; first = its lowest index; B[i][first] NaN -> first; otherwise the arg-max over the
 * non-NaN scores, the lowest index on ties.  With finite scores that is the n largest in descending order, ties by
 * ascending index; t_1 is exactly mf_backend_recommend's best[i].  scores[i][r] = B[i][t_r] bit for bit (sequential k,
 * unfused, mat2d.c:100-113), NaN where t_r = -1.  n < 1 or items == NULL -> MF_ERR_ARGUMENT, n > MF_TOPN_MAX ->
 * MF_ERR_UNSUPPORTED, both before any HIP call.  scores may be NULL. */
#define MF_TOPN_MAX 32
int mf_backend_recommend_topn(const mf_problem *p, const double *L, const double *R, int32_t n, int32_t *items,
                              double *scores, int device);
/* factorize + top-N: the twin of mf_backend_run_top1 (no copy-back of the factors) */
int mf_backend_run_topn(const mf_problem *p, const double *L0, const double *R0, int32_t n, int32_t *items, double *scores,
                        int device);

/* The same on several GPUs of ONE process: users are cut into ndev contiguous blocks balanced by entry count,
 * L blocks are private, R is replicated and summed after every item sweep (the decomposition of
 * matFact-mpi.c:155-214 with the 8x1 grid of mpiutil.c:54-88; items are cut instead when items > users).  The sum
 * is the MPI_Iallreduce of matFact-mpi.c:207-208: environment MF_MULTI_REDUCE=peer (default) uses a hand-written
 * peer-to-peer reduce over xGMI (needs peer access between distinct devices, MF_ERR_UNSUPPORTED otherwise),
 * MF_MULTI_REDUCE=rccl uses ncclAllReduce(ncclDouble, ncclSum) on a communicator made by ncclCommInitAll (needs
 * distinct devices).  The reduce runs on its own stream beside the user sweep.  devices[] lists HIP ordinals; with
 * the peer reducer an ordinal may repeat (several shards on one GPU -- how the path is tested on a one-GPU box).
 * ndev <= 16.
 *
 * The result, bit for bit (peer reducer; tests/test_multi_shards.py holds the run to a numpy model of these lines):
 *   - The cut side "A" is the users when users >= items, else the items; "B" is the other factor.  With the items cut
 *     the roles of (row, L) and (col, R) are exchanged and nothing else changes: file order is untouched.
 *   - Blocks.  cnt[k] = entries whose A key is < k (cnt[nkeys] = nnz).  begin[0] = 0, begin[ndev] = nkeys and, for
 *     g = 1 .. ndev-1 in turn with ONE cursor u that starts at 0 and only moves forward: target = cnt[nkeys] * g / ndev
 *     (integer division); while u < nkeys and cnt[u] < target, ++u; begin[g] = u.  Shard g owns the keys
 *     [begin[g], begin[g+1]) and their entries, in file order (a stable bucketing when the file is not sorted by the A
 *     key).  A block may be empty (begin[g] == begin[g+1]: a few heavy rows hold the entries, or nnz = 0, when every key
 *     goes to the last shard); such a shard still sweeps, seeds if it is shard 0 and takes part in the sum.
 *   - One iteration.  Every shard g forms, from the old A block and the old B, the new rows of its A block and its
 *     partial P_g of B exactly as the serial program forms them over the shard's entries in file order; P_0 starts
 *     from the old B (shard 0 seeds, whether or not it owns entries), every other P_g from +0.0.
 *   - B_new = (((P_0 + P_1) + P_2) + ... + P_{ndev-1}), element by element in double precision, left to right in shard
 *     order, as IEEE 754 defines the sum: NaN and infinities propagate (+inf + -inf = NaN, sign and payload of a NaN
 *     unspecified).  The device buffers are summed whole, row padding included (the padding is +0.0 in every shard and
 *     is not returned).  One shard adds nothing: its result is that of mf_backend_run.
 *   - Hence, with two or more shards, an element of B that receives no entry keeps its old value -- except a -0.0,
 *     which comes back as +0.0 ((-0.0) + 0.0); with one shard it stays -0.0.
 *   - best[] is mf_backend_recommend of the factors this call returns, not of the serial program's: a near-tie can
 *     resolve differently.  The result does not depend on MF_MULTI_THREADS.
 * Errors.  ndev outside 1..16, a NULL pointer, a negative size and an entry with row outside [0, users) or col outside
 * [0, items) give MF_ERR_ARGUMENT before the first HIP call (on a machine without a GPU too), L, R and best untouched;
 * then a device ordinal that does not exist gives MF_ERR_NO_DEVICE.  A call after a refused one is not affected by it. */
int mf_backend_run_multi(const mf_problem *p, double *L, double *R, int32_t *best, const int *devices, int ndev);
/* Host wall-clock of the last mf_backend_run_multi of this process: set-up (bucketing + plan builds + uploads),
 * iterations, recommendations; info[0] = shards, info[1] = reducer (0 peer, 1 rccl), info[2] = 1 when the shards
 * were slices of the caller's array (input sorted by the cut key: no bucketing pass).  Any pointer may be NULL. */
int mf_backend_multi_last_timing(double *setup_s, double *iterate_s, double *recommend_s, int *info);
/* More of the same run: enqueue_s = host time the slowest enqueueing thread spent issuing the iterations' launches, event
 * records and waits (everything of iterate_s but the final synchronize; small against iterate_s = the host is not the
 * bound); entry_passes = passes of the host over all nnz entries during set-up (1: the counting pass; 2: + the stable
 * scatter of an input not sorted by the cut key) -- independent of the shard count; host_threads = threads that
 * enqueued (the shard count, or 1 with MF_MULTI_THREADS=0).  Any pointer may be NULL. */
int mf_backend_multi_last_counters(double *enqueue_s, int64_t *entry_passes, int *host_threads);

/* ------------------------------------------------------------------------------------------ LEVEL 2 */

typedef struct mf_plan mf_plan;

/* One contiguous block of users (all of them for a single-GPU run) with its entries in SoA form. */
typedef struct mf_shard {
	int32_t users_total;
	int32_t items;
	int32_t features;
	int32_t user_begin;      /* first user of this shard (BLOCK_LOW, mpiutil.h:8)        */
	int32_t user_count;      /* users in this shard (BLOCK_SIZE, mpiutil.h:10-11)        */
	int64_t nnz;             /* entries whose row lies in [user_begin, user_begin+count) */
	const int32_t *row;      /* GLOBAL user ids, file order                              */
	const int32_t *col;
	const double *val;
	double alpha;
	int32_t device;          /* HIP device ordinal                                       */
	int32_t flags;           /* MF_PLAN_* bits                                           */
	void *items_ext[2];      /* optional caller-owned DEVICE buffers (items*features doubles each) for the
	                            two generations of R, e.g. torch tensors handed to a collective; NULL = own */
	void *users_ext[2];      /* the same for the two generations of this shard's L block (user_count*features
	                            doubles each); only a 2-D tile needs them (L summed over the grid row) */
	int32_t items_pitch;     /* row pitch, in doubles, of the caller-owned items_ext / users_ext buffers: 0 = features */
	int32_t users_pitch;     /* (rows packed); otherwise even and >= features -- mf_backend_row_pitch(features) is the
	                            pitch the plan gives its own buffers (rows padded to whole 128-byte lines where that
	                            saves gathered lines); the buffers then hold rows * pitch doubles */
} mf_shard;

/* A TILE of the reference's 2-D process grid (matFact-mpi.c:155-214, grid from create_balanced_grid,
 * mpiutil.c:54-88) is a shard that also holds only a block of the items: the caller passes `items` = the
 * block's item count and `col` relative to the block's first item (entries[n].col - offset_col,
 * matFact-mpi.c:193), exactly as user ids are relative to user_begin inside the plan.  Item indices that
 * mf_plan_recommend* return are then block-relative too. */

#define MF_PLAN_DEFAULT 0   /* no flag bits are defined: every sum is formed in the serial order */

int mf_plan_create(mf_plan **out, const mf_shard *shard);
/* Row pitch (doubles) the plan uses for factor buffers it owns, for this K: features, or features rounded up so that
 * a row is a whole number of 128-byte lines (a gathered row of 8K bytes otherwise touches a line more than its bytes
 * wherever it happens to start: 80-byte rows 1.5 lines on average instead of 1).  The pitch of a live plan's L and R
 * buffers -- what mf_plan_items_next() and friends point at -- is reported by mf_plan_row_pitch. */
int mf_backend_row_pitch(int features);
int mf_plan_row_pitch(mf_plan *plan, int32_t *users_pitch, int32_t *items_pitch);
void mf_plan_destroy(mf_plan *plan);

/* The plan's stream: hipStream_t as void*.  Every launch, copy and memset of every plan entry point is ordered on it, so
 * a caller that enqueues its own work on the same stream (a collective on mf_plan_items_next(), a copy into the current
 * buffers) needs no host synchronisation between that work and the plan's (tests/test_stream_order.py holds every line
 * below on a stream that is busy when the library is called).
 *   - Entry points that only ENQUEUE and return: mf_plan_iterate (and mf_plan_iterate_monitored between its evaluation
 *     points), mf_plan_sweep_items, mf_plan_sweep_users, mf_plan_sweep_users_seeded, mf_plan_project, mf_plan_als_solve,
 *     mf_plan_als_normal, mf_plan_als_solve_normal and mf_plan_gram without a host pointer.  What they
 *     write may be read by work enqueued on the stream after the call returns, or by the host after
 *     mf_plan_synchronize.  A HIP graph that mf_plan_iterate builds is captured on and replayed into this stream.
 *   - Host only, no device work: mf_plan_flip, the setters and getters of the update rule, the pointer and pitch
 *     queries, mf_plan_describe.  A setter holds from the next launch that is enqueued.
 *   - COMPLETE ON RETURN (they enqueue behind whatever the stream holds and wait for it): everything that returns data
 *     to the host -- mf_plan_download_*, mf_plan_recommend*, mf_plan_rank_heldout, mf_plan_similar_items, mf_plan_loss,
 *     mf_plan_penalty, mf_plan_weight_total, mf_plan_bounds_active, mf_plan_als_info, mf_plan_gram with a host pointer, mf_plan_implicit_objective, mf_plan_predict, mf_plan_timing_read, an evaluation
 *     point of mf_plan_iterate_monitored --, mf_plan_upload_factors, mf_plan_upload_previous, mf_plan_set_heldout,
 *     mf_plan_synchronize, mf_plan_create*, and mf_plan_destroy, which waits for the stream before it frees anything:
 *     caller-owned buffers hold the results of all enqueued work when it returns.
 *   - The side stream of the extreme rows is the plan's own affair: it is forked from and joined to the plan's stream
 *     inside every call (mf_plan_iterate joins the item sweep's ordered sums behind the user sweep, in front of the
 *     flip), so nothing is left running beside the plan's stream when a call returns.
 *   - mf_plan_set_stream waits for the stream it leaves, then switches: work enqueued before the call is complete, work
 *     after it is ordered on the new stream only.
 *   - NULL selects the plan's own stream, created non-blocking.  The handle of the legacy default stream is NULL too, so
 *     that stream cannot be chosen, and the plan's own stream is not ordered against it: a caller whose other work runs
 *     on the default stream synchronises on the host or passes a stream of its own. */
int mf_plan_set_stream(mf_plan *plan, void *hip_stream);

/* host -> HBM: this shard's rows of L (user_count x K) and the whole of R (items x K). */
int mf_plan_upload_factors(mf_plan *plan, const double *L_block, const double *R);
int mf_plan_download_factors(mf_plan *plan, double *L_block, double *R);

/* Single-shard iteration loop: per iteration one item sweep and one user sweep from the frozen
 * generation into the next one, then flip (matFact.c:36-54; the two mat2d_copy are the ping-pong). */
int mf_plan_iterate(mf_plan *plan, int iters);

/* Sharded iteration, mirroring matFact-mpi.c:185-209 --
 *   mf_plan_sweep_items: R_next = (seed_from_old ? R_cur : 0) + sum over LOCAL entries   (:187,:190-205)
 *   mf_plan_sweep_users: L_next = L_cur + sum over local entries (L is private to the shard)
 *   caller SUM-all-reduces the buffer mf_plan_items_next() over the ranks             (:208)
 *   mf_plan_flip: next becomes current                                               */
int mf_plan_sweep_items(mf_plan *plan, int seed_from_old);
int mf_plan_sweep_users(mf_plan *plan);
void *mf_plan_items_next(mf_plan *plan);     /* device pointer, items rows of items_pitch doubles */
void *mf_plan_items_current(mf_plan *plan);
int mf_plan_flip(mf_plan *plan);

/* 2-D tiles: the L block is shared by the ranks of a grid row and summed over them like R is over a grid
 * column (the two MPI_Iallreduce of matFact-mpi.c:207-208) --
 *   mf_plan_sweep_users_seeded: L_next = (seed_from_old ? L_cur : 0) + sum over LOCAL entries  (:188)
 *   caller SUM-all-reduces mf_plan_users_next() over the grid row, mf_plan_items_next() over the grid column. */
int mf_plan_sweep_users_seeded(mf_plan *plan, int seed_from_old);
void *mf_plan_users_next(mf_plan *plan);     /* device pointer, user_count rows of users_pitch doubles */
void *mf_plan_users_current(mf_plan *plan);

/* Recommendations for this shard's users against the current R; best has user_count entries.
 * Default form: scores on the FP64 matrix cores (MFMA), every user whose best/second-best margin is not
 * provably larger than the rounding bound re-scored in the reference's exact order, so the result is the
 * reference's arg-max in all cases.  MF_RECOMMEND_IMPL=exact forces the exact form for every user. */
int mf_plan_recommend(mf_plan *plan, int32_t *best);
/* users the last mf_plan_recommend sent through the exact pass (-1 when the exact form ran for all) */
int mf_plan_recommend_info(mf_plan *plan, int64_t *exact_pass_users);

/* Top-N for this shard's users (semantics: mf_backend_recommend_topn).  Default form: the N+1 best matrix-core scores
 * per user; a user is certified when no non-finite score was seen and a_N - a_{N+1} exceeds the margin of
 * mf_plan_recommend (or it has at most N unrated items), and its N members are then re-scored exactly and ordered;
 * everyone else goes through the exact pass.  Matrix-core forms exist for K = 20c <= 100, 16c <= 128 and 256; other K,
 * and MF_RECOMMEND_IMPL=exact, run the exact pass for every user.  Item indices are block-relative on a 2-D tile. */
int mf_plan_recommend_topn(mf_plan *plan, int32_t n, int32_t *items, double *scores);
/* the last mf_plan_recommend_topn: users that went through the exact pass (-1 when the exact form ran for all) and
 * the form that ran (0 exact for all users, 1 matrix cores at two workgroups per CU, 2 matrix cores at one per CU;
 * -1 before the first call; 0 and 0 after a call on a plan without users).  Either pointer may be NULL. */
int mf_plan_recommend_topn_info(mf_plan *plan, int64_t *exact_pass_users, int32_t *mfma_form);

/* ---- Similar items: the top-N neighbours of an item's row of R among the OTHER items, by dot product or by cosine ("people
 * who liked X also liked ...").  An extension (the reference has no such query), so the definition is this library's; it
 * fixes the order of every floating-point operation.  The operand matrix Q (items x K) comes from the plan's current R:
 *   MF_SIMILAR_DOT     Q = R;
 *   MF_SIMILAR_COSINE  s_j = ((0.0 + R[j][0]*R[j][0]) + R[j][1]*R[j][1]) + ..., k ascending, multiply and add unfused;
 *                      n_j = sqrt(s_j), correctly rounded; Q[j][k] = R[j][k] / n_j, correctly rounded IEEE division.  Nothing
 *                      is special-cased: a zero row gives 0/0 = NaN, an infinite norm 0 or NaN, a sum that underflows to 0
 *                      +-inf; the rule below says what happens to NaN scores.
 * Scores S[j][j'] = dot(Q[j], Q[j']), sequential k from 0.0, unfused: mf_plan_predict's bits for L = R = Q.  The candidates
 * of item j are C_j = { j' in [0, items) : j' != j }.  Row t of the result belongs to query[t] and is the rule of
 * mf_backend_recommend_topn applied to S[query[t]][.] over C_query[t]: print_output's rule n times, each pick removed --
 * empty set -> -1; first = its lowest index; S[.][first] NaN -> first; otherwise the arg-max over the non-NaN scores, the
 * lowest index on ties -- and scores[t][r] = S[query[t]][items[t][r]] bit for bit, NaN where the item is -1.
 * query == NULL: all items in ascending order, nq must equal the plan's item count; otherwise nq item ids in any order,
 * repeats allowed, each with a row of its own.  items and scores are nq x n, row-major; 1 <= n <= MF_TOPN_MAX; scores may
 * be NULL.  Before any HIP call: NULL items, n < 1, an unknown metric, nq < 0, a query id out of range or query == NULL
 * with nq != items -> MF_ERR_ARGUMENT; n > MF_TOPN_MAX -> MF_ERR_UNSUPPORTED; no factors uploaded -> MF_ERR_STATE.  nq == 0:
 * MF_OK and nothing is written.  On a 2-D tile the query works among the tile's own items, like every other item index; a
 * user shard holds the whole of R, so any shard answers.
 * Default form: mf_plan_recommend_topn's passes on other operands -- the rows of Q (or the gathered query rows) against
 * Q under a mask of one item per row, the query itself; the margin is mf_backend_recommend_margin(K) * ||Q_j|| * max ||Q||.
 * Q is formed again on every call. */
#define MF_SIMILAR_DOT    0
#define MF_SIMILAR_COSINE 1
int mf_plan_similar_items(mf_plan *plan, int metric, const int32_t *query, int32_t nq, int32_t n, int32_t *items,
                          double *scores);
/* the last mf_plan_similar_items: queries that went through the exact pass (-1 when the exact form ran for all) and the
 * form that ran (0 exact for all, 1 matrix cores at two workgroups per CU, 2 at one per CU; -1 before the first call; 0 and
 * 0 after a call with nq == 0).  Independent of mf_plan_recommend_topn_info.  Either pointer may be NULL. */
int mf_plan_similar_items_info(mf_plan *plan, int64_t *exact_pass_queries, int32_t *mfma_form);
/* level 1: host R (items x features, row-major) in, the rows out, on a throw-away plan without entries */
int mf_backend_similar_items(const double *R, int32_t items, int32_t features, int metric, const int32_t *query, int32_t nq,
                             int32_t n, int32_t *out_items, double *out_scores, int device);

/* Partial result of the sequential scan of print_output (matFact.c:13-23) over this plan's items, in a form
 * that can be combined over the item blocks of a grid row (what MPI_Reduce(max_cmp) does at matFact-mpi.c:98):
 * the scan keeps the FIRST unrated item until a strictly greater score appears, and a NaN score never compares
 * greater, so per user the partial state is
 *   best/score  arg-max and max over the unrated items with a non-NaN score, lowest index on ties (-1: none),
 *               score being the reference's B[i][j] bit for bit (sequential k, unfused);
 *   first       the first unrated item (-1: every item rated);  first_nan  its score is NaN.
 * Combining blocks left to right: first = the first block's that has one; best = the greater score, the earlier
 * block on ties; answer = first < 0 ? -1 : first_nan ? first : best.  Exact form for every user. */
typedef struct mf_candidate {
	double score;
	int32_t best;
	int32_t first;
	int32_t first_nan;
	int32_t reserved;
} mf_candidate;
int mf_plan_recommend_scored(mf_plan *plan, mf_candidate *out);   /* user_count entries */
/* the same for n listed users of this shard only (local ids); out[t] belongs to users[t] */
int mf_plan_recommend_scored_users(mf_plan *plan, const int32_t *users, int32_t n, mf_candidate *out);

/* Pass 1 alone, for a certification ACROSS the item blocks of a grid row: per user the best and second-best
 * MATRIX-CORE (approximate) scores over this plan's unrated items, the arg-best (-1: none) and whether a
 * non-finite score was seen; norm[i] = ||L[i]||_2; *rmax = max_j ||R[j]||_2 over this plan's items.  Any score
 * is within 2*gamma_K*||l||*||r|| of the reference's, so with R = the largest rmax of the row and the margin
 * thr_i = mf_backend_recommend_margin(K) * norm[i] * R:  best_w - max(second_w, best_c for c != w) > thr_i and no
 * non-finite flag in any block  =>  arg_w IS the reference's answer.  Everyone else is re-scored exactly
 * (mf_plan_recommend_scored_users) and merged as described above. */
typedef struct mf_filter {
	double best, second;
	int32_t arg;
	int32_t nonfinite;
} mf_filter;
int mf_plan_recommend_filter(mf_plan *plan, mf_filter *out, double *norm, double *rmax);
double mf_backend_recommend_margin(int features);   /* 8 * (K + 8) * 2^-53 */

/* ---- Loss: the squared error of L R^T over an entry set E -- the plan's training entries or a held-out set -- for the
 * plan's current factors.  An extension (the reference computes no loss), so the definition is this library's; it fixes
 * the order of every floating-point operation, and the result is the same bits whatever kernel form, chunk size or
 * shard count produced it:
 *   1. p_n = dot(L[i_n], R[j_n]): k ascending from 0.0, multiply and add unfused (mat2d.c:126-139) = B[i][j] of
 *      mf_plan_predict bit for bit;
 *   2. d_n = a_n - p_n, q_n = d_n * d_n (no alpha);
 *   3. row sum s_i = (((0.0 + q_n0) + q_n1) + ...) over the entries of user i in the order the caller gave them
 *      (0.0 for a user without entries);
 *   4. users are cut into blocks of MF_LOSS_BLOCK consecutive users counted from GLOBAL user 0; T_b = the s_i of block b
 *      added in ascending i from 0.0; SSE = the T_b added in ascending b from 0.0;
 *   5. count = |E|; RMSE = sqrt(SSE / count) in double on the host (NaN when count == 0).
 * NaN and infinities propagate by these rules (a NaN result is a NaN; which sign and payload it carries is the hardware's
 * choice, as IEEE 754 leaves it).  A shard's mf_loss.sse is step 4 over ITS users (blocks still cut at
 * global multiples of MF_LOSS_BLOCK); shard totals cannot be added to the single-plan bits -- concatenate the shards'
 * row_sse and apply mf_backend_loss_total.  On a 2-D tile the loss is that of the tile's own entries. */
#define MF_LOSS_BLOCK 1024
#define MF_LOSS_TRAIN 0
#define MF_LOSS_HELDOUT 1
typedef struct mf_loss { double sse; int64_t count; } mf_loss;          /* rmse = sqrt(sse / count) */

/* Held-out set resident in the plan: n triples (GLOBAL user ids inside the shard's range, items inside [0, items), else
 * MF_ERR_ARGUMENT and nothing changes), bucketed by user stably: inside a user the caller's order is kept; it may be
 * unsorted and may repeat training pairs.  A new set replaces the old one; n = 0 removes it. */
int mf_plan_set_heldout(mf_plan *plan, int64_t n, const int32_t *row, const int32_t *col, const double *val);
/* which = MF_LOSS_TRAIN | MF_LOSS_HELDOUT (no held-out set: MF_ERR_STATE).  row_sse: user_count doubles or NULL. */
int mf_plan_loss(mf_plan *plan, int which, mf_loss *out, double *row_sse);
/* step 4 on the host: the same bits as the device total for row sums of `users` consecutive users from user_begin
 * (plain C++, no HIP call: works without a GPU) */
int mf_backend_loss_total(const double *row_sse, int32_t user_begin, int32_t users, double *sse);

typedef struct mf_loss_point { int32_t iter; int32_t reserved; mf_loss train, heldout; } mf_loss_point;
/* Runs up to `iters` iterations.  Evaluates before the first one (iter 0), after every `every`-th and after the last
 * one run.  Stops after an evaluation at which rmse_prev - rmse <= tol * rmse_prev, rmse being the held-out RMSE
 * when a set is present and the training RMSE otherwise; with tol > 0 a NaN RMSE also stops; with tol <= 0 nothing
 * stops the loop.  Without a held-out set a point's heldout is {0.0, 0}.  trace receives at most cap points (NULL/0:
 * none), *points = points evaluated, *iters_done = iterations run (either may be NULL).  The factors are then those of
 * mf_plan_iterate(*iters_done) bit for bit. */
int mf_plan_iterate_monitored(mf_plan *plan, int iters, int every, double tol, mf_loss_point *trace, int cap,
                              int *points, int *iters_done);
/* level 1: host buffers in, the training loss of these factors out (factors are not changed) */
int mf_backend_loss(const mf_problem *p, const double *L, const double *R, mf_loss *out, double *row_sse, int device);

/* ---- L2 regularisation (weight decay): the update rule for the objective SSE + lambda_users ||L||^2 + lambda_items ||R||^2.
 * An extension (the reference has none), so the definition is this library's; it fixes every rounding.  Per side, lambda
 * is finite and >= 0 and defaults to 0.  On the host, in double:
 *   c2 = alpha * 2;   d_side = 1.0 - c2 * lambda_side   (two roundings: the product, then the subtraction).
 * A seeded sweep of side X over the frozen X_old, Y_old:
 *   e_n         = c2 * (val_n - dot_n)        unchanged: dot_n from the UNshrunk X_old and Y_old
 *   X_new[r][k] = (...((X_old[r][k] * d_side) + e_0*Y[idx_0][k]) + e_1*Y[idx_1][k]) + ...
 * -- one more rounded multiply, unfused with the add that follows; the entries in the order of the plain sweep.  An
 * unseeded sweep (seed_from_old = 0) starts from 0.0 as before: in a sharded or tiled run the decay is applied once, by
 * the root that seeds.  Nothing is special-cased: a d below 0 is the caller's business; inf * 0, NaN and subnormals follow
 * IEEE 754.  lambda = 0 gives d = 1.0 (whatever alpha is, a non-finite one included) and x * 1.0 is x bit for bit: with
 * both at 0 every result is that of the plain rule.
 * mf_plan_set_regularization: NaN, infinite or negative lambda -> MF_ERR_ARGUMENT before any HIP call and nothing
 * changes; legal at any time, before the upload too; in force from the next sweep or mf_plan_iterate* call on, for
 * every way the plan iterates (mf_plan_iterate, mf_plan_iterate_monitored, mf_plan_sweep_items, mf_plan_sweep_users[_seeded]).
 * mf_backend_run_multi does not regularise.  mf_plan_describe appends lambda=<users>/<items> when either is non-zero. */
int mf_plan_set_regularization(mf_plan *plan, double lambda_users, double lambda_items);
int mf_plan_get_regularization(mf_plan *plan, double *lambda_users, double *lambda_items);   /* either may be NULL */
/* The penalty's two norms for the current factors, next to mf_plan_loss: users_sq = ||L_block||_F^2, items_sq = ||R||_F^2,
 * in a fixed order.  Row sums s_r = ((0.0 + x_0*x_0) + x_1*x_1) + ..., k ascending, unfused (the s_j of
 * MF_SIMILAR_COSINE); rows -> total by step 4 of the loss: blocks of MF_LOSS_BLOCK rows cut at global multiples (the
 * GLOBAL user index for L, the item index for R), T_b summed in ascending order from 0.0, the total over ascending b --
 * mf_backend_loss_total is the host twin (user_begin = 0 for the items).  user_rows: user_count doubles, item_rows: items
 * doubles; any pointer may be NULL.  No factors: MF_ERR_STATE.  The objective is then
 * sse + lambda_users * users_sq + lambda_items * items_sq in whatever order the caller chooses. */
int mf_plan_penalty(mf_plan *plan, double *users_sq, double *items_sq, double *user_rows, double *item_rows);
/* level 1: mf_backend_run under regularisation -- L0 / R0 go in as L and R, the final factors come back; best == NULL: no
 * recommendation.  A bad lambda -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_reg(const mf_problem *p, double *L, double *R, int32_t *best, double lambda_users, double lambda_items,
                       int device);

/* ---- Frozen factor columns: a column of a factor matrix that a sweep leaves alone.  An extension (the reference has
 * none), so the definition is this library's; it fixes every bit.  Each side has one frozen column index, or -1 for none
 * (the default).  For a sweep of side X with frozen column f >= 0, for every row r of the launch, bit for bit:
 *   X_new[r][f] = seed_from_old ? X_old[r][f] : 0.0
 * -- whatever e_n, Y and d are: a NaN or infinite e_n does not reach the column, the weight decay is not applied to it, and a
 * row without entries obeys it too.  Every other column is exactly what it is without a frozen column, decay included, and
 * dot_n reads the frozen column like any other.  The unseeded form writes 0.0, so the caller's sum over shards or tiles
 * gives back X_old -- with one exception: a frozen -0.0 comes back as +0.0 from a sum with an unseeded shard ((-0.0) + 0.0).
 * mf_plan_set_frozen_columns: a column < -1 or >= features -> MF_ERR_ARGUMENT before any HIP call and nothing changes;
 * legal at any time, before the upload too; in force from the next sweep or mf_plan_iterate* call on, for every way the
 * plan iterates (read at every launch, like the decay).  mf_backend_run_multi does not freeze.  mf_plan_describe appends
 * frozen=<users>/<items> when either is >= 0.
 *
 * Biases on top.  With K = F + 2 columns,
 *   L' = [ L (F columns) | b_user | 1.0 ]   users' column F+1 frozen
 *   R' = [ R (F columns) | 1.0    | b_item ] items' column F   frozen
 * the sequential dot is ((dot_F + b_u*1.0) + 1.0*b_i) and the bias column's update is b*d + sum e_n*1.0 (e_n*1.0 is e_n):
 * the model a ~ mu + b_user + b_item + l.r on values centred by mu, and every pass that reads L.R^T (recommend, top-N,
 * ranks, loss, predict) works on it unchanged.  The bias columns decay with their side's lambda, like any free column. */
int mf_plan_set_frozen_columns(mf_plan *plan, int32_t users_col, int32_t items_col);
int mf_plan_get_frozen_columns(mf_plan *plan, int32_t *users_col, int32_t *items_col);   /* either may be NULL */
/* Host helpers (no HIP call).  mf_backend_bias_mean: s = ((0.0 + v_0) + v_1) + ... in the given order, mu = s / (double) n;
 * n == 0 gives 0.0.  mf_backend_bias_pack: out is rows x (F+2), packed; side 1 (users) writes [X | bias | 1.0], side 0
 * (items) writes [X | 1.0 | bias]; bias == NULL means zeros.  mf_backend_bias_unpack is the inverse; either of X and bias
 * may be NULL. */
int mf_backend_bias_mean(const double *val, int64_t n, double *mu);
int mf_backend_bias_pack(const double *X, const double *bias, int32_t rows, int32_t F, int side, double *out);
int mf_backend_bias_unpack(const double *in, int32_t rows, int32_t F, int side, double *X, double *bias);
/* level 1: the biased model.  p->features = F is the latent count; L, R, user_bias and item_bias go in as the initial values
 * and come back final; *mu goes out.  The run is mf_backend_run_reg on K = F + 2 with the values a_n - mu (one rounding
 * each), the packed factors and the frozen columns F+1 (users) and F (items); best is mf_plan_recommend on that plan
 * (NULL: no recommendation).  Bad lambdas or NULL factors, biases or mu -> MF_ERR_ARGUMENT before any HIP call; F + 2 beyond
 * the largest supported K (4096) -> MF_ERR_UNSUPPORTED. */
int mf_backend_run_biased(const mf_problem *p, double *L, double *R, double *user_bias, double *item_bias, double *mu,
                          int32_t *best, double lambda_users, double lambda_items, int device);

/* ---- Heavy-ball momentum: the step of a side also carries beta times its previous step.  An extension (the reference
 * has none), so the definition is this library's; it fixes every rounding.  Per side, beta is finite and >= 0 and defaults
 * to 0.  For a seeded sweep of side X with beta != 0, for every row r of the launch and every column k that is not the
 * side's frozen column:
 *   v    = X_old[r][k] - X_prev[r][k]          one rounded subtraction
 *   m    = beta * v                            one rounded multiply
 *   seed = (X_old[r][k] * d) + m               the decay's multiply, then one rounded add; nothing fused
 *   X_new[r][k] = (...((seed + e_0*Y[idx_0][k]) + e_1*Y[idx_1][k]) + ...)      unchanged
 * e_n and dot_n are unchanged: they see X_old and Y_old only.  A frozen column keeps X_old's bits (0.0 unseeded): neither
 * decay nor momentum reaches it.  An unseeded sweep starts from 0.0 and takes no momentum: in a sharded or tiled run the
 * root that seeds applies it once, like the decay.  With beta == 0 the term is absent -- not "+ 0.0": the bits are those
 * without momentum, and a plan with both betas at 0 launches the same kernels as before.  Nothing is special-cased:
 * inf - inf is NaN, subnormals and signed zeros follow IEEE 754.  One consequence: a -0.0 element that moves under momentum
 * from rest comes out of the seed as +0.0, because (-0.0 * d) + (+0.0) is +0.0.
 *
 * X_prev is the side's history: the content of the side's next-generation buffer (mf_plan_users_next / mf_plan_items_next)
 * at launch -- after a seeded sweep and a flip, the generation before X_old.  The exception is a side AT REST: there
 * X_prev = X_old by definition, so v = x - x.  A side is at rest after mf_plan_upload_factors, and after
 * mf_plan_set_momentum changes its beta from 0 to non-zero (a plain run maintains no history); it leaves rest with its first
 * seeded momentum sweep (the library then copies current -> next in front of the launch) or with mf_plan_upload_previous.
 * A change between two non-zero betas keeps the history.  beta >= 1 is the caller's business, like a negative d.
 * mf_plan_set_momentum: NaN, infinite or negative beta -> MF_ERR_ARGUMENT before any HIP call and nothing changes; legal
 * at any time, before the upload too; read at every launch, for every way the plan iterates (mf_plan_iterate,
 * mf_plan_iterate_monitored, mf_plan_sweep_items, mf_plan_sweep_users[_seeded]).  mf_backend_run_multi does not use
 * momentum.  mf_plan_describe appends momentum=<users>/<items> when either is non-zero. */
int mf_plan_set_momentum(mf_plan *plan, double beta_users, double beta_items);
int mf_plan_get_momentum(mf_plan *plan, double *beta_users, double *beta_items);   /* either may be NULL */
/* The previous generation, host <-> the next-generation buffers, on the plan's stream, rows K doubles apart on the host
 * like mf_plan_upload_factors.  Upload: either pointer may be NULL, which leaves that side alone; a side given is no
 * longer at rest.  Download: the inverse; a side at rest returns its current factors; either pointer may be NULL.  No
 * factors: MF_ERR_STATE.  With the two, a momentum run resumes bit for bit: download the current and the previous
 * generation, and later upload both into a plan with the same betas. */
int mf_plan_upload_previous(mf_plan *plan, const double *L_prev_block, const double *R_prev);
int mf_plan_download_previous(mf_plan *plan, double *L_prev_block, double *R_prev);
/* level 1: mf_backend_run_reg with momentum, from rest.  A bad lambda or beta -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_momentum(const mf_problem *p, double *L, double *R, int32_t *best, double lambda_users, double lambda_items,
                            double beta_users, double beta_items, int device);

/* ---- Per-entry confidence weights: the entries are not equally trustworthy (confidence by play count, time decay,
 * inverse-propensity weights, down-weighted sampled negatives, weight 0 to hold a fold out without rebuilding the problem).
 * An extension (the reference has none), so the definition is this library's; it fixes every rounding.  A plan may carry
 * one weight w_n (double) per training entry, given with the entries, in the order of mf_shard.row / col / val.  In every
 * sweep of either side, for every entry:
 *   dot_n  unchanged
 *   e_n  = (c2 * (val_n - dot_n)) * w_n
 * -- the plain e_n is formed first, then one more rounded multiply follows, unfused.  X_new accumulates e_n * Y[idx_n][k]
 * exactly as before, from the same seed, in the same order; decay, frozen column and momentum are untouched.  w_n == 1.0
 * gives the plain bits.  Nothing is special-cased or validated: inf * 0 is NaN, and a negative or NaN weight is the
 * caller's business, like beta >= 1.  One consequence: a zero weight gives a product e_n * y of +-0.0 -- not "no term" --, so
 * an accumulator that holds -0.0 comes out +0.0 wherever such a product is +0.0 ((-0.0) + (+0.0)); where no accumulator is
 * +-0.0, weight 0 is leaving the entry out.  Zero-weight entries stay "rated" for the recommendation mask, the ranks and top-N.
 *
 * Training loss.  On a weighted plan MF_LOSS_TRAIN is the weighted objective, the one the sweeps descend: step 2 of the loss
 * becomes q_n = (d_n * d_n) * w_n, one more rounded multiply; steps 3 to 5 are unchanged and count stays |E|.
 * mf_plan_iterate_monitored therefore monitors the weighted training RMSE.  The held-out set stays unweighted.  With all
 * weights 1.0 the loss is the unweighted bits.
 *
 * mf_plan_create_weighted: mf_plan_create with `weight`, shard->nnz doubles that are copied (the caller's array is not
 * needed after the call).  weight == NULL is mf_plan_create in every respect: the same kernels, the same mf_plan_describe.
 * The weights are fixed for the plan's life.  A weighted plan runs the weighted twins of the kernels of an unweighted one --
 * the same forms, chosen by the same rules -- and keeps the weights in CSR and in CSC order beside the values (2 x 8 bytes
 * per entry of device memory); mf_plan_describe appends weighted=1, which means that every sweep and loss kernel the string
 * names runs as its weighted twin (the names printed are those of the unweighted plan of the same shape).  mf_backend_run_multi does not weight: a sharded caller
 * of the plan API gives each shard the weights of its own entries.
 * mf_plan_weight_total: the w_n added per user in entry order from 0.0 (row_w, user_count doubles), the rows then combined
 * by step 4 of the loss (sum_w) -- mf_backend_loss_total is the host twin --, for a caller that normalises.  Either pointer
 * may be NULL; an unweighted plan returns MF_ERR_STATE. */
int mf_plan_create_weighted(mf_plan **out, const mf_shard *shard, const double *weight);
int mf_plan_weight_total(mf_plan *plan, double *sum_w, double *row_w);
/* level 1: mf_backend_run_momentum on a weighted plan (weight: p->nnz doubles in the order of p->entries, or NULL).  A bad
 * lambda or beta, or NULL L / R, -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_weighted(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                            double lambda_items, double beta_users, double beta_items, int device);

/* ---- Box-constrained factors: projected gradient descent onto [lo, hi], of which non-negative factorisation (NMF) is the
 * lo = 0, hi = +inf case; an upper bound keeps a diverging run finite.  An extension (the reference has none), so the
 * definition is this library's.  Each side (0 = items, 1 = users) has lo, hi and columns; the default is -inf, +inf, -1.
 * columns == -1 means all K columns; otherwise 0 <= columns <= K and the columns k < columns are bounded -- a leading range,
 * so that the bias columns of the layout [ L | b_user | 1.0 ] stay free at columns = F.
 *
 * A SEEDED sweep of side X finishes each row exactly as without bounds -- seed, decay, momentum, every e_n * Y in order --
 * and then, for every bounded column k that is not the side's frozen column:
 *   y = X_new[r][k];   if (y < lo) y = lo;   if (y > hi) y = hi;   X_new[r][k] = y;
 * with IEEE 754 comparisons and selects, never a max/min instruction (those return the operand that is not NaN).  So a NaN
 * stays the same NaN (both comparisons are false), -inf becomes lo and +inf becomes hi, -0.0 under lo = 0.0 stays -0.0, and
 * a value equal to a bound keeps its own bits.  The frozen column keeps X_old's bits whatever `columns` is: frozen wins.
 * Rows without entries are projected too; the padding of a row is never touched.  With the default bounds -- and with any
 * two infinite bounds -- every result keeps the bits it has without this section.  e_n, dot_n, the loss, the penalty and every L R^T pass are
 * unchanged; under momentum X_prev and X_old are projected values, and the definition of v does not change.
 *
 * An UNSEEDED sweep (seed_from_old = 0) does not project: a partial sum must not be clamped.  A sharded caller of the plan API
 * therefore leaves the summed side unbounded on every shard, sums, and calls mf_plan_project on that side's
 * next-generation buffer; the private side is bounded in its sweep.  mf_backend_run_multi does not bound.
 *
 * mf_plan_set_bounds: legal at any time, before the upload too; read at every launch, like the decay, for every way the plan
 * iterates.  A NaN bound, lo > hi, columns < -1, columns > K or an unknown side -> MF_ERR_ARGUMENT before any HIP call,
 * with nothing changed.  mf_plan_get_bounds is its inverse (any pointer may be NULL).
 * mf_plan_project: the clamp above, in place, on the side's current (generation 0) or next (generation 1) buffer: the
 * bounded, non-frozen columns of every row, on the plan's stream -- for the sharded caller after its sum, and for a caller
 * who wants uploaded factors made feasible.  Without factors MF_ERR_STATE.
 * mf_plan_bounds_active: over the bounded non-frozen columns of the side's current factor, at_lo = elements == lo, at_hi =
 * elements == hi, inside = elements strictly between -- IEEE comparisons, so a NaN is in none of the three and -0.0 is
 * at lo = 0.0: the sparsity an NMF user looks at.  Complete on return; any pointer may be NULL.
 * mf_plan_describe appends bounds=<users>/<items> when either side has a finite bound over at least one column: a side as
 * [lo,hi]x<columns> (the bounds in %.17g, the columns counted, K for -1), or - for a side without. */
typedef struct mf_bounds {
	double lo, hi;
	int32_t columns;
} mf_bounds;
int mf_plan_set_bounds(mf_plan *plan, int side, double lo, double hi, int32_t columns);
int mf_plan_get_bounds(mf_plan *plan, int side, double *lo, double *hi, int32_t *columns);
int mf_plan_project(mf_plan *plan, int side, int generation);
int mf_plan_bounds_active(mf_plan *plan, int side, int64_t *at_lo, int64_t *at_hi, int64_t *inside);
/* level 1: mf_backend_run_weighted plus one record per side (NULL: unbounded).  A bad record (as mf_plan_set_bounds, with
 * K = p->features), a bad lambda or beta, or NULL L / R -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_bounded(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                           double lambda_items, double beta_users, double beta_items, const mf_bounds *bounds_users,
                           const mf_bounds *bounds_items, int device);

/* ---- Adaptive step sizes: AdaGrad, RMSProp and Adam, a per-element step in place of the one global alpha.  An extension
 * (the reference has none), so the definition is this library's.  Each side (0 = items, 1 = users, as mf_plan_set_bounds
 * counts them) has its own record; the default kind is MF_OPT_NONE.  eta is finite and > 0; eps is finite and > 0, so a
 * zero accumulator gives 0 / eps = 0 and never a NaN; beta1 is in [0, 1) and read by ADAM only; beta2 is in [0, 1) -- for
 * RMSPROP it is its rho, ADAGRAD ignores it.
 *
 * A SEEDED sweep of a side X with kind != NONE is defined as follows.  Every operation is rounded once and nothing is
 * fused; sqrt and / are correctly rounded (IEEE 754).
 *   1. g[r][k] = the bits an UNSEEDED sweep of that side writes: 0.0 + every e_n * Y in the side's entry order (e_n the
 *      weighted one on a weighted plan), no decay, no box, 0.0 in the frozen column.
 *   2. Per side and per step two scalars, 1.0 at rest: with ADAM  p1 = p1 * beta1,  p2 = p2 * beta2  -- sequential
 *      products, one per seeded adaptive sweep of the side; the other kinds leave them at 1.0 --, then  c1 = 1.0 - p1,
 *      c2 = 1.0 - p2.  `steps` counts the seeded adaptive sweeps of the side, whatever the kind.
 *   3. Per element outside the frozen column  q = g * g  and, with ob1 = 1.0 - beta1 and ob2 = 1.0 - beta2 formed once,
 *        ADAGRAD:  v' = v + q;                                                     mh = g;        vh = v'
 *        RMSPROP:  v' = (beta2 * v) + (ob2 * q);                                   mh = g;        vh = v'
 *        ADAM:     m' = (beta1 * m) + (ob1 * g);  v' = (beta2 * v) + (ob2 * q);    mh = m' / c1;  vh = v' / c2
 *      then for every kind  s = sqrt(vh);  den = s + eps;  u = mh / den;  step = eta * u;  x' = (x * d) + step,  d the
 *      side's decay exactly as a seeded sweep forms it (1.0 - (alpha * 2) * lambda; 1.0 at lambda = 0).  Then the box
 *      projection above on the bounded columns, then the frozen select: the frozen column keeps X_old's bits, and its m and
 *      v keep theirs.
 *   4. g carries the plain rule's 2 * alpha (e_n = (alpha * 2) * (a_n - dot_n)): the adaptive step is invariant to that
 *      scale except against eps -- v holds (2 alpha)^2 times the squared gradient, so eps is compared with 2 alpha times
 *      the gradient's root mean square.  alpha still sets d.
 * e_n, dot_n, the loss, the penalty and every L R^T pass see nothing new.  Rows without entries take the formula with
 * g = 0; the padding of a row is never touched.  An UNSEEDED sweep of an adaptive side is the unseeded sweep, untouched.
 *
 * State: m (ADAM only) and v per side, rows x K doubles, zero at rest, with steps, p1 and p2.  The state returns to rest on
 * mf_plan_upload_factors, on a change of the side's kind and on mf_plan_reset_adaptive; a change of eta, beta1, beta2 or
 * eps alone keeps it.  Momentum: a side cannot have beta != 0 and kind != NONE (X_new carries g, so X_prev is gone) --
 * whichever of mf_plan_set_momentum / mf_plan_set_adaptive comes second returns MF_ERR_UNSUPPORTED with nothing changed.
 * While either side is adaptive mf_plan_iterate runs the two sweeps (not the errors + streams iteration, not the toy
 * loop); with MF_OPT_NONE on both sides the plan launches the kernels and produces the bits it does without this section.
 *
 * mf_plan_set_adaptive: NULL or kind NONE turns the rule off.  An unknown side or kind, eta or eps not finite or not > 0, a
 * beta the kind reads outside [0, 1) -> MF_ERR_ARGUMENT before any HIP call, with nothing changed.  mf_plan_get_adaptive is
 * its inverse (a side without a rule reads kind NONE and zeros).
 * mf_plan_adaptive_finish: treats the side's next-generation buffer as g and applies steps 2 - 3 to every row, on the
 * plan's stream: what a sharded caller of the plan API calls on the summed side after its sum (the sweeps unseeded), as it
 * calls mf_plan_project for a bounded one.  Without factors, or on a side of kind NONE, MF_ERR_STATE.
 * mf_plan_download_adaptive_state / mf_plan_upload_adaptive_state: m and v as rows x K doubles (the side's rows: items, or
 * the shard's users), steps, p1 and p2; any pointer may be NULL; a side at rest downloads zeros, 0 and 1.0, a side that is
 * not ADAM zeros for m.  With them and the factors a run resumes bit for bit.  Both need factors (MF_ERR_STATE); a side of
 * kind NONE is at rest and downloads as such, an upload to it is MF_ERR_STATE; an upload of a negative steps or of a p that
 * is NaN -> MF_ERR_ARGUMENT.  An upload leaves what it is not given as it is.
 * mf_plan_describe appends adaptive=<users>/<items> when either side has a rule: a side as adam(eta,b1,b2,eps),
 * rmsprop(eta,rho,eps), adagrad(eta,eps) -- the numbers in %.17g -- or - for a side without. */
enum { MF_OPT_NONE = 0, MF_OPT_ADAGRAD = 1, MF_OPT_RMSPROP = 2, MF_OPT_ADAM = 3 };
typedef struct mf_adaptive {
	int32_t kind;                   /* MF_OPT_NONE | MF_OPT_ADAGRAD | MF_OPT_RMSPROP | MF_OPT_ADAM */
	double eta, beta1, beta2, eps;
} mf_adaptive;
int mf_plan_set_adaptive(mf_plan *plan, int side, const mf_adaptive *rule);
int mf_plan_get_adaptive(mf_plan *plan, int side, mf_adaptive *rule);
int mf_plan_reset_adaptive(mf_plan *plan, int side);
int mf_plan_adaptive_finish(mf_plan *plan, int side);
int mf_plan_download_adaptive_state(mf_plan *plan, int side, double *m, double *v, int64_t *steps, double *p1, double *p2);
int mf_plan_upload_adaptive_state(mf_plan *plan, int side, const double *m, const double *v, const int64_t *steps, const double *p1,
                                  const double *p2);
/* level 1: mf_backend_run_bounded without the betas, plus one rule per side (NULL: the plain step).  A bad rule, record or
 * lambda, or NULL L / R -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_adaptive(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                            double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items,
                            const mf_adaptive *adaptive_users, const mf_adaptive *adaptive_items, int device);

/* ---- Alternating least squares: with one side frozen, every row of the other side is the solution of its own K x K ridge
 * regression.  An extension (the reference has only the gradient step), so the definition is this library's.  Sides are
 * counted as everywhere: 0 = items, 1 = users.
 *
 * mf_plan_als_solve(plan, side, other_generation) computes, for every row r of side X, a new row into X's next-generation
 * buffer.  It reads Y = the other side's current buffer (other_generation 0) or next buffer (1), X_old = X's current
 * buffer, and the row's entries n = 0 .. cnt-1 in the side's entry order (CSR order for users, CSC order for items: the
 * order the sweeps walk): a_n the value, w_n the weight (weighted plan only), y_n the Y row of the entry's other index.
 * Every operation is rounded once and nothing is fused; sqrt and / are correctly rounded (IEEE 754).
 *    1. With a frozen column f on this side  xf = X_old[r][f]  and  a'_n = a_n - (xf * y_n[f]);  otherwise a'_n = a_n.
 *    2. yw_n[q] = y_n[q] * w_n on a weighted plan, yw_n[q] = y_n[q] otherwise.
 *    3. Lower triangle of the Gram matrix, p >= q: G[p][q] starts at 0.0; for n ascending
 *       G[p][q] = G[p][q] + (y_n[p] * yw_n[q]).
 *    4. Right-hand side: b[p] starts at 0.0; for n ascending  b[p] = b[p] + (a'_n * yw_n[p]).
 *    5. Ridge:  G[p][p] = G[p][p] + ridge,  ridge = lambda_side (MF_ALS_RIDGE) or lambda_side * (double) cnt
 *       (MF_ALS_RIDGE_COUNT, the "weighted-lambda" ALS of Zhou et al.).
 *    6. Frozen column f:  G[f][q] = 0.0 for q < f,  G[p][f] = 0.0 for p > f,  G[f][f] = 1.0,  b[f] = xf: the other columns
 *       then get the bits of the reduced (K-1)-column system.
 *    7. Cholesky G = C C^T, for j ascending:  s = G[j][j];  for t < j ascending  s = s - (C[j][t] * C[j][t]);  if !(s > 0.0)
 *       the row is NOT POSITIVE DEFINITE (a NaN fails too);  C[j][j] = sqrt(s);  for each i > j:  s = G[i][j];  for t < j
 *       ascending  s = s - (C[i][t] * C[j][t]);  C[i][j] = s / C[j][j].  (The kernels are right-looking: column t's rank-1
 *       update is applied in the order t = 0, 1, ..., which is this chain element by element.)
 *    8. Forward solve, column-oriented: for j ascending  z[j] = b[j] / C[j][j],  then for every i > j
 *       b[i] = b[i] - (C[i][j] * z[j]): element i loses its terms one by one, t ascending.
 *    9. Backward solve, column-oriented: for j descending  x[j] = z[j] / C[j][j],  then for every i < j
 *       z[i] = z[i] - (C[j][i] * x[j]): element i loses its terms one by one, t descending from K-1.
 *   10. The box projection of mf_plan_set_bounds on the bounded columns, then the frozen select: the frozen column keeps
 *       X_old's bits.  A row without entries keeps X_old's bits and is not projected; a row that is not positive definite
 *       keeps X_old's bits too.  The padding of a row is never touched.
 * alpha is not read.  lambda, the weights, the frozen columns and the bounds are read at every launch, as the decay is.
 * The objective a solve cannot increase is mf_plan_loss (training; weighted on a weighted plan) plus lambda times
 * mf_plan_penalty's squares -- under MF_ALS_RIDGE_COUNT the per-row squares times the row counts.
 *
 * mf_plan_set_als: MF_ALS_OFF (the default), MF_ALS_RIDGE or MF_ALS_RIDGE_COUNT; mf_plan_get_als is its inverse.  An unknown
 * kind -> MF_ERR_ARGUMENT.  K > 128 -> MF_ERR_UNSUPPORTED (the triangle of a row lives in LDS).  Momentum or an adaptive
 * side together with ALS is refused: whichever of mf_plan_set_momentum / mf_plan_set_adaptive / mf_plan_set_als comes
 * second returns MF_ERR_UNSUPPORTED with nothing changed.  While the kind is not OFF one iteration of mf_plan_iterate and
 * of mf_plan_iterate_monitored is  als_solve(users, 0);  als_solve(items, 1);  flip  -- Gauss-Seidel: the item solve reads
 * the new L -- as eager launches on the plan's stream, no captured graph.  The sweep entry points stay gradient sweeps.
 * With the kind OFF the plan launches the kernels and produces the bits it does without this section.
 * mf_plan_als_solve only enqueues.  An unknown side or generation -> MF_ERR_ARGUMENT before any HIP call; without factors,
 * or with the kind OFF, MF_ERR_STATE.  The user solve works on any shard (rows of L are private); the item solve on a plan
 * that does not hold all users -- a shard, a 2-D tile -- returns MF_ERR_UNSUPPORTED (an item's Gram matrix is a sum over all
 * users), and so does mf_plan_iterate under ALS there.
 * mf_plan_als_info: the rows of the side's last solve that were solved, kept because they have no entries, kept because they
 * are not positive definite (zeros before the first solve).  Complete on return; any pointer may be NULL.
 * mf_plan_describe appends als=ridge|ridge-count and als_form=<form>(chunk=<entries per gather chunk>) while the kind is not
 * OFF.  The forms (MF_ALS_FORM=wg|wave: one 256-thread workgroup per row, any K; one wave per row, K <= 32; by default the
 * wave form up to K = 16) give the same bits. */
enum { MF_ALS_OFF = 0, MF_ALS_RIDGE = 1, MF_ALS_RIDGE_COUNT = 2 };
int mf_plan_set_als(mf_plan *plan, int kind);
int mf_plan_get_als(mf_plan *plan, int *kind);
int mf_plan_als_solve(mf_plan *plan, int side, int other_generation);
int mf_plan_als_info(mf_plan *plan, int side, int64_t *solved, int64_t *kept_empty, int64_t *kept_not_pd);
/* level 1: pr->iters ALS iterations from the factors in L and R, the plan session above on a whole-problem plan (weighted
 * when `weight` is given).  A bad kind, record or lambda, or NULL L / R -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_als(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                       double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, int kind, int device);

/* ---- Implicit feedback (Hu, Koren, Volinsky 2008): every user x item pair counts.  A pair that is not an entry is a 0.0 at
 * confidence 1; entry n is its value a_n at confidence c_n = 1 + conf * w_n (w_n = 1 on a plan without weights).  The model is
 * this library's definition in every rounding: FP64, every operation rounded once, nothing fused, sqrt and / correctly
 * rounded, no matrix-core instruction.  Three parts: the Gram matrix of a whole side, the solve, the objective.
 *
 * mf_plan_gram(plan, side, generation, triangle): S = X^T X over ALL rows of X = the side's current (generation 0) or next (1)
 * buffer -- on a shard the plan's own block of the users.  The result is the lower triangle S[p][q], p >= q, packed row by row
 * (S[p][q] at p (p + 1) / 2 + q), K (K + 1) / 2 doubles.  Order of the sum: the rows are cut into blocks of MF_LOSS_BLOCK
 * consecutive rows counted from row 0 of the plan's buffer; T_b[p][q] starts at 0.0 and takes T = T + (x_i[p] * x_i[q]) for i
 * ascending inside block b; S[p][q] is the T_b added in ascending b from 0.0.  A row without entries counts like any other;
 * the padding of a row is never read.  NaN, infinities and signed zeros follow IEEE 754.  The result does not depend on the
 * grid or on any switch.  triangle == NULL: the call only enqueues and S stays in a plan-owned buffer (allocated on first
 * use, with blocks x K (K + 1) / 2 doubles of partial sums); otherwise the call is complete on return.  No factors ->
 * MF_ERR_STATE; an unknown side or generation -> MF_ERR_ARGUMENT before any HIP call; K > 128 -> MF_ERR_UNSUPPORTED.
 *
 * The solve: mf_plan_set_als(plan, MF_ALS_IMPLICIT).  (The kind's number is 4: 3 stays an unknown kind.)  Under it
 * mf_plan_als_solve(plan, side, other_generation) first enqueues the Gram S of Y = the other side in that generation, then
 * solves every row of the side by steps 1-10 of the ALS definition above with these changes:
 *    1, 2. e_n = conf * w_n on a weighted plan and e_n = conf otherwise;  c_n = 1.0 + e_n;  ye_n[q] = y_n[q] * e_n;
 *          ac_n = a_n * c_n.  A frozen column on the solved side is REFUSED: MF_ERR_UNSUPPORTED from mf_plan_als_solve and from
 *          mf_plan_iterate*, checked at launch, before any HIP call -- the all-pairs term of a frozen column needs a correction
 *          (the column's share of S would have to move to the right-hand side) that this library does not define.
 *    3.    G[p][q] starts at S[p][q], not at 0.0; then G[p][q] = G[p][q] + (y_n[p] * ye_n[q]) for n ascending.
 *    4.    b[p] starts at 0.0; then b[p] = b[p] + (ac_n * y_n[p]) for n ascending.
 *    5.    ridge = lambda_side.
 *    7-10. unchanged: Cholesky, the two solves, the box, the counters.
 * A row WITHOUT ENTRIES is solved like any other: its sums are empty, G = S + ridge and b = 0, the chain yields +0.0 in every
 * column, then the box applies (lo under a positive lo).  That is the model's exact minimiser for a cold row.  It is counted
 * as solved or as not positive definite; kept_empty is 0 under this kind.  A NaN in Y makes S NaN: every row is then not
 * positive definite and keeps X_old's bits.
 * conf: mf_plan_set_confidence, default 1.0, read at every launch; not finite or < 0 -> MF_ERR_ARGUMENT, nothing changes.
 * One iteration of mf_plan_iterate and of mf_plan_iterate_monitored under this kind is  gram(items, current);
 * als_solve(users, 0);  gram(users, next);  als_solve(items, 1);  flip  -- eager launches on the plan's stream.  Both forms
 * (MF_ALS_FORM) give the same bits; the LDS of a row is that of a weighted plan's (two tiles, y and ye).  As under the other
 * kinds: the item solve on a shard or a 2-D tile is MF_ERR_UNSUPPORTED, momentum and adaptive sides are refused, K > 128 is
 * MF_ERR_UNSUPPORTED.  mf_backend_run_als takes the explicit kinds only.  mf_plan_describe appends
 * als=implicit conf=<%.17g> als_form=<form>(chunk=<entries>).
 *
 * The objective: mf_plan_implicit_objective fills {all_sq, observed, count} for the current factors;
 *   objective = all_sq + observed + lambda_users * users_sq + lambda_items * items_sq
 * with mf_plan_penalty's norms, in whatever order the caller chooses.
 *   all_sq   = sum over ALL pairs of (l_u . r_i)^2 = <L^T L, R^T R>: the two Grams of the current factors (SL of the users, SR of
 *              the items), then on the host t = 0.0 and t = t + (SL[p][q] * SR[p][q]) over the full K x K matrices, p ascending
 *              then q ascending, the upper triangle read through symmetry.  mf_backend_gram_dot is that sum (plain C++).
 *   observed = what the entries add to it: per training entry p_n = mf_plan_predict's bits, d_n = a_n - p_n,
 *              q_n = (c_n * (d_n * d_n)) - (p_n * p_n), c_n as in the solve; row sums and block totals by steps 3-4 of the loss.
 *   count    = the training entries.
 * Complete on return; works with any kind set.  No factors -> MF_ERR_STATE; K > 128 -> MF_ERR_UNSUPPORTED.  On a shard both
 * parts are those of the plan's own users. */
enum { MF_ALS_IMPLICIT = 4 };
typedef struct mf_implicit_objective {
	double all_sq, observed;
	int64_t count;
} mf_implicit_objective;
int mf_plan_gram(mf_plan *plan, int side, int generation, double *triangle);
int mf_plan_set_confidence(mf_plan *plan, double conf);
int mf_plan_get_confidence(mf_plan *plan, double *conf);
int mf_plan_implicit_objective(mf_plan *plan, mf_implicit_objective *out);
/* left, right: packed lower triangles of two symmetric K x K matrices (plain C++, no HIP call: works without a GPU) */
int mf_backend_gram_dot(const double *left, const double *right, int32_t features, double *out);
/* level 1: mf_backend_run_als under MF_ALS_IMPLICIT with the confidence `conf`.  A bad record, lambda or conf, or NULL L / R ->
 * MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_implicit(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                            double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, double conf, int device);

/* ---- ALS on user shards: the solve cut at the normal equations.  An item's Gram matrix is a sum over all users, and a shard
 * holds a part of it.  The normal equations of a row are linear in its entries, so every shard forms its part, the caller
 * sums the parts elementwise in FP64 (one collective over one buffer, as it sums mf_plan_items_next()), and every shard solves
 * the sums redundantly, as it keeps its replica of R.  Sides are 0 = items and 1 = users; T = K (K + 1) / 2.
 *
 * The record.  A NORMAL RECORD of a row is `pitch` doubles: N[0 .. T) the packed lower triangle, G[p][q] at p (p + 1) / 2 + q;
 * N[T .. T + K) is b; N[T + K] is the row's entry count as a double; the remaining slots up to
 * mf_backend_als_normal_pitch(K) are +0.0 pads.  mf_backend_als_normal_pitch(features) is the smallest even number
 * >= T + K + 1 (even, so that 16-byte stores work; 0 for features < 1; plain C++, no HIP call).  A caller may pass a larger
 * even pitch: the doubles of a record beyond the minimum pitch are never read or written.
 * The buffer.  Caller-owned device memory of (rows + 1) * pitch doubles, 16-byte aligned, rows = the side's row count in the
 * plan (the items, or the plan's own users).  The plan allocates none of it.
 *
 * mf_plan_als_normal(plan, side, other_generation, device_normal, pitch) only enqueues.  For every row r of the side it
 * writes record r:
 *   - steps 1-4 of the ALS definition (explicit kinds) or of the implicit kind's steps 1-4, over the plan's OWN entries of
 *     the row in the side's entry order; the frozen column's a'_n reads X_old as there;
 *   - the triangle starts at 0.0 under EVERY kind: under MF_ALS_IMPLICIT S is not added here;
 *   - a row without local entries gets +0.0 in every slot; the count slot is (double) cnt;
 *   - record `rows` is the GRAM RECORD: under MF_ALS_IMPLICIT its triangle slots hold the bits of
 *     mf_plan_gram(plan, side ^ 1, other_generation), the Gram of the plan's own block of the other side (enqueued by this
 *     call, copied on the device), its other slots +0.0; under the explicit kinds the whole record is +0.0.
 * After the call every double of the buffer up to the minimum pitch of each record is defined: the caller needs no memset.
 * The caller's sum.  The caller sums the buffers of the plans that partition the OTHER side, elementwise in FP64, in an order
 * that is its business, exactly as for mf_plan_items_next(), and writes the sum where each plan will read it.
 *
 * mf_plan_als_solve_normal(plan, side, device_normal, pitch) only enqueues.  For every row r:  cntd = N[r][T + K];
 * G[p][q] = N[r][tri] under the explicit kinds and  G[p][q] = N[rows][tri] + N[r][tri]  under MF_ALS_IMPLICIT (one rounded
 * add, S on the left);  b[p] = N[r][T + p].  Then steps 5-10 of the ALS definition unchanged: ridge = lambda_side or
 * lambda_side * cntd (MF_ALS_RIDGE_COUNT), the frozen cut with xf = X_old[r][f], Cholesky, the two solves, the box, the
 * frozen select, into the side's next buffer.  Under the explicit kinds a row with !(cntd > 0.0) keeps X_old's bits and
 * counts as kept_empty; under MF_ALS_IMPLICIT every row is solved.  mf_plan_als_info(side) then reports this solve.
 *
 * What follows from the definition:
 *   - on a plan that holds all users, under the explicit kinds, als_normal then als_solve_normal gives the bits and the
 *     counters of mf_plan_als_solve: the chain from 0.0 is the same chain;
 *   - under MF_ALS_IMPLICIT it does not:  S + (0.0 + t1 + ...)  is not  ((S + t1) + ...).  It is defined by the steps above;
 *   - on shards, a row that only one shard has entries for gets the single plan's bits under the explicit kinds:
 *     x + (+0.0) keeps x, and a chain from +0.0 never ends at -0.0.
 *
 * Refusals, all before any HIP call and with nothing changed: an unknown side or generation, a NULL or misaligned buffer, an
 * odd pitch or one below mf_backend_als_normal_pitch(K) -> MF_ERR_ARGUMENT; no factors or the kind MF_ALS_OFF ->
 * MF_ERR_STATE; conjugate-gradient steps set for the plan's kind (they need a sum per step), K > 128, or a frozen column on
 * the solved side under MF_ALS_IMPLICIT -> MF_ERR_UNSUPPORTED.  mf_plan_als_solve(items) and mf_plan_iterate stay refused on
 * a shard.  Both forms (MF_ALS_FORM) give the same bits; the solve needs T + 3 K doubles of LDS per row. */
int64_t mf_backend_als_normal_pitch(int32_t features);
int mf_plan_als_normal(mf_plan *plan, int side, int other_generation, void *device_normal, int64_t pitch);
int mf_plan_als_solve_normal(mf_plan *plan, int side, const void *device_normal, int64_t pitch);

/* ---- Box-constrained ALS: with a box on a side (mf_plan_set_bounds; lo = 0, hi = inf is non-negative factorisation) the
 * direct solve above is the unconstrained minimiser, clamped (step 10).  That is not the minimiser of the row's constrained
 * ridge problem.  With box sweeps set, a row is instead solved by cyclic coordinate descent on its normal equations G x = b,
 * every coordinate step exact within the box (Hsieh and Dhillon, KDD 2011; the `cd` solver of NMF; HALS).
 *
 * mf_plan_set_als_box(plan, sweeps) / mf_plan_get_als_box(plan, &sweeps), 0 <= sweeps <= MF_ALS_BOX_MAX_SWEEPS = 256.
 * sweeps = 0, the default, is the library without this section, bit for bit and kernel for kernel.  The setting is read at
 * every launch.  With sweeps > 0 the direct row solve (mf_plan_als_solve, and so mf_plan_iterate*) does steps 1-6 of the ALS
 * definition unchanged under the plan's kind (MF_ALS_RIDGE, MF_ALS_RIDGE_COUNT), likewise steps 1-5 of MF_ALS_IMPLICIT (its
 * Gram enqueued first, as there); steps 7-10 are replaced by B0-B4.
 * Notation: Gs[p][t] is the symmetric read of the packed lower triangle, G[max(p,t)][min(p,t)];  f the side's frozen column or
 * none;  xf = X_old[r][f];  (lo, hi, columns) the side's box, columns = 0 meaning that no column is bounded (a side whose
 * bounds are both infinite).  Every operation is rounded once and nothing is fused; / is correctly rounded.  box_clamp is the
 * projection of mf_plan_set_bounds, two compares and two selects: a NaN stays the NaN it is, -0.0 stays under lo = 0, a value
 * equal to a bound keeps its bits.
 *   B0. Diagonal test.  For j ascending: if !(G[j][j] > 0.0) the row is NOT POSITIVE DEFINITE (a NaN fails too): it keeps
 *       X_old's bits, is not projected and is counted kept_not_pd.  This is WEAKER than Cholesky's test on purpose: a singular G
 *       with a positive diagonal is a well-defined coordinate-descent problem, is solved, and is counted as solved.
 *   B1. Start.  x[p] = X_old[r][p];  for p < columns  x[p] = box_clamp(x[p], lo, hi);  x[f] = xf (the frozen column is not
 *       clamped).
 *   B2. Residual.  res[p] = b[p];  then for t = 0 .. K-1 ascending  res[p] = res[p] - (Gs[p][t] * x[t]).  All t, f included:
 *       step 6 has zeroed column f and put 1.0 on its diagonal, nothing is special-cased.
 *   B3. Sweeps.  For s = 1 .. sweeps, for j = 0 .. K-1 ascending, j != f:
 *         d = res[j] / G[j][j];  y = x[j] + d;  if j < columns  y = box_clamp(y, lo, hi);  dl = y - x[j];  x[j] = y;
 *         for every p in 0 .. K-1, j included:  res[p] = res[p] - (Gs[p][j] * dl).
 *       The update is applied when dl is +-0.0 too (-0.0 - (-0.0) is +0.0: skipping it would change bits).
 *   B4. Store.  X_new[r][p] = x[p]; column f gets X_old's bits.  The padding of a row is never touched.
 * The sweep count is fixed, there is no convergence test: the bits are defined.
 * Rows without entries: under the explicit kinds they keep X_old's bits and count as kept_empty, as in the direct solve.  Under
 * MF_ALS_IMPLICIT they are solved like any other row: they move towards the minimiser +0.0 but do not reach it in a fixed
 * number of sweeps -- this DIFFERS from the direct implicit solve, which yields +0.0 (then the box) for a cold row.
 * With sweeps > 0 mf_plan_als_solve_normal runs its steps 5-6 and then B0-B4 on the summed record; mf_plan_als_normal is
 * untouched.
 *
 * What follows from the definition:
 *   - on a plan that holds all users, under the explicit kinds, als_normal then als_solve_normal gives the bits and the
 *     counters of mf_plan_als_solve, as without box sweeps;
 *   - with lo = hi = c on all columns every solved row is c in every bounded column;
 *   - both forms (MF_ALS_FORM=wg|wave) give the same bits, and neither needs more LDS than the direct solve: x and res live in
 *     the 3 K doubles that held the diagonal of C, z and x.
 *
 * Refusals, all before any HIP call and with nothing changed: sweeps < 0 or > MF_ALS_BOX_MAX_SWEEPS -> MF_ERR_ARGUMENT.
 * Conjugate-gradient steps in force (mf_plan_set_als_cg > 0, or mf_plan_set_implicit_cg > 0 under MF_ALS_IMPLICIT) together with
 * box sweeps -> MF_ERR_UNSUPPORTED: whichever of mf_plan_set_als_box / mf_plan_set_als_cg / mf_plan_set_implicit_cg /
 * mf_plan_set_als comes second returns it, the way momentum and ALS refuse each other (implicit steps set under another kind
 * are not in force: it is then mf_plan_set_als(MF_ALS_IMPLICIT) that is refused).  K > 128 with a kind set ->
 * MF_ERR_UNSUPPORTED.  A frozen column under MF_ALS_IMPLICIT stays refused at launch; momentum and adaptive sides stay refused
 * under ALS; the item solve on a shard stays MF_ERR_UNSUPPORTED.
 * mf_plan_describe appends  als_box=<sweeps>  behind als_form=... while a kind is set and sweeps > 0.
 * Not part of this: coordinate descent without forming G (K > 128), box sweeps combined with CG, a convergence-based stop, a
 * frozen column under the implicit kind. */
#define MF_ALS_BOX_MAX_SWEEPS 256
int mf_plan_set_als_box(mf_plan *plan, int sweeps);
int mf_plan_get_als_box(mf_plan *plan, int *sweeps);
/* level 1: pr->iters ALS iterations of `kind` (MF_ALS_RIDGE, MF_ALS_RIDGE_COUNT or MF_ALS_IMPLICIT) with `sweeps` box sweeps per
 * row (0: the direct solve); conf is read under MF_ALS_IMPLICIT only.  A bad kind, record, lambda, sweep count or (under the
 * implicit kind) conf, or NULL L / R -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_als_box(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                           double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, int kind, double conf,
                           int sweeps, int device);

/* ---- ALS by conjugate gradient: a fixed, small number of conjugate-gradient (CG) steps per row, warm-started from the row's
 * current value, in place of the direct solve above (Takacs, Pilaszy, Tikk, RecSys 2011).  The Gram matrix of a row is never
 * formed -- its product with a vector p is  sum_n w_n y_n (y_n . p) + ridge p  -- so K goes up to MF_ALS_CG_MAX_K = 256.
 *
 * mf_plan_set_als_cg(plan, steps) / mf_plan_get_als_cg(plan, &steps).  steps = 0, the default, is the direct solve: every
 * bit and every launched kernel is what it is without this section.  1 <= steps <= MF_ALS_CG_MAX_STEPS switches the solve to
 * CG: with the kind MF_ALS_RIDGE or MF_ALS_RIDGE_COUNT set, mf_plan_als_solve(plan, side, other_generation) then computes
 * every row r of side X as below.  The setting is read at every launch.
 *
 * Inputs as in steps 1-10 of the direct definition: Y the other side in the named generation, X_old X's current buffer, the
 * row's entries n = 0 .. cnt-1 in the side's entry order, a_n the value, w_n the weight (weighted plan only), y_n the Y row,
 * f the side's frozen column or none, ridge = lambda_side or lambda_side * (double) cnt under MF_ALS_RIDGE_COUNT.  FP64
 * throughout, every operation rounded once, nothing fused, / correctly rounded, no matrix-core instruction.
 * dot(u, v) is  s = 0.0,  then  s = s + (u[k] * v[k])  for k = 0 .. K-1 ascending.  The padding of a row is never read or
 * written.
 *   C0. x = X_old[r][0..K).
 *   C1. For every entry:  t_n = dot(y_n, x);  d_n = a_n - t_n;  dw_n = d_n * w_n on a weighted plan, dw_n = d_n otherwise.
 *   C2. g[k] starts at 0.0; for n ascending  g[k] = g[k] + (dw_n * y_n[k]).  Then  r[k] = g[k] - (ridge * x[k]);  with a
 *       frozen column  r[f] = 0.0.
 *   C3. p = r;  rs = dot(r, r).
 *   C4. For s = 1 .. steps:
 *       a. If rs == 0.0 leave the loop (a NaN is not equal and goes on).
 *       b. u_n = dot(y_n, p);  uw_n = u_n * w_n on a weighted plan, u_n otherwise.
 *       c. q[k] starts at 0.0; for n ascending  q[k] = q[k] + (uw_n * y_n[k]).  Then  q[k] = q[k] + (ridge * p[k]);  with a
 *          frozen column  q[f] = 0.0.
 *       d. pq = dot(p, q).  If !(pq > 0.0) the row is NOT POSITIVE DEFINITE (a NaN fails too): it keeps X_old's bits, is
 *          counted as such, and ends here.
 *       e. alpha = rs / pq;  x[k] = x[k] + (alpha * p[k]);  r[k] = r[k] - (alpha * q[k]).
 *       f. rn = dot(r, r);  beta = rn / rs;  p[k] = r[k] + (beta * p[k]);  rs = rn.  (After the last step this sub-step does
 *          not reach the stored row; the kernels skip it.)
 *   C5. The box projection of mf_plan_set_bounds on the bounded columns, then the frozen select (column f keeps X_old's
 *       bits), then the store.  The row is counted as solved.
 * A row without entries keeps X_old's bits, is not projected and is counted kept_empty, as in the direct solve.  Nothing else
 * is special: infinities, NaN, subnormals and signed zeros follow IEEE 754 through the steps.  alpha of the plan is not read.
 * The three counters are mf_plan_als_info's, unchanged in meaning, and the objective a step cannot increase in exact
 * arithmetic is the one the direct definition names.
 *
 * Limits and refusals.  1 <= K <= 256 under CG: with the steps set, mf_plan_set_als accepts K up to 256 (a caller at K in
 * 129..256 sets the steps first); with steps = 0 it refuses K > 128 as before.  mf_plan_set_als_cg returns
 * MF_ERR_UNSUPPORTED with nothing changed for nonzero steps at K > 256 and for steps = 0 while an ALS kind is on and K > 128;
 * steps < 0 or > MF_ALS_CG_MAX_STEPS -> MF_ERR_ARGUMENT before any HIP call.  MF_ALS_IMPLICIT together with CG is refused:
 * whichever of mf_plan_set_als / mf_plan_set_als_cg comes second returns MF_ERR_UNSUPPORTED with nothing changed.  Momentum
 * and adaptive sides stay refused with ALS, the item solve on a shard or a 2-D tile stays MF_ERR_UNSUPPORTED, the user solve
 * works on any shard.  mf_plan_als_solve only enqueues on the plan's stream, under CG as without.  One iteration of
 * mf_plan_iterate / mf_plan_iterate_monitored is the same  als_solve(users, 0);  als_solve(items, 1);  flip.
 * While CG is on and a kind is set mf_plan_describe appends  als=ridge|ridge-count als_cg=<steps>
 * als_cg_form=<form>(chunk=<entries>)  without als_form=.  The forms (MF_ALS_CG_FORM=fixed|dma|general: a compile-time K of
 * the sweeps' list, any even K, any K; by default the first of these that takes the K) give the same bits.
 * Not part of this: CG under the implicit kind through these two calls (it has a switch of its own: the next section),
 * preconditioning, a residual-based stop, K above 256, sharded item solves. */
#define MF_ALS_CG_MAX_STEPS 256
#define MF_ALS_CG_MAX_K     256
int mf_plan_set_als_cg(mf_plan *plan, int steps);
int mf_plan_get_als_cg(mf_plan *plan, int *steps);
/* level 1: mf_backend_run_als with the steps (0: the direct solve).  Bad arguments -> MF_ERR_ARGUMENT before any HIP call. */
int mf_backend_run_als_cg(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                          double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, int kind, int steps,
                          int device);

/* ---- Implicit-feedback ALS by conjugate gradient: the CG steps above under MF_ALS_IMPLICIT, warm-started from the row's
 * current value, in place of the per-row Cholesky (Hu, Koren, Volinsky, ICDM 2008, solved as Takacs, Pilaszy, Tikk do).  The
 * matrix of a row, S + sum_n e_n y_n y_n^T + ridge I, is never formed: its product with a vector v is
 * sum_n e_n y_n (y_n . v) + S v + ridge v.
 *
 * mf_plan_set_implicit_cg(plan, steps) / mf_plan_get_implicit_cg(plan, &steps).  0 <= steps <= MF_ALS_CG_MAX_STEPS; anything
 * else -> MF_ERR_ARGUMENT before any HIP call with nothing changed.  The call is accepted under any kind and in any order with
 * mf_plan_set_als; the value is read at every launch, and only while the kind is MF_ALS_IMPLICIT.  steps = 0, the default, is
 * the direct implicit solve: every bit and every launched kernel is what it is without this section.  (mf_plan_set_als_cg
 * together with MF_ALS_IMPLICIT stays refused: that switch belongs to the explicit kinds.)
 *
 * With steps > 0 under MF_ALS_IMPLICIT, mf_plan_als_solve(plan, side, other_generation)
 *   1. enqueues the Gram S of Y = the other side in that generation: mf_plan_gram's bits;
 *   2. copies the packed triangle into a plan-owned K x K square with an even row stride (an elementwise copy, no arithmetic;
 *      the pad column of an odd K is +0.0);
 *   3. computes every row r of the side X by J0 .. J5.
 * FP64 throughout, every operation rounded once, nothing fused, / correctly rounded, no matrix-core instruction.  dot(u, v) is
 * the serial chain of the CG section.  S(k, j) is S[max(k,j)][min(k,j)].  ridge = lambda_side.  e_n = conf * w_n on a weighted
 * plan and e_n = conf otherwise.  The row's entries n = 0 .. cnt-1 come in the side's entry order; a_n is the value, y_n the Y
 * row.  The padding of a row is never read or written.
 *   J0. x = X_old[r][0..K).
 *   J1. For every entry:  c_n = 1.0 + e_n;  ac_n = a_n * c_n;  t_n = dot(y_n, x);  d_n = ac_n - (e_n * t_n).
 *   J2. g[k] starts at 0.0; for n ascending  g[k] = g[k] + (d_n * y_n[k]).
 *       sx[k] starts at 0.0; for j = 0 .. K-1 ascending  sx[k] = sx[k] + (S(k, j) * x[j]).
 *       r[k] = (g[k] - sx[k]) - (ridge * x[k]).
 *   J3. p = r;  rs = dot(r, r).
 *   J4. For s = 1 .. steps:
 *       a. If rs == 0.0 leave the loop (a NaN is not equal and goes on).
 *       b. u_n = dot(y_n, p);  ue_n = u_n * e_n.
 *       c. q[k] starts at 0.0; for n ascending  q[k] = q[k] + (ue_n * y_n[k]).
 *          sp[k] is formed like sx, with p in place of x.
 *          q[k] = (q[k] + sp[k]) + (ridge * p[k]).
 *       d, e, f. exactly C4d, C4e and C4f: pq = dot(p, q), NOT POSITIVE DEFINITE when !(pq > 0.0), alpha, x, r, rn, beta, p;
 *          the last step's f is skipped.
 *   J5. The box projection of mf_plan_set_bounds on the bounded columns, then the store.  The row is counted as solved.
 * A row WITHOUT ENTRIES is solved like any other: its entry sums are empty.  kept_empty is 0 under this kind, as in the direct
 * implicit solve.  A NaN in Y makes S NaN: every row is then not positive definite and keeps X_old's bits.  In exact
 * arithmetic K steps reach the solution of the direct implicit solve, and no step increases the row's quadratic.
 *
 * Limits and refusals are those of the direct implicit kind: a frozen column on the solved side is refused at launch
 * (MF_ERR_UNSUPPORTED before any HIP call), momentum and adaptive sides are refused, the item solve on a shard or a 2-D tile
 * is MF_ERR_UNSUPPORTED, K <= 128 (S is mf_plan_gram's).  One iteration of mf_plan_iterate / mf_plan_iterate_monitored keeps
 * its order:  gram(items, current);  als_solve(users, 0);  gram(users, next);  als_solve(items, 1);  flip.  While the steps
 * are on and the kind is implicit mf_plan_describe appends  als=implicit conf=<%.17g> implicit_cg=<steps>
 * als_cg_form=<form>(chunk=<entries>)  without als_form=.  The forms are the CG section's (MF_ALS_CG_FORM) and give the same
 * bits.
 * Not part of this: K above 128, a frozen column, preconditioning, a residual-based stop, sharded item solves. */
int mf_plan_set_implicit_cg(mf_plan *plan, int steps);
int mf_plan_get_implicit_cg(mf_plan *plan, int *steps);
/* level 1: mf_backend_run_implicit with the steps (0: the direct solve; mf_backend_run_implicit is this call with 0).  Bad
 * arguments, the steps among them -> MF_ERR_ARGUMENT before any HIP call, nothing touched. */
int mf_backend_run_implicit_cg(const mf_problem *p, const double *weight, double *L, double *R, int32_t *best, double lambda_users,
                               double lambda_items, const mf_bounds *bounds_users, const mf_bounds *bounds_items, double conf,
                               int steps, int device);

/* ---- Ranks of the held-out entries: where each held-out item lands in its user's recommendation order, for the plan's
 * current factors.  An extension (the reference ranks nothing), so the definition is this library's.  For held-out entry
 * n = (i, j, a) -- the rating a plays no part --
 *   C_i      = the items user i has NOT rated in the training entries: exactly the set mf_plan_recommend* choose from
 *              (block-relative on a 2-D tile, like every other item index: a tile ranks among its own items);
 *   B[i][.]  = the exact scores (mat2d_prod, mat2d.c:100-113: sequential k from 0.0, multiply and add unfused) --
 *              mf_plan_predict's bits;
 *   j not in C_i (the pair is also a training pair)  ->  rank[n] = MF_RANK_MASKED;
 *   B[i][j] is NaN                                   ->  rank[n] = MF_RANK_NAN;
 *   otherwise rank[n] = #{ j' in C_i, j' != j : B[i][j'] > B[i][j]  or  (B[i][j'] == B[i][j] and j' < j) },
 * comparisons as IEEE 754 defines them: a NaN B[i][j'] never counts, +0.0 == -0.0, equal infinities tie.  rank[n] is
 * 0-based and reported in the order the caller gave the entries to mf_plan_set_heldout.  Other held-out items of the
 * same user stay candidates; a pair given twice gets the same rank twice.  For a user none of whose candidate scores is
 * NaN:  rank[n] = r < N  <=>  mf_plan_recommend_topn(N) has items[i][r] == j, for every N <= MF_TOPN_MAX.
 * Default form: one counting pass over L R^T on the FP64 matrix cores; an entry is certified when no open item's
 * approximate score lies within the margin of mf_plan_recommend around B[i][j] and none is non-finite, every other entry
 * is counted again with exact scores, so the result is the definition's in all cases.  Matrix-core forms exist for the K
 * of mf_plan_recommend_topn; other K, and MF_RECOMMEND_IMPL=exact, count exactly for every entry. */
#define MF_RANK_MASKED (-1)
#define MF_RANK_NAN    (-2)
/* rank: one int32 per held-out entry, the caller's order.  No held-out set or no factors: MF_ERR_STATE; rank == NULL:
 * MF_ERR_ARGUMENT; both before any HIP call. */
int mf_plan_rank_heldout(mf_plan *plan, int32_t *rank);
/* the last mf_plan_rank_heldout: entries that went through the exact pass (-1 when the exact form ran for all) and the
 * form that ran (0 exact for all, 1 matrix cores at two workgroups per CU, 2 at one per CU; -1 before the first call).
 * Either pointer may be NULL. */
int mf_plan_rank_heldout_info(mf_plan *plan, int64_t *exact_pass_entries, int32_t *mfma_form);

typedef struct mf_rank_metrics {
	int64_t evaluated, masked, nan;   /* rank >= 0, == MF_RANK_MASKED, == MF_RANK_NAN */
	int64_t users;                    /* users with at least one evaluated entry */
	int64_t hits;                     /* evaluated entries with rank < cutoff */
	double hit_rate;                  /* (double) hits / (double) evaluated */
	double mrr;                       /* (sum over n ascending, from 0.0, of 1.0 / (double) (rank[n] + 1)) / evaluated */
	double ndcg;                      /* mean over those users, ascending user id, of DCG_i / IDCG_i */
} mf_rank_metrics;
/* Hit rate, mean reciprocal rank and NDCG at `cutoff` from a rank vector (plain C++, no HIP call: works without a GPU).
 * row[n] = the user of entry n (any ids >= 0, any order).  DCG_i = sum, in the caller's order from 0.0, over the user's
 * evaluated entries with rank < cutoff of 1.0 / log2((double) (rank + 2)); IDCG_i = sum for r = 0 .. min(h_i, cutoff) - 1 of
 * 1.0 / log2((double) (r + 2)), h_i = the user's evaluated entries.  evaluated == 0: the three doubles are NaN.  cutoff is
 * not limited by MF_TOPN_MAX.  cutoff < 1, a rank < MF_RANK_NAN or a negative user id: MF_ERR_ARGUMENT.  Ranks of user
 * shards concatenate: the metrics of the whole are those of the concatenated vectors. */
int mf_backend_rank_metrics(const int32_t *rank, const int32_t *row, int64_t n, int32_t cutoff, mf_rank_metrics *out);

/* Dense predictions of this shard's users, B (user_count x items, row-major) = L R^T exactly as mat2d_prod
 * (mat2d.c:100-113) forms them; for debug dumps of SMALL instances (user_count*items <= 2^26). */
int mf_plan_predict(mf_plan *plan, double *B);

int mf_plan_synchronize(mf_plan *plan);

/* Per-launch device timing (HIP events on the plan's stream).  After mf_plan_timing(plan, 1) every
 * sweep launch is bracketed by events; mf_plan_timing_read drains them (synchronises) and reports
 * launch counts and summed milliseconds of the item sweeps and of the user sweeps. */
int mf_plan_timing(mf_plan *plan, int enable);
int mf_plan_timing_read(mf_plan *plan, int64_t *item_launches, double *item_ms,
                        int64_t *user_launches, double *user_ms);

/* The user sweep in item bands.  A seeded user sweep of the plain rule (no decay, momentum, frozen column, bounds, weights
 * or adaptive side) may run as several launches on the plan's stream, each walking the entries of every row that fall in
 * one range of item ids and handing the partial row on through the next-generation buffer -- the same adds in the same
 * order, so the same bits as one launch.  The library decides when the plan is created (large uniformly rated item factors
 * and long enough rows; MF_SWEEP_BANDS=<n> sets the count, 0 turns the bands off) and needs rows of ascending item ids.
 * Per-launch timing counts the sequence as one user launch.  mf_plan_describe appends user_bands=<n> while the next seeded
 * user sweep would run in n bands; an unseeded sweep always is one launch. */

/* Introspection for tests/bench: name of the sweep kernel variant chosen for this K, LDS bytes, chunk. */
int mf_plan_describe(mf_plan *plan, char *buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif /* MATFACT_HIP_H */
