/*
 * mmsbm_hip.h -- C ABI of the MI355X-native (gfx950) EM core for the Mixed-Membership
 * Stochastic Block Model.
 *
 * This is the drop-in boundary for the hot path of eudald-seeslab/mmsbm (paths below
 * are relative to the reference checkout):
 *
 *   src/backend.py:16-22              load_backend(name) -> (compute_omegas,
 *                                     update_coefficients, prod_dist, name)
 *   src/kernels_numpy.py:21-36        compute_omegas(data, theta, eta, pr)
 *   src/kernels_numpy.py:43-79        update_coefficients(data, theta, eta, pr)
 *   src/kernels_numpy.py:86-96        prod_dist(data, theta, eta, pr)
 *   src/expectation_maximization.py:118-120,152-155,157-167
 *                                     normalize_with_d / normalize_with_self / compute_likelihood
 *   src/mmsbm.py:243-256              the per-restart EM loop
 *
 * The reference has no native layer; a Python module `kernels_hip` binds these entry
 * points with ctypes.  Conventions:
 *
 *   - plain C types only; every host buffer is owned by the caller, C-contiguous,
 *     float64 / int32, and is never retained after the call returns;
 *   - host-side parameter layouts are the reference's: theta (U,K), eta (I,L),
 *     pr (K,L,R), row-major;
 *   - every function returns 0 on success or an MMSBM_E_* code; the message for the
 *     calling thread's last failure is mmsbm_hip_last_error();
 *   - a context is bound to one device and one stream and must be driven by one host
 *     thread at a time; distinct contexts (e.g. one per GPU) are independent;
 *   - there is no CPU fallback: without a usable HIP device every call fails.
 */
#ifndef MMSBM_HIP_H
#define MMSBM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMSBM_HIP_ABI_VERSION 1

enum {
  MMSBM_OK = 0,
  MMSBM_E_INVALID = 1,     /* bad argument (null pointer, index out of range, size) */
  MMSBM_E_HIP = 2,         /* a HIP runtime call failed                              */
  MMSBM_E_NODEVICE = 3,    /* no usable gfx950 device                                */
  MMSBM_E_UNSUPPORTED = 4, /* shape outside what the kernels are instantiated for    */
  MMSBM_E_TOOLARGE = 5,    /* output would exceed the caller's capacity / byte cap   */
  MMSBM_E_INTERNAL = 6
};

typedef struct mmsbm_hip_ctx mmsbm_hip_ctx;

/* ---- library / device ---------------------------------------------------------- */
int mmsbm_hip_abi_version(void);
/* Identity of the kernel sources this binary was compiled from: the first 16 hex digits of the SHA-256 over
 * every file under mmsbm_amd/csrc (name, NUL, contents; in name order) -- what mmsbm_amd/build.py computes
 * and bench.py / profiles/pmc_summary.json record, so that a measurement can say which kernels really ran.
 * "unknown" when the library was built without the build script. */
const char *mmsbm_hip_build_id(void);
const char *mmsbm_hip_last_error(void);
int mmsbm_hip_device_count(int *count);
/* name: caller buffer of name_len bytes; arch e.g. "gfx950:sramecc+:xnack-". */
int mmsbm_hip_device_info(int device, char *name, int name_len, int *compute_units,
                          int64_t *global_mem_bytes);
/* PCI bus id of the device ("0000:05:00.0", hipDeviceGetPCIBusId): with the name, what tells the ranks of a
 * multi-GPU job apart -- bench.py prints it per rank so that a line proves which GPUs it ran on. */
int mmsbm_hip_device_pci(int device, char *bus_id, int bus_id_len);
/* Device memory that is free right now / in total (hipMemGetInfo): what batches of restart
 * slots are sized from -- other contexts and processes on the same GPU already count. */
int mmsbm_hip_device_mem(int device, int64_t *free_bytes, int64_t *total_bytes);

/* ---- context = (device, encoded training triples) -------------------------------- */
/* Replaces the per-call re-gathering of `data` in src/kernels_numpy.py:26-28 and the
 * degree pre-computation of src/mmsbm.py:100-111.  user/item/rating: n_obs int32 ids in
 * [0,U) / [0,I) / [0,R).  Uploads, sorts (rating,item)-major and user-major, builds the
 * CSR offsets and degrees once.  swap_sides != 0 lets the library pair ratings with the
 * users instead of the items when that is the smaller table (results are identical up
 * to summation order); pass 0 for the default, -1 for "choose automatically". */
int mmsbm_hip_create(int device, int64_t n_obs, int32_t n_users, int32_t n_items,
                     int32_t n_ratings, int32_t k_groups, int32_t l_groups,
                     const int32_t *user, const int32_t *item, const int32_t *rating,
                     int swap_sides, mmsbm_hip_ctx **out);
int mmsbm_hip_destroy(mmsbm_hip_ctx *ctx);
/* dims[0..7] = n_obs, U, I, R, K, L, n_pairs (distinct (item,rating) pairs), swapped */
int mmsbm_hip_dims(const mmsbm_hip_ctx *ctx, int64_t dims[8]);
/* d_u (U) and d_i (I): rows per user / item, floored at 1 (src/mmsbm.py:106-111). */
int mmsbm_hip_degrees(const mmsbm_hip_ctx *ctx, int64_t *d_user, int64_t *d_item);
/* The index this context's kernels read, for tests: which 0 .. 15 as mmsbm_hip_layout_array below (the 4-int records
 * flattened; out == NULL queries *count), 16 item_grid ([I][R] pair ids, -1: none; empty when the context has no grid),
 * 17 lik_units (the likelihood's 64-pair units, records like mv_chunks), 18 mv_chunk_off.  Every array that has a device
 * buffer -- pair_off, pair_user, pair_item, user_off, user_pair, item_off, item_pairs, item_deg, mv_chunks, the work
 * items and split segments of both sides, item_grid, lik_units, mv_chunk_off -- is copied from that buffer, device to
 * host, after the context's stream has been synchronised; rating_off, chunk_off and chunks are the context's host copy
 * (it keeps them nowhere else).  All in INTERNAL terms: in a swapped context (dims[7]) the "users" are the caller's items
 * and the pairs are (user, rating) combinations.  Read-only: touches no slot, no session and no EM state.
 * MMSBM_E_INVALID: null context or count, unknown which, capacity below the count.
 * mmsbm_hip_get_option(ctx, "gpu_layout") reads which builder sorted this index: 1 the device, 0 the host. */
int mmsbm_hip_index_array(mmsbm_hip_ctx *ctx, int which, int32_t *out, int64_t capacity, int64_t *count);

/* ---- parameters (device resident between calls) ---------------------------------- */
int mmsbm_hip_set_params(mmsbm_hip_ctx *ctx, const double *theta, const double *eta,
                         const double *pr);
int mmsbm_hip_get_params(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr);
/* The random initialisation of src/mmsbm.py:224-233 ON the device, bit for bit:
 * theta0 = rng.random((U,K)) / d_u, then eta0 = rng.random((I,L)) / d_i, drawn from the PCG64
 * stream (numpy's default_rng) whose state is pcg64_state = { state_hi, state_lo, inc_hi, inc_lo }
 * (numpy: bit_generator.state["state"]["state" | "inc"], split in 64-bit halves).  pr is the
 * third draw -- p0 (K,L,R), already normalised -- which the caller makes on the host from the
 * same stream advanced by U*K + I*L draws (it is tiny).  Equivalent to
 * set_params(theta0, eta0, pr) without generating or moving the two big tables on the host. */
int mmsbm_hip_init_params(mmsbm_hip_ctx *ctx, const uint64_t pcg64_state[4], const double *pr);
/* Host-only: n doubles of that stream starting `offset` draws in (what Generator.random gives
 * after advancing); lets the generator be checked against numpy without a GPU. */
int mmsbm_hip_pcg64_doubles(const uint64_t pcg64_state[4], uint64_t offset, int64_t n, double *out);

/* ---- restart slots: several restarts of one training set in one context ------------- */
/* The reference runs its `sampling` restarts as independent processes over the same triples
 * (src/mmsbm.py:182-185; batching them is the TODO of README.md:188).  A context can hold
 * n_slots independent parameter sets ("slots") that share the sorted triples on the device:
 * mmsbm_hip_em_iterate advances ALL slots with one set of kernel launches (in the two triple
 * passes one group of lanes walks a segment for all slots: one index stream, one contiguous row
 * gather for every restart), every other entry point (set/get_params, update_coefficients, likelihood,
 * compute_omegas, prod_dist) acts on the SELECTED slot.  Slots never interact: slot s holds
 * exactly what a one-slot context given the same parameters would hold, bit for bit.
 * set_slots drops all parameters (set_params must follow for every slot) and selects slot 0 -- also when n_slots is
 * the count the context already has; a new context has one slot.  It leaves every open session (predict, recommend,
 * similar, held-out) as it is: a session holds its own copy of what each add took from a slot, so what was added
 * stays, and slots given parameters afterwards can be added to the same session. */
int mmsbm_hip_set_slots(mmsbm_hip_ctx *ctx, int n_slots);
int mmsbm_hip_select_slot(mmsbm_hip_ctx *ctx, int slot);
/* Any output may be NULL.  bytes_per_slot: device memory one more slot costs (a failed
 * set_slots -- out of device memory -- leaves the context with ONE slot and no parameters). */
int mmsbm_hip_slots(const mmsbm_hip_ctx *ctx, int *n_slots, int *selected,
                    int64_t *bytes_per_slot);

/* ---- the hot loop: src/mmsbm.py:243-250 ------------------------------------------- */
/* n_iters x { update_coefficients; theta = n_theta/d_u; eta = n_eta/d_i;
 * pr = normalize_with_self(n_pr) } entirely on the device; enqueues on the context's
 * stream and returns without synchronising. */
int mmsbm_hip_em_iterate(mmsbm_hip_ctx *ctx, int n_iters);
int mmsbm_hip_synchronize(mmsbm_hip_ctx *ctx);

/* One un-normalised M-step from the current parameters (src/kernels_numpy.py:43-79).
 * Outputs in host layout; the context's parameters are left unchanged.  Any output
 * pointer may be NULL. */
int mmsbm_hip_update_coefficients(mmsbm_hip_ctx *ctx, double *n_theta, double *n_eta,
                                  double *n_pr);

/* src/expectation_maximization.py:157-167 on the current parameters. */
int mmsbm_hip_likelihood(mmsbm_hip_ctx *ctx, double *out);
/* What a finished restart hands back (src/mmsbm.py:256-269): the likelihood and the parameters of the
 * selected slot in one call -- the same values as mmsbm_hip_likelihood + mmsbm_hip_get_params, with the
 * parameter download and its host-side unpacking overlapped with the likelihood kernels (at K = L = 50 and
 * 10M ratings each of the two takes ~33 ms).  theta / eta / pr may be NULL. */
int mmsbm_hip_result(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr, double *likelihood);

/* src/kernels_numpy.py:21-36: (N,K,L) tensor in the ORIGINAL row order of the triples
 * given to create().  Contract / test use only: refuses if N*K*L > capacity_elems. */
int mmsbm_hip_compute_omegas(mmsbm_hip_ctx *ctx, double *out, int64_t capacity_elems);

/* src/kernels_numpy.py:86-96 for n_pairs (user,item) pairs; out is (n_pairs, R). */
int mmsbm_hip_prod_dist(mmsbm_hip_ctx *ctx, int64_t n_pairs, const int32_t *user,
                        const int32_t *item, double *out);

/* ---- predict / score on the device: src/mmsbm.py:297-315 and 488-539 ------------------ */
/* A session over n_rows test triples (ids as in create(); rating = the true rating index;
 * rating_weights: R doubles, the values the reference multiplies the distribution with --
 * its `self.ratings`, src/mmsbm.py:95,518):
 *   begin  uploads the rows; closes any earlier predict session, once its own arguments are accepted;
 *   add    evaluates prod_dist for the SELECTED slot's current parameters, adds it to the
 *          running sum over restarts (in call order, which is numpy's order for
 *          np.array(rats).mean(axis=0)) and returns that restart's indicators;
 *   finish divides by the number of adds, returns the mean distribution (n_rows x R, may be
 *          NULL) and ITS indicators, and closes the session: its device buffers are freed,
 *          whether finish succeeds or not.
 * stats[6] = { rows kept (distribution not all zero), argmax == real, |argmax - real| <= 1,
 *              sum |argmax - real|, real == round(P . w), sum |P . w - real| }, from which
 * accuracy = [1]/[0], one_off = [2]/[0], mae = 1 - [4]/[0], s2 = [3], s2pond = [5]
 * (src/mmsbm.py:530-539).  Counts are exact; argmax takes the first maximum like np.argmax. */
int mmsbm_hip_predict_begin(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user,
                            const int32_t *item, const int32_t *rating,
                            const double *rating_weights);
int mmsbm_hip_predict_add(mmsbm_hip_ctx *ctx, double stats[6]);
int mmsbm_hip_predict_finish(mmsbm_hip_ctx *ctx, double *mean_dist, double stats[6]);

/* ---- top-N recommendation: the best n items per user (mmsbm_amd/csrc/recommend.hpp) ---------------------------- */
/* A session shaped like predict's:
 *   begin  rating_weights: R finite doubles w (the reference's `self.ratings` for the expected rating, one-hot for
 *          P(rating = r)); exclude_train != 0 leaves out the items a user has in the training triples (a pair that
 *          occurs several times counts once).  Closes any earlier recommend session; a predict session is untouched.
 *   add    folds the SELECTED slot's current parameters into the session (the slot itself is left unchanged);
 *   query  for n_users external user ids: score_w(u, i) = (1/S) sum_s sum_r w_r P_s(r | u, i) over the S added slots,
 *          every training item i a candidate, and per user the n best -- score descending, equal scores (exact
 *          fp64 equality) by ascending item id.  items / scores: n_users x n, row b holding counts[b] entries followed
 *          by item -1 / score -inf (scores and counts may be NULL).  A user's scores depend on that user and the items
 *          only: bitwise the same whatever the other users of the call and from call to call.  May be repeated;
 *   end    releases the session's device memory.
 * mmsbm_hip_get_option(ctx, "recommend_ms") reads the device time of the last query's kernels (HIP events).
 * 1 <= n <= MMSBM_HIP_RECOMMEND_MAX_N (larger n: MMSBM_E_UNSUPPORTED).  MMSBM_E_TOOLARGE where the device memory
 * the session needs is not free.  These launches are not part of an EM iteration (mmsbm_hip_kernel_count). */
#define MMSBM_HIP_RECOMMEND_MAX_N 1024
int mmsbm_hip_recommend_begin(mmsbm_hip_ctx *ctx, const double *rating_weights, int exclude_train);
int mmsbm_hip_recommend_add(mmsbm_hip_ctx *ctx);
int mmsbm_hip_recommend_query(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n, int32_t *items,
                              double *scores, int32_t *counts);
int mmsbm_hip_recommend_end(mmsbm_hip_ctx *ctx);
/* Like query, but the users are caller-given theta rows: theta [S][n_users][K] (external K) for the S added slots in
 * add order, folded with each slot's p and the session's weights exactly as add folds the slot's own theta -- so a
 * slot's own row gives bitwise the scores query gives for that user.  Excluded items come from a CSR list: user b
 * leaves out seen_items[seen_offsets[b] .. seen_offsets[b + 1]) (item ids in the session's catalogue [0, I) -- [0, I +
 * n_new) after recommend_add_items -- repeats allowed);
 * seen_offsets NULL: nothing excluded (the session's exclude_train does not apply to these users). */
int mmsbm_hip_recommend_query_theta(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                    const int64_t *seen_offsets, const int32_t *seen_items, int32_t n,
                                    int32_t *items, double *scores, int32_t *counts);
/* Positions of caller-given items in each user's full recommendation order, within the open recommend session.
 * user b's items: items[offsets[b] .. offsets[b+1]) (ids in the session's catalogue, repeats allowed, any order).
 * positions: offsets[n_users] int32 out, 0 = not a candidate.  candidates (may be NULL): n_users int32 out.
 * With the scores and candidates of query: position(u, t) = 1 + #{candidates j : score(u, j) > score(u, t), or
 * score(u, j) == score(u, t) and j < t} for a candidate t, 0 for an excluded item of u;
 * candidates(u) = I - |distinct excluded items of u| (I: the session's catalogue, I + n_new after
 * recommend_add_items; excluded: the training items while exclude_train is set, plus the added items whose seen list
 * names u).  So a candidate at position p <= n is
 * item p - 1 of query's row for n.  Bitwise independent of the other users of the call; only users holding items are
 * scored; touches no slot and no session.  MMSBM_E_TOOLARGE where the device memory a batch needs is not free.
 * mmsbm_hip_get_option(ctx, "position_ms") reads the device time of the last call's kernels (HIP events). */
int mmsbm_hip_recommend_positions(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users,
                                  const int64_t *offsets, const int32_t *items,
                                  int32_t *positions, int32_t *candidates);
/* Appends n_new items to the open session's catalogue, after every recommend_add: eta [S][n_new][L] (external L) for
 * the S added slots in add order, folded with each slot's W exactly as add folds the slot's own eta.  New item j gets
 * id I + j.  seen_offsets / seen_users (CSR over the new items, user ids in [0, U), repeats allowed; NULL: none):
 * the training users that have rated new item j -- that (user, item) pair is then left out like a training pair
 * (also when exclude_train is 0).  From here on query, query_theta and positions rank all I + n_new items; a training
 * item's score is bitwise what it was before the call.  Once per session, after the first add and before any further
 * add (otherwise MMSBM_E_INVALID); n_new == 0 changes nothing. */
int mmsbm_hip_recommend_add_items(mmsbm_hip_ctx *ctx, int32_t n_new, const double *eta,
                                  const int64_t *seen_offsets, const int32_t *seen_users);

/* The m best (user, item) pairs of the whole request, within the open recommend session (mmsbm_amd/csrc/top_pairs.hpp):
 * candidates are all pairs (u, i), u in users[0 .. n_users) (distinct external ids, any order; users NULL: every
 * training user, n_users ignored), i in the session's catalogue, without the pairs the session leaves out for u;
 * score_w(u, i) bit for bit what query returns for the pair; order: score descending, equal scores (exact fp64
 * equality) by ascending user id, then ascending item id.  out_users / out_items / out_scores: m entries each, the first
 * *count = min(m, candidates) hold the answer, the rest -1 / -1 / -inf.  The answer does not depend on how the work is
 * split: option "top_pairs_groups" (0: the library's choice, else the number of workgroups, at most 4096) changes the
 * time only.  No buffer of n_users x items exists: device memory is O(groups x m + n_users), the launches of a query
 * do not depend on the sizes.  mmsbm_hip_get_option(ctx, "top_pairs_ms") reads the device time of the last call's
 * kernels (HIP events).  MMSBM_E_INVALID: no session, no slot added, an id out of range, a repeated id, m < 1;
 * m > MMSBM_HIP_TOP_PAIRS_MAX_M: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory of the lists is not
 * free.  Touches no slot, no EM state and no predict / similar session; the recommend session stays open. */
#define MMSBM_HIP_TOP_PAIRS_MAX_M 1024
int mmsbm_hip_recommend_top_pairs(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t m,
                                  int32_t *out_users, int32_t *out_items, double *out_scores, int32_t *count);

/* The same question for m beyond MMSBM_HIP_TOP_PAIRS_MAX_M (mmsbm_amd/csrc/pairs_bulk.hpp): candidates, scores and order
 * are recommend_top_pairs', for 1 <= m <= MMSBM_HIP_TOP_PAIRS_BULK_MAX_M.  The bar -- the score of the last returned
 * pair -- is found exactly by a radix select over the score tiles, the pairs above it and the ties the order admits are
 * written by count-then-write, and the entries are sorted on the device; nothing of size n_users x items exists, device
 * memory is O(m + n_users).  out_users / out_items / out_scores: m entries each, the first *count = min(m, candidates)
 * hold the answer, the rest -1 / -1 / -inf.  *bar: the score of the last returned pair (+0.0 for a zero of either sign;
 * -inf without candidates); counts[0]: candidates that score strictly above the bar, counts[1]: exactly the bar (fp64
 * equality), counts[2]: candidates -- so recommend_audience at min_score = *bar over every item returns counts[0] +
 * counts[1] pairs of these users.  Options "pairs_bulk_groups" (workgroups, 0 .. 4096), "pairs_bulk_bits" (bits per
 * digit of the select, 0 .. 12) -- 0: the library's choice -- and "pairs_bulk_collect" (the select stops and sorts a
 * bin of at most this many keys; 0: never; at most 2^24) change the time only; "pairs_bulk_ms" reads the device time
 * of the last call, "pairs_bulk_passes" / "pairs_bulk_collected" the passes it ran and the keys it sorted.  Refusals as
 * recommend_top_pairs: MMSBM_E_INVALID for no session, no slot added, an id out of range, a repeated id, m < 1, a null
 * pointer; m > MMSBM_HIP_TOP_PAIRS_BULK_MAX_M: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory for
 * min(m, candidates) entries is not free.  Touches no slot, no EM state and no other session; the recommend session
 * stays open and answers as before.
 * recommend_pair_bar: the same request, *bar and counts alone -- the select and one counting pass, no output buffers. */
#define MMSBM_HIP_TOP_PAIRS_BULK_MAX_M 67108864
int mmsbm_hip_recommend_top_pairs_bulk(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int64_t m,
                                       int32_t *out_users, int32_t *out_items, double *out_scores, int64_t *count,
                                       double *bar, int64_t counts[3]);
int mmsbm_hip_recommend_pair_bar(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int64_t m, double *bar,
                                 int64_t counts[3]);

/* Item-side queries of the open recommend session (mmsbm_amd/csrc/audience.hpp): who should see an item.  items[0 ..
 * n_items): ids in the session's catalogue (training items, and I .. I + n_new - 1 after recommend_add_items), any
 * order, repeats allowed.  score_w(u, i) is bit for bit what query returns for the pair, in swapped and unswapped
 * contexts; the pair (u, i) is left out exactly when query leaves i out for u (the training pairs while exclude_train
 * is set, the seen lists of recommend_add_items always, a duplicate pair once), so candidates(i) = U - |distinct
 * excluded users of i|.  The item -> users lists are the transpose of the session's lists, built by the first of these
 * calls and again after recommend_add_items.  Both touch no slot, no EM state and no other session; the recommend
 * session stays open and its later answers are bitwise unchanged.  MMSBM_E_INVALID: no session, no slot added, an id
 * outside the catalogue, a null pointer where one is needed.
 *
 * query_items: the n best candidate users of each item; order: score descending, equal scores (exact fp64 equality)
 * by ascending user id.  users / scores [n_items][n], row b holds counts[b] = min(n, candidates) entries, the rest
 * -1 / -inf (scores, counts may be NULL).  A row depends on its item only.  n < 1: MMSBM_E_INVALID; n >
 * MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory a batch needs is not free.
 * The kernels are query's own with the two tables exchanged; "recommend_ms" reads their device time. */
int mmsbm_hip_recommend_query_items(mmsbm_hip_ctx *ctx, int64_t n_items, const int32_t *items, int32_t n,
                                    int32_t *users, double *scores, int32_t *counts);
/* audience: for each item every candidate user with score_w(u, i) >= min_score (finite; the comparison is made on the
 * final score, the quotient by the number of slots), in ascending user id, as a CSR: offsets[n_items + 1] (always
 * filled), item b's users[offsets[b] .. offsets[b + 1]) and their scores.  users == NULL: sizes only (scores ignored).
 * users given and capacity < offsets[n_items]: MMSBM_E_TOOLARGE with offsets filled and nothing else written; the caller
 * allocates and calls again.  No buffer of U x n_items scores exists: a fused kernel counts per (item, 128-user tile),
 * a small kernel turns the counts into offsets, and the fused kernel runs again to write.  The result does not depend
 * on how the work is split: options "audience_rows" (items per counting batch) and "audience_entries" (entries per
 * writing batch at most; a larger item goes alone), 0: the library's choice, change time and memory only.
 * "audience_ms" reads the device time of the call's kernels.  A non-finite min_score: MMSBM_E_INVALID;
 * MMSBM_E_TOOLARGE also where the device memory of a batch is not free. */
int mmsbm_hip_recommend_audience(mmsbm_hip_ctx *ctx, int64_t n_items, const int32_t *items, double min_score,
                                 int64_t capacity, int64_t *offsets, int32_t *users, double *scores);

/* Queries within a part of the catalogue, inside the open recommend session (mmsbm_amd/csrc/catalogue.hpp): the items
 * in stock, of one category, released this week; items a user has dismissed; the candidates a cheap retriever proposes.
 * score_w(u, i) is bit for bit what query returns for the pair, in swapped and unswapped contexts, and the order is
 * query's (score descending, equal scores by ascending item id) cut to the candidates: each answer is the user's row
 * of query(n = all items), filtered to the candidates and cut to n.  Output as query's: items / scores [n_users][n],
 * row b holding counts[b] = min(n, candidates left) entries, then -1 / -inf (scores, counts may be NULL).  All three
 * touch no slot, no EM state, no other session and nothing of the recommend session: a later query answers as before.
 * "recommend_ms" reads the device time of the call's kernels.  MMSBM_E_INVALID (before any launch): no session, no
 * slot added, an id out of range, a candidate list that is not strictly ascending (a repeat included), a bad CSR,
 * n < 1; n > MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory is not free.
 *
 * query_within: the candidates are cand_items[0 .. n_cand), strictly ascending ids of the session's catalogue (ids of
 * recommend_add_items included), shared by the users of the call; cand_items NULL: the whole catalogue (n_cand
 * ignored) -- then, without excl_offsets, the call IS query.  Left out for row b: what query leaves out for users[b],
 * and excl_items[excl_offsets[b] .. excl_offsets[b + 1]) (excl_offsets: int64 [n_users + 1] or NULL; ids of the
 * catalogue, any order, repeats allowed, items outside the candidates are ignored).  The lists go by the row's place in
 * the request: a user asked twice may carry two lists.  n_cand == 0: every count is 0.  The scores of n_users x n_cand
 * pairs are formed, not n_users x items: the candidates' rows are gathered into a compact table first.
 *
 * query_theta_within: query_theta (caller-given theta rows, seen lists per row) within cand_items as above.
 *
 * rank: row b's candidates are cand_items[offsets[b] .. offsets[b + 1]) (offsets: int64 [n_users + 1]), each list
 * strictly ascending, of any length; users may repeat.  What query leaves out for users[b] is left out.  One wave per
 * row scores and selects its list; no buffer of scores exists. */
int mmsbm_hip_recommend_query_within(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                     const int32_t *cand_items, const int64_t *excl_offsets,
                                     const int32_t *excl_items, int32_t n, int32_t *items, double *scores,
                                     int32_t *counts);
int mmsbm_hip_recommend_query_theta_within(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                           const int64_t *seen_offsets, const int32_t *seen_items, int32_t n_cand,
                                           const int32_t *cand_items, int32_t n, int32_t *items, double *scores,
                                           int32_t *counts);
int mmsbm_hip_recommend_rank(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, const int64_t *offsets,
                             const int32_t *cand_items, int32_t n, int32_t *items, double *scores, int32_t *counts);

/* Per-category caps, inside the open recommend session (mmsbm_amd/csrc/quota.hpp): at most cat_caps[g] items of
 * category g in a row's list -- two per brand, one sponsored item, none of a category that is blocked (cap 0).
 * Category g holds the catalogue items cat_items[cat_offsets[g] .. cat_offsets[g + 1]) (cat_offsets: int64
 * [n_cats + 1]; ids of the session's catalogue, those of recommend_add_items included; strictly ascending inside a
 * category, no item in two categories); an item in no category is uncapped.  The one definition: take query_within's
 * full order of row b's candidates (score descending, equal scores by ascending item id; what query leaves out,
 * cand_items and excl_* applied first), walk it, take an item unless cat_caps[g] items of its category were taken
 * before it, stop after n.  A capped-out or excluded item never counts towards a category; the scores are query's bit
 * for bit; a cap >= n has no effect; n_cats == 0 IS query_within (query_theta_within).  The answer is exact at any
 * catalogue size: the walk equals the top n of the items whose rank inside their own category is at most the cap, which
 * a mask over the batch's scores leaves before the unchanged selection.  Arguments and output otherwise as query_within
 * / query_theta_within; "recommend_ms" reads the device time of the call's kernels.  MMSBM_E_INVALID (before any
 * launch): what query_within / query_theta_within refuse, n_cats < 0, a bad CSR, an item id out of range, a category
 * that is not strictly ascending, an item in two categories, a negative cap; n > MMSBM_HIP_RECOMMEND_MAX_N:
 * MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory is not free. */
int mmsbm_hip_recommend_query_quota(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                    const int32_t *cand_items, const int64_t *excl_offsets, const int32_t *excl_items,
                                    int64_t n_cats, const int64_t *cat_offsets, const int32_t *cat_items,
                                    const int32_t *cat_caps, int32_t n, int32_t *items, double *scores,
                                    int32_t *counts);
int mmsbm_hip_recommend_query_theta_quota(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                          const int64_t *seen_offsets, const int32_t *seen_items, int32_t n_cand,
                                          const int32_t *cand_items, int64_t n_cats, const int64_t *cat_offsets,
                                          const int32_t *cat_items, const int32_t *cat_caps, int32_t n, int32_t *items,
                                          double *scores, int32_t *counts);

/* Category-level recommendation, inside the open recommend session (mmsbm_amd/csrc/shelves.hpp): which categories
 * ("shelves") to show a row -- the rows of a front page -- and each shelf's best items.  The categories are given as the
 * quota entries give them (cat_offsets int64 [n_cats + 1], cat_items: ids of the session's catalogue, those of
 * recommend_add_items included; strictly ascending inside a category, no item in two categories); an item in none of
 * them belongs to no shelf.  The one definition: for row b take query_within's candidates (what query leaves out,
 * cand_items and excl_* applied) with their scores, query's bit for bit.  For category g let s_1, s_2, ... be its
 * candidates' scores in query's order (score descending, equal scores by ascending item id) and a their number.
 * a < min_items: the category is no candidate of the row.  Otherwise t = min(depth, a) and the category's VALUE is
 * ((..((s_1 + s_2) + s_3) + ..) + s_t) / t: the additions left to right from s_1, one IEEE division (depth 1: the best
 * item's score, bit for bit; depth >= a: the mean of all).  The row's shelves are the n_shelves categories of largest
 * value, equal values by ascending category index of the call; the items of a shelf are the first min(per_shelf, a) of
 * s_1, s_2, ...  A row's answer depends on that row alone.
 * Output: shelf_cats (category indices of the call) / shelf_values / shelf_available (a) [n_users][n_shelves], row b
 * holding shelf_counts[b] entries, then -1 / -inf / 0; items / scores [n_users][n_shelves][per_shelf], shelf k of row b
 * holding item_counts[b * n_shelves + k] entries, then -1 / -inf; with per_shelf == 0 the last three may be NULL.
 * n_cats == 0, or no category with a candidate item: every row is empty and nothing is launched.  Arguments otherwise
 * as query_within / query_theta_within; "recommend_ms" reads the device time of the call's kernels.  MMSBM_E_INVALID
 * (before any launch): what query_within / query_theta_within refuse, n_cats < 0, a bad CSR, an item id out of range, a
 * category that is not strictly ascending, an item in two categories, depth < 1, min_items < 1, n_shelves < 1,
 * per_shelf < 0, a null output that is needed; depth, n_shelves or per_shelf > MMSBM_HIP_RECOMMEND_MAX_N:
 * MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory is not free. */
int mmsbm_hip_recommend_query_shelves(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                      const int32_t *cand_items, const int64_t *excl_offsets,
                                      const int32_t *excl_items, int64_t n_cats, const int64_t *cat_offsets,
                                      const int32_t *cat_items, int32_t depth, int32_t min_items, int32_t n_shelves,
                                      int32_t per_shelf, int32_t *shelf_cats, double *shelf_values,
                                      int32_t *shelf_available, int32_t *shelf_counts, int32_t *items, double *scores,
                                      int32_t *item_counts);
int mmsbm_hip_recommend_query_theta_shelves(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                            const int64_t *seen_offsets, const int32_t *seen_items, int32_t n_cand,
                                            const int32_t *cand_items, int64_t n_cats, const int64_t *cat_offsets,
                                            const int32_t *cat_items, int32_t depth, int32_t min_items,
                                            int32_t n_shelves, int32_t per_shelf, int32_t *shelf_cats,
                                            double *shelf_values, int32_t *shelf_available, int32_t *shelf_counts,
                                            int32_t *items, double *scores, int32_t *item_counts);

/* Randomised top-N with logged propensities, inside the open recommend session (mmsbm_amd/csrc/explore.hpp): every
 * other query returns the same list on every call, so items just below the cut are never shown and nothing logged can
 * evaluate another policy.  query_explore draws row b's list WITHOUT replacement from the Plackett-Luce distribution
 * over query_within's candidates of the row (what query leaves out, cand_items and excl_* applied) with utilities
 * score / temperature, and returns the probability of every position.  The one definition, for user u = users[b]:
 *   r(u, i)   the double numpy's Generator.random() returns as draw number u * 2^32 + i (counting from 0) of the PCG64
 *             stream pcg64_state = { state_hi, state_lo, inc_hi, inc_lo } (as mmsbm_hip_init_params takes it): in numpy,
 *             bg.advance(u << 32 | i), then one random().  A function of the stream, u and i alone;
 *   g(u, i)   E = -log(1 - r), E = 2^-54 where r = 0; g = -log(E): always finite;
 *   key       s(u, i) + temperature * g(u, i): the product rounded, then the sum rounded (no fma); s: query's bits;
 *   list      the n candidates of largest key, key descending, equal keys by ascending item id;
 *   propensity of position t = 1 .. counts[b]: with m = the row's largest candidate score and
 *             e_i = exp((s_i - m) / temperature), e_t / R_t where R_t = the sum of e_i over the candidates not ranked
 *             above t -- accumulated from those candidates in a fixed order, never as a difference, so the last
 *             remaining candidate of a row has propensity exactly 1.0.  The product of a row's propensities is the
 *             probability of its list.
 * Output as query_within's, scores being the SCORES of the listed items (not the keys), plus propensity [n_users][n],
 * padded with 0 (scores, propensity, counts may be NULL).  A row depends on its user and the arguments alone, bit for
 * bit.  The temperature floor: a score lies in [min w, max w] of the session's weights, and (max w - min w) /
 * temperature > 700 is refused -- below that temperature the policy is query's list to within 1e-300, and no e_i
 * underflows above it.  "recommend_ms" reads the device time of the call's kernels.  MMSBM_E_INVALID (before any
 * launch): what query_within refuses, a temperature that is not finite, <= 0 or below the floor, a null pcg64_state;
 * n > MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory is not free (a second
 * batch buffer holds the unperturbed scores).
 *
 * list_propensity: what the policy WOULD have given lists that somebody else logged.  Row b's list is
 * list_items[list_offsets[b] .. list_offsets[b + 1]) (list_offsets: int64 [n_users + 1]; distinct ids of the session's
 * catalogue, at most MMSBM_HIP_RECOMMEND_MAX_N, taken in the order given); scores / propensity [list_offsets[n_users]]
 * (scores may be NULL).  An item that is no candidate of the row gets propensity 0 and score -inf, and the rest of the
 * list is computed as if it were absent; otherwise the definition above, without noise and seed: applied to
 * query_explore's own output with the same arguments it returns that call's propensity bits.  MMSBM_E_INVALID: what
 * query_within refuses, the temperature as above, a bad CSR, an id out of range, an item twice in a list; a list longer
 * than MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED.
 *
 * explore_noise: r and g of the definition for n_pairs arbitrary pairs of non-negative int32 ids, computed on the
 * device by the function the perturbation calls -- the noise of a logged impression can be derived again.  Needs no
 * session and no parameters. */
int mmsbm_hip_recommend_query_explore(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                      const int32_t *cand_items, const int64_t *excl_offsets,
                                      const int32_t *excl_items, int32_t n, double temperature,
                                      const uint64_t pcg64_state[4], int32_t *items, double *scores,
                                      double *propensity, int32_t *counts);
int mmsbm_hip_recommend_list_propensity(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                        const int32_t *cand_items, const int64_t *excl_offsets,
                                        const int32_t *excl_items, double temperature, const int64_t *list_offsets,
                                        const int32_t *list_items, double *scores, double *propensity);
int mmsbm_hip_explore_noise(mmsbm_hip_ctx *ctx, const uint64_t pcg64_state[4], int64_t n_pairs, const int32_t *users,
                            const int32_t *items, double *r, double *g);

/* Capacity-aware allocation, inside the open recommend session (mmsbm_amd/csrc/allocate.hpp): items run out.  Every
 * user of the request asks for n items, item i of the session's catalogue (the items of recommend_add_items included)
 * can be given out caps[i] times: stock, a reviewer's load, coupons per product.  The one definition: take all pairs
 * (u, i) of the request's users and the catalogue that query does not leave out for u, walk them in top_pairs' order
 * (score descending, equal scores by ascending user id, then ascending item id) and take a pair iff u holds fewer than n
 * items and i was given out fewer than caps[i] times.  caps[i] = 0 takes the item out, a negative cap -- and a cap >=
 * n_users -- is unlimited; with every cap unlimited the answer IS query's, and the scores are always query's bits.
 * users: DISTINCT ids (the constraint couples users, not request rows), or NULL: all training users, n_users = their
 * number.  The answer is computed by rounds of user-proposing deferred acceptance, which reach the walk's answer -- the
 * only stable matching under one strict order of the pairs -- without sorting the pairs; *rounds: the rounds run,
 * *converged: 1 when the last of them changed nothing.  After max_rounds rounds that still changed a threshold the
 * answer is cut to a feasible one (rows of at most n, no item beyond its cap; some users may hold fewer items than the
 * walk gives them) and *converged is 0.  Output otherwise as query: rows padded with -1 / -inf, counts[b] the length of
 * row b, which may be below n.  Options "allocate_ms" (device time of the whole call, HIP events) and "allocate_rounds".
 * MMSBM_E_INVALID (before any launch): no session or no slot added, an id out of range, a repeated user id, n < 1,
 * max_rounds < 1, a null caps, rounds or converged; MMSBM_E_UNSUPPORTED: n > MMSBM_HIP_RECOMMEND_MAX_N, or a cap above
 * MMSBM_HIP_RECOMMEND_MAX_N and below n_users (it could bind beyond what a selection holds); MMSBM_E_TOOLARGE where the
 * device memory is not free.  Touches no slot and no other session; later queries of the session answer as before. */
int mmsbm_hip_recommend_allocate(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n,
                                 const int32_t *caps, int32_t max_rounds, int32_t *items, double *scores,
                                 int32_t *counts, int32_t *rounds, int32_t *converged);

/* Welfare-maximising assignment, inside the open recommend session (mmsbm_amd/csrc/assign.hpp): every user of the
 * request gets AT MOST ONE item, item i of the session's catalogue at most caps[i] users (0: none; negative, or >=
 * n_users: unlimited), and  sum of the assigned scores + (unassigned users) x reserve  is as large as it can be, within
 * (assigned users) x epsilon.  allocate above answers the same caps with the one stable assignment; this is the one of
 * largest total, and it prices the items.  The candidates are query's (the session's exclusions), the scores its bits.
 * The answer is computed by a forward auction in Jacobi rounds from prices 0 (the definition, step by step, heads
 * assign.hpp): item i holds caps[i] slots (price, holder); every user without an item bids for its best item at the
 * items' cheapest slot prices, the bid (p1 + (v1 - v2)) + epsilon, or drops out for good when no candidate is worth more
 * than reserve; an item takes its k-th highest bid into its k-th cheapest slot while bid > price, and the holder it
 * displaces bids again.  Doubles are only added, subtracted and compared, so the prices are reproducible bit for bit.
 * users: DISTINCT ids in any order, or NULL: all training users, n_users = their number.  Output by request row b:
 * items[b] (-1: unassigned), scores[b] (-inf), paid[b] (the price of the slot it holds; 0: unassigned or an unlimited
 * item), pi[b] = max(reserve, max over its candidates of score - price[i]) at the final prices; by catalogue item i:
 * price[i] its cheapest slot (0: unlimited, +inf: caps[i] = 0), price_sum[i] the sum of its slot prices, load[i] the
 * users that hold it.  sum(pi) + sum(price_sum) bounds the optimum from above whatever the prices, so the caller sees
 * the gap without solving anything; at convergence the gap is at most (assigned users) x epsilon.  *rounds: the rounds
 * run; *converged: 0 when max_rounds rounds left somebody bidding (the answer is feasible, the bound still holds).
 * Options "assign_ms" (device time of the whole call, HIP events), "assign_rounds" and "assign_bids" (the bids of all
 * rounds).  MMSBM_E_INVALID (before any launch): no session or no slot added, an id out of range, a repeated user id,
 * epsilon not finite, not positive or below (largest - smallest rating weight) x 2^-40 (a bid could fail to raise a
 * price by an ulp), reserve NaN or +inf, max_rounds < 1, a null caps or output; MMSBM_E_UNSUPPORTED: a cap above
 * MMSBM_HIP_RECOMMEND_MAX_N and below n_users; MMSBM_E_TOOLARGE where the device memory is not free (two doubles and
 * two ints of state and a bid per request user, a price and a holder per slot, one batch of scores).  Touches no slot
 * and no other session; later queries of the session answer as before. */
int mmsbm_hip_recommend_assign(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, const int32_t *caps,
                               double reserve, double epsilon, int32_t max_rounds, int32_t *items, double *scores,
                               double *paid, double *pi, double *price, double *price_sum, int32_t *load,
                               int32_t *rounds, int32_t *converged);

/* ---- nearest items / users: the n most similar rows of one side (mmsbm_amd/csrc/similar.hpp) -------------------- */
/* A session of its own beside the recommend session (either may be open while the other is):
 *   begin  side 0: items, 1: users (external sides).  Closes any earlier similarity session;
 *   add    the SELECTED slot's rating profiles and group masses join the session (the slot itself is left unchanged):
 *          items  q_s[i, k, r] = sum_l eta_s[i, l] p_s[k, l, r],    m_s[k] = sum_u theta_s[u, k];
 *          users  q_s[u, l, r] = sum_k theta_s[u, k] p_s[k, l, r],  m_s[l] = sum_i eta_s[i, l];
 *   query  for n_rows ids of the side (repeats allowed, any order): over the S added slots
 *          D(i, j) = ( sum_s sum_k sum_r m_s[k] (q_s[i,k,r] - q_s[j,k,r])^2 ) / (S U)        (users: / (S I))
 *          in the direct form (subtract, square, accumulate: D(i, i) = 0 and identical rows are at distance exactly 0),
 *          and per id the n nearest OTHER rows -- D ascending, equal D (exact fp64 equality) by ascending id.
 *          out_ids / distance: n_rows x n, row b holding counts[b] = min(n, rows - 1) entries followed by id -1 /
 *          distance +inf (distance and counts may be NULL).  A row's answer depends on that id only: bitwise the same
 *          whatever the other ids of the call, the slots the context holds beyond those added, and the side layout;
 *   end    releases the session's device memory (so does mmsbm_hip_destroy).
 * mmsbm_hip_get_option(ctx, "similar_ms") reads the device time of the last query's kernels (HIP events).
 * MMSBM_E_INVALID: side not 0 / 1, add or query without begin, query before the first add, an id outside the side's
 * range, n < 1; n > MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory of the
 * profile tables (rows x groups x R doubles per slot) or of a batch is not free.  Touches no slot, no EM state and no
 * predict / recommend session. */
int mmsbm_hip_similar_begin(mmsbm_hip_ctx *ctx, int side);
int mmsbm_hip_similar_add(mmsbm_hip_ctx *ctx);
int mmsbm_hip_similar_query(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *ids, int32_t n, int32_t *out_ids,
                            double *distance, int32_t *counts);
int mmsbm_hip_similar_end(mmsbm_hip_ctx *ctx);

/* ---- diversified top-N and the distance of given pairs (mmsbm_amd/csrc/diverse.hpp) ------------------------------- */
/* similar_pairs: distance[e] = D(a[e], b[e]) of the open similarity session (either side), e < n_pairs; ids of the
 * session's side, any order, repeats allowed.  The number is query's for the pair, bit for bit, with a[e] as the query
 * row: D(a, b) and D(b, a) have equal bits, D(a, a) and D between identical rows is +0.0.  MMSBM_E_INVALID: no session,
 * no slot added, an id out of range, negative n_pairs.
 *
 * recommend_diverse: the greedy re-ranking of each user's `pool` best candidates, with score(u, i) of the open
 * recommend session and D(i, j) of the open similarity session of side ITEMS.  For request row b:
 *   pool   P = the row recommend_query_within(users, cand_items, excl_*, n = pool) returns: the same exclusions, the
 *          same optional candidate subset, the same order and score bits; M = its count;
 *   pick 1 t_1 = P[0];
 *   pick j (j = 2 .. min(n, M)): over the i of P not picked yet, m_i = min over a < j of D(t_a, i),
 *          v_i = fma(trade_off, m_i, score_i) (one rounding); t_j = the i with the largest v_i, equal v_i (exact fp64
 *          equality) to the earlier place in P.
 * items / scores / distances: [n_users][n]; row b holds counts[b] = min(n, M) picks -- the item, its score (the pool's
 * bits) and m at the moment of the pick, the distance to the nearest earlier pick (+inf for pick 1) -- then -1 / -inf /
 * +inf (scores, distances, counts may be NULL).  trade_off is in score units per unit of distance: at 0 the answer is
 * recommend_query_within(n), bit for bit; as it grows the list tends to the farthest-point order inside the pool.  A
 * row's answer depends on its user and the arguments only.  The pool never visits the host.
 * THE CALLER'S CONTRACT: both sessions hold the same slots, added in the same order -- the library checks that their
 * numbers agree and cannot check more.
 * MMSBM_E_INVALID (before any launch): no recommend session or no slot added to it; no similarity session, one of side
 * users, or no slot added to it; the two sessions' slot counts differ; the recommend session's catalogue was grown by
 * recommend_add_items; an id out of range; cand_items not strictly ascending; a bad CSR; n < 1; pool < n; trade_off
 * negative, NaN or infinite.  pool > MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device
 * memory is not free (the rows of a request are taken in parts while the pool lists, n_users x pool x 12 bytes, are
 * not; option "diverse_rows": rows per part, 0 = the library's choice -- time and memory, never the answer).
 *
 * Both write nothing of any session, slot or predict session: a later query answers as before.  "diverse_ms" reads the
 * device time of the last call's kernels. */
int mmsbm_hip_similar_pairs(mmsbm_hip_ctx *ctx, int64_t n_pairs, const int32_t *a, const int32_t *b, double *distance);
int mmsbm_hip_recommend_diverse(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                const int32_t *cand_items, const int64_t *excl_offsets, const int32_t *excl_items,
                                int32_t n, int32_t pool, double trade_off, int32_t *items, double *scores,
                                double *distances, int32_t *counts);

/* Group queries of the open recommend session (mmsbm_amd/csrc/group.hpp): what a set of users should get together.
 * Group g's members are members[offsets[g] .. offsets[g + 1]): ids of training users, in any order, distinct within a
 * group (a user may be in several groups).  With score(m, i) the score recommend_query gives the pair, bit for bit, the
 * group's value of item i is
 *   MMSBM_HIP_GROUP_MIN    least misery:   min_m score(m, i)
 *   MMSBM_HIP_GROUP_MAX    most pleasure:  max_m score(m, i)
 *   MMSBM_HIP_GROUP_COUNT  approval:       the number of members with score(m, i) >= bar, as a double (`bar` is
 *                          compared with the final score, the quotient by S; it is ignored by the other modes)
 *   MMSBM_HIP_GROUP_MEAN   the score of the group's mean row: per slot xbar[j] = (x[m_0, j] + x[m_1, j] + ...) / |g|,
 *                          one chain from +0.0 in the member order given, then the fma chain and the division by S of
 *                          recommend_query.  A group of one gets its member's scores, bit for bit
 * formed without a buffer of members x items (device memory: groups of a batch x items, the lists, the member ids).
 * Candidates: cand_items as in recommend_query_within (n_cand strictly ascending ids of the session's catalogue; NULL:
 * the whole catalogue, the items of recommend_add_items included, n_cand ignored), without every item that ANY member
 * has in the session's excluded lists (the training pairs while exclude_train is set, the seen lists of
 * recommend_add_items).  items / scores: n_groups x n, row g holding counts[g] = min(n, candidates left) entries --
 * value descending, equal values (exact fp64 equality) by ascending item id -- followed by item -1 / value -inf
 * (scores and counts may be NULL); a group without members has count 0.  The value of (g, i) depends on g's members
 * and i alone (MEAN: and on their order): bitwise the same wherever g stands in the request, whatever the other groups
 * are, and in swapped and unswapped contexts.  Touches no slot, no EM state and no other session; the recommend session
 * stays open and answers as before.  mmsbm_hip_get_option(ctx, "group_ms") reads the device time of the call's kernels.
 * MIN, MAX and COUNT do not depend on how the member rows are dealt to workgroups (option "group_run_blocks": blocks of
 * 8 member rows per workgroup and item tile, 0 = the library's choice -- time, never the answer).
 * MMSBM_E_INVALID (before any launch): no recommend session or no slot added to it, a bad CSR, an id out of range, a
 * member repeated within a group, an unknown mode, a bar that is not finite in COUNT mode, cand_items not strictly
 * ascending, n < 1.  n > MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory is
 * not free. */
#define MMSBM_HIP_GROUP_MIN 0
#define MMSBM_HIP_GROUP_MAX 1
#define MMSBM_HIP_GROUP_COUNT 2
#define MMSBM_HIP_GROUP_MEAN 3
int mmsbm_hip_recommend_query_groups(mmsbm_hip_ctx *ctx, int64_t n_groups, const int64_t *offsets,
                                     const int32_t *members, int mode, double bar, int32_t n_cand,
                                     const int32_t *cand_items, int32_t n, int32_t *items, double *scores,
                                     int32_t *counts);

/* Greedy assortment selection of the open recommend session (mmsbm_amd/csrc/assortment.hpp): which c items serve a set
 * of users best TOGETHER.  users: n_users ids of training users, strictly ascending.  With a(u, i) the undivided sum of
 * recommend_query's fma chain (score = a / S, bit for bit) and a pair ELIGIBLE unless i is in u's excluded list of the
 * session (the training pairs while exclude_train is set, the seen lists of recommend_add_items), a round's gain of item
 * i is the sum over the users of
 *   MMSBM_HIP_ASSORT_BEST   max(0, a(u, i) - best[u]) on eligible pairs; best[u] starts at level x S (`level`: the
 *                           floor, finite) and rises to a(u, i*) with every item i* taken
 *   MMSBM_HIP_ASSORT_REACH  1.0 where the pair is eligible, u is not covered yet and score(u, i) >= level (`level`: the
 *                           bar, finite, compared with the final score); a taken item covers the users it reaches
 * The given items (n_given ids of the session's catalogue, in the order given) are applied to the state first and are
 * never chosen; then at most c rounds take the candidate (cand_items as in recommend_query_within; NULL: the whole
 * catalogue, n_cand ignored) of largest gain, equal gains by the smaller item id, and stop early when that gain is not
 * > 0 or no candidate is left.  items / gains [c]: the *count items taken in order and each round's gain -- divided by S
 * once in BEST mode, a whole number of users in REACH mode -- followed by -1 / 0.0.  *stop: MMSBM_HIP_ASSORT_STOP_C
 * (count == c), _NO_GAIN or _NO_CANDIDATES.  given_gains [n_given]: each given item's gain over the state before it.
 * served_items / served_scores [n_users]: per user the item that serves them (BEST: the earliest item of their best
 * score; REACH: the item that covered them first) and its score, or -1 / -inf; read from the state on the device.
 * The rounds are enqueued without a host wait between them: a stop flag on the device makes the launches behind it
 * return at once.  REACH depends on nothing but the arguments; BEST sums doubles in an order fixed by the launch plan
 * (the CU count and option "assortment_run_blocks": blocks of 8 user rows per workgroup and item tile, 0 = the library's
 * choice): the same bits from call to call, possibly other last bits under another plan.  Option
 * "assortment_part_bytes" (0 = 64 MB) bounds the runs' partial sums per batch of item tiles -- time, never the answer.
 * Touches no slot, no EM state
 * and no other session.  mmsbm_hip_get_option(ctx, "assortment_ms") reads the device time of the call's kernels; with
 * option "assortment_timing" set, "assortment_gain_ms" / "assortment_pick_ms" / "assortment_update_ms" hold its split.
 * MMSBM_E_INVALID (before any launch): no recommend session or no slot added to it, an id out of range, users or
 * cand_items not strictly ascending, an unknown mode, a level that is not finite, c < 0.  c > MMSBM_HIP_ASSORT_MAX_C:
 * MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory is not free. */
#define MMSBM_HIP_ASSORT_BEST 0
#define MMSBM_HIP_ASSORT_REACH 1
#define MMSBM_HIP_ASSORT_MAX_C 1024
#define MMSBM_HIP_ASSORT_STOP_C 0
#define MMSBM_HIP_ASSORT_STOP_NO_GAIN 1
#define MMSBM_HIP_ASSORT_STOP_NO_CANDIDATES 2
int mmsbm_hip_recommend_assortment(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int mode, double level,
                                   int32_t n_given, const int32_t *given_items, int32_t n_cand,
                                   const int32_t *cand_items, int32_t c, int32_t *items, double *gains, int32_t *count,
                                   int32_t *stop, double *given_gains, int32_t *served_items, double *served_scores);

/* Ensemble-aware queries of the open recommend session (mmsbm_amd/csrc/ensemble.hpp): how far the added slots -- the
 * restarts -- AGREE about a pair.  With x_s / y_s the folded factors the session holds for slot s (add order),
 *   a_s(u, i) = ONE fma chain over j = 0 .. rank - 1 ascending from +0.0 of x_s[u, j] y_s[i, j]
 * -- the bits recommend_query returns as the score in a session that holds slot s alone -- and, per pair, every product
 * and sum rounded on its own (no contraction):
 *   worst = min_s a_s                       best = max_s a_s
 *   d_s = a_s - a_0   (s = 1 .. S - 1)      D = ((+0.0 + d_1) + d_2) + ...     Q = ((+0.0 + d_1 d_1) + d_2 d_2) + ...
 *   mean = a_0 + D / S
 *   var  = max(S Q - D D, +0.0) / (S S)     std = sqrt(var)                    (population form: divide by S)
 *   lcb  = mean - risk std                  (product rounded, then the subtraction)
 * Slots that agree on a pair give std = +0.0 and mean = a_0 exactly; S = 1 gives recommend_query's bits in every mode.
 *
 * query_ensemble: recommend_query_within -- the same candidates (cand_items: n_cand strictly ascending ids of the
 * session's catalogue, the items of recommend_add_items included; NULL: all of it, n_cand ignored), the same exclusions
 * (the session's lists while exclude_train is set, the seen lists of recommend_add_items, and the query's own
 * excl_items[excl_offsets[b] .. excl_offsets[b + 1]) by request row, excl_offsets NULL: none), the same output -- with
 * the value of a pair being, by mode,
 *   MMSBM_HIP_ENSEMBLE_MIN  worst      MMSBM_HIP_ENSEMBLE_MAX  best      MMSBM_HIP_ENSEMBLE_LCB  lcb
 * (`risk` is read by LCB alone: > 0 ranks by a lower confidence bound, 0 by the mean, < 0 explores where the slots
 * disagree).  Order: value descending, equal values (exact fp64 equality) by ascending item id.
 *
 * pair_spread: for n_pairs caller-given pairs (users[e], items[e]) -- ids of training users and of the session's
 * catalogue, any order, repeats allowed -- stats[e * 4 ...] = mean, std, worst, best, and, unless per_slot is NULL,
 * per_slot[s * n_pairs + e] = a_s.  The same chains as query_ensemble's: a returned pair's worst / best / mean - risk std
 * are the query's bits.  No row of scores is formed.
 *
 * A value depends on its pair alone: bitwise the same whatever the other rows of the call, the candidate set, the slots
 * the context holds beyond those added, and in swapped and unswapped contexts.  Both touch no slot, no EM state and no
 * other session; the recommend session stays open and answers as before.  mmsbm_hip_get_option(ctx, "ensemble_ms") reads
 * the device time of the last call's kernels.
 * MMSBM_E_INVALID (before any launch): no recommend session or no slot added to it, an id out of range, cand_items not
 * strictly ascending, a bad CSR, n < 1, an unknown mode, a risk that is not finite in LCB mode.
 * n > MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory is not free. */
#define MMSBM_HIP_ENSEMBLE_MIN 0
#define MMSBM_HIP_ENSEMBLE_MAX 1
#define MMSBM_HIP_ENSEMBLE_LCB 2
int mmsbm_hip_recommend_query_ensemble(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int mode, double risk,
                                       int32_t n_cand, const int32_t *cand_items, const int64_t *excl_offsets,
                                       const int32_t *excl_items, int32_t n, int32_t *items, double *scores,
                                       int32_t *counts);
int mmsbm_hip_recommend_pair_spread(mmsbm_hip_ctx *ctx, int64_t n_pairs, const int32_t *users, const int32_t *items,
                                    double *stats, double *per_slot);

/* ---- the items whose rating tells most about a user: the n largest information gains (mmsbm_amd/csrc/inform.hpp) -- */
/* A session of its own beside the predict, recommend, similar, overlap, explain and held-out sessions (any of them may
 * be open meanwhile):
 *   begin  closes any earlier inform session;
 *   add    the SELECTED slot joins the session (the slot itself is left unchanged), in external terms: its theta rows,
 *          the items' rating profiles q_s[i, k, r] = sum_l eta_s[i, l] p_s[k, l, r] (l ascending), their entropies
 *          h_s[i, k] = sum_r phi(q_s[i, k, r]) (r ascending from +0.0; phi(x) = x > 0 ? -(x log x) : +0.0) and the sums
 *          sum_u theta_s[u, k] (thread t of 256 adds rows t, t + 256, ... ascending from +0.0, then the 256 partial
 *          sums are halved 8 times);
 *   query  for n_users ids of training users (repeats allowed, any order): over the S added slots
 *            gain_s(u, i) = H( sum_k theta_s[u,k] q_s[i,k,.] ) - sum_k theta_s[u,k] h_s[i,k]         (nats)
 *            gain(u, i)   = ( sum_s max(gain_s(u, i), +0.0) ) / S,     0 <= gain <= log min(K, R)
 *          -- the information a rating of item i carries about the group user u acts from -- built as: s ascending; r
 *          ascending, m_r one fma chain over k ascending from +0.0, H += phi(m_r); lin one fma chain over k of
 *          theta h; acc += max(H - lin, +0.0); one division by S.  A one-hot theta row gives exactly +0.0 for every
 *          item.  Per id the n items of largest gain -- gain descending, equal gains (exact fp64 equality) by
 *          ascending item id -- among cand_items (n_cand strictly ascending item ids; NULL: every item, n_cand
 *          ignored), without the user's training items when exclude_train is not 0 and without row b's own list
 *          excl_items[excl_offsets[b] .. excl_offsets[b + 1]) (any order, repeats allowed; excl_offsets NULL: none).
 *          items / gains: n_users x n, row b holding counts[b] entries followed by item -1 / gain -inf (gains and
 *          counts may be NULL).  A row's answer depends on that user and the arguments only: bitwise the same whatever
 *          the other users of the call, the slots the context holds beyond those added, and the side layout;
 *   query_theta  the same for caller-given users: theta[S][n_users][K], one block per added slot in add order, entries
 *          finite and >= 0; seen_offsets / seen_items: the items row b leaves out (NULL: none).  A slot's own theta row
 *          gives the bits query gives for that user;
 *   mean_theta   out[S][K] = ( sum_u theta_s[u, k] ) / U of the added slots: the membership of a user about whom
 *          nothing is known;
 *   end    releases the session's device memory (so does mmsbm_hip_destroy).
 * mmsbm_hip_get_option(ctx, "inform_ms") reads the device time of the last query's kernels (HIP events).
 * MMSBM_E_INVALID (before any launch): add, query, query_theta or mean_theta without begin; query, query_theta or
 * mean_theta before the first add; an id out of range; cand_items not strictly ascending; a bad CSR; n < 1; a theta
 * entry that is NaN, infinite or negative.  n > MMSBM_HIP_RECOMMEND_MAX_N: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where
 * the device memory of the slots' tables ((U K + I K (R + 1)) doubles per slot) or of a batch is not free.  Touches no
 * slot, no EM state and no other session. */
int mmsbm_hip_inform_begin(mmsbm_hip_ctx *ctx);
int mmsbm_hip_inform_add(mmsbm_hip_ctx *ctx);
int mmsbm_hip_inform_query(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                           const int32_t *cand_items, const int64_t *excl_offsets, const int32_t *excl_items,
                           int exclude_train, int32_t n, int32_t *items, double *gains, int32_t *counts);
int mmsbm_hip_inform_query_theta(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                                 const int32_t *seen_items, int32_t n_cand, const int32_t *cand_items, int32_t n,
                                 int32_t *items, double *gains, int32_t *counts);
int mmsbm_hip_inform_mean_theta(mmsbm_hip_ctx *ctx, double *out);
int mmsbm_hip_inform_end(mmsbm_hip_ctx *ctx);

/* ---- the overlap of the restarts' groups: the Gram matrix of the membership tables (mmsbm_amd/csrc/overlap.hpp) ---- */
/* A session of its own beside the predict, recommend, similar and held-out sessions (any of them may be open meanwhile):
 *   begin  side 0: items (eta, G = L groups), 1: users (theta, G = K groups); external sides.  Closes any earlier
 *          overlap session;
 *   add    the SELECTED slot's table of that side joins the session as slot s = the number of adds so far, copied in
 *          external terms (the caller's rows and the caller's group order; the slot itself is left unchanged);
 *   query  over the S added slots, F = S G: out is F x F doubles, row-major,
 *          out[(s G + a) F + (t G + b)] = sum_row x_s[row, a] x_t[row, b]
 *          -- how much of the population group a of slot s and group b of slot t share;
 *   end    releases the session's device memory (so does mmsbm_hip_destroy).
 * Operation order: the rows are cut into slabs of a fixed length (2,048); inside a slab an output is one fma chain over
 * the rows in ascending order from +0.0; the slabs' partial results are combined in a fixed pairwise tree in slab order;
 * no atomics.  An output depends on its two columns and on the number of rows only, bit for bit: not on S, on the
 * other slots, on the launch shape, on the side layout or on slots the context holds beyond those added; out[a][b] and
 * out[b][a] are the same bits.
 * mmsbm_hip_get_option(ctx, "overlap_ms") reads the device time of the last query's kernels (HIP events).
 * MMSBM_E_INVALID: side not 0 / 1, add or query without begin, query before the first add, a selected slot without
 * parameters, out == NULL; MMSBM_E_TOOLARGE where the device memory of the session tables (rows x G doubles per slot),
 * of the slabs' partial results or of the F x F result is not free.  Touches no slot, no EM state and no other session;
 * set_slots keeps the session's tables. */
int mmsbm_hip_overlap_begin(mmsbm_hip_ctx *ctx, int side);
int mmsbm_hip_overlap_add(mmsbm_hip_ctx *ctx);
int mmsbm_hip_overlap_query(mmsbm_hip_ctx *ctx, double *out);
int mmsbm_hip_overlap_end(mmsbm_hip_ctx *ctx);

/* ---- why a recommendation: which of a user's training rows carry it (mmsbm_amd/csrc/explain.hpp) ------------------- */
/* With eta and p fixed, the theta half of the M-step is an average over the user's training rows j = (u, i_j, r_j):
 *   v_j[k] = sum_l p[k, l, r_j] eta[i_j, l],  c_j[k] = theta_u[k] v_j[k] / max(theta_u . v_j, eps),
 *   theta'_u[k] = (1/d_u) sum_j c_j[k],
 * and score_w(u, t) = sum_k theta_u[k] g_t[k] with g_t[k] = sum_l W[k, l] eta[t, l] is linear in theta.  So
 *   a(u, t, j) = (1/d_u) sum_k c_j[k] g_t[k]
 * is the part of the recommendation of t to u that training row j carries: over ALL rows of u the a add up to the score
 * under one more theta update, which is score_w(u, t) itself at a fixed point of EM; d_u a(u, t, j) is the score u
 * would have for t if judged from row j alone.  Over the S added slots a is the mean of the slots' a, as the score is.
 * A session of its own beside the other five (any of them may be open meanwhile):
 *   begin  the R rating weights (finite), and the training rows of every external user in the order they were given to
 *          mmsbm_hip_create (duplicate triples are separate rows).  Closes any earlier explain session;
 *   add    the SELECTED slot joins: external copies of its theta, G = eta W^T, p and eta (the slot is left unchanged);
 *   query  occurrence b of the request is user users[b] with the candidate items items[offsets[b] .. offsets[b + 1])
 *          (training item ids, any order, repeats allowed; a user may appear more than once; offsets ascending from 0).
 *          Pair q, counted in that flattened order, gets row q of hist_items / hist_ratings / contribution (n entries
 *          each): the counts[q] = min(n, d_u) rows of u with the largest a(u, t, j), as (item, rating id, a), followed
 *          by -1 / -1 / -inf; order: a descending, exactly equal a (fp64 equality) by ascending history item id, then
 *          ascending rating id.  explained[q] = the sum of a over all d_u rows, score[q] = score_w(u, t), degree[q] =
 *          d_u.  Every output except hist_items may be NULL;
 *   end    releases the session's device memory (so does mmsbm_hip_destroy).
 * Operation order: v one fma chain over l ascending from +0.0 (fold-in's); theta . v one fma chain over k ascending;
 * one division 1 / max(dot, eps), c[k] = (theta[k] v[k]) times it; per row ONE fma chain over f = s K + k ascending of
 * c_s[k] G_s[t, k], divided once by the product S d_u formed in double; explained: row j is added to partial sum j mod
 * 64 in ascending row order and the 64 partial sums are added by the butterfly 1, 2, 4 ... 32 (a tree fixed by d_u
 * alone); score: one fma chain over f of theta_s[u, k] G_s[t, k], divided by S -- bit for bit recommend_query's score
 * where K <= L, equal up to rounding where K > L (recommend folds W into theta there).  No atomics.  A pair's answer
 * depends on its user, its item and the added slots only, bit for bit: not on the other pairs of the call, on the
 * batches, on the side layout or on slots the context holds beyond those added.  The c rows (S K doubles per training
 * row) exist per batch of requested users only: option "explain_rows" (training rows per batch, 0: the library's choice;
 * a user with more rows is a batch of its own) changes time and memory, never the answer.  "explain_ms" reads the device
 * time of the last query's kernels (HIP events).
 * MMSBM_E_INVALID: add or query without begin, query before the first add, a selected slot without parameters, an id
 * out of range, offsets not ascending from 0, n < 1, a non-finite weight, a null pointer where one is needed; n >
 * MMSBM_HIP_RECOMMEND_MAX_N or K > MMSBM_HIP_FOLD_IN_MAX_K: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device
 * memory of the session's tables or of a batch is not free.  Touches no slot, no EM state and no other session. */
int mmsbm_hip_explain_begin(mmsbm_hip_ctx *ctx, const double *rating_weights);
int mmsbm_hip_explain_add(mmsbm_hip_ctx *ctx);
int mmsbm_hip_explain_query(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, const int64_t *offsets,
                            const int32_t *items, int32_t n, int32_t *hist_items, int32_t *hist_ratings,
                            double *contribution, int32_t *counts, double *explained, double *score, int32_t *degree);
int mmsbm_hip_explain_end(mmsbm_hip_ctx *ctx);

/* ---- which training rows look wrong: leave-one-out reliability (mmsbm_amd/csrc/loo.hpp) ---------------------------- */
/* The probability of every training row under parameters that never saw it.  The M-step writes theta_u as the average
 * of its rows' shares (the identity explain rests on) and eta_i likewise, so one EM step without row j is a downdate
 * of two sums.  Per added slot, in EXTERNAL k, l, r, for training row j = (u, i, r) with that slot's theta, eta, p:
 *   v_j[k] = sum_l p[k,l,r] eta[i,l]         one fma chain over l ascending from +0.0 (fold-in's v)
 *   w_j[l] = sum_k p[k,l,r] theta[u,k]       one fma chain over k ascending from +0.0
 *   fit_j  = sum_k theta[u,k] v_j[k]         one fma chain over k ascending from +0.0 (the in-sample probability: the
 *                                            P_s(m) of mmsbm_hip_heldout_add, bit for bit)
 *   inv    = 1 / max(fit_j, eps)             ONE division, eps = DBL_EPSILON
 *   c_j[k] = (theta[u,k] v_j[k]) inv         e_j[l] = (eta[i,l] w_j[l]) inv
 *   C_u = sum_{j in u} c_j    E_i = sum_{j in i} e_j    (the n_theta / n_eta of mmsbm_hip_update_coefficients)
 *   theta-[k] = max(C_u[k] - c_j[k], 0) / (d_u - 1);  d_u = 1: theta-bar[k], the mean theta row over the U users
 *   eta-[l]   = max(E_i[l] - e_j[l], 0) / (d_i - 1);  d_i = 1: eta-bar[l], the mean eta row over the I items
 *   rel_j = sum_k theta-[k] (sum_l p[k,l,r] eta-[l])  inner fma chain over l, outer fma chain over k, from +0.0
 * p stays the fitted p on purpose: a row is one of d_u rows of its user but one of very many soft counts of a block,
 * and (n - omega) / (N - omega) is ill-conditioned for a block that only this row supports.  Over the S added slots
 * reliability_j = (sum_s rel_{s,j}) / S and fitted_j = (sum_s fit_{s,j}) / S (slots added ascending from +0.0, one
 * division), surprise_j = -log(max(reliability_j, eps)); a user's (item's) surprise is the mean of surprise_j over its
 * rows, fitted_surprise the same built from fitted_j.
 * Order of every sum over the rows of a user (item): rows in ascending position in the training table, cut into chunks
 * of 64; a chunk's rows added one after the other from +0.0, then the chunk sums one after the other from +0.0 (the
 * means: then one division by d) -- a tree fixed by d alone; theta-bar / eta-bar: thread t of 256 adds rows t, t + 256,
 * ... from +0.0, the 256 sums are halved 8 times, one division.  No atomics.  Every number depends on its row, its
 * user's rows, its item's rows and the added slots only, bit for bit: not on the other rows asked for, on the side
 * layout or on slots the context holds beyond those added.
 * A session of its own beside the others (any of them may be open meanwhile):
 *   begin   the training table as given to mmsbm_hip_create (duplicate triples are separate rows) by user and by item.
 *           Closes any earlier loo session;
 *   add     the SELECTED slot joins: its C and E are formed, then rel and fit of every row are added to the rows'
 *           running sums (the slot is left unchanged).  Nothing of size n_obs x K exists at any time: device memory of
 *           a session is O(U K + I L + n_obs);
 *   rows    fitted and reliability (either may be NULL) at the n_rows positions rows[] of the training table, or of
 *           every row in training order when rows == NULL (n_rows is then ignored; n_obs doubles each);
 *   sides   U (I) doubles each, any may be NULL: the users' (items') surprise and fitted_surprise; NaN without rows;
 *   lowest  the m rows of smallest reliability among the rows whose user is flagged in user_flags (U bytes, non-zero =
 *           flagged; NULL: every user) AND whose item is flagged in item_flags (I bytes; NULL: every item): rows[] and
 *           reliability[] (m entries each), reliability ascending, exactly equal doubles by ascending position; *count
 *           (may be NULL) = how many there are, the rest is (-1, +inf);
 *   end     releases the session's device memory (so does mmsbm_hip_destroy).
 * mmsbm_hip_get_option(ctx, "loo_ms") reads the device time of the last add's or query's kernels (HIP events),
 * "loo_sums_ms" / "loo_rows_ms" those of the last add's sums pass and row pass.
 * MMSBM_E_INVALID: add or query without begin, a query before the first add, a selected slot without parameters, m < 1
 * or m > MMSBM_HIP_LOO_MAX_M, a row position outside [0, n_obs), a null pointer where one is needed; K or L >
 * MMSBM_HIP_FOLD_IN_MAX_K: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory of the session or of a query
 * is not free.  Touches no slot, no EM state and no other session; set_slots keeps the session's sums. */
#define MMSBM_HIP_LOO_MAX_M 1024
int mmsbm_hip_loo_begin(mmsbm_hip_ctx *ctx);
int mmsbm_hip_loo_add(mmsbm_hip_ctx *ctx);
int mmsbm_hip_loo_rows(mmsbm_hip_ctx *ctx, int64_t n_rows, const int64_t *rows, double *fitted, double *reliability);
int mmsbm_hip_loo_sides(mmsbm_hip_ctx *ctx, double *user_surprise, double *user_fitted_surprise,
                        double *item_surprise, double *item_fitted_surprise);
int mmsbm_hip_loo_lowest(mmsbm_hip_ctx *ctx, int32_t m, const uint8_t *user_flags, const uint8_t *item_flags,
                         int64_t *rows, double *reliability, int32_t *count);
int mmsbm_hip_loo_end(mmsbm_hip_ctx *ctx);

/* ---- held-out log-likelihood of every restart slot, and parameter snapshots (mmsbm_amd/csrc/heldout.hpp) ------------ */
/* For a row m = (u, i, r) (external ids) and the parameters of slot s:
 *   t_s[k] = sum_l p_s[k, l, r] eta_s[i, l]     one fma chain over l ascending, from +0.0
 *   P_s(m) = sum_k theta_s[u, k] t_s[k]         one fma chain over k ascending, from +0.0
 *   ll_s   = sum_m log(max(P_s(m), eps))        eps = DBL_EPSILON, the clamp of mmsbm_hip_likelihood
 * -- the predictive log-likelihood of rows the fit has not seen, not the omega form of mmsbm_hip_likelihood.  A session
 * of its own beside the predict, recommend and similar sessions (any of them may be open meanwhile):
 *   begin  n_rows rows, ids as in create(); the rows are ordered by rating once and stay on the device.  Closes any
 *          earlier held-out session -- once its own arguments are accepted: a refused begin (an id out of range,
 *          n_rows >= 2^31) changes nothing and an earlier session stays open.  n_rows == 0 is valid (every ll is 0.0);
 *   eval   loglik[s] = ll_s of the CURRENT parameters of EVERY slot s < n_slots, in one set of launches (two, whatever
 *          the number of slots).  Changes nothing: the monitor of a fit, called between two mmsbm_hip_em_iterate;
 *   add    the SELECTED slot: *loglik = ll_s, and P_s(m) is added to the running per-row sum (in call order);
 *   mean   over the S adds so far: mean_p[m] = (sum_s P_s(m)) / S -- one division --, n_rows doubles in REQUEST order
 *          (may be NULL), and *loglik = sum_m log(max(mean_p[m], eps)): the log-likelihood of the ensemble predict uses;
 *   end    releases the session's device memory (so does mmsbm_hip_destroy).
 * P_s(m) depends on that row's theta row, eta row and p_r only, bit for bit: not on the other rows, the number of
 * slots, which slot, the launch shape or the side layout.  The sum over the rows runs in an order fixed by the
 * session's rows alone (blocks of 256 rows of one rating, a fixed tree inside a block and over the blocks, no atomics):
 * ll_s is bitwise the same from call to call and from slot count to slot count.
 * mmsbm_hip_get_option(ctx, "heldout_ms") reads the device time of the last eval or add: HIP events around its two launches,
 * without the copy of the results.  MMSBM_E_INVALID: no session open, an id or rating out of range, a slot without parameters (eval: any slot; add: the
 * selected one), mean before any add; n_rows >= 2^31: MMSBM_E_UNSUPPORTED; MMSBM_E_TOOLARGE where the device memory of
 * the session is not free.  Touches no slot, no EM state and no other session; set_slots keeps the session's rows. */
int mmsbm_hip_heldout_begin(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user, const int32_t *item,
                            const int32_t *rating);
int mmsbm_hip_heldout_eval(mmsbm_hip_ctx *ctx, double *loglik);
int mmsbm_hip_heldout_add(mmsbm_hip_ctx *ctx, double *loglik);
int mmsbm_hip_heldout_mean(mmsbm_hip_ctx *ctx, double *mean_p, double *loglik);
int mmsbm_hip_heldout_end(mmsbm_hip_ctx *ctx);
/* A slot's best parameters so far, kept on the device: save copies the SELECTED slot's current theta, eta and p into
 * that slot's snapshot (device to device, enqueued on the context's stream, no wait; a later save replaces it); get
 * returns the selected slot's snapshot as mmsbm_hip_get_params returns parameters (any output may be NULL).  The first
 * save allocates room for every slot (MMSBM_E_TOOLARGE where it is not free); set_slots drops all snapshots.
 * MMSBM_E_INVALID: save on a slot without parameters, get with nothing saved for the selected slot. */
int mmsbm_hip_snapshot_save(mmsbm_hip_ctx *ctx);
int mmsbm_hip_snapshot_get(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr);

/* ---- fold-in: theta of new users under the fitted eta and p (mmsbm_amd/csrc/fold_in.hpp) ----------------------- */
/* The SELECTED slot's eta and p stay fixed; for new users 0 .. n_new-1, given their rows (user in [0, n_new), item in
 * [0, I), rating in [0, R), external ids), n_iters times
 *   theta'_u[k] = (1/d_u) sum_{rows j of u} theta_u[k] v_j[k] / max(theta_u . v_j, eps),
 *   v_j[k] = sum_l p[k, l, r_j] eta[i_j, l]
 * -- the theta half of the M-step.  theta0 (n_new x K) may be NULL: uniform 1/K.  tol > 0: a user stops after the
 * first iteration whose max_k |theta' - theta| <= tol; tol <= 0: all n_iters.  theta: n_new x K out; iters (may be
 * NULL): the iterations each user ran.  A user without rows gets theta0 and 0 iterations.  A user's rows are taken in
 * request order; its theta depends on its own rows only (bitwise, whatever the other users of the call).  Touches no
 * slot, no EM state and no predict / recommend session.  K <= MMSBM_HIP_FOLD_IN_MAX_K (larger: MMSBM_E_UNSUPPORTED);
 * MMSBM_E_TOOLARGE where the device memory a batch of users needs is not free.
 * mmsbm_hip_get_option(ctx, "fold_in_ms") reads the device time of the last fold-in's kernels (HIP events). */
#define MMSBM_HIP_FOLD_IN_MAX_K 1024
int mmsbm_hip_fold_in(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user, const int32_t *item,
                      const int32_t *rating, int32_t n_new, int32_t n_iters, double tol,
                      const double *theta0, double *theta, int32_t *iters);
/* The same for new ITEMS: the SELECTED slot's theta and p stay fixed; for new items 0 .. n_new-1, given their rows
 * (user in [0, U), item in [0, n_new), rating in [0, R), external ids), n_iters times
 *   eta'_i[l] = (1/d_i) sum_{rows j of i} eta_i[l] v_j[l] / max(eta_i . v_j, eps),
 *   v_j[l]    = sum_k p[k, l, r_j] theta[u_j, k]                                  (k ascending)
 * -- the eta half of the M-step.  eta0 (n_new x L) may be NULL: uniform 1/L.  tol, iters, rows without an item, request
 * order and independence, side effects, MMSBM_E_TOOLARGE and "fold_in_ms" as mmsbm_hip_fold_in;
 * L <= MMSBM_HIP_FOLD_IN_MAX_K (larger: MMSBM_E_UNSUPPORTED).  Bitwise equal to mmsbm_hip_fold_in on a context over
 * the transposed problem (users and items exchanged, theta and eta exchanged, p transposed in (k, l)). */
int mmsbm_hip_fold_in_items(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user, const int32_t *item,
                            const int32_t *rating, int32_t n_new, int32_t n_iters, double tol,
                            const double *eta0, double *eta, int32_t *iters);

/* ---- measurement ------------------------------------------------------------------ */
/* Runs n_iters EM iterations bracketed by HIP events on the context's stream; returns
 * the elapsed device time of the whole region in milliseconds (synchronises). */
int mmsbm_hip_time_iterations(mmsbm_hip_ctx *ctx, int n_iters, float *elapsed_ms);
/* Number of kernel launches in one EM iteration and their names. */
int mmsbm_hip_kernel_count(void);
const char *mmsbm_hip_kernel_name(int index);
/* Runs n_iters iterations with a HIP event pair around EVERY kernel launch (on the
 * context's stream) and returns the mean duration per launch, in microseconds, for each
 * of the mmsbm_hip_kernel_count() kernels, plus launches per iteration. */
int mmsbm_hip_profile_iterations(mmsbm_hip_ctx *ctx, int n_iters, float *mean_us,
                                 int *launches_per_iter);
/* Algorithmic bytes (read, written) of kernel `index` for this context's shapes; the
 * accounting is stated in DESIGN.md. */
int mmsbm_hip_kernel_bytes(const mmsbm_hip_ctx *ctx, int index, int64_t *bytes_read,
                           int64_t *bytes_written);
/* Tuning aid: launches ONE stage of the iteration (index as in mmsbm_hip_kernel_name) `reps`
 * times back to back on the context's stream and returns the mean time per launch.  The
 * stage's outputs overwrite scratch/next buffers: call set_params again before trusting the
 * context's state. */
int mmsbm_hip_time_stage(mmsbm_hip_ctx *ctx, int stage, int reps, float *mean_us);
/* The library chooses its kernels from the shape and the data; these few switches exist because the tests compare
 * forms with each other (none is needed for normal use, and nothing that was measured and rejected is kept behind a
 * switch -- EXPERIMENTS.md has those): "graph" 0/1 (the same switch as mmsbm_hip_set_graph_mode), "fused" 0/1 (two
 * launches per iteration instead of four: small problems; 1 is refused where the form does not exist), "mfma" 0/1/2
 * (the pair stage on the matrix cores, v_mfma_f64_16x16x4_f64: 0 the vector-ALU form, 1 on -- the one-block kernel for
 * K, L <= 64, else the blocked kernels --, 2 the blocked kernels whatever the shape; create() turns it on for
 * K x L > 1024; environment MMSBM_HIP_NO_MFMA=1 keeps it off), "quad" 0/1 (vector-ALU form of long rows: the A launch
 * as a persistent four-unit pipeline), "lik_fast" 0/1/2 (likelihood: a logarithm per element / logarithm tables, a
 * group of lanes per triple / 2 = the default: a wave per pair or a lane per triple where those apply), "lik_g"
 * 0/1/2/4/8 (lanes per triple of the table form, 0 = automatic), "predict_fast" 0/1 (prod_dist / predict through the
 * table of p_r eta_i over every (item, rating) combination -- the default where the rows are not far fewer than the
 * items -- or through the one-thread-per-row kernels), "nt_out" 0..15 (bits: non-temporal stores of the T / A rows,
 * of the theta' rows, non-temporal loads of the segments' own rows; 8: whatever the data; results are bitwise the same),
 * "a_units" 0..16 (matrix-core pair stage only: 64-pair units per workgroup of the A launch, which writes rows only and
 * so walks the units in runs of its own length; 0 = the library's choice -- the length that fills its last round of
 * workgroups; the rows are bitwise the same for every value), "pass_dense" -1/0/1 (big problems of small tiles: the
 * two triple passes and the T + S stage of a committed iteration in one launch, the C rows kept in LDS -- three launches
 * per iteration; -1 the library's choice by size, 0 off, 1 on wherever the form applies: one restart slot per launch, K
 * of 17..32, L <= 24, no work lists; results are bitwise the same). */
int mmsbm_hip_set_option(mmsbm_hip_ctx *ctx, const char *name, double value);
/* Reads a switch back ("pass_dense" reads 1 when the next committed iteration takes that form, else 0); also the
 * read-only "launches" -- the FAMILY of forms the next iteration takes, not a count: 2 = the two launches of small
 * problems, 4 = the separate stages, with or without "pass_dense"; a committed iteration really takes
 * launches - pass_dense launches --, "ranges_pairs" / "ranges_users" (ranges the XCD-local work
 * list of that pass uses, 1 = off), "items_pairs" / "items_users" (work items, 0 = segments as
 * they are), "splits_pairs" / "splits_users" (segments cut into pieces), "fused_split" (bit 0 / 1: whole-segment lists of
 * the two-launch form built for the pair / user side), "item_grid" (1: at least half of the (item, rating) combinations
 * occur and R <= 16, so the item sums walk a fixed-width grid of pair ids; 0: the items' pair lists), "gpu_layout" (1: the
 * index's sorts ran on the device -- 100,000 triples and more, or MMSBM_HIP_GPU_LAYOUT=1, and ratings x items below 2^31 --, 0: on the host), "chunk_pairs" (pairs per pair-stage workgroup at most), "n_chunks"
 * (pair-stage workgroups = slabs, padding included), "a_chunks" (workgroups of the matrix-core A launch when it walks
 * runs of its own; 0: the T + S launch's list serves) and "wide" (1: K, L beyond the 64-pair LDS stage -- the vector form of the pair stage is then the plain
 * wide-row kernels; they run when "mfma" reads 0, the blocked matrix-core kernels when it reads 2). */
int mmsbm_hip_get_option(const mmsbm_hip_ctx *ctx, const char *name, double *value);
/* How em_iterate launches: 0 (default) = eager launches on the context's stream; 1 = replay
 * a captured hipGraph of two iterations. */
int mmsbm_hip_set_graph_mode(mmsbm_hip_ctx *ctx, int enabled);

/* ---- host-only helpers (no device needed) ------------------------------------------- */
/* The sorted CSR-style layout create() uploads, exposed so it can be checked on a
 * machine without a GPU.  which: 0 pair_off, 1 pair_user, 2 pair_item, 3 rating_off,
 * 4 user_off, 5 user_pair, 6 item_off, 7 item_pairs, 8 item_deg, 9 chunk_off,
 * and arrays of 4-int records: 10 chunks and 11 mv_chunks (rating, q_begin, q_end, 0),
 * 12 / 13 work items of the pair / user segments (segment, begin, end, partial slot or -1;
 * empty when no segment is longer than 64 triples), 14 / 15 split segments (segment, first
 * partial slot, pieces, 0).  Pass out == NULL to query count. */
typedef struct mmsbm_hip_layout mmsbm_hip_layout;
int mmsbm_hip_layout_build(int64_t n_obs, int32_t n_users, int32_t n_items,
                           int32_t n_ratings, const int32_t *user, const int32_t *item,
                           const int32_t *rating, int32_t target_chunks,
                           mmsbm_hip_layout **out);
int mmsbm_hip_layout_array(const mmsbm_hip_layout *layout, int which, int32_t *out,
                           int64_t capacity, int64_t *count);
int mmsbm_hip_layout_free(mmsbm_hip_layout *layout);
/* Small problems with uneven degrees (the two-launch iteration): the lists that give every workgroup WHOLE segments
 * -- all pieces of a cut segment -- so that their partial rows are added up in its LDS instead of in a combine
 * launch.  side 0: pair segments, the 64-pair units rebuilt with at most cap_items work items each; side 1: user
 * segments, workgroups of at most cap_items items (a longer segment gets a workgroup of its own).  which: 0 units
 * (items begin, end, splits begin, end), 1 work items in (segment, piece) order (segment, begin, end, workgroup-local
 * partial row or -1), 2 split segments (segment, first local partial row, pieces, 1 = combined in the strided order
 * seg_combine_both_kernel adds splits of many pieces in), 3 the rebuilt unit list as (rating, q_begin, q_end, 0)
 * (side 0), 4 { most partial rows a workgroup holds, 1 if the lists could be built }.  Pass out == NULL to query count. */
int mmsbm_hip_layout_fused(const mmsbm_hip_layout *layout, int side, int32_t cap_items, int which, int32_t *out,
                           int64_t capacity, int64_t *count);
/* No exception ever crosses this ABI: every entry point runs inside one handler that turns whatever is thrown
 * -- the library's own errors, std::exception, std::bad_alloc, and anything else -- into a status code and a
 * message for mmsbm_hip_last_error().  This entry throws on purpose from inside that handler so the rule can be
 * tested without a GPU: kind 0 nothing (returns MMSBM_OK), 1 std::invalid_argument (MMSBM_E_INVALID), 2
 * std::runtime_error, 3 std::bad_alloc, 4 an int, 5 a class not derived from std::exception (all four:
 * MMSBM_E_INTERNAL). */
int mmsbm_hip_selftest_throw(int kind);

#ifdef __cplusplus
}
#endif
#endif /* MMSBM_HIP_H */
