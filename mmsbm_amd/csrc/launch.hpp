// launch.hpp -- what every launching translation unit shares: the launch macros (with the optional launch log), views of
// the context's tables, and the stage entry points that live in other translation units
// Included by every translation unit of the library (prelude.hpp), after context.hpp.
#pragma once

// ---- stage entry points: each is defined in the translation unit that holds its kernels ----------------------------
namespace mmsbm_hip_impl {

// tu_seg.hip -- the two triple passes.  with_pairs / with_users select the segment sets of this launch (both: one
// launch, the pair segments' workgroups first); `st` is the stream it goes to.
void stage_seg(mmsbm_hip_ctx *c, bool commit, bool with_pairs, bool with_users, hipStream_t st);
// tu_pair.hip (vector ALUs) / tu_mfma.hip (matrix cores) -- T = P^T C and the K x L slabs for p
void stage_dense_valu(mmsbm_hip_ctx *c);
void stage_dense_mfma(mmsbm_hip_ctx *c);
// ... and A[q,:] from (eta, pT) of parameter buffer `slot` into atab[a_slot] -- or, with `grid` set, the same mat-vec
// over every (item, rating) combination into the plain table btab (prod_dist / predict)
void stage_matvec_a_valu(mmsbm_hip_ctx *c, int slot, int a_slot, bool grid);
void stage_matvec_a_mfma(mmsbm_hip_ctx *c, int slot, int a_slot, bool grid);
int mfma_a_blocks_per_cu(const mmsbm_hip_ctx *c);  // workgroups of the matrix-core A launch a CU holds (occupancy query)
// tu_etap.hip -- eta_new ; p_new, pT_new, raw n_p
void stage_eta_p(mmsbm_hip_ctx *c, bool commit);
// tu_fused.hip -- small problems: the iteration in two launches
void stage_fused_pairs(mmsbm_hip_ctx *c);
void stage_fused_tail(mmsbm_hip_ctx *c, bool commit);
// ... and the two triple passes with the T + S stage of a committed iteration in one launch (pass_dense.hpp)
void stage_pass_dense(mmsbm_hip_ctx *c);
// tu_once.hip -- once-per-run kernels, with the host side of the entries that run them.  likelihood of the selected slot
// (the caller holds a OneSlot): likelihood_enqueue puts the kernels onto the context's stream without waiting and returns
// the number of partial sums in lik_part; likelihood_finish fetches them and adds them up in workgroup order
int likelihood_enqueue(mmsbm_hip_ctx *c);
double likelihood_finish(mmsbm_hip_ctx *c, int n_parts);
void init_rows_launch(mmsbm_hip_ctx *c, const uint64_t pcg64_state[4]);
// ... the selected slot (the caller holds a OneSlot), arguments checked: omega[n,k,l] in the caller's orientation;
// P[m, r] of n_pairs (user, item) rows; the predict session of mmsbm_hip_predict_* (stats: the six sums of the slot
// just added / of the mean; mean_dist: null or [rows][R])
void compute_omegas(mmsbm_hip_ctx *c, double *out, int64_t n_elems);
void prod_dist(mmsbm_hip_ctx *c, int64_t n_pairs, const int32_t *user, const int32_t *item, double *out);
void predict_begin(mmsbm_hip_ctx *c, int64_t n_rows, const int32_t *user, const int32_t *item, const int32_t *rating,
                   const double *rating_weights);
void predict_add(mmsbm_hip_ctx *c, double *stats);
void predict_finish(mmsbm_hip_ctx *c, double *mean_dist, double *stats);

// tu_serve_frame.hip -- the out-of-line half of the serving frame (serve_frame.hpp declares the rest of it); of use
// beyond the serving units:
// MMSBM_E_TOOLARGE "<what> needs ... MB of device memory" unless `bytes` (plus 64 MB) are free (fold-in too)
void require_free_mem(size_t bytes, const std::string &what);
// the training rows' external ids in the order they were given, with their ratings on request (null: not wanted)
void train_id_columns(mmsbm_hip_ctx *c, std::vector<int32_t> &user, std::vector<int32_t> &item,
                      std::vector<int32_t> *rating);
// The serving entry points take a request as the values of abi_request.hpp -- UserQuery (users, candidate subset, the
// query's own excluded items by request row), ThetaQuery (caller-given theta rows, their seen lists, the subset), Subset,
// RowCsr, Categories -- and write to its output values (TopNOut, ShelfOut, AssignOut); arguments checked.
// tu_recommend.hip -- top-N recommendation (recommend.hpp): the session of mmsbm_hip_recommend_*
void recommend_begin(mmsbm_hip_ctx *c, const double *weights, int exclude_train);
void recommend_add(mmsbm_hip_ctx *c);  // the selected slot (the caller holds a OneSlot)
void recommend_query(mmsbm_hip_ctx *c, const UserRows &users, int n, const TopNOut &out);
void recommend_positions(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int64_t *offsets,
                         const int32_t *items, int32_t *positions, int32_t *candidates);
void recommend_add_items(mmsbm_hip_ctx *c, int32_t n_new, const double *eta, const int64_t *seen_off,
                         const int32_t *seen_users);
// ... queries within a part of the catalogue (catalogue.hpp); without a subset and lists: the whole catalogue;
// recommend_rank: one ascending, distinct candidate list per request row
void recommend_query_within(mmsbm_hip_ctx *c, const UserQuery &q, int n, const TopNOut &out);
void recommend_query_theta(mmsbm_hip_ctx *c, const ThetaQuery &q, int n, const TopNOut &out);
void recommend_rank(mmsbm_hip_ctx *c, const UserRows &users, const RowCsr &lists, int n, const TopNOut &out);
// ... the same two queries with capped categories (quota.hpp): at most caps[g] items of category g enter a row's list
void recommend_query_quota(mmsbm_hip_ctx *c, const UserQuery &q, const Categories &cats, int n, const TopNOut &out);
void recommend_query_theta_quota(mmsbm_hip_ctx *c, const ThetaQuery &q, const Categories &cats, int n, const TopNOut &out);
// ... category-level recommendation (shelves.hpp): the categories as the quota queries' (no caps)
void recommend_query_shelves(mmsbm_hip_ctx *c, const UserQuery &q, const Categories &cats, const ShelfAsk &ask,
                             const ShelfOut &out);
void recommend_query_theta_shelves(mmsbm_hip_ctx *c, const ThetaQuery &q, const Categories &cats, const ShelfAsk &ask,
                                   const ShelfOut &out);
// tu_rerank.hip -- the queries of the recommend session that add a stage of their own to the frame.  Randomised top-N
// with propensities (explore.hpp): a temperature above the session's floor and the four words of a PCG64 stream; the
// propensities of caller-given lists (distinct items per row); r and g of given (user, item) pairs, no session needed
void recommend_query_explore(mmsbm_hip_ctx *c, const UserQuery &q, int n, double temperature, const uint64_t pcg64_state[4],
                             const TopNOut &out, double *propensity);
void recommend_list_propensity(mmsbm_hip_ctx *c, const UserQuery &q, double temperature, const RowCsr &lists, double *scores,
                               double *propensity);
void explore_noise(mmsbm_hip_ctx *c, const uint64_t pcg64_state[4], int64_t n_pairs, const int32_t *users,
                   const int32_t *items, double *r, double *g);
// ... and the ensemble-aware queries (ensemble.hpp): mode: MMSBM_HIP_ENSEMBLE_*; stats [n_pairs][4], per_slot
// [S][n_pairs] or null
void recommend_query_ensemble(mmsbm_hip_ctx *c, const UserQuery &q, int mode, double risk, int n, const TopNOut &out);
void recommend_pair_spread(mmsbm_hip_ctx *c, int64_t n_pairs, const int32_t *users, const int32_t *items, double *stats,
                           double *per_slot);
// ... and the group queries (group.hpp): one row of distinct members per group; mode: MMSBM_HIP_GROUP_*
void recommend_query_groups(mmsbm_hip_ctx *c, int64_t n_groups, const RowCsr &members, int mode, double bar,
                            const Subset &cand, int n, const TopNOut &out);
// ... and the two queries of diverse.hpp: the distance of given pairs of the similarity session's side, and the
// diversified top-N, which reads the recommend session and the similarity session (side items)
void similar_pairs(mmsbm_hip_ctx *c, int64_t n_pairs, const int32_t *a, const int32_t *b, double *distance);
void recommend_diverse(mmsbm_hip_ctx *c, const UserQuery &q, int n, int pool, double trade_off, const TopNOut &out,
                       double *distances);
// tu_pairs.hip -- the m best pairs of the whole model (top_pairs.hpp): users ascending and distinct
void recommend_top_pairs(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int m, int32_t *out_users,
                         int32_t *out_items, double *out_scores, int32_t *count);
// ... the same question for m up to MMSBM_HIP_TOP_PAIRS_BULK_MAX_M (pairs_bulk.hpp): users ascending and distinct;
// out_* null: the bar and the counts alone; counts: above the bar, at the bar, candidates
void recommend_top_pairs_bulk(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int64_t m, int32_t *out_users,
                              int32_t *out_items, double *out_scores, int64_t *count, double *bar, int64_t counts[3]);
// tu_pairs_bulk.hip -- its device sorts: n keys descending; n (user << 32 | item, score) entries into the query's order
void pairs_bulk_sort_desc(mmsbm_hip_ctx *c, const uint64_t *keys, uint64_t *sorted, size_t n);
void pairs_bulk_order(mmsbm_hip_ctx *c, const uint64_t *key, const double *score, size_t n, uint64_t *out_key,
                      double *out_score);
// tu_market.hip -- the item side and capacity.  Item-side queries of the recommend session (audience.hpp): item ids inside
// the session's catalogue; out.items: the users
void recommend_query_items(mmsbm_hip_ctx *c, int64_t n_items, const int32_t *items, int n, const TopNOut &out);
void recommend_audience(mmsbm_hip_ctx *c, int64_t n_items, const int32_t *items, double min_score, int64_t capacity,
                        int64_t *offsets, int32_t *users, double *scores);
// ... capacity-aware allocation (allocate.hpp): every user of the request (distinct ids) asks for n items, the caps as
// planned by plan_allocate (serve_plan.hpp); at most max_rounds rounds
void recommend_allocate(mmsbm_hip_ctx *c, const UserRows &users, int n, const AllocPlan &plan, int max_rounds,
                        const TopNOut &out, int32_t *rounds, int32_t *converged);
// ... welfare-maximising assignment (assign.hpp): one item per user of the request (distinct ids) at most, the caps as
// planned by plan_assign (serve_plan.hpp); its sort of a round's bids (tu_pairs_bulk.hip): the places by (item, bid
// descending, place)
void recommend_assign(mmsbm_hip_ctx *c, const UserRows &users, const AssignPlan &plan, double reserve, double eps,
                      int max_rounds, const AssignOut &out);
size_t assign_sort_bytes(size_t n);
void assign_sort_bids(hipStream_t st, void *tmp, size_t bytes, const int32_t *item, const double *bid,
                      const uint32_t *place, uint32_t *sorted, size_t n);
// ... and greedy assortment selection (assortment.hpp): users ascending and distinct; mode: MMSBM_HIP_ASSORT_*; level:
// the floor or the bar
void recommend_assortment(mmsbm_hip_ctx *c, const UserRows &users, int mode, double level, const int32_t *given,
                          int n_given, const Subset &cand, int n_pick, int32_t *items, double *gains, int32_t *count,
                          int32_t *stop, double *given_gains, int32_t *served_items, double *served_scores);
// tu_similar.hip -- nearest items / users (similar.hpp): the session of mmsbm_hip_similar_*; out.scores: the distances
void similar_begin(mmsbm_hip_ctx *c, int side);
void similar_add(mmsbm_hip_ctx *c);  // the selected slot (the caller holds a OneSlot)
void similar_query(mmsbm_hip_ctx *c, int64_t n_rows, const int32_t *ids, int n, const TopNOut &out);
// ... and the most informative items of a user (inform.hpp): the session of mmsbm_hip_inform_*; out.scores: the gains
void inform_begin(mmsbm_hip_ctx *c);
void inform_add(mmsbm_hip_ctx *c);  // the selected slot (the caller holds a OneSlot)
void inform_query(mmsbm_hip_ctx *c, const UserQuery &q, bool exclude_train, int n, const TopNOut &out);
void inform_query_theta(mmsbm_hip_ctx *c, const ThetaQuery &q, int n, const TopNOut &out);
void inform_mean_theta(mmsbm_hip_ctx *c, double *out);
// ... and the overlap of the restarts' groups (overlap.hpp): the session of mmsbm_hip_overlap_*, arguments checked
void overlap_begin(mmsbm_hip_ctx *c, int side);
void overlap_add(mmsbm_hip_ctx *c);  // the selected slot (the caller holds a OneSlot)
void overlap_query(mmsbm_hip_ctx *c, double *out);

// tu_fold_in.hip -- fold new users (items_side: new items) into the selected slot's fitted eta (theta) and p
// (fold_in.hpp), arguments checked; x0, x: theta0, theta (eta0, eta); items_side: item[m] in [0, n_new), user[m] in [0, U)
void fold_in(mmsbm_hip_ctx *c, bool items_side, int64_t n_rows, const int32_t *user, const int32_t *item,
             const int32_t *rating, int32_t n_new, int32_t n_iters, double tol, const double *x0, double *x,
             int32_t *iters);

// tu_heldout.hip -- held-out log-likelihood (heldout.hpp): the session of mmsbm_hip_heldout_*, arguments checked
void heldout_begin(mmsbm_hip_ctx *c, int64_t n_rows, const int32_t *user, const int32_t *item, const int32_t *rating);
// the slots [first, first + n_slots): loglik[s] of each; add: also P into the running per-row sum (one slot)
void heldout_eval(mmsbm_hip_ctx *c, int first, int n_slots, bool add, double *loglik);
void heldout_mean(mmsbm_hip_ctx *c, double *mean_p, double *loglik);

// tu_explain.hip -- which of a user's training rows carry a recommendation (explain.hpp): the session of
// mmsbm_hip_explain_*, arguments checked
void explain_begin(mmsbm_hip_ctx *c, const double *weights);
void explain_add(mmsbm_hip_ctx *c);  // the selected slot (the caller holds a OneSlot)
void explain_query(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int64_t *offsets, const int32_t *items,
                   int n, int32_t *hist_items, int32_t *hist_ratings, double *contribution, int32_t *counts,
                   double *explained, double *score, int32_t *degree);

// ... and the leave-one-out reliability of the training rows (loo.hpp): the session of mmsbm_hip_loo_*, arguments
// checked; rows: positions in the training table (null: every row); flags: per external user / item (null: everyone)
void loo_begin(mmsbm_hip_ctx *c);
void loo_add(mmsbm_hip_ctx *c);  // the selected slot (the caller holds a OneSlot)
void loo_rows(mmsbm_hip_ctx *c, int64_t n_rows, const int64_t *rows, double *fitted, double *reliability);
void loo_sides(mmsbm_hip_ctx *c, double *user_surprise, double *user_fitted_surprise, double *item_surprise,
               double *item_fitted_surprise);
void loo_lowest(mmsbm_hip_ctx *c, int m, const uint8_t *user_flags, const uint8_t *item_flags, int64_t *rows,
                double *reliability, int32_t *count);

// tu_iterate.hip -- the EM iteration: the launches of the form the context's StepPlan gives (step_plan.hpp), the
// cur / a_ok / graph_exec state machine, and the timers.  Dispatchers first:
void stage_dense(mmsbm_hip_ctx *c);
void stage_matvec_a(mmsbm_hip_ctx *c, int slot, int a_slot, bool grid = false);
void ensure_a(mmsbm_hip_ctx *c);  // atab[cur] = A of the current parameters, for every slot the next launches cover
// one iteration of the slots [base_slot, base_slot + launch_slots); commit off: the raw numerators stay in the other
// buffers and cur does not move (update_coefficients).  run_iterations: n committed ones, replayed from a captured
// graph two at a time when "graph" is on
void launch_iteration(mmsbm_hip_ctx *c, bool commit);
void run_iterations(mmsbm_hip_ctx *c, int n);
// the matrix-core A launch's own runs of `units` 64-pair units per workgroup (0: balanced against the CUs)
void build_a_runs(mmsbm_hip_ctx *c, int units);
// the bodies of mmsbm_hip_time_iterations / profile_iterations / kernel_bytes / time_stage, parameters present
float time_iterations(mmsbm_hip_ctx *c, int n_iters);
void profile_iterations(mmsbm_hip_ctx *c, int n_iters, float *mean_us, int *launches_per_iter);
void kernel_bytes(const mmsbm_hip_ctx *c, int index, int64_t *bytes_read, int64_t *bytes_written);
void time_stage(mmsbm_hip_ctx *c, int stage, int reps, float *mean_us);

// tu_create.hip -- building a context (arguments and device index checked), the per-restart state, the index read-back
mmsbm_hip_ctx *context_create(int device, int64_t n_obs, int32_t n_users, int32_t n_items, int32_t n_ratings,
                              int32_t k_groups, int32_t l_groups, const int32_t *user, const int32_t *item,
                              const int32_t *rating, int swap_sides);
void set_slots(mmsbm_hip_ctx *c, int n_slots);  // drops every slot's parameters and the snapshots, selects slot 0
// which: 0 .. 18 (mmsbm_hip_index_array); count always, out (of `capacity` int32) when not null
void index_array(mmsbm_hip_ctx *c, int which, int32_t *out, int64_t capacity, int64_t *count);

// tu_params.hip -- parameters in and out, host layout (K, L, R) / external sides <-> the device's tables; the selected
// slot (the caller holds a OneSlot where the entry's launches need one), arguments checked
void set_params(mmsbm_hip_ctx *c, const double *theta, const double *eta, const double *pr);
void init_params(mmsbm_hip_ctx *c, const uint64_t pcg64_state[4], const double *pr);
void get_params(mmsbm_hip_ctx *c, double *theta, double *eta, double *pr);
void update_coefficients(mmsbm_hip_ctx *c, double *n_theta, double *n_eta, double *n_pr);  // one uncommitted iteration
void fetch_result(mmsbm_hip_ctx *c, double *theta, double *eta, double *pr, double *likelihood);
void snapshot_save(mmsbm_hip_ctx *c);
void snapshot_get(mmsbm_hip_ctx *c, double *theta, double *eta, double *pr);

// tu_options.hip -- the option table behind mmsbm_hip_set_option / get_option; an unknown (set: or read-only) name is
// std::invalid_argument "unknown option: <name>".  A successful set drops the captured graphs
void set_option(mmsbm_hip_ctx *c, const std::string &name, double value);
double get_option(const mmsbm_hip_ctx *c, const std::string &name);

// ---- launch log (MMSBM_HIP_LAUNCH_LOG=<file>; tu_iterate.hip) --------------------------------------------------------
// Host-side only: which kernel instantiations a process launched, how often, and under which test
// (MMSBM_HIP_LAUNCH_TAG at a kernel's first launch).  Appended to the file when a context is destroyed and at exit;
// scripts/kernel_coverage.py diffs it against the compiled set.  Nothing in the kernels knows about it.
extern bool g_launch_log_on;
void launch_log_note(const void *host_fn);
void launch_log_flush();

}  // namespace mmsbm_hip_impl

namespace {

template <class K>
inline void note_launch(K kernel) {
  if (g_launch_log_on) launch_log_note(reinterpret_cast<const void *>(kernel));
}

// One kernel launch.  KERNEL in parentheses when its template arguments hold commas.
#define LAUNCH(KERNEL, GRID, BLOCK, LDS, STREAM, ...)                                                        \
  do {                                                                                                       \
    note_launch(KERNEL);                                                                                     \
    hipLaunchKernelGGL(KERNEL, GRID, dim3(BLOCK), static_cast<uint32_t>(LDS), STREAM, __VA_ARGS__);          \
  } while (0)
// ... of a stage: with the stage's event pair attached to the launch when the stage is timed as that kernel
// (LaunchScope::ext), else plain.
#define LAUNCH_IN(LS, KERNEL, GRID, BLOCK, LDS, STREAM, ...)                                                  \
  do {                                                                                                       \
    note_launch(KERNEL);                                                                                     \
    if ((LS).ext())                                                                                          \
      hipExtLaunchKernelGGL(KERNEL, GRID, dim3(BLOCK), static_cast<uint32_t>(LDS), STREAM, (LS).e0, (LS).e1, 0, __VA_ARGS__); \
    else                                                                                                     \
      hipLaunchKernelGGL(KERNEL, GRID, dim3(BLOCK), static_cast<uint32_t>(LDS), STREAM, __VA_ARGS__);        \
  } while (0)

template <class K>
void allow_big_lds(K kernel, size_t bytes) {
  if (bytes > kLdsBudget)
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(bytes)));
}

// split (main/tail) tables -- see RowTab: theta and A are the gathered ones, eta/C/T stream
inline RowTab plain_tab(double *base, int width, size_t slot_stride = 0) {
  return RowTab{base, base, width, 0, width, 0, slot_stride, 0};
}
// A gathered table (theta, A) as seen from restart slot `slot`: the n_slots copies of every row are
// interleaved (RowTab), main parts of all rows first, then the tail parts.
inline RowTab gather_tab(const mmsbm_hip_ctx *c, double *base, size_t rows, int slot) {
  int mw = (c->kp / 16) * 16;  // whole 128-byte main lines + a tail row
  if (mw == 0) mw = c->kp;
  const int tw = c->kp - mw, ns = c->n_slots;
  return RowTab{base + static_cast<size_t>(slot) * mw,
                base + rows * static_cast<size_t>(ns) * mw + static_cast<size_t>(slot) * tw,
                mw, tw, ns * mw, ns * tw, static_cast<size_t>(mw), static_cast<size_t>(tw)};
}
// (`b` = which of the two ping-pong buffers; the restart slot is c->base_slot)
inline RowTab theta_tab(const mmsbm_hip_ctx *c, int b) {
  return gather_tab(c, c->theta[b].ptr, static_cast<size_t>(c->n_users), c->base_slot);
}
// eta streams: one plain table per slot.  Of the SELECTED slot (single-restart entry points)
inline RowTab eta_tab(const mmsbm_hip_ctx *c, int b) { return plain_tab(c->eta[b].at(c->sel), c->lp); }
inline RowTab a_tab(const mmsbm_hip_ctx *c, int b) {
  return gather_tab(c, c->atab[b].ptr, static_cast<size_t>(c->n_pairs), c->base_slot);
}
inline dim3 slot_grid(const mmsbm_hip_ctx *c, int blocks) {
  return dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(c->launch_slots), 1);
}
// A pair of arguments given by external side, (users' side, items' side) -- theta and eta, the user and the item id
// column -- as (internal users' side, internal items' side): exchanged in a swapped context
template <class T>
inline std::pair<T *, T *> internal_sides(const mmsbm_hip_ctx *c, T *users_side, T *items_side) {
  return c->swapped ? std::make_pair(items_side, users_side) : std::make_pair(users_side, items_side);
}
// Single-restart entry points: launches and copies cover the selected slot only.
struct OneSlot {
  mmsbm_hip_ctx *c;
  int b, n;
  explicit OneSlot(mmsbm_hip_ctx *ctx) : c(ctx), b(ctx->base_slot), n(ctx->launch_slots) {
    c->base_slot = c->sel;
    c->launch_slots = 1;
  }
  ~OneSlot() { c->base_slot = b; c->launch_slots = n; }
};

// The selected slot's current parameters in EXTERNAL terms (the caller holds a OneSlot), whichever internal side holds
// the caller's users: element (k, l, r) of p at p[r * rs + k * ks + l * ls] -- internal (k, l), or (l, k) when the
// context is swapped -- and the caller's users' / items' rows (theta / eta, or eta / theta when swapped).  The serving
// paths (recommend, similar, fold-in) read the model through this and nothing else, so a swapped context gives them
// the same values in the same order.
struct ExtSlot {
  const double *p;
  size_t rs;
  int ks, ls;
  RowTab users, items;
};
inline ExtSlot ext_slot(const mmsbm_hip_ctx *c) {
  const RowTab th = theta_tab(c, c->cur), et = eta_tab(c, c->cur);
  return ExtSlot{c->p[c->cur].at(c->sel), static_cast<size_t>(c->kp) * c->lp, c->swapped ? 1 : c->lp,
                 c->swapped ? c->lp : 1, c->swapped ? et : th, c->swapped ? th : et};
}
// ... and those of a given slot, no OneSlot needed, with the distance to the next slot's copy in both tables (RowTab
// so_m / so_t; p: the SlotBuf's stride) -- a launch that covers several slots steps from this one with slot_tab
inline ExtSlot ext_slot(const mmsbm_hip_ctx *c, int slot) {
  const RowTab th = gather_tab(c, c->theta[c->cur].ptr, static_cast<size_t>(c->n_users), slot);
  const RowTab et = plain_tab(c->eta[c->cur].at(slot), c->lp, c->eta[c->cur].stride);
  return ExtSlot{c->p[c->cur].at(slot), static_cast<size_t>(c->kp) * c->lp, c->swapped ? 1 : c->lp,
                 c->swapped ? c->lp : 1, c->swapped ? et : th, c->swapped ? th : et};
}

// Non-temporal stores for the rows the next launch gathers (T, A, theta'): one restart per launch and rows of up to
// 32 groups.  Measured per iteration, plain -> non-temporal (scripts/ab_fused.sh, variants side by side on one box): C1
// 11.3 -> 11.2 us, C2 20.3 -> 19.5, 600k ratings at K = L = 20 67.2 -> 66.0, C3 95.3 -> 93.8, 3M 302.3 -> 297.2, 10M
// 886 -> 880; with restart slots nothing or a loss (C3 x 2 165.8 -> 166.9, C3 x 8 591 -> 597), theta' at K = L = 50
// +0.3 %.  C rows, eta' and the slabs the same way: +0.3, +0.3 and +1.0 us at C3 -- they stay plain stores.  Loads:
// the segments' own rows in seg_pass as non-temporal loads C3 94.1 -> 93.5 (kept, same condition); the T rows in
// item_sum +1.6 us, the index stream +0.3, C rows in T + S and the slabs in p_update nothing.
// Only for data whose segments are all short and alike (no work lists on either side): with heavy-tailed degrees the
// rows of busy users and popular items are gathered again and again and a long segment's own row is read by every one
// of its pieces -- there every one of these hints costs (1M ratings, K = L = 20, per iteration, none / T and A rows /
// theta' rows / own-row loads / all: log-normal degrees 90.2 / 90.6 / 91.5 / 95.9 / 96.8 us, Zipf(1.2) 93.9 / 95.5 /
// 99.2 / 103.6 / 104.7; 100k ratings of 943 users: 28.2 / 29.2 / 28.2 / 28.4 / 29.4; scripts/nt_time.py).
inline int nt_on(const mmsbm_hip_ctx *c) {
  const bool plain_data = (c->lay.pair_work.items.empty() && c->lay.user_work.items.empty()) || (c->nt_out & 8);  // (8: tuning, whatever the data)
  return (plain_data && c->launch_slots == 1 && c->kp <= 32 && c->lp <= 32) ? (c->nt_out & 7) : 0;
}

}  // namespace
