// context.hpp -- host side: device buffers, the context (mmsbm_hip_ctx), launch bookkeeping
// Included by every translation unit of the library (prelude.hpp).
#pragma once

namespace {

// ======================================================================================
// host side
// ======================================================================================
// one (G, VEC) instantiation per group_code (shapes.hpp)
#define DISPATCH_GV(code, CALL)                                   \
  switch (code) {                                                 \
    case 0: CALL(4, 4); break;                                    \
    case 1: CALL(8, 4); break;                                    \
    case 2: CALL(16, 4); break;                                   \
    case 3: CALL(32, 4); break;                                   \
    case 4: CALL(64, 4); break;                                   \
    case 5: CALL(64, 8); break;                                   \
    default: CALL(64, 16); break;                                 \
  }

}  // namespace

namespace mmsbm_hip_impl {  // (members of mmsbm_hip_ctx: one type in every translation unit)

template <class T>
struct DevBuf {
  T *ptr = nullptr;
  size_t count = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
  }
  void alloc(size_t n) {
    release();
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ptr), std::max<size_t>(n, 1) * sizeof(T)));
    count = n;  // (only once the memory is there: a failed allocation leaves an empty buffer)
  }
  void upload(const std::vector<T> &h, hipStream_t s) {
    alloc(h.size());
    if (!h.empty())
      HIP_CHECK(hipMemcpyAsync(ptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void swap(DevBuf &o) {
    using std::swap;
    swap(ptr, o.ptr);
    swap(count, o.count);
  }
};

// A session table of `slots` slots, `per_slot` doubles each, grown by one slot: `next` becomes the table of slots + 1 with
// the earlier slots copied as they are (device to device, on `s`); returns the new slot.  The caller checks the memory
// first, fills the new slot, and swaps `next` in once its kernels have run.
inline double *grow_by_slot(const DevBuf<double> &tab, size_t per_slot, int slots, hipStream_t s, DevBuf<double> &next) {
  next.alloc((static_cast<size_t>(slots) + 1) * per_slot);
  if (slots > 0)
    HIP_CHECK(hipMemcpyAsync(next.ptr, tab.ptr, sizeof(double) * slots * per_slot, hipMemcpyDeviceToDevice, s));
  return next.ptr + static_cast<size_t>(slots) * per_slot;
}

// A per-restart table: `slots` copies, `stride` doubles apart (whole 128-byte lines, so every
// copy keeps the alignment of the first).
struct SlotBuf : DevBuf<double> {
  size_t stride = 0;
  void alloc_slots(size_t per_slot, int slots) {
    stride = (per_slot + 15) / 16 * 16;
    alloc(stride * static_cast<size_t>(slots));
  }
  double *at(int slot) const { return ptr + static_cast<size_t>(slot) * stride; }
};

// Pinned host staging: parameter rows travel as ONE contiguous copy in the device layout
// (packed / unpacked on the host by a few threads) instead of strided 2-D copies from
// pageable memory.
struct PinBuf {
  double *ptr = nullptr;
  size_t cap = 0, used = 0;
  PinBuf() = default;
  PinBuf(const PinBuf &) = delete;
  PinBuf &operator=(const PinBuf &) = delete;
  ~PinBuf() {
    if (ptr) (void)hipHostFree(ptr);
  }
  void reset(size_t need) {
    used = 0;
    if (need <= cap) return;
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    cap = 0;
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ptr), need * sizeof(double), hipHostMallocDefault));
    cap = need;
  }
  double *take(size_t n) {
    double *r = ptr + used;
    used += n;
    return r;
  }
};

// The items a query leaves out per row of the table it scores (device; off indexed by the row's id): null off -- none
struct SeenLists {
  const int32_t *off = nullptr, *items = nullptr;
};

// The recommend session (mmsbm_hip_recommend_begin .. end; recommend.hpp): the slots' folded factors, external sides.
// Created by recommend_begin, dropped whole by recommend_begin and recommend_end.
struct RecSession {
  DevBuf<double> x, y, w;               // [slot][U][rank], [slot][items][rank], the R rating weights
  DevBuf<double> wk;                    // [slot][K][L]: each slot's W (recommend_query_theta folds caller rows)
  DevBuf<int32_t> seen_off, seen;       // per external user: its distinct excluded items, ascending (excl)
  std::vector<int32_t> seen_off_h;      // seen_off on the host (candidate counts of recommend_positions)
  DevBuf<int32_t> by_item_off, by_item; // per item of the catalogue: its excluded users, ascending -- the transpose of
  bool by_item_built = false;           // seen_off / seen, built by the first item-side query (audience.hpp)
  int slots = 0;                        // slots added
  int items = 0;                        // the session's catalogue: I, or I + n_new after recommend_add_items
  int rank = 0;
  int users = 0;                        // U
  bool excl = false;                    // seen_* in use: exclude_train, or seen lists of recommend_add_items
  double w_min = 0.0, w_max = 0.0;      // the smallest and the largest rating weight: every score lies between them
  SeenLists seen_lists() const { return {excl ? seen_off.ptr : nullptr, seen.ptr}; }
  size_t x_stride() const { return static_cast<size_t>(users) * rank; }  // doubles between two slots of x
};

// The similarity session (mmsbm_hip_similar_begin .. end; similar.hpp): the added slots' profiles and group masses of
// one external side.  Created by similar_begin, dropped whole by similar_begin and similar_end.
struct SimSession {
  DevBuf<double> q;                     // [slot][rows][width]: the rating profiles
  DevBuf<double> mf;                    // [slot][width]: the mass of the group each profile entry belongs to
  int side = 0;                         // 0: items, 1: users (external sides)
  int slots = 0;                        // slots added
  int rows = 0;                         // rows of the side: I, or U
  int others = 0;                       // rows of the other side (the masses sum to it): U, or I
  int width = 0;                        // profile entries per row: K R, or L R
};

// The overlap session (mmsbm_hip_overlap_begin .. end; overlap.hpp): the added slots' membership tables of one external
// side.  Created by overlap_begin, dropped whole by overlap_begin and overlap_end; set_slots leaves it alone (it holds
// copies of the rows, nothing of a slot).
struct OvlSession {
  DevBuf<double> x;                     // [slot][rows][groups]
  int side = 0;                         // 0: items (eta, L groups), 1: users (theta, K groups); external sides
  int slots = 0;                        // slots added
  int rows = 0;                         // rows of the side: I, or U
  int groups = 0;                       // G: L, or K
};

// The held-out session (mmsbm_hip_heldout_begin .. end; heldout.hpp): the request's rows rating-major, cut into blocks
// of one rating, and the running per-row sum of the slots added.  Created by heldout_begin, dropped whole by
// heldout_begin and heldout_end; set_slots leaves it alone (it holds rows, no parameters).
struct HoldSession {
  DevBuf<int32_t> user, item, orig;     // external ids in session order, and each row's place in the request
  DevBuf<int4> blocks;                  // (rating, first row, rows, 0)
  DevBuf<double> sum;                   // [rows], request order: P added by every heldout_add
  DevBuf<double> part, out, mean;       // [slots][blocks] block sums, [slots] results, [rows] of heldout_mean
  int64_t rows = 0;
  int n_blocks = 0;
  int part_slots = 0;                   // slots `part` and `out` are sized for
  int slots = 0;                        // slots added: heldout_add calls so far
};

// The predict/score session (mmsbm_hip_predict_begin .. finish): the test rows, internal sides, and the running sum of
// the added slots' rating distributions.  Created by predict_begin, dropped whole by predict_begin and predict_finish.
struct PredictSession {
  DevBuf<int32_t> u, i, r;              // [rows]: internal user, internal item, true rating
  DevBuf<double> sum, w, part;          // [rows][R] distributions added so far, the R rating weights, sums per workgroup
  int64_t rows = 0;
  int slots = 0;                        // slots added: predict_add calls so far
};

// The explain session (mmsbm_hip_explain_begin .. end; explain.hpp): external copies of what the attribution of a score
// to the user's training rows reads, per added slot, and the training rows per external user.  Created by explain_begin,
// dropped whole by explain_begin and explain_end; set_slots leaves it alone (it holds copies, nothing of a slot).
struct ExpSession {
  DevBuf<double> w;                     // the R rating weights
  DevBuf<double> th, g;                 // [slot][U][K] theta, [slot][I][K] G = eta W^T
  DevBuf<double> p, eta;                // [slot][R][K][L] p in external (k, l), [slot][I][L] eta: what v needs
  DevBuf<int64_t> off;                  // [U + 1]: the training rows of every external user, in the order given
  DevBuf<int32_t> item, rating;         // [n_obs]: their items and ratings (duplicate triples are separate rows)
  std::vector<int64_t> off_h;           // off on the host (degrees, batches)
  int slots = 0;                        // slots added
};

// The inform session (mmsbm_hip_inform_begin .. end; inform.hpp): external copies of what the information gain of a
// (user, item) pair reads, per added slot, and (built by the first query that excludes them) every user's training
// items.  Created by inform_begin, dropped whole by inform_begin and inform_end; set_slots leaves it alone (it holds
// copies, nothing of a slot).
struct InfSession {
  DevBuf<double> th;                    // [slot][U][K] theta
  DevBuf<double> q;                     // [slot][I][K R]: the items' rating profiles (sim_profile_kernel)
  DevBuf<double> h;                     // [slot][I][K]: the entropy of each profile row (inf_entropy_kernel)
  DevBuf<double> mass;                  // [slot][K]: sum_u theta[u, k] (sim_mass_kernel); theta-bar is this over U
  DevBuf<int32_t> seen_off, seen;       // per external user: its distinct training items, ascending
  bool seen_built = false;
  int slots = 0;                        // slots added
};

// The leave-one-out session (mmsbm_hip_loo_begin .. end; loo.hpp): the training table in the order it was given, its
// rows by user and by item cut into chunks, the C and E of the slot being added and the rows' running sums.  Created
// by loo_begin, dropped whole by loo_begin and loo_end; set_slots leaves it alone (it holds sums, nothing of a slot).
struct LooSession {
  struct Side {                         // the rows of every user (or item), ascending position in the training table
    DevBuf<int64_t> off, chunk_off;     // [segments + 1]: first row / first chunk of a segment
    DevBuf<int32_t> rows, chunk_seg;    // [n_obs] positions in the training table; [chunks] the segment of a chunk
    DevBuf<double> num, part;           // [segments][groups] C (or E) of the last add; [chunks][max(groups, 2)] chunk sums
    DevBuf<double> bar, surprise;       // [groups] the mean row of the last add; [segments][2] mean surprises (finish)
    std::vector<int64_t> off_h;         // off on the host (degrees)
    int64_t chunks = 0;
  } by_user, by_item;
  DevBuf<int32_t> user, item, rating;   // [n_obs] external ids, training order
  DevBuf<double> fit;                   // [n_obs] fit_j of the slot being added
  DevBuf<double> rel_sum, fit_sum;      // [n_obs] running sums over the slots added
  DevBuf<double> rel, fitted, sur, fsur;  // [n_obs] the finished columns of the slots added so far
  bool finished = false;                // ... are those of `slots`
  int slots = 0;                        // slots added
};

// The serving calls whose kernels are timed (mmsbm_hip_ctx::last_ms), in the order of their "<name>_ms" options:
// recommend_query / recommend_query_items, fold_in / fold_in_items, recommend_positions, recommend_top_pairs,
// recommend_audience, similar_query, overlap_query, heldout_eval / heldout_add, explain_query, recommend_diverse /
// similar_pairs, inform_query / inform_query_theta, recommend_query_groups, recommend_query_ensemble / recommend_pair_spread,
// loo_add / loo_rows / loo_sides / loo_lowest (and, of the last loo_add alone, its sums pass and its row pass),
// recommend_allocate, recommend_top_pairs_bulk, recommend_assortment, recommend_assign
enum TimedCall { T_RECOMMEND = 0, T_FOLD_IN, T_POSITIONS, T_TOP_PAIRS, T_AUDIENCE, T_SIMILAR, T_OVERLAP, T_HELDOUT, T_EXPLAIN, T_DIVERSE, T_INFORM, T_GROUP, T_ENSEMBLE, T_LOO, T_LOO_SUMS, T_LOO_ROWS, T_ALLOCATE, T_TOP_PAIRS_BULK, T_ASSORT, T_ASSIGN, T_COUNT };

}  // namespace mmsbm_hip_impl

namespace {

// fn(first_row, last_row) over [0, rows), on up to 8 host threads when the table is large
template <class F>
void for_row_blocks(int rows, size_t row_doubles, F &&fn) {
  const size_t total = static_cast<size_t>(rows) * row_doubles;
  unsigned nt = total < (size_t(1) << 19) ? 1u : std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  if (nt <= 1) {
    fn(0, rows);
    return;
  }
  std::vector<std::thread> th;
  const int per = (rows + static_cast<int>(nt) - 1) / static_cast<int>(nt);
  for (unsigned t = 0; t < nt; ++t) {
    const int a = static_cast<int>(t) * per, b = std::min(rows, a + per);
    if (a < b) th.emplace_back([&fn, a, b] { fn(a, b); });
  }
  for (auto &x : th) x.join();
}

// The n pairs (key[m], value m) grouped by key < n_keys (counting sort): returns off [n_keys + 1], and put(m, at) is told
// the place `at` in [off[key[m]], off[key[m] + 1]) of pair m -- a key's pairs keep the order of the request.
template <class Off, class Put>
std::vector<Off> group_by_key(const int32_t *key, int64_t n, int n_keys, Put &&put) {
  std::vector<Off> off(static_cast<size_t>(n_keys) + 1, 0);
  for (int64_t m = 0; m < n; ++m) off[static_cast<size_t>(key[m]) + 1]++;
  for (int k = 0; k < n_keys; ++k) off[k + 1] += off[k];
  std::vector<Off> pos(off.begin(), off.end() - 1);
  for (int64_t m = 0; m < n; ++m) put(m, pos[key[m]]++);
  return off;
}

// Every group of (off, val) ascending and distinct, in place (off and val shrink to what is kept)
inline void sort_unique_groups(std::vector<int32_t> &off, std::vector<int32_t> &val) {
  int32_t w = 0;
  for (size_t g = 0; g + 1 < off.size(); ++g) {
    const int32_t a = off[g], b = off[g + 1];
    std::sort(val.begin() + a, val.begin() + b);
    off[g] = w;
    for (int32_t e = a; e < b; ++e)
      if (e == a || val[e] != val[e - 1]) val[w++] = val[e];
  }
  off.back() = w;
  val.resize(static_cast<size_t>(w));
}

// the stages by KernelId (step_plan.hpp)
const char *const kKernelNames[K_COUNT] = {"seg_pass_kernel", "pair_block_kernel(T+S)", "eta_p_kernel",
                                           "pair_block_kernel(A)", "pairs_fused_kernel", "tail_fused_kernel"};


}  // namespace


struct mmsbm_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // parameter downloads that overlap kernels of `stream` (mmsbm_hip_result)
  hipStream_t xfer = nullptr;         // when set: the stream copy_rows / fetch_params use instead of `stream`
  bool swapped = false;
  // external dims
  int64_t n_obs = 0;
  int ext_users = 0, ext_items = 0, ext_k = 0, ext_l = 0;
  // internal dims ("item" = the side paired with the rating)
  int n_users = 0, n_items = 0, n_ratings = 0, k = 0, l = 0, kp = 0, lp = 0;
  int n_pairs = 0, n_chunks = 0;
  int code_k = 0, code_l = 0;
#ifdef MMSBM_ABLATE
  int ablate = 0;           // diagnostic build (-DMMSBM_ABLATE): phases the pair stage / eta_p skip, set by mmsbm_hip_time_stage
#endif
  PairPlan pp;  // the pair stage's launch plan: its form and geometry (pair_plan.hpp)
  // prod_dist / predict through B[(item, rating), :] = p_r eta_i (predict_rows_kernel)
  DevBuf<int32_t> grid_item;          // item of pair q = r * I + i, every (item, rating) combination
  DevBuf<mmsbm::Chunk> grid_chunks;   // its rating-homogeneous chunks
  int grid_n_chunks = 0;
  DevBuf<double> btab;                // [I * R][kp], of the slot being scored
  bool predict_fast = true;
  int seg_batch = 4;  // row gathers a group of seg_pass keeps in flight (4, or 8)
  // the iteration's form -- two launches (fused_small.hpp), three (pass_dense.hpp) or four: what was asked for and the
  // facts about the data that decide it (step_plan.hpp)
  StepPlan step;
  // the whole-segment lists of the two-launch form (step.fs_pairs / step.fs_users; layout.hpp: FusedLists)
  DevBuf<mmsbm::FusedUnit> fp_units, fu_units;
  DevBuf<mmsbm::WorkItem> fp_items, fu_items;
  DevBuf<mmsbm::FusedSplit> fp_splits, fu_splits;
  int fp_max_parts = 0, fu_max_parts = 0, fu_blocks = 0;
  std::vector<char> a_ok;     // per slot: atab[cur] holds A of the CURRENT parameters (the fused form computes A at
                               // the start of an iteration, so after a committed fused iteration it does not)
  int nt_out = 7;          // option "nt_out" (bits: 1 T and A rows, 2 theta' rows as non-temporal stores, 4 the segments' own rows as non-temporal loads) where that pays (nt_on, launch.hpp)
  int ranges_pairs = 1, ranges_users = 1;  // XCD-local work lists: ranges the gathered table is cut into
  int n_cus = 256;
  bool gpu_layout = false;  // the index's sorts ran on the device (build_index; option "gpu_layout")
  mmsbm::Layout lay;  // host copy (degrees, sizes)
  DevBuf<int32_t> pair_off, pair_user, pair_item, user_off, user_pair, item_off, item_pairs,
      item_deg, mv_chunk_off, orig_u, orig_i, orig_r;
  DevBuf<int32_t> item_grid;  // [n_items][n_ratings] pair ids (-1: none); only for dense (item, rating) grids
  DevBuf<mmsbm::Chunk> mv_chunks;
  DevBuf<mmsbm::Chunk> lik_units;  // 64-pair units for the likelihood kernel (mv_chunks may hold 256)
  DevBuf<mmsbm::Chunk> a_chunks;   // matrix-core A launch: its own runs of units (balanced_run_units, tu_iterate.hip), when they differ from mv_chunks
  int n_a_chunks = 0, a_units = 0;   // (a_units: 64-pair units per workgroup of that launch; option "a_units")
  int n_lik_units = 0;
  DevBuf<mmsbm::WorkItem> pair_items, user_items;   // only when some segment is long
  DevBuf<mmsbm::SplitSeg> pair_splits, user_splits;
  // Per-restart state, one copy per slot.  A context carries n_slots independent restarts
  // (parameter sets) over the SAME triples; em_iterate advances all of them with one set of
  // launches (blockIdx.y = slot), the single-restart entry points act on slot `sel`.
  int n_slots = 1, sel = 0;
  int base_slot = 0, launch_slots = 1;  // what the next launches cover: [base_slot, base_slot + launch_slots)
  SlotBuf pair_parts, user_parts;
  SlotBuf theta[2], eta[2], p[2], pt[2], atab[2], ctab, ttab, partial, npr;
  DevBuf<double> lik_part;
  DevBuf<double> lg_theta, lg_eta, lg_p;  // logarithm tables of the selected slot (likelihood)
  int lik_mode = 2;                       // option "lik_fast": 0 log per element, 1 log tables, 2 a wave per pair where it applies
  int lik_g = 0;                          // option "lik_g": lanes per triple (0 = automatic)
  PinBuf pin;  // host staging for set_params / get_params / update_coefficients
  // the open sessions; null: none
  std::unique_ptr<mmsbm_hip_impl::PredictSession> ps;  // predict / score
  std::unique_ptr<mmsbm_hip_impl::RecSession> rc;      // recommend
  std::unique_ptr<mmsbm_hip_impl::SimSession> sm;      // similarity
  std::unique_ptr<mmsbm_hip_impl::OvlSession> ov;      // overlap
  std::unique_ptr<mmsbm_hip_impl::HoldSession> ho;     // held-out
  std::unique_ptr<mmsbm_hip_impl::ExpSession> ex;      // explain
  std::unique_ptr<mmsbm_hip_impl::InfSession> inf;     // inform
  std::unique_ptr<mmsbm_hip_impl::LooSession> loo;     // leave-one-out
  float last_ms[T_COUNT] = {};              // device time of the last call's kernels, per TimedCall (options "<name>_ms")
  int top_groups = 0;                       // option "top_pairs_groups": workgroups of gtop_fused_kernel (0: 2 per CU)
  int pb_groups = 0, pb_bits = 0;           // options "pairs_bulk_groups" / "pairs_bulk_bits" (pairs_bulk.hpp; 0: the library's choice)
  int64_t pb_collect = kPbDefaultCollect;   // option "pairs_bulk_collect": the bin size at which the select stops and sorts
  int pb_passes = 0;                        // of the last bulk query: histogram passes run, keys collected (0: no early stop)
  int64_t pb_collected = 0;
  int64_t aud_rows = 0;                     // option "audience_rows": items per COUNT batch (0: the library's choice)
  int64_t aud_entries = 0;                  // option "audience_entries": entries per WRITE batch at most (0: likewise)
  int64_t exp_rows = 0;                     // option "explain_rows": training rows per batch of explain_query (0: likewise)
  int64_t div_rows = 0;                     // option "diverse_rows": request rows per call of recommend_diverse (0: likewise)
  int64_t grp_run = 0;                      // option "group_run_blocks": 8-row blocks of members per run of grp_tile_kernel (0: likewise)
  int alloc_rounds = 0;                     // option "allocate_rounds": the rounds of the last recommend_allocate
  int asg_rounds = 0;                       // option "assign_rounds": the rounds of the last recommend_assign
  int64_t asg_bids = 0;                     // option "assign_bids": the bids of all its rounds
  int64_t asrt_run = 0;                     // option "assortment_run_blocks": 8-row blocks of users per run of asrt_gain_kernel (0: likewise)
  int64_t asrt_part = 0;                    // option "assortment_part_bytes": the partial buffer of a batch of item tiles (0: kAsrtPartBytes)
  bool asrt_timing = false;                 // option "assortment_timing": events between the phases of every round
  float asrt_ms[3] = {};                    // ... of the last recommend_assortment: its gain + join, pick and update kernels
  // snapshots (mmsbm_hip_snapshot_save / get): a second copy of theta, eta and p in the layout of theta[cur], eta[cur]
  // and p[cur], every slot's place in it filled by that slot's last save; allocated by the first save, dropped by set_slots
  DevBuf<double> snap_theta;
  SlotBuf snap_eta, snap_p;
  std::vector<char> snap_have;              // per slot: a snapshot has been saved
  int cur = 0;
  std::vector<char> have;  // per slot: set_params has been called
  bool graph_mode = false;  // replay a captured two-iteration hipGraph instead of eager launches
  hipGraphExec_t graph_exec[2] = {nullptr, nullptr};  // indexed by `cur` at capture time
  // per-launch profiling
  bool profiling = false;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> prof_events;

  // the form of the next iteration of the slots [base_slot, base_slot + launch_slots), under the options in force
  StepForm form(bool commit) const { return step.form(pp, launch_slots, commit); }
  void drop_graphs() {
    for (auto &g : graph_exec) {
      if (g) (void)hipGraphExecDestroy(g);
      g = nullptr;
    }
  }
  void drop_snapshots() {
    snap_theta.release();
    snap_eta.release();
    snap_p.release();
    snap_have.clear();
  }
  ~mmsbm_hip_ctx() {
    drop_graphs();
    for (auto &pe : prof_events) {
      (void)hipEventDestroy(pe.second.first);
      (void)hipEventDestroy(pe.second.second);
    }
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {


// Optional event pair of one stage (mmsbm_hip_profile_iterations).  Normally the events are recorded on the
// stream in front of and behind the stage's launches, which adds the launch gaps to what they measure
// (seg_pass at C3: 64.8 us against 62.2 in the kernel trace).  A stage that is ONE kernel can hand the pair
// to the launch itself instead (hipExtLaunchKernelGGL): the events then carry the kernel's own begin and end
// time stamps -- what rocprofv3 reports.
struct LaunchScope {
  mmsbm_hip_ctx *c;
  int id;
  bool kernel_events;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  LaunchScope(mmsbm_hip_ctx *ctx, int kid, bool one_kernel = false) : c(ctx), id(kid), kernel_events(one_kernel) {
    if (c->profiling) {
      HIP_CHECK(hipEventCreate(&e0));
      HIP_CHECK(hipEventCreate(&e1));
      if (!kernel_events) HIP_CHECK(hipEventRecord(e0, c->stream));
    }
  }
  bool ext() const { return c->profiling && kernel_events; }  // the launch takes e0 / e1
  void done() {
    HIP_CHECK(hipGetLastError());
    if (c->profiling) {
      if (!kernel_events) HIP_CHECK(hipEventRecord(e1, c->stream));
      c->prof_events.push_back({id, {e0, e1}});
    }
  }
};

void use_device(const mmsbm_hip_ctx *c) { HIP_CHECK(hipSetDevice(c->device)); }

}  // namespace

namespace mmsbm_hip_impl {  // (an argument of the serving frame, serve_frame.hpp: one type in every translation unit)

// Device time between two points of a stream: start() and stop() record, ms() reads it once the stream has passed
// stop().  The events are destroyed on every way out of the scope.
struct EventPair {
  struct Event {
    hipEvent_t e = nullptr;
    Event() { HIP_CHECK(hipEventCreate(&e)); }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { (void)hipEventDestroy(e); }
  } e0, e1;
  void start(hipStream_t s) { HIP_CHECK(hipEventRecord(e0.e, s)); }
  void stop(hipStream_t s) { HIP_CHECK(hipEventRecord(e1.e, s)); }
  void wait() { HIP_CHECK(hipEventSynchronize(e1.e)); }   // the host waits for stop()'s point of the stream
  float ms() const {
    float v = 0.f;
    HIP_CHECK(hipEventElapsedTime(&v, e0.e, e1.e));
    return v;
  }
};

}  // namespace mmsbm_hip_impl
