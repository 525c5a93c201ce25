// tu_create.hip -- building a context: the shape plan, the index (sorted on the host or on the device, layout_gpu.hpp),
// its work lists and uploads, and the per-restart state (alloc_state, also behind set_slots); with the read-back of the
// index (index_array).  Host code only.
#include "prelude.hpp"
#include "layout_gpu.hpp"

namespace mmsbm_hip_impl {

namespace {

// ---- building a context: the steps of context_create, in the order it calls them -----------------------------------------

// The create-time tuning switches.  Read from the environment by every mmsbm_hip_create call (not when the library is
// loaded: callers set and unset them between contexts), here and nowhere else.
struct CreateKnobs {
  bool force_wide = false;      // the wide-row kernels whatever the shape
  int gpu_layout = -1;          // 0 / 1: the layout's sorts on the host / on the device whatever the size (-1: by size)
  bool no_mfma = false;         // the pair stage of big tiles stays on the vector ALUs
  int mfma_chunk = 0;           // tuning: pairs per workgroup of big tiles, a multiple of 64 in 64 .. 1,024 (0: not set)
  bool no_ranges = false;       // no XCD-local work lists
  int ranges_pairs = 0, ranges_users = 0;  // tuning: "pairs,users" forced range counts, 1 .. 512 each (0: not set)
  bool no_fused_split = false;  // no whole-segment lists for the two-launch form
  int fused_ucap = 0;           // tuning: work items per workgroup of its user side (0: not set)
  bool no_fused = false;        // four launches per iteration whatever the size
  bool no_itemgrid = false;     // no fixed-width grid of pair ids
  bool timing = false;          // where the time of building a context goes (stderr)
};
CreateKnobs read_create_knobs() {
  CreateKnobs k;
  auto is_set = [](const char *name) { return std::getenv(name) != nullptr; };
  k.force_wide = is_set("MMSBM_HIP_FORCE_WIDE");
  if (const char *g = std::getenv("MMSBM_HIP_GPU_LAYOUT")) k.gpu_layout = std::atoi(g) != 0;
  k.no_mfma = is_set("MMSBM_HIP_NO_MFMA");
  if (const char *e = std::getenv("MMSBM_HIP_MFMA_CHUNK")) k.mfma_chunk = std::min(std::max(std::atoi(e) / 64 * 64, 64), kMfmaChunkPairs);
  k.no_ranges = is_set("MMSBM_HIP_NO_RANGES");
  if (const char *f = std::getenv("MMSBM_HIP_RANGES")) {
    int a = 0, b = 0;
    if (std::sscanf(f, "%d,%d", &a, &b) == 2 && a >= 1 && b >= 1 && a <= 512 && b <= 512) { k.ranges_pairs = a; k.ranges_users = b; }
  }
  k.no_fused_split = is_set("MMSBM_HIP_NO_FUSED_SPLIT");
  if (const char *e = std::getenv("MMSBM_HIP_FUSED_UCAP")) k.fused_ucap = std::max(1, std::atoi(e));
  k.no_fused = is_set("MMSBM_HIP_NO_FUSED");
  k.no_itemgrid = is_set("MMSBM_HIP_NO_ITEMGRID");
  k.timing = is_set("MMSBM_HIP_TIMING");
  return k;
}

struct CreateLaps {  // (CreateKnobs::timing) one line per step: the time since the line before
  bool on;
  std::chrono::steady_clock::time_point clk = std::chrono::steady_clock::now();
  void operator()(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[mmsbm_hip_create] %-28s %8.2f ms\n", what,
                 std::chrono::duration<double, std::milli>(now - clk).count());
    clk = now;
  }
};

// Which side is paired with the rating, the internal dims, their padding and group codes
void plan_sides(mmsbm_hip_ctx *c, int device, int64_t n_obs, int32_t n_users, int32_t n_items, int32_t n_ratings,
                int32_t k_groups, int32_t l_groups, int swap_sides) {
  c->device = device;
  c->swapped = swap_sides > 0 || (swap_sides < 0 && n_users < n_items);
  c->n_obs = n_obs;
  c->ext_users = n_users; c->ext_items = n_items; c->ext_k = k_groups; c->ext_l = l_groups;
  c->n_ratings = n_ratings;
  if (c->swapped) {
    c->n_users = n_items; c->n_items = n_users; c->k = l_groups; c->l = k_groups;
  } else {
    c->n_users = n_users; c->n_items = n_items; c->k = k_groups; c->l = l_groups;
  }
  c->kp = pad_dim(c->k); c->lp = pad_dim(c->l);
  c->code_k = group_code(c->kp); c->code_l = group_code(c->lp);
  // small problems leave most CUs a couple of workgroups: the triple passes are then bound by the rounds of
  // dependent gathers per segment, and eight rows in flight per group beat four (C1 16.8 -> 16.1 us, C2 29.7 ->
  // 29.1 us per iteration); at C3 four are better (95.3 vs 97.3 us)
  c->seg_batch = c->n_obs <= 300000 ? 8 : 4;
}

// The device, its CU count (chunk lengths and persistent grids are sized from it) and the two streams
void open_device(mmsbm_hip_ctx *c) {
  HIP_CHECK(hipSetDevice(c->device));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && cus > 0)
    c->n_cus = cus;
  HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
}

// The id columns in the caller's order (the element-wise kernels keep them so), internal sides: enqueued on c->stream
void upload_ids(mmsbm_hip_ctx *c, const int32_t *iu, const int32_t *ii, const int32_t *rating) {
  const size_t bytes = sizeof(int32_t) * static_cast<size_t>(c->n_obs);
  HIP_CHECK(hipMemcpyAsync(c->orig_u.ptr, iu, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_CHECK(hipMemcpyAsync(c->orig_i.ptr, ii, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_CHECK(hipMemcpyAsync(c->orig_r.ptr, rating, bytes, hipMemcpyHostToDevice, c->stream));
}

// The sorts: on the host for small inputs (14 ms at 1M ratings), on the device beyond kGpuLayoutMin triples
// (layout_gpu.hpp; CreateKnobs::gpu_layout forces either).  Returns whether they ran on the device: pair_user and
// user_pair then stay where they were built (owned by the context's buffers from here on) and the id columns are
// uploaded already; after the host's sorts upload_index() sends all of them.
bool build_index(mmsbm_hip_ctx *c, const CreateKnobs &knobs, const int32_t *iu, const int32_t *ii, const int32_t *rating,
                 CreateLaps &lap) {
  const int64_t n_obs = c->n_obs;
  bool gpu_layout = knobs.gpu_layout >= 0 ? knobs.gpu_layout != 0 : n_obs >= kGpuLayoutMin;
  // (the device sort packs (rating, item) into 31 bits; sparser key spaces stay on the host)
  if (static_cast<uint64_t>(c->n_ratings) * static_cast<uint64_t>(c->n_items) >= (uint64_t(1) << 31)) gpu_layout = false;
  if (gpu_layout) {  // (the host's sorts check the ids themselves)
    mmsbm::validate_triples(n_obs, c->n_users, c->n_items, c->n_ratings, iu, ii, rating);
    lap("id checks");
  }
  c->orig_u.alloc(n_obs); c->orig_i.alloc(n_obs); c->orig_r.alloc(n_obs);
  if (!gpu_layout) {
    mmsbm::build_layout(n_obs, c->n_users, c->n_items, c->n_ratings, iu, ii, rating, 512, c->lay);
    lap("host layout (sorts)");
    return false;
  }
  if (n_obs > 0) {
    upload_ids(c, iu, ii, rating);
    HIP_CHECK(hipStreamSynchronize(c->stream));  // the caller's buffers are free again
    lap("id upload");
  }
  mmsbm::gpu_layout::DeviceArrays dev_idx;
  try {
    mmsbm::gpu_layout::sort_stage(c->stream, n_obs, c->n_users, c->n_items, c->n_ratings, c->orig_u.ptr,
                                  c->orig_i.ptr, c->orig_r.ptr, c->lay, dev_idx);
  } catch (const std::invalid_argument &) {
    throw;
  } catch (const std::exception &e) {
    throw ApiError(MMSBM_E_HIP, std::string("device layout: ") + e.what());
  } catch (...) {
    throw ApiError(MMSBM_E_INTERNAL, "device layout: unknown exception (not derived from std::exception)");
  }
  c->pair_user.ptr = dev_idx.pair_user; c->pair_user.count = static_cast<size_t>(n_obs);
  c->user_pair.ptr = dev_idx.user_pair; c->user_pair.count = static_cast<size_t>(n_obs);
  mmsbm::finish_layout(c->lay, 512);
  lap("device layout (sorts)");
  return true;
}

// The pair stage's plan applied to the index: the unit list rebuilt to the plan's chunk length.  Returns the 64-pair units
// as the layout built them: the likelihood (likelihood_units_kernel: <= 64 pairs) keeps that list whatever replaces it
// here or in build_fused_lists().
std::vector<mmsbm::Chunk> apply_pair_plan(mmsbm_hip_ctx *c, const PairPlan &plan) {
  std::vector<mmsbm::Chunk> units64 = c->lay.mv_chunks;
  c->n_lik_units = static_cast<int>(units64.size());
  c->pp = plan;
  if (plan.wide || plan.big_tile()) mmsbm::build_mv_chunks(c->lay, plan.chunk_pairs);
  c->n_pairs = c->lay.n_pairs;
  c->n_chunks = static_cast<int>(c->lay.mv_chunks.size());
  return units64;
}

// Dense data: XCD-local work lists (layout.hpp) -- every segment cut at fixed borders of the gathered index, each
// range's work on one XCD, whose L2 then holds that slice of the table
void build_range_worklists(mmsbm_hip_ctx *c, const CreateKnobs &knobs, bool gpu_layout) {
  if (c->kp > kMaxGroupRow) {  // rows beyond the widest group-of-lanes instantiation: seg_wide_kernel, whole segments
    c->lay.pair_work = mmsbm::WorkList();
    c->lay.user_work = mmsbm::WorkList();
    return;
  }
  if (knobs.no_ranges) return;
  const int64_t n_obs = c->n_obs;
  const int per = kBlock / group_lanes(c->code_k);
  const size_t row_bytes = static_cast<size_t>(c->kp) * sizeof(double);
  const int64_t mean_p = c->n_pairs > 0 ? n_obs / c->n_pairs : 0, mean_u = n_obs / std::max(c->n_users, 1);
  int rp = mmsbm::range_count(static_cast<size_t>(c->n_users) * row_bytes, mean_p);   // pair pass gathers theta
  int ru = mmsbm::range_count(static_cast<size_t>(c->n_pairs) * row_bytes, mean_u);   // user pass gathers A
  // ... unless the table's hot rows (what one L2 keeps by itself) already take most of the gathers:
  // theta rows are gathered once per triple of that user, A rows once per triple of that pair
  // Where the rows one L2 keeps by itself already take half of the gathers (heavy-tailed gather
  // counts, or a table only a few times an L2) there is little left to win: measured +16 % (50M
  // ratings, log-normal item popularity, 8.5 MB table) and +24 % (Zipf(1.2) degrees) if cut anyway.
  const int64_t fit = static_cast<int64_t>(mmsbm::kRangeSliceBytes / row_bytes);
  if (rp > 1 && mmsbm::hot_fraction(c->lay.user_off, fit) > 0.5) rp = 1;
  if (ru > 1 && mmsbm::hot_fraction(c->lay.pair_off, fit) > 0.5) ru = 1;
  if (knobs.ranges_pairs > 0) { rp = knobs.ranges_pairs; ru = knobs.ranges_users; }
  // (device layout: the index arrays live on the device, so the borders are found there and only the
  // cut positions -- segments x (ranges + 1) integers -- come back)
  std::vector<int32_t> cuts_p, cuts_u;
  if (gpu_layout && rp > 1) cuts_p = mmsbm::gpu_layout::range_cuts(c->stream, c->lay.pair_off, c->pair_user.ptr, c->n_users, rp);
  if (gpu_layout && ru > 1) cuts_u = mmsbm::gpu_layout::range_cuts(c->stream, c->lay.user_off, c->user_pair.ptr, c->n_pairs, ru);
  if (rp > 1)
    mmsbm::build_worklist_ranges(c->lay.pair_off, c->lay.pair_user.data(), c->n_users, rp,
                                 mmsbm::item_length(n_obs, c->n_pairs), per, c->lay.pair_work,
                                 gpu_layout ? cuts_p.data() : nullptr);
  if (ru > 1)
    mmsbm::build_worklist_ranges(c->lay.user_off, c->lay.user_pair.data(), c->n_pairs, ru,
                                 mmsbm::item_length(n_obs, c->n_users), per, c->lay.user_work,
                                 gpu_layout ? cuts_u.data() : nullptr);
  c->ranges_pairs = rp;
  c->ranges_users = ru;
}

// The facts about the data that the form of an iteration is decided by (step_plan.hpp), once the pair stage's plan and
// the work lists stand; build_fused_lists() adds the whole-segment lists it builds
void plan_step(mmsbm_hip_ctx *c) {
  StepPlan &s = c->step;
  s.n_obs = c->n_obs; s.kp = c->kp; s.lp = c->lp; s.code_k = c->code_k; s.code_l = c->code_l; s.n_chunks = c->n_chunks;
  s.items_pairs = !c->lay.pair_work.items.empty(); s.items_users = !c->lay.user_work.items.empty();
  s.cut_pairs = !c->lay.pair_work.splits.empty(); s.cut_users = !c->lay.user_work.splits.empty();
}

// Whole pair segments for the workgroups of the two-launch form: the 64-pair units rebuilt with at most 64 work items
// each.  The capped unit list REPLACES the plain one -- both forms of the iteration then run it, so that their S sums
// associate the same way -- but only once it is certain that the two-launch form can use it: a pair of more than 64
// pieces, or partial rows beyond the LDS, and the plain list is back.
void build_fused_pair_lists(mmsbm_hip_ctx *c) {
  const mmsbm::SegPieces sp = mmsbm::segment_pieces(c->lay.pair_off, c->lay.pair_work);
  const std::vector<mmsbm::Chunk> plain_chunks = c->lay.mv_chunks;
  const std::vector<int32_t> plain_off = c->lay.mv_chunk_off;
  if (mmsbm::build_mv_chunks_capped(c->lay, sp, mmsbm::kMvChunkPairs, kUnitPairs)) {
    const mmsbm::FusedLists fl = mmsbm::build_fused_pairs(c->lay, sp);
    if (pairs_fused_lds(c->kp, c->lp, fl.max_parts) <= kLdsMax) {
      c->fp_units.upload(fl.units, c->stream); c->fp_items.upload(fl.items, c->stream);
      c->fp_splits.upload(fl.splits, c->stream);
      HIP_CHECK(hipStreamSynchronize(c->stream));  // (`fl` is a local)
      c->fp_max_parts = fl.max_parts;
      c->step.fs_pairs = true;
    }
  }
  if (!c->step.fs_pairs) { c->lay.mv_chunks = plain_chunks; c->lay.mv_chunk_off = plain_off; }
  c->n_chunks = c->step.n_chunks = static_cast<int>(c->lay.mv_chunks.size());  // (either list)
}
// ... and whole user segments: a user whose pieces' partial rows exceed the LDS budget leaves the data with the
// separate launches
void build_fused_user_lists(mmsbm_hip_ctx *c, const CreateKnobs &knobs) {
  const mmsbm::SegPieces sp = mmsbm::segment_pieces(c->lay.user_off, c->lay.user_work);
  // work items per workgroup: one round of its groups of lanes
  const int ucap = knobs.fused_ucap > 0 ? knobs.fused_ucap : kBlock / group_lanes(c->code_k);
  const mmsbm::FusedLists fl = mmsbm::build_fused_users(sp, ucap);
  if (static_cast<size_t>(fl.max_parts) * c->kp * sizeof(double) > kFusedSplitLds) return;
  c->fu_units.upload(fl.units, c->stream); c->fu_items.upload(fl.items, c->stream);
  c->fu_splits.upload(fl.splits, c->stream);
  HIP_CHECK(hipStreamSynchronize(c->stream));  // (`fl` is a local)
  c->fu_max_parts = fl.max_parts;
  c->fu_blocks = static_cast<int>(fl.units.size());
  c->step.fs_users = true;
}
// Small problems with uneven degrees (round 4): their segments are cut into pieces by build_range_worklists(); give
// every workgroup of the two-launch form WHOLE segments (layout.hpp: FusedLists) so that the pieces' partial rows meet
// in its LDS instead of in a combine launch.
void build_fused_lists(mmsbm_hip_ctx *c, const CreateKnobs &knobs, CreateLaps &lap) {
  if (!c->step.lists_wanted(c->pp) || knobs.no_fused_split) return;
  if (c->step.cut_pairs) build_fused_pair_lists(c);
  if (c->step.cut_users) build_fused_user_lists(c, knobs);
  lap("whole-segment lists (two launches)");
}

// At least half of all (item, rating) combinations occur and R is small: a fixed-width grid of pair ids
void upload_item_grid(mmsbm_hip_ctx *c) {
  const int n_ratings = c->n_ratings;
  if (n_ratings > 16 || static_cast<int64_t>(c->n_pairs) * 2 < static_cast<int64_t>(c->n_items) * n_ratings) return;
  std::vector<int32_t> grid(static_cast<size_t>(c->n_items) * n_ratings, -1);
  for (int r = 0; r < n_ratings; ++r)
    for (int32_t q = c->lay.rating_off[static_cast<size_t>(r)]; q < c->lay.rating_off[static_cast<size_t>(r) + 1]; ++q)
      grid[static_cast<size_t>(c->lay.pair_item[static_cast<size_t>(q)]) * n_ratings + r] = q;
  c->item_grid.upload(grid, c->stream);
  HIP_CHECK(hipStreamSynchronize(c->stream));  // `grid` is a local
}

// Everything the kernels index by, onto the device.  After the host's sorts (`gpu_layout` false) that includes
// pair_user, user_pair and the id columns; the device's sorts left all five in place (build_index).
void upload_index(mmsbm_hip_ctx *c, const CreateKnobs &knobs, bool gpu_layout, const std::vector<mmsbm::Chunk> &units64,
                  const int32_t *iu, const int32_t *ii, const int32_t *rating) {
  hipStream_t s = c->stream;
  c->pair_off.upload(c->lay.pair_off, s);
  c->pair_item.upload(c->lay.pair_item, s);
  c->user_off.upload(c->lay.user_off, s);
  if (!gpu_layout) {
    c->pair_user.upload(c->lay.pair_user, s);
    c->user_pair.upload(c->lay.user_pair, s);
  }
  c->item_off.upload(c->lay.item_off, s);
  c->item_pairs.upload(c->lay.item_pairs, s);
  c->item_deg.upload(c->lay.item_deg, s);
  if (!knobs.no_itemgrid) upload_item_grid(c);
  c->mv_chunks.upload(c->lay.mv_chunks, s);
  build_a_runs(c, 0);
  c->lik_units.upload(units64, s);
  c->mv_chunk_off.upload(c->lay.mv_chunk_off, s);
  c->pair_items.upload(c->lay.pair_work.items, s);
  c->user_items.upload(c->lay.user_work.items, s);
  c->pair_splits.upload(c->lay.pair_work.splits, s);
  c->user_splits.upload(c->lay.user_work.splits, s);
  if (!gpu_layout && c->n_obs > 0) upload_ids(c, iu, ii, rating);
  HIP_CHECK(hipStreamSynchronize(s));  // nothing of the caller's (or create's) host memory is still being read
}

// (Re)allocate the per-restart state for `slots` parameter sets; nothing is kept.
void alloc_state(mmsbm_hip_ctx *c, int slots) {
  hipStream_t s = c->stream;
  HIP_CHECK(hipStreamSynchronize(s));
  c->drop_graphs();
  const size_t klr = static_cast<size_t>(c->n_ratings) * c->kp * c->lp;
  auto zeroed = [&](SlotBuf &b, size_t per_slot) {
    b.alloc_slots(per_slot, slots);
    HIP_CHECK(hipMemsetAsync(b.ptr, 0, sizeof(double) * std::max<size_t>(b.count, 1), s));
  };
  for (int b = 0; b < 2; ++b) {
    zeroed(c->theta[b], static_cast<size_t>(c->n_users) * c->kp);
    zeroed(c->eta[b], static_cast<size_t>(c->n_items) * c->lp);
    zeroed(c->p[b], klr);
    zeroed(c->pt[b], klr);
    zeroed(c->atab[b], static_cast<size_t>(c->n_pairs) * c->kp);
  }
  // (the scratch tables too: every entry a kernel reads is written by the launch before it -- audited, EXPERIMENTS.md
  // -- but padding rows and the slabs of empty units then hold zeros rather than whatever the pages held before)
  zeroed(c->ctab, static_cast<size_t>(c->n_pairs) * c->kp);
  zeroed(c->ttab, static_cast<size_t>(c->n_pairs) * c->lp);
  zeroed(c->partial, c->lay.mv_chunks.size() * c->kp * c->lp);
  zeroed(c->npr, klr);
  zeroed(c->pair_parts, static_cast<size_t>(c->lay.pair_work.n_parts) * c->kp);
  zeroed(c->user_parts, static_cast<size_t>(c->lay.user_work.n_parts) * c->kp);
  HIP_CHECK(hipStreamSynchronize(s));
  c->n_slots = slots;
  c->sel = 0;
  c->base_slot = 0;
  c->launch_slots = slots;
  c->cur = 0;
  c->have.assign(static_cast<size_t>(slots), 0);
  c->a_ok.assign(static_cast<size_t>(slots), 0);
}

}  // namespace

mmsbm_hip_ctx *context_create(int device, int64_t n_obs, int32_t n_users, int32_t n_items, int32_t n_ratings,
                              int32_t k_groups, int32_t l_groups, const int32_t *user, const int32_t *item,
                              const int32_t *rating, int swap_sides) {
  const CreateKnobs knobs = read_create_knobs();
  CreateLaps lap{knobs.timing};
  std::unique_ptr<mmsbm_hip_ctx> c(new mmsbm_hip_ctx());
  plan_sides(c.get(), device, n_obs, n_users, n_items, n_ratings, k_groups, l_groups, swap_sides);
  const auto [iu, ii] = internal_sides(c.get(), user, item);  // the id columns of the internal sides
  const PairPlan shape = plan_pair_shape(c->kp, c->lp, knobs.force_wide);
  lap("checks");
  open_device(c.get());
  const bool gpu_layout = build_index(c.get(), knobs, iu, ii, rating, lap);
  c->gpu_layout = gpu_layout;
  const std::vector<mmsbm::Chunk> units64 =
      apply_pair_plan(c.get(), plan_pair_forms(shape, c->lay.n_pairs, c->n_cus, knobs.no_mfma, knobs.mfma_chunk));
  build_range_worklists(c.get(), knobs, gpu_layout);
  lap("xcd-local work lists");
  plan_step(c.get());
  build_fused_lists(c.get(), knobs, lap);
  // small problems (where eight rows in flight pay, plan_sides): two launches per iteration instead of four
  c->step.fused = c->step.fused_default(c->pp, knobs.no_fused);
  upload_index(c.get(), knobs, gpu_layout, units64, iu, ii, rating);
  lap("index uploads");
  alloc_state(c.get(), 1);
  c->lik_part.alloc(4096);
  HIP_CHECK(hipStreamSynchronize(c->stream));
  lap("state allocation");
  return c.release();
}

void set_slots(mmsbm_hip_ctx *ctx, int n_slots) {
  HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (a snapshot copy may still be on its way)
  ctx->drop_snapshots();
  if (n_slots == ctx->n_slots) {
    ctx->have.assign(static_cast<size_t>(n_slots), 0);
    ctx->a_ok.assign(static_cast<size_t>(n_slots), 0);
    ctx->sel = 0;
    return;
  }
  try {
    alloc_state(ctx, n_slots);
  } catch (...) {  // most likely out of device memory: leave a consistent one-slot context
    (void)hipGetLastError();
    try { alloc_state(ctx, 1); } catch (...) {}
    throw;
  }
}

// What has a device buffer is read back from it (the device-built pair_user / user_pair exist nowhere else); rating_off,
// chunk_off and chunks are host-only members of the context.
void index_array(mmsbm_hip_ctx *ctx, int which, int32_t *out, int64_t capacity, int64_t *count) {
  const mmsbm::Layout &L = ctx->lay;
  const int32_t *host = nullptr;
  const void *dev = nullptr;
  size_t n = 0;  // in int32
  auto from_dev = [&](const auto &buf) {
    dev = buf.ptr;
    n = buf.count * (sizeof(*buf.ptr) / sizeof(int32_t));
  };
  switch (which) {
    case 0: from_dev(ctx->pair_off); break;
    case 1: from_dev(ctx->pair_user); break;
    case 2: from_dev(ctx->pair_item); break;
    case 3: host = L.rating_off.data(); n = L.rating_off.size(); break;
    case 4: from_dev(ctx->user_off); break;
    case 5: from_dev(ctx->user_pair); break;
    case 6: from_dev(ctx->item_off); break;
    case 7: from_dev(ctx->item_pairs); break;
    case 8: from_dev(ctx->item_deg); break;
    case 9: host = L.chunk_off.data(); n = L.chunk_off.size(); break;
    case 10: host = reinterpret_cast<const int32_t *>(L.chunks.data()); n = L.chunks.size() * 4; break;
    case 11: from_dev(ctx->mv_chunks); break;
    case 12: from_dev(ctx->pair_items); break;
    case 13: from_dev(ctx->user_items); break;
    case 14: from_dev(ctx->pair_splits); break;
    case 15: from_dev(ctx->user_splits); break;
    case 16: from_dev(ctx->item_grid); break;
    case 17: from_dev(ctx->lik_units); break;
    case 18: from_dev(ctx->mv_chunk_off); break;
    default: throw std::invalid_argument("unknown index array");
  }
  *count = static_cast<int64_t>(n);
  if (!out) return;
  if (capacity < *count) throw std::invalid_argument("buffer too small");
  if (n == 0) return;
  if (host) {
    std::memcpy(out, host, sizeof(int32_t) * n);
    return;
  }
  use_device(ctx);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  HIP_CHECK(hipMemcpy(out, dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
}

}  // namespace mmsbm_hip_impl
