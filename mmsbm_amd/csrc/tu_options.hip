// tu_options.hip -- the options: one row per name.  get: its value now; set: null for a read-only name, else the value's
// check and what setting it does.  mmsbm_hip_get_option and mmsbm_hip_set_option both walk this table and nothing else.
// Host code only.
#include "prelude.hpp"

namespace mmsbm_hip_impl {

namespace {

struct Option {
  const char *name;
  double (*get)(const mmsbm_hip_ctx *);
  void (*set)(mmsbm_hip_ctx *, double);
};
using Ctx = mmsbm_hip_ctx;
// "audience_rows" / "audience_entries" / "explain_rows" / "diverse_rows" / "group_run_blocks" / "assortment_run_blocks" / "assortment_part_bytes": 0 .. 2^31 - 1, whole
void set_audience(int64_t &field, const char *name, double v) {
  if (v < 0 || v > 2147483647.0 || v != std::floor(v)) throw std::invalid_argument(std::string(name) + ": 0 .. 2^31 - 1");
  field = static_cast<int64_t>(v);
}
const Option kOptions[] = {
    {"graph", [](const Ctx *c) -> double { return c->graph_mode; }, [](Ctx *c, double v) { c->graph_mode = v != 0.0; }},
    // 0: the A launch through pair_block like every other shape
    // (create() also requires unit runs of four -- big_chunk == 4 * kMvChunkPairs, plan_pair_forms -- and this option
    // never has: with longer runs it turns on what create() left off.  Whether that is meant is open; both are as they were)
    {"quad", [](const Ctx *c) -> double { return c->pp.quad_a; }, [](Ctx *c, double v) { c->pp.set_quad(v != 0.0); }},
    // the pair stage on the matrix cores: 0 off, 1 on (one-block form if K, L <= 64, else the blocked form), 2 the
    // blocked form whatever the shape
    {"mfma", [](const Ctx *c) -> double { return c->pp.mfma ? 1.0 : (c->pp.mfma_big ? 2.0 : 0.0); },
     [](Ctx *c, double v) { c->pp.set_mfma(v); }},
    // 0: prod_dist / predict through the per-row kernels (R K L multiply-adds per row)
    {"predict_fast", [](const Ctx *c) -> double { return c->predict_fast; }, [](Ctx *c, double v) { c->predict_fast = v != 0.0; }},
    // two launches per iteration (small tiles, unsplit segments); any problem size
    {"fused", [](const Ctx *c) -> double { return c->step.fused; },
     [](Ctx *c, double v) { c->step.set_fused(v != 0.0, c->step.two_possible(c->pp)); }},
    // 0: plain stores for every output row; bits: 1 T and A rows, 2 theta' rows, 4 own-row loads.  Reads as what is in use
    {"nt_out", [](const Ctx *c) -> double { return nt_on(c); },
     [](Ctx *c, double v) {
       if (v < 0 || v > 15) throw std::invalid_argument("nt_out: 0 .. 15");
       c->nt_out = static_cast<int>(v);
     }},
    // device time of the last call's kernels (TimedCall, context.hpp)
    {"recommend_ms", [](const Ctx *c) -> double { return c->last_ms[T_RECOMMEND]; }, nullptr},
    {"fold_in_ms", [](const Ctx *c) -> double { return c->last_ms[T_FOLD_IN]; }, nullptr},
    {"position_ms", [](const Ctx *c) -> double { return c->last_ms[T_POSITIONS]; }, nullptr},
    {"similar_ms", [](const Ctx *c) -> double { return c->last_ms[T_SIMILAR]; }, nullptr},
    {"top_pairs_ms", [](const Ctx *c) -> double { return c->last_ms[T_TOP_PAIRS]; }, nullptr},
    {"overlap_ms", [](const Ctx *c) -> double { return c->last_ms[T_OVERLAP]; }, nullptr},
    {"heldout_ms", [](const Ctx *c) -> double { return c->last_ms[T_HELDOUT]; }, nullptr},
    {"audience_ms", [](const Ctx *c) -> double { return c->last_ms[T_AUDIENCE]; }, nullptr},
    {"explain_ms", [](const Ctx *c) -> double { return c->last_ms[T_EXPLAIN]; }, nullptr},
    {"diverse_ms", [](const Ctx *c) -> double { return c->last_ms[T_DIVERSE]; }, nullptr},
    {"inform_ms", [](const Ctx *c) -> double { return c->last_ms[T_INFORM]; }, nullptr},
    {"group_ms", [](const Ctx *c) -> double { return c->last_ms[T_GROUP]; }, nullptr},
    {"ensemble_ms", [](const Ctx *c) -> double { return c->last_ms[T_ENSEMBLE]; }, nullptr},
    // ... of the last loo_add or loo query (loo.hpp); of the last loo_add alone: its sums pass and its row pass
    {"loo_ms", [](const Ctx *c) -> double { return c->last_ms[T_LOO]; }, nullptr},
    {"loo_sums_ms", [](const Ctx *c) -> double { return c->last_ms[T_LOO_SUMS]; }, nullptr},
    {"loo_rows_ms", [](const Ctx *c) -> double { return c->last_ms[T_LOO_ROWS]; }, nullptr},
    // ... of the last recommend_allocate as a whole (allocate.hpp), and the rounds it took
    {"allocate_ms", [](const Ctx *c) -> double { return c->last_ms[T_ALLOCATE]; }, nullptr},
    // ... of the last top_pairs_bulk / pair_bar as a whole (pairs_bulk.hpp), the histogram passes it ran and the keys it
    // collected when it stopped early (0: it did not)
    {"pairs_bulk_ms", [](const Ctx *c) -> double { return c->last_ms[T_TOP_PAIRS_BULK]; }, nullptr},
    {"pairs_bulk_passes", [](const Ctx *c) -> double { return c->pb_passes; }, nullptr},
    {"pairs_bulk_collected", [](const Ctx *c) -> double { return static_cast<double>(c->pb_collected); }, nullptr},
    {"allocate_rounds", [](const Ctx *c) -> double { return c->alloc_rounds; }, nullptr},
    // ... of the last recommend_assortment as a whole (assortment.hpp) and, of its rounds while "assortment_timing" is
    // set (events between the phases of every round), of the gain + join, the pick and the update kernels
    {"assortment_ms", [](const Ctx *c) -> double { return c->last_ms[T_ASSORT]; }, nullptr},
    {"assortment_gain_ms", [](const Ctx *c) -> double { return c->asrt_ms[0]; }, nullptr},
    {"assortment_pick_ms", [](const Ctx *c) -> double { return c->asrt_ms[1]; }, nullptr},
    {"assortment_update_ms", [](const Ctx *c) -> double { return c->asrt_ms[2]; }, nullptr},
    {"assortment_timing", [](const Ctx *c) -> double { return c->asrt_timing; }, [](Ctx *c, double v) { c->asrt_timing = v != 0.0; }},
    // ... of the last recommend_assign as a whole (assign.hpp), its rounds and the bids of all of them
    {"assign_ms", [](const Ctx *c) -> double { return c->last_ms[T_ASSIGN]; }, nullptr},
    {"assign_rounds", [](const Ctx *c) -> double { return c->asg_rounds; }, nullptr},
    {"assign_bids", [](const Ctx *c) -> double { return static_cast<double>(c->asg_bids); }, nullptr},
    // workgroups of gtop_fused_kernel (top_pairs.hpp); 0: the library's choice
    {"top_pairs_groups", [](const Ctx *c) -> double { return c->top_groups; },
     [](Ctx *c, double v) {
       if (v < 0 || v > 4096 || v != std::floor(v)) throw std::invalid_argument("top_pairs_groups: 0 .. 4096");
       c->top_groups = static_cast<int>(v);
     }},
    // top_pairs_bulk (pairs_bulk.hpp): workgroups of its tile launches and bits per digit of the select (0: the library's
    // choice); the bin size at which the select stops and sorts the bin (0: never).  None changes the answer
    {"pairs_bulk_groups", [](const Ctx *c) -> double { return c->pb_groups; },
     [](Ctx *c, double v) {
       if (v < 0 || v > kPbMaxGroups || v != std::floor(v)) throw std::invalid_argument("pairs_bulk_groups: 0 .. 4096");
       c->pb_groups = static_cast<int>(v);
     }},
    {"pairs_bulk_bits", [](const Ctx *c) -> double { return c->pb_bits; },
     [](Ctx *c, double v) {
       if (v < 0 || v > kPbDevMaxBits || v != std::floor(v)) throw std::invalid_argument("pairs_bulk_bits: 0 .. 12");
       c->pb_bits = static_cast<int>(v);
     }},
    {"pairs_bulk_collect", [](const Ctx *c) -> double { return static_cast<double>(c->pb_collect); },
     [](Ctx *c, double v) {
       if (v < 0 || v > static_cast<double>(kPbMaxCollect) || v != std::floor(v)) throw std::invalid_argument("pairs_bulk_collect: 0 .. 2^24");
       c->pb_collect = static_cast<int64_t>(v);
     }},
    // recommend_audience (audience.hpp): items per COUNT batch, entries per WRITE batch at most; 0: the library's choice.
    // Neither changes the answer
    {"audience_rows", [](const Ctx *c) -> double { return static_cast<double>(c->aud_rows); },
     [](Ctx *c, double v) { set_audience(c->aud_rows, "audience_rows", v); }},
    {"audience_entries", [](const Ctx *c) -> double { return static_cast<double>(c->aud_entries); },
     [](Ctx *c, double v) { set_audience(c->aud_entries, "audience_entries", v); }},
    // explain_query (explain.hpp): training rows per batch; 0: the library's choice.  It does not change the answer
    {"explain_rows", [](const Ctx *c) -> double { return static_cast<double>(c->exp_rows); },
     [](Ctx *c, double v) { set_audience(c->exp_rows, "explain_rows", v); }},
    // recommend_diverse (diverse.hpp): request rows per call; 0: the library's choice.  It does not change the answer
    {"diverse_rows", [](const Ctx *c) -> double { return static_cast<double>(c->div_rows); },
     [](Ctx *c, double v) { set_audience(c->div_rows, "diverse_rows", v); }},
    // recommend_query_groups (group.hpp): blocks of 8 member rows per run of groups, rounded up to whole steps of 16; a
    // longer group is cut into fragments of that length.  0: the library's choice.  It does not change the answer
    {"group_run_blocks", [](const Ctx *c) -> double { return static_cast<double>(c->grp_run); },
     [](Ctx *c, double v) { set_audience(c->grp_run, "group_run_blocks", v); }},
    // recommend_assortment (assortment.hpp): blocks of 8 user rows per run, rounded up to whole steps of 16.  0: the
    // library's choice.  REACH does not depend on it; BEST may differ in the last bits of a gain sum
    {"assortment_run_blocks", [](const Ctx *c) -> double { return static_cast<double>(c->asrt_run); },
     [](Ctx *c, double v) { set_audience(c->asrt_run, "assortment_run_blocks", v); }},
    // ... and the bytes of the runs' partial sums per batch of item tiles (0: 64 MB).  It does not change the answer
    {"assortment_part_bytes", [](const Ctx *c) -> double { return static_cast<double>(c->asrt_part); },
     [](Ctx *c, double v) { set_audience(c->asrt_part, "assortment_part_bytes", v); }},
    // the form FAMILY of an iteration at the current slot count: 2 = the two launches of fused_small.hpp, 4 = the separate
    // stages, with or without "pass_dense" -- the launches a committed iteration really takes are launches - pass_dense
    {"launches", [](const Ctx *c) -> double { return StepPlan::launches_family(c->form(true)); }, nullptr},
    // the triple passes and the T + S stage of a committed iteration in one launch (pass_dense.hpp).  Set: -1 the
    // library's choice by size, 0 off, 1 on wherever the form applies.  Reads 1 when the next committed iteration takes it
    {"pass_dense", [](const Ctx *c) -> double { return c->form(true) == StepForm::Three ? 1 : 0; },
     [](Ctx *c, double v) { c->step.set_pass_dense(v); }},
    {"wide", [](const Ctx *c) -> double { return c->pp.wide; }, nullptr},
    // 0: a logarithm per element; 1: logarithm tables, a group of lanes per triple; 2: where it applies a wave per pair
    // (lik_fact.hpp), else as 1
    {"lik_fast", [](const Ctx *c) -> double { return c->lik_mode; },
     [](Ctx *c, double v) {
       if (v != 0.0 && v != 1.0 && v != 2.0) throw std::invalid_argument("lik_fast: 0, 1 or 2");
       c->lik_mode = static_cast<int>(v);
     }},
    {"lik_g", [](const Ctx *c) -> double { return c->lik_g; },
     [](Ctx *c, double v) {
       const int g = static_cast<int>(v);
       if (g != 0 && g != 1 && g != 2 && g != 4 && g != 8) throw std::invalid_argument("lik_g: 0, 1, 2, 4 or 8");
       c->lik_g = g;
     }},
    {"ranges_pairs", [](const Ctx *c) -> double { return c->ranges_pairs; }, nullptr},  // XCD-local work lists,
    {"ranges_users", [](const Ctx *c) -> double { return c->ranges_users; }, nullptr},  // ranges per pass (1 = off)
    {"chunk_pairs", [](const Ctx *c) -> double { return c->pp.chunk_pairs; }, nullptr},  // pairs per pair-stage workgroup at most
    {"n_chunks", [](const Ctx *c) -> double { return c->n_chunks; }, nullptr},  // pair-stage workgroups (= slabs), padding included
    // 64-pair units per workgroup of the matrix-core A launch (reads 0: not on the matrix cores; set 0: the library's own balance)
    {"a_units", [](const Ctx *c) -> double { return c->a_units; },
     [](Ctx *c, double v) {
       if (v < 0 || v > kMfmaChunkPairs / kUnitPairs) throw std::invalid_argument("a_units: 0 .. 16");
       use_device(c);
       HIP_CHECK(hipStreamSynchronize(c->stream));
       build_a_runs(c, static_cast<int>(v));
     }},
    // workgroups of the matrix-core A launch when it walks runs of its own (0: the T + S launch's)
    {"a_chunks", [](const Ctx *c) -> double { return c->n_a_chunks; }, nullptr},
    {"items_pairs", [](const Ctx *c) -> double { return static_cast<double>(c->lay.pair_work.items.size()); }, nullptr},
    {"items_users", [](const Ctx *c) -> double { return static_cast<double>(c->lay.user_work.items.size()); }, nullptr},
    // segments cut into pieces
    {"splits_pairs", [](const Ctx *c) -> double { return static_cast<double>(c->lay.pair_work.splits.size()); }, nullptr},
    {"splits_users", [](const Ctx *c) -> double { return static_cast<double>(c->lay.user_work.splits.size()); }, nullptr},
    // whole-segment lists built (1 pair side, 2 user side)
    {"fused_split", [](const Ctx *c) -> double { return (c->step.fs_pairs ? 1 : 0) + (c->step.fs_users ? 2 : 0); }, nullptr},
    // item_sum walks the fixed-width grid of pair ids (tu_create.hip: upload_item_grid)
    {"item_grid", [](const Ctx *c) -> double { return c->item_grid.count ? 1 : 0; }, nullptr},
    // the index's sorts ran on the device (tu_create.hip: build_index)
    {"gpu_layout", [](const Ctx *c) -> double { return c->gpu_layout ? 1 : 0; }, nullptr},
};
const Option *find_option(const std::string &name) {
  for (const Option &o : kOptions)
    if (name == o.name) return &o;
  return nullptr;
}

}  // namespace

// A successful set drops the captured graphs: they hold the launches of the plan they were captured under
void set_option(mmsbm_hip_ctx *ctx, const std::string &name, double value) {
  const Option *o = find_option(name);
  if (!o || !o->set) throw std::invalid_argument("unknown option: " + name);
  o->set(ctx, value);
  ctx->drop_graphs();
}

double get_option(const mmsbm_hip_ctx *ctx, const std::string &name) {
  const Option *o = find_option(name);
  if (!o) throw std::invalid_argument("unknown option: " + name);
  return o->get(ctx);
}

}  // namespace mmsbm_hip_impl
