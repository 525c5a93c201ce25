// Host-only check of mmsbm_amd/csrc/step_plan.hpp, built with -fsanitize=address,undefined by
// tests/test_step_plan_cpu.py.  The form of an EM iteration -- two, three or four launches -- was decided by five free
// predicates over the context until StepPlan took their place; they are transcribed below, literally, over a plain
// struct of the facts they read (Parent): the reference.  For every padded shape of K, L = 1 .. 80, under the pair
// stage's real plans (as created, and after options "mfma" and "quad"), crossed with every fact about the data, every
// ask, the restart slots of a launch and ratings placed on both sides of each size threshold, StepPlan must answer what
// the predicates answered -- the form, and everything the iteration, its timers and the options derived from it.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../mmsbm_amd/csrc/layout.hpp"
#include "../../mmsbm_amd/csrc/shapes.hpp"
#include "../../mmsbm_amd/csrc/pair_plan.hpp"
#include "../../mmsbm_amd/csrc/step_plan.hpp"

using namespace mmsbm_hip_impl;

// ---- the parent commit's rules (tu_iterate.hip, tu_create.hip, tu_options.hip before step_plan.hpp) ----------------------
namespace parent {

constexpr long long kFusedRatingsMax = 1500000;
constexpr long long kFusedWorkMax = 14000000, kFusedWorkMaxSplit = 18000000;
constexpr long long kPassDenseWorkMin = 20000000;

struct Work { bool items_empty, splits_empty; };
struct Ctx {   // the fields of mmsbm_hip_ctx the predicates read; pp_*: the two answers of its PairPlan
  bool fused, fused_forced;
  int pass_dense;
  bool fs_pairs, fs_users;
  int launch_slots;
  int64_t n_obs;
  int kp, lp, code_k, code_l, n_chunks;
  Work pair_work, user_work;
  bool pp_fused_shape_ok, pp_pass_dense_shape_ok;
};

bool fused_shape_ok(const Ctx *c) { return c->code_k <= 1 && c->code_l <= 1 && c->n_chunks > 0 && c->pp_fused_shape_ok; }
bool fused_possible(const Ctx *c) {
  return fused_shape_ok(c) && (c->pair_work.splits_empty || c->fs_pairs) && (c->user_work.splits_empty || c->fs_users);
}
bool pass_dense_possible(const Ctx *c) {
  return c->launch_slots == 1 && c->code_k == 1 && c->code_l <= 1 && c->n_chunks > 0 && c->pp_pass_dense_shape_ok &&
         c->pair_work.items_empty && c->user_work.items_empty && c->pair_work.splits_empty && c->user_work.splits_empty;
}
bool use_fused(const Ctx *c) {
  const bool cut = !c->pair_work.splits_empty || !c->user_work.splits_empty;
  if (c->pass_dense == 1 && !c->fused_forced && pass_dense_possible(c)) return false;
  return c->fused && fused_possible(c) &&
         (c->fused_forced || c->n_obs * c->launch_slots * (c->kp + c->lp) <= (cut ? kFusedWorkMaxSplit : kFusedWorkMax));
}
bool use_pass_dense(const Ctx *c) {
  if (c->pass_dense == 0 || use_fused(c) || !pass_dense_possible(c)) return false;
  return c->pass_dense == 1 || c->n_obs * (c->kp + c->lp) >= kPassDenseWorkMin;
}

// What the callers made of the two answers (asked once per grid point below: the callers asked again at every site).
struct Use { bool fused, pass_dense; };
// launch_iteration: the launches it made, and a_ok of the launch's slots when it returned
StepForm launched(Use use, bool commit) {
  if (use.fused) return StepForm::Two;
  return (commit && use.pass_dense) ? StepForm::Three : StepForm::Four;
}
bool ensured_a(Use use) { return !use.fused; }   // ... and run_iterations before a capture
bool a_ok_after(Use use, bool commit) {
  if (use.fused) return !commit;   // mark_a(c, !commit)
  return true;                     // ensure_a, then (commit) mark_a(c, true)
}
bool a_ok_after_replay(Use use) { return !use.fused; }
// time_stage returned 0 us without a launch, kernel_bytes 0 bytes
bool stage_skipped(Use use, int stage) { return use.pass_dense && stage == K_DENSE; }
int launches_option(Use use) { return use.fused ? 2 : 4; }
int pass_dense_option(Use use) { return use.pass_dense ? 1 : 0; }
// create(): build_fused_lists went on (knob no_fused_split apart); the default of `fused` (knob no_fused apart)
bool lists_built(const Ctx *c) {
  const bool cut_p = !c->pair_work.splits_empty, cut_u = !c->user_work.splits_empty;
  return !(c->n_obs > kFusedRatingsMax || !fused_shape_ok(c) || !(cut_p || cut_u));
}
bool fused_default(const Ctx *c) { return c->n_obs <= kFusedRatingsMax && fused_possible(c); }

}  // namespace parent

static long fails = 0;
static int g_kp = 0, g_lp = 0, g_variant = 0;
#define CHECK(x)                                                                                                 \
  do {                                                                                                           \
    if (!(x) && ++fails <= 20) std::printf("FAILED %s (kp %d, lp %d, plan variant %d) line %d\n", #x, g_kp, g_lp, g_variant, __LINE__); \
  } while (0)

static PairPlan variant_of(PairPlan p, int v) {
  switch (v) {
    case 1: p.set_mfma(0); break;
    case 2: p.set_mfma(1); break;
    case 3: p.set_mfma(2); break;
    case 4: p.set_quad(false); break;
    case 5: p.set_quad(true); break;
    default: break;
  }
  return p;
}

// ratings on both sides of every size threshold of the shape and slot count, ascending and distinct
static std::vector<int64_t> rating_counts(int kp, int lp, int slots) {
  std::vector<int64_t> n = {1000, parent::kFusedRatingsMax, parent::kFusedRatingsMax + 1};
  const int64_t per = static_cast<int64_t>(slots) * (kp + lp);
  for (long long t : {parent::kFusedWorkMax, parent::kFusedWorkMaxSplit, parent::kPassDenseWorkMin}) {
    // the largest count whose work is at or below the threshold and the smallest above it (<= kFusedWorkMax); the
    // smallest that reaches it and the one before (>= kPassDenseWorkMin): the same two unless the threshold is a multiple
    const int64_t at = t / per, up = (t + per - 1) / per;
    n.insert(n.end(), {at, at + 1, up - 1, up});
  }
  std::sort(n.begin(), n.end());
  n.erase(std::unique(n.begin(), n.end()), n.end());
  return n;
}

static int rank_of(StepForm f) { return f == StepForm::Two ? 0 : f == StepForm::Four ? 1 : 2; }

int main() {
  std::vector<int> dims;
  for (int d = 1; d <= 80; ++d)
    if (dims.empty() || dims.back() != pad_dim(d)) dims.push_back(pad_dim(d));
  long points = 0, plans = 0, reached[3] = {0, 0, 0}, walks = 0;
  for (int kp : dims)
    for (int lp : dims) {
      g_kp = kp; g_lp = lp;
      const PairPlan made = plan_pair_forms(plan_pair_shape(kp, lp, false), 50000, 256, false, 0);
      std::vector<PairPlan> seen;
      for (int variant = 0; variant < 6; ++variant) {
        g_variant = variant;
        const PairPlan pp = variant_of(made, variant);
        bool again = false;   // (an option that changed nothing: the same plan, checked already)
        for (const PairPlan &q : seen)
          again = again || (q.mfma == pp.mfma && q.mfma_big == pp.mfma_big && q.quad_a == pp.quad_a);
        if (again) continue;
        seen.push_back(pp);
        ++plans;
        for (int facts = 0; facts < (1 << 9); ++facts) {
          parent::Ctx ref{};
          StepPlan sp;
          ref.kp = sp.kp = kp; ref.lp = sp.lp = lp;
          ref.pp_fused_shape_ok = pp.two_shape_ok();
          ref.pp_pass_dense_shape_ok = pp.pass_dense_shape_ok();
          // the shape's own group codes, or (off) one no form but the separate launches takes
          ref.code_k = sp.code_k = (facts & 1) ? group_code(kp) : 2;
          ref.code_l = sp.code_l = (facts & 2) ? group_code(lp) : 2;
          sp.items_pairs = facts & 4; sp.items_users = facts & 8;
          sp.cut_pairs = facts & 16; sp.cut_users = facts & 32;
          ref.pair_work = {!sp.items_pairs, !sp.cut_pairs};
          ref.user_work = {!sp.items_users, !sp.cut_users};
          ref.fs_pairs = sp.fs_pairs = facts & 64; ref.fs_users = sp.fs_users = facts & 128;
          ref.n_chunks = sp.n_chunks = (facts >> 8) & 1;
          CHECK(sp.two_shape_ok(pp) == parent::fused_shape_ok(&ref));
          CHECK(sp.two_possible(pp) == parent::fused_possible(&ref));
          for (int slots : {1, 2, 16}) {
            ref.launch_slots = slots;
            const std::vector<int64_t> counts = rating_counts(kp, lp, slots);
            for (int ask = 0; ask < 12; ++ask) {
              ref.fused = sp.fused = ask & 1; ref.fused_forced = sp.fused_forced = ask & 2;
              ref.pass_dense = sp.pass_dense = ask / 4 - 1;
              for (int64_t n_obs : counts) {
                ref.n_obs = sp.n_obs = n_obs;
                if (slots == 1 && ask == 0) {
                  CHECK(sp.lists_wanted(pp) == parent::lists_built(&ref));
                  CHECK(sp.fused_default(pp, false) == parent::fused_default(&ref) && !sp.fused_default(pp, true));
                }
                const parent::Use use{parent::use_fused(&ref), parent::use_pass_dense(&ref)};
                for (int commit = 0; commit < 2; ++commit) {
                  const StepForm f = sp.form(pp, slots, commit);
                  ++points;
                  ++reached[rank_of(f)];
                  CHECK(f == parent::launched(use, commit));
                  CHECK(commit || f != StepForm::Three);
                  CHECK(StepPlan::needs_a_before(f) == parent::ensured_a(use));
                  CHECK(StepPlan::a_valid_after(f, commit) == parent::a_ok_after(use, commit));
                  if (!commit) continue;   // what the parent asked of the next COMMITTED iteration
                  CHECK(StepPlan::a_valid_after(f, true) == parent::a_ok_after_replay(use));
                  CHECK(StepPlan::launches_family(f) == parent::launches_option(use));
                  CHECK((f == StepForm::Three ? 1 : 0) == parent::pass_dense_option(use));
                  for (int stage = 0; stage < K_COUNT; ++stage)
                    CHECK(StepPlan::stage_runs(f, static_cast<KernelId>(stage)) == !parent::stage_skipped(use, stage));
                }
              }
            }
            // the default ask -- what create() leaves -- along growing ratings: two launches, then four, then three;
            // never back, and never from two to three
            for (int commit = 0; commit < 2; ++commit) {
              int before = 0;
              for (int64_t n_obs : counts) {
                sp.n_obs = n_obs;
                sp.fused_forced = false; sp.pass_dense = -1;
                sp.fused = sp.fused_default(pp, false);
                const int now = rank_of(sp.form(pp, slots, commit));
                CHECK(now >= before && !(before == 0 && now == 2));
                before = now;
              }
              ++walks;
            }
          }
        }
      }
    }
  // the option transitions: today's refusals and messages, and the ask they leave
  {
    StepPlan sp;
    std::string said;
    try { sp.set_fused(true, false); } catch (const std::invalid_argument &e) { said = e.what(); }
    if (said != "fused: not available for this shape / data" || sp.fused || sp.fused_forced) { std::printf("FAILED: set_fused refusal\n"); ++fails; }
    sp.set_fused(true, true);
    if (!sp.fused || !sp.fused_forced) { std::printf("FAILED: set_fused on\n"); ++fails; }
    sp.set_fused(false, false);
    if (sp.fused || sp.fused_forced) { std::printf("FAILED: set_fused off\n"); ++fails; }
    for (double v : {-1.0, 0.0, 1.0}) {
      sp.set_pass_dense(v);
      if (sp.pass_dense != static_cast<int>(v)) { std::printf("FAILED: set_pass_dense %g\n", v); ++fails; }
    }
    for (double v : {-2.0, 0.5, 2.0}) {
      said.clear();
      try { sp.set_pass_dense(v); } catch (const std::invalid_argument &e) { said = e.what(); }
      if (said != "pass_dense: -1, 0 or 1" || sp.pass_dense != 1) { std::printf("FAILED: set_pass_dense refusal %g\n", v); ++fails; }
    }
  }
  std::printf("shapes %zu, plans %ld, grid points %ld: two launches %ld, three %ld, four %ld; default walks %ld\n",
              dims.size() * dims.size(), plans, points, reached[0], reached[2], reached[1], walks);
  if (!reached[0] || !reached[1] || !reached[2]) { std::printf("FAILED: a form no grid point reached\n"); ++fails; }
  if (dims.size() != 20) { std::printf("FAILED: %zu padded values\n", dims.size()); ++fails; }
  if (fails) { std::printf("step plan check: %ld failure(s)\n", fails); return 1; }
  std::printf("step plan check: ok\n");
  return 0;
}
