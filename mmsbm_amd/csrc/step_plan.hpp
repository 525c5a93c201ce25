// step_plan.hpp -- the form of an EM iteration as ONE value: two launches (fused_small.hpp), three (pass_dense.hpp,
// committed iterations only) or the four separate ones.  Host arithmetic on plain numbers and on PairPlan only -- no HIP
// type, no context -- so that the size rules, which no test of a few seconds can reach on a device, are checked on the CPU
// over every shape (tests/native/step_plan_check.cpp).  Included after pair_plan.hpp.  create() fills in the facts about
// the data and the default ask (tu_create.hip), options "fused" and "pass_dense" change the ask through set_fused /
// set_pass_dense (tu_options.hip), and the iteration, its timers and the options that show the form (tu_iterate.hip,
// tu_options.hip) read form() and the rules below: nothing else decides.
#pragma once

namespace mmsbm_hip_impl {  // (StepPlan is a member of mmsbm_hip_ctx: one type in every translation unit)

// The stages a launch is timed as: the four launches of an iteration -- or, for small problems, the two of
// fused_small.hpp.  With pass_dense.hpp the merged launch (pass_dense_kernel) is timed as stage K_SEG and K_DENSE has no
// launch: the names (kKernelNames, context.hpp) stay as they are.
enum KernelId { K_SEG = 0, K_DENSE, K_ETAP, K_MATVEC_A, K_FUSED_PAIRS, K_FUSED_TAIL, K_COUNT };

enum class StepForm { Two, Three, Four };

// Two launches while the launches' work is small: ratings x restart slots x (K + L, padded) <= 14M (measured per
// iteration, two / four launches.  One slot, K = L = 10: 100k ratings 20.2 / 29.3 us, 300k 28.7 / 37.0, 500k 37.8 /
// 43.5; K = L = 16: 400k 36.0 / 41.7; K = L = 20: 100k 28.4 / 37.6, 300k 50.1 / 50.1, 600k 69.4 / 67.5, 1M 105.0 / 95.6.  100k ratings at K = L = 10
// with 2 / 4 / 8 / 16 slots: 26.5 / 32.4, 40.9 / 42.8, 68.0 / 64.9, 119.9 / 115.9 -- with several slots the four-launch
// form shares the index stream among them)
// Data whose segments are cut into pieces pays a combine launch in the separate form (five launches): there the two
// launches win a little further out (log-normal popularity, separate / two, scripts/fused_split_sweep.py: 400k ratings
// K = L = 10 38.4 / 31.3 us, 700k 43.8 / 39.8; 300k K = L = 20 45.1 / 41.4, 600k 54.0 / 65.5; 1M x 100k x 20k K = L = 10
// 77.3 / 92.6) -- up to 18M.
constexpr long long kFusedWorkMax = 14000000, kFusedWorkMaxSplit = 18000000;
// ... and the ratings up to which create() builds the form's whole-segment lists and turns it on
constexpr long long kFusedRatingsMax = 1500000;
// Three launches from the size at which they pay, ratings x (K + L, padded): above the two-launch form's range
// (kFusedWorkMax), so that no shape goes from two launches to this form (measured per iteration: EXPERIMENTS.md, section C)
constexpr long long kPassDenseWorkMin = 20000000;
static_assert(kPassDenseWorkMin > kFusedWorkMaxSplit, "no shape changes from two launches to three");

struct StepPlan {
  // ---- what the caller asked for ----
  bool fused = false;         // small problems: two launches per iteration (create(): fused_default; option "fused")
  bool fused_forced = false;  // option "fused" = 1: whatever the size (else: while the work is within kFusedWorkMax)
  int pass_dense = -1;        // option "pass_dense": -1 the library's choice by size, 0 off, 1 on wherever the form applies
  // ---- the facts about the data, fixed at create() ----
  int64_t n_obs = 0;
  int kp = 0, lp = 0, code_k = 0, code_l = 0;  // the padded shape and its group codes (shapes.hpp)
  int n_chunks = 0;                            // workgroups of the pair stage
  bool items_pairs = false, items_users = false;  // the side has a work list (layout.hpp: WorkList::items)
  bool cut_pairs = false, cut_users = false;      // ... with segments cut into pieces (WorkList::splits)
  // the whole-segment lists create() built for such data: every segment's pieces inside one workgroup of the two-launch
  // form (layout.hpp: FusedLists), pair side (the units of pairs_fused_kernel) and / or user side (blocks of tail_fused_kernel)
  bool fs_pairs = false, fs_users = false;
  // (what an option can change later -- the pair stage's plan, the restart slots of a launch -- is not kept here: it is
  // an argument of every question)

  // ---- two launches: small problems (fused_small.hpp) ----
  // everything but the data: the kernels exist for this shape
  bool two_shape_ok(const PairPlan &pp) const { return code_k <= 1 && code_l <= 1 && n_chunks > 0 && pp.two_shape_ok(); }
  // A work list that only ORDERS whole segments is fine (the pair units ignore it -- every segment's result is its
  // own -- and the user pass follows it as before); segments cut into pieces need all pieces of a segment inside one
  // workgroup: the lists create() builds for small problems (fs_pairs / fs_users; round 4)
  bool two_possible(const PairPlan &pp) const { return two_shape_ok(pp) && (!cut_pairs || fs_pairs) && (!cut_users || fs_users); }
  // create(): the whole-segment lists are worth building; the default of `fused` once they are (no_fused:
  // MMSBM_HIP_NO_FUSED).  Small problems: where eight rows in flight pay (tu_create.hip: plan_sides)
  bool lists_wanted(const PairPlan &pp) const { return n_obs <= kFusedRatingsMax && two_shape_ok(pp) && (cut_pairs || cut_users); }
  bool fused_default(const PairPlan &pp, bool no_fused) const { return n_obs <= kFusedRatingsMax && two_possible(pp) && !no_fused; }

  // ---- three launches: big problems of small tiles, the triple passes and the T + S stage in one (pass_dense.hpp) ----
  // Everything but the size: one restart per launch, the small-tile T + S body at 256 threads (its split of a unit's
  // pairs among the slab copies is what the merged kernel mirrors), eight-lane groups on the gathered side, whole
  // segments on both sides (no work lists), every workgroup of the pair stage a single 64-pair unit.
  bool three_possible(const PairPlan &pp, int launch_slots) const {
    return launch_slots == 1 && code_k == 1 && code_l <= 1 && n_chunks > 0 && pp.pass_dense_shape_ok() && !items_pairs &&
           !items_users && !cut_pairs && !cut_users;
  }

  // ---- the form of the next iteration over `launch_slots` restart slots ----
  // commit off (update_coefficients) needs the raw numerators of the separate launches and keeps them: never Three.
  // (two_possible every time: options set after create() -- "mfma", "quad" ... -- change what it depends on)
  StepForm form(const PairPlan &pp, int launch_slots, bool commit) const {
    // (option "pass_dense" = 1 asks for three launches before two; a forced "fused" wins)
    const bool three_first = pass_dense == 1 && !fused_forced && three_possible(pp, launch_slots);
    if (!three_first && fused && two_possible(pp) &&
        (fused_forced || n_obs * launch_slots * (kp + lp) <= ((cut_pairs || cut_users) ? kFusedWorkMaxSplit : kFusedWorkMax)))
      return StepForm::Two;
    if (commit && pass_dense != 0 && three_possible(pp, launch_slots) &&
        (pass_dense == 1 || n_obs * (kp + lp) >= kPassDenseWorkMin))
      return StepForm::Three;
    return StepForm::Four;
  }

  // ---- what a form means to the iteration's state and to the timers ----
  // atab[cur] = A of the current parameters is what the separate stages start from; the two launches compute A on
  // their way (ensure_a, tu_iterate.hip)
  static bool needs_a_before(StepForm f) { return f != StepForm::Two; }
  // ... and whether that still holds after an iteration of the form: the separate stages end a committed iteration
  // with A of the new parameters and leave it alone otherwise; the two launches wrote A of the parameters they
  // started from, which a commit replaces
  static bool a_valid_after(StepForm f, bool commit) { return f != StepForm::Two || !commit; }
  // A stage id has a launch of its own to time and to count bytes for (any stage of either family may be timed alone,
  // whatever the iteration takes): with three launches K_SEG is the merged launch and K_DENSE has none
  static bool stage_runs(StepForm f, KernelId id) { return !(f == StepForm::Three && id == K_DENSE); }
  // the form FAMILY option "launches" reads: 2 = the two launches, 4 = the separate stages, merged or not
  static int launches_family(StepForm f) { return f == StepForm::Two ? 2 : 4; }

  // ---- the option transitions ----
  // Option "fused": any problem size once set; `possible`: two_possible() of the plan in force
  void set_fused(bool on, bool possible) {
    if (on && !possible) throw std::invalid_argument("fused: not available for this shape / data");
    fused = fused_forced = on;
  }
  void set_pass_dense(double value) {
    if (value != -1.0 && value != 0.0 && value != 1.0) throw std::invalid_argument("pass_dense: -1, 0 or 1");
    pass_dense = static_cast<int>(value);
  }
};

}  // namespace mmsbm_hip_impl
