// tu_iterate.hip -- the EM iteration of the Mixed-Membership Stochastic Block Model on the MI355X (gfx950 / CDNA4): the
// order of its launches in each of its forms, the graph replay, and the timers around them.  Host code only; every
// kernel lives in the unit of its stage (launch.hpp lists them), and which form an iteration takes is the context's
// StepPlan's answer (step_plan.hpp), asked for once per iteration.
//
// What the reference computes per EM iteration (src/kernels_numpy.py:43-79 followed by
// src/mmsbm.py:248-250), for every observed triple n = (u, i, r):
//
//   omega[n,k,l] = theta[u,k] eta[i,l] p[k,l,r]        s_n = sum_kl omega[n,k,l]
//   n_theta[u,k] = sum_{n: u_n=u} sum_l omega/max(s_n,eps)      (and the same for eta, p)
//
// materialising the (N,K,L) tensor several times.  The library never builds omega.  With
// a "pair" q = a distinct (item, rating) combination and
//
//   A[q,k]   = sum_l p[k,l,r_q] eta[i_q,l]                       (pair_matvec, K-side)
//   w_n      = 1 / max(theta[u_n,:] . A[q_n,:], eps)
//   n_theta[u,k] = theta[u,k] * sum_{n in user u} A[q_n,k] w_n   (seg_pass, user segments)
//   C[q,k]   = sum_{n in pair q} theta[u_n,k] w_n                (seg_pass, pair segments)
//   T[q,l]   = sum_k p[k,l,r_q] C[q,k]                           (pair_matvec, L-side)
//   n_eta[i,l] = eta[i,l] * sum_{q in item i} T[q,l]             (item_sum)
//   n_p[k,l,r] = p[k,l,r] * sum_{q: r_q=r} C[q,k] eta[i_q,l]     (p_partial, p_update)
//
// which is the same sum re-associated: O(N K + Q K L) flops instead of O(N K L), two
// row-gather passes over the triples (sorted user-major and (rating,item)-major), every
// reduction a segmented reduction in registers (no atomics: results are bitwise
// reproducible), all arithmetic float64: the triple passes and the small-tile pair stage on the vector ALU,
// the pair stage of big rating tiles (K x L > 1024) on the matrix cores (v_mfma_f64_16x16x4_f64).
//
// Written for gfx950 only: 64-wide wavefronts, DPP cross-lane reductions, LDS-staged
// rating tiles.
//
// Who owns which field of the context's iteration state:
//   cur          which of the two parameter buffers is current.  launch_iteration flips it after a committed iteration;
//                run_iterations puts it back when a capture fails.  Nobody else writes it (tu_create.hip's alloc_state
//                starts it at 0).
//   step         the iteration's form (step_plan.hpp): the facts are create()'s (tu_create.hip), the ask changes through
//                set_fused / set_pass_dense (tu_options.hip).  This unit only reads it: form(), and the rules of a form.
//   a_ok[slot]   atab[cur] holds A of the slot's current parameters.  Written by ensure_a (StepPlan::needs_a_before) and
//                by mark_a, at the end of launch_iteration and after a replay in run_iterations, both by the one rule
//                StepPlan::a_valid_after.  Outside this unit only where a slot's
//                parameters arrive -- set_params / init_params (tu_params.hip) mark the slot they filled -- and where
//                the state is reset (set_slots, tu_create.hip).
//   graph_exec   the captured two-iteration graphs, by `cur` at capture time: captured, instantiated and replayed by
//                run_iterations only.  Dropped (mmsbm_hip_ctx::drop_graphs) by whatever changes the launches they
//                hold: set_option (tu_options.hip) and alloc_state (tu_create.hip).
//   profiling, prof_events   set around its iterations by profile_iterations, filled by the stages' LaunchScope,
//                emptied by collect_profile.
#include "prelude.hpp"

#include <unistd.h>

#include <map>
#include <mutex>

namespace mmsbm_hip_impl {

// ---- launch log (launch.hpp) -------------------------------------------------------------------------------------------
bool g_launch_log_on = std::getenv("MMSBM_HIP_LAUNCH_LOG") != nullptr && std::getenv("MMSBM_HIP_LAUNCH_LOG")[0] != 0;

namespace {
struct LaunchLog {
  struct Rec { long long count = 0; std::string name, tag; };
  std::mutex mu;
  std::map<const void *, Rec> seen;   // host-side kernel handle -> launches since the last flush, name, tag of the first one
  void note(const void *fn) {
    std::lock_guard<std::mutex> lock(mu);
    Rec &r = seen[fn];
    if (r.count++ == 0 && r.name.empty()) {
      // (the name is asked for HERE, with the runtime alive and the kernel about to be launched -- not at exit, when
      // the runtime may already be gone)
      const char *name = hipKernelNameRefByPtr(fn, nullptr);
      char buf[64];
      std::snprintf(buf, sizeof buf, "%p", fn);
      r.name = (name && name[0]) ? name : buf;
      const char *t = std::getenv("MMSBM_HIP_LAUNCH_TAG");
      r.tag = t ? t : "-";
    }
  }
  // one line per kernel: pid <tab> launches <tab> mangled name <tab> tag; appended in ONE write, so that the lines of
  // several processes sharing the file do not interleave.  Counts restart from zero, names and tags are kept.  No HIP
  // call in here: it also runs when the library is unloaded.
  void flush() {
    std::lock_guard<std::mutex> lock(mu);
    const char *path = std::getenv("MMSBM_HIP_LAUNCH_LOG");
    if (!path || !path[0]) return;
    std::string out;
    for (auto &kv : seen) {
      if (kv.second.count == 0) continue;
      out += std::to_string(static_cast<long long>(getpid())) + "\t" + std::to_string(kv.second.count) + "\t" +
             kv.second.name + "\t" + kv.second.tag + "\n";
      kv.second.count = 0;
    }
    if (out.empty()) return;
    if (FILE *f = std::fopen(path, "a")) {
      std::fwrite(out.data(), 1, out.size(), f);
      std::fclose(f);
    }
  }
  ~LaunchLog() { flush(); }
};
LaunchLog &launch_log() {
  static LaunchLog log;   // (flushed once more when the library is unloaded / the process exits)
  return log;
}
}  // namespace

void launch_log_note(const void *host_fn) { launch_log().note(host_fn); }
void launch_log_flush() {
  if (g_launch_log_on) launch_log().flush();
}

// ---- the form of the pair stage the context's shape and options select ------------------------------------------------
void stage_dense(mmsbm_hip_ctx *c) {  // T = P^T C  and the K x L slabs for p
  if (c->n_chunks == 0) return;
  if (c->pp.on_mfma()) stage_dense_mfma(c);
  else stage_dense_valu(c);
}
void stage_matvec_a(mmsbm_hip_ctx *c, int slot, int a_slot, bool grid) {
  if (c->pp.on_mfma()) stage_matvec_a_mfma(c, slot, a_slot, grid);
  else stage_matvec_a_valu(c, slot, a_slot, grid);
}

// atab[cur] = A of the current parameters, for every slot the next launches cover (see mmsbm_hip_ctx::a_ok)
void ensure_a(mmsbm_hip_ctx *c) {
  bool ok = true;
  for (int s = c->base_slot; s < c->base_slot + c->launch_slots; ++s) ok = ok && c->a_ok[static_cast<size_t>(s)];
  if (ok) return;
  const bool prof = c->profiling;  // (not a launch of the iteration being profiled)
  c->profiling = false;
  stage_matvec_a(c, c->cur, c->cur);
  c->profiling = prof;
  for (int s = c->base_slot; s < c->base_slot + c->launch_slots; ++s) c->a_ok[static_cast<size_t>(s)] = 1;
}

namespace {

// Units per workgroup for a launch whose workgroups each walk a run of 64-pair units of one rating, `slots` of them
// resident at a time: the launch lasts rounds x (units + a prologue of ~0.6 unit-times: the tile into LDS, the item ids,
// the first rows' latency -- measured at C5, EXPERIMENTS.md), and rounds is an INTEGER (with 768 slots C5's 15,616 units in
// runs of 8 are 1,952 workgroups = 2.54 rounds, paid as 3 = 24 unit-times; in runs of 11 they are 1.9 rounds, paid as 2 = 22).
// Workgroups are counted by the rule the run list is built by (layout.hpp: padded_chunk_count).
inline int balanced_run_units(const std::vector<int32_t> &rating_off, int slots, int lo, int hi) {
  int best = hi;
  double best_cost = 1e300;
  const bool align = mmsbm::chunk_align_on();
  const int n_ratings = static_cast<int>(rating_off.size()) - 1;
  for (int u = hi; u >= lo; --u) {
    long long wgs = 0;
    for (int r = 0; r < n_ratings; ++r)
      wgs += mmsbm::padded_chunk_count(rating_off[static_cast<size_t>(r) + 1] - rating_off[static_cast<size_t>(r)],
                                       u * kUnitPairs, n_ratings, align);
    const double cost = static_cast<double>((wgs + slots - 1) / std::max(slots, 1)) * (u + 0.6);
    if (cost < best_cost * 0.97) { best_cost = cost; best = u; }   // (longer runs win ties: fewer prologues)
  }
  return best;
}

void mark_a(mmsbm_hip_ctx *c, bool ok) {
  for (int s = c->base_slot; s < c->base_slot + c->launch_slots; ++s) c->a_ok[static_cast<size_t>(s)] = ok ? 1 : 0;
}

}  // namespace

// The A launch of the matrix-core pair stage writes rows only -- nothing ties its workgroups to the T + S launch's
// slabs -- so it walks the same units in runs of its own length: `units` 64-pair units per workgroup, or (0) as many as
// make its last round of workgroups (nearly) full (balanced_run_units; C5: runs of 11 units where the T + S launch takes
// 8).  Same rows, bit for bit.  n_a_chunks = 0: the T + S launch's own list serves.
void build_a_runs(mmsbm_hip_ctx *c, int units) {
  c->n_a_chunks = 0;
  c->a_chunks.release();
  if (!c->pp.mfma || c->n_pairs <= 0) return;
  const int now = c->pp.chunk_pairs / kUnitPairs, most = kMfmaChunkPairs / kUnitPairs;
  int a_units = units > 0 ? std::min(units, most)
                          : balanced_run_units(c->lay.rating_off, mfma_a_blocks_per_cu(c) * c->n_cus, std::max(2, now / 2),
                                               std::min(2 * now, most));
  c->a_units = a_units;
  if (a_units == now) return;
  mmsbm::Layout tmp;   // (only the fields build_mv_chunks reads and writes)
  tmp.n_ratings = c->lay.n_ratings; tmp.rating_off = c->lay.rating_off;
  mmsbm::build_mv_chunks(tmp, a_units * kUnitPairs);
  c->a_chunks.upload(tmp.mv_chunks, c->stream);
  HIP_CHECK(hipStreamSynchronize(c->stream));   // (`tmp` is a local)
  c->n_a_chunks = static_cast<int>(tmp.mv_chunks.size());
}

// ---- one iteration in the form the context's plan gives (step_plan.hpp) -------------------------------------------------
void launch_iteration(mmsbm_hip_ctx *c, bool commit) {
  const StepForm form = c->form(commit);
  if (StepPlan::needs_a_before(form)) ensure_a(c);
  switch (form) {
    case StepForm::Two: stage_fused_pairs(c); stage_fused_tail(c, commit); break;  // (A of the current parameters on its way)
    case StepForm::Three: stage_pass_dense(c); stage_eta_p(c, commit); break;
    case StepForm::Four: stage_seg(c, commit, true, true, c->stream); stage_dense(c); stage_eta_p(c, commit); break;
  }
  if (commit) {
    if (form != StepForm::Two) stage_matvec_a(c, c->cur ^ 1, c->cur ^ 1);  // (A of the new parameters: a_valid_after)
    c->cur ^= 1;
  }
  mark_a(c, StepPlan::a_valid_after(form, commit));
}

// n committed iterations: graph replays of two iterations each when enabled, the rest eager
void run_iterations(mmsbm_hip_ctx *c, int n) {
  if (c->graph_mode && !c->profiling) {
    const StepForm form = c->form(true);  // (of every iteration of this call: nothing it depends on changes in here)
    while (n >= 2) {
      const int slot = c->cur;
      if (!c->graph_exec[slot]) {
        if (StepPlan::needs_a_before(form)) ensure_a(c);  // (outside the capture: a replay must not repeat it)
        hipGraph_t graph = nullptr;
        HIP_CHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        try {
          launch_iteration(c, true);
          launch_iteration(c, true);
        } catch (...) {
          (void)hipStreamEndCapture(c->stream, &graph);
          if (graph) (void)hipGraphDestroy(graph);
          c->cur = slot;
          throw;
        }
        HIP_CHECK(hipStreamEndCapture(c->stream, &graph));
        hipError_t e = hipGraphInstantiate(&c->graph_exec[slot], graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess)
          throw ApiError(MMSBM_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        // capture only records: cur is back where it started and nothing has run yet
      }
      HIP_CHECK(hipGraphLaunch(c->graph_exec[slot], c->stream));
      // (a replay runs none of launch_iteration's host code: its last line, by the same rule)
      mark_a(c, StepPlan::a_valid_after(form, true));
      n -= 2;
    }
  }
  for (; n > 0; --n) launch_iteration(c, true);
}

// ---- the timers and the byte model -----------------------------------------------------------------------------------
float time_iterations(mmsbm_hip_ctx *c, int n_iters) {
  EventPair ev;
  ev.start(c->stream);
  run_iterations(c, n_iters);
  ev.stop(c->stream);
  ev.wait();
  return ev.ms();
}

namespace {
void collect_profile(mmsbm_hip_ctx *c, float *mean_us, int *launches, int n_iters) {
  std::vector<double> tot(K_COUNT, 0.0);
  std::vector<int> cnt(K_COUNT, 0);
  for (auto &pe : c->prof_events) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, pe.second.first, pe.second.second));
    tot[pe.first] += ms * 1000.0;
    cnt[pe.first]++;
    (void)hipEventDestroy(pe.second.first);
    (void)hipEventDestroy(pe.second.second);
  }
  c->prof_events.clear();
  for (int i = 0; i < K_COUNT; ++i) {
    mean_us[i] = cnt[i] ? static_cast<float>(tot[i] / cnt[i]) : 0.f;
    if (launches) launches[i] = n_iters > 0 ? cnt[i] / n_iters : 0;
  }
}
}  // namespace

void profile_iterations(mmsbm_hip_ctx *c, int n_iters, float *mean_us, int *launches_per_iter) {
  HIP_CHECK(hipStreamSynchronize(c->stream));
  c->profiling = true;
  try {
    for (int it = 0; it < n_iters; ++it) launch_iteration(c, true);
    HIP_CHECK(hipStreamSynchronize(c->stream));
  } catch (...) {
    c->profiling = false;
    throw;
  }
  c->profiling = false;
  collect_profile(c, mean_us, launches_per_iter, n_iters);
}

void kernel_bytes(const mmsbm_hip_ctx *ctx, int index, int64_t *bytes_read, int64_t *bytes_written) {
  const int64_t N = ctx->n_obs, U = ctx->n_users, I = ctx->n_items, R = ctx->n_ratings;
  const int64_t K = ctx->k, L = ctx->l, Q = ctx->n_pairs;
  const int64_t C = static_cast<int64_t>(ctx->lay.mv_chunks.size());
  int64_t rd = 0, wr = 0;
  const StepForm form = ctx->form(true);
  const bool merged = form == StepForm::Three;  // K_SEG is the merged launch of pass_dense.hpp
  switch (index) {
    case K_SEG:  // two passes: index + one gathered K-row per triple; fixed rows and offsets once
      rd = 2 * N * (4 + 8 * K) + (U + Q) * (8 * K + 4);
      wr = (U + Q) * 8 * K;
      if (merged) {  // no C rows out; gathered eta rows + item ids + one tile per unit in, T rows + slabs out
        rd += Q * (8 * L + 4) + C * 8 * K * L;
        wr += Q * (8 * L - 8 * K) + C * 8 * K * L;
      }
      break;
    case K_DENSE:  // C rows + gathered eta rows + item ids + one tile per block; T rows + slabs
      if (!StepPlan::stage_runs(form, K_DENSE)) break;
      rd = Q * (8 * K + 8 * L + 4) + C * 8 * K * L;
      wr = Q * 8 * L + C * 8 * K * L;
      break;
    case K_ETAP:  // slabs + p ; T rows through the item CSR + eta
      rd = C * 8 * K * L + R * 8 * K * L + Q * (8 * L + 4) + I * (8 * L + 8);
      wr = 3 * R * 8 * K * L + I * 8 * L;
      break;
    case K_MATVEC_A: rd = Q * (8 * L + 4) + C * 8 * K * L; wr = Q * 8 * K; break;
    case K_FUSED_PAIRS:  // gathered eta rows + ids, the pair pass's index + theta row per triple, two tiles per block
      rd = Q * (8 * L + 4 + 4) + N * (4 + 8 * K) + 2 * C * 8 * K * L;
      wr = Q * (8 * K + 8 * L) + C * 8 * K * L;
      break;
    case K_FUSED_TAIL:   // the user pass + the slabs and p + T rows through the item lists
      rd = N * (4 + 8 * K) + U * (8 * K + 4) + C * 8 * K * L + R * 8 * K * L + Q * (8 * L + 4) + I * (8 * L + 8);
      wr = U * 8 * K + 3 * R * 8 * K * L + I * 8 * L;
      break;
    default: throw std::invalid_argument("kernel index out of range");
  }
  *bytes_read = rd * ctx->n_slots;  // one launch covers every restart slot
  *bytes_written = wr * ctx->n_slots;
}

void time_stage(mmsbm_hip_ctx *ctx, int stage, int reps, float *mean_us) {
#ifdef MMSBM_ABLATE
  ctx->ablate = stage >> 8;  // diagnostic build: bits 8.. = phases to skip
  stage &= 0xff;
  struct Reset { mmsbm_hip_ctx *c; ~Reset() { c->ablate = 0; } } reset{ctx};
#else
  if (stage >> 8)
    throw ApiError(MMSBM_E_UNSUPPORTED, "time_stage: phase ablation (stage bits 8+) needs the diagnostic build (-DMMSBM_ABLATE, csrc/unity.hip)");
#endif
  if (!mean_us || reps <= 0 || stage < 0 || stage >= K_COUNT)
    throw std::invalid_argument("bad argument");
  if ((stage == K_FUSED_PAIRS || stage == K_FUSED_TAIL) && !ctx->step.two_possible(ctx->pp))
    throw std::invalid_argument("time_stage: the two-launch kernels do not apply to this shape / data");
  use_device(ctx);
  ensure_a(ctx);
  // (with the triple passes and the T + S stage in one launch, stage K_SEG is that launch and K_DENSE has none: 0 us)
  const StepForm form = ctx->form(true);
  if (!StepPlan::stage_runs(form, static_cast<KernelId>(stage))) {
    *mean_us = 0.f;
    return;
  }
  auto one = [&] {
    switch (stage) {
      case K_SEG:
        if (form == StepForm::Three) stage_pass_dense(ctx);
        else stage_seg(ctx, true, true, true, ctx->stream);
        break;
      case K_DENSE: stage_dense(ctx); break;
      case K_ETAP: stage_eta_p(ctx, true); break;
      case K_FUSED_PAIRS: stage_fused_pairs(ctx); break;
      case K_FUSED_TAIL: stage_fused_tail(ctx, true); break;
      default: stage_matvec_a(ctx, ctx->cur, ctx->cur ^ 1); break;
    }
  };
  for (int w = 0; w < 3; ++w) one();
  EventPair ev;
  ev.start(ctx->stream);
  for (int r = 0; r < reps; ++r) one();
  ev.stop(ctx->stream);
  ev.wait();
  *mean_us = ev.ms() * 1000.f / reps;
}

}  // namespace mmsbm_hip_impl
