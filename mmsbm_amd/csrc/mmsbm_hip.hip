// mmsbm_hip.hip -- MI355X (gfx950 / CDNA4) EM core for the Mixed-Membership Stochastic
// Block Model, behind the C ABI of include/mmsbm_hip.h.
//
// What the reference computes per EM iteration (src/kernels_numpy.py:43-79 followed by
// src/mmsbm.py:248-250), for every observed triple n = (u, i, r):
//
//   omega[n,k,l] = theta[u,k] eta[i,l] p[k,l,r]        s_n = sum_kl omega[n,k,l]
//   n_theta[u,k] = sum_{n: u_n=u} sum_l omega/max(s_n,eps)      (and the same for eta, p)
//
// materialising the (N,K,L) tensor several times.  This file never builds omega.  With
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

#include "prelude.hpp"
#include "layout_gpu.hpp"
#include "pcg64.hpp"

#include <unistd.h>

#include <map>
#include <mutex>

namespace {

thread_local std::string g_last_error;

template <class F>
int guarded(F &&f) {
  try {
    f();
    return MMSBM_OK;
  } catch (const ApiError &e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::invalid_argument &e) {
    g_last_error = e.what();
    return MMSBM_E_INVALID;
  } catch (const std::bad_alloc &) {
    g_last_error = "host allocation failed";
    return MMSBM_E_INTERNAL;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return MMSBM_E_INTERNAL;
  } catch (...) {  // anything that is not a std::exception (a library's own type, a thrown int): a status, never a
                   // process death across the C ABI
    g_last_error = "unknown exception (not derived from std::exception)";
    return MMSBM_E_INTERNAL;
  }
}

}  // namespace

// ---- launch log (launch.hpp) -------------------------------------------------------------------------------------------
namespace mmsbm_hip_impl {

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

}  // namespace mmsbm_hip_impl

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

// ---- small problems: the iteration in two launches (fused_small.hpp) -------------------------------------
bool fused_shape_ok(const mmsbm_hip_ctx *c) {  // (everything but the data: the kernels exist for this shape)
  return c->code_k <= 1 && c->code_l <= 1 && c->n_chunks > 0 && c->pp.fused_shape_ok();
}
bool fused_possible(const mmsbm_hip_ctx *c) {
  // A work list that only ORDERS whole segments is fine (the pair units ignore it -- every segment's result is its
  // own -- and the user pass follows it as before); segments cut into pieces need all pieces of a segment inside one
  // workgroup: the lists create() builds for small problems (fs_pairs / fs_users; round 4)
  return fused_shape_ok(c) && (c->lay.pair_work.splits.empty() || c->fs_pairs) &&
         (c->lay.user_work.splits.empty() || c->fs_users);
}

void mark_a(mmsbm_hip_ctx *c, bool ok) {
  for (int s = c->base_slot; s < c->base_slot + c->launch_slots; ++s) c->a_ok[static_cast<size_t>(s)] = ok ? 1 : 0;
}

// Two launches while the launches' work is small: ratings x restart slots x (K + L, padded) <= 14M (measured per
// iteration, two / four launches.  One slot, K = L = 10: 100k ratings 20.2 / 29.3 us, 300k 28.7 / 37.0, 500k 37.8 /
// 43.5; K = L = 16: 400k 36.0 / 41.7; K = L = 20: 100k 28.4 / 37.6, 300k 50.1 / 50.1, 600k 69.4 / 67.5, 1M 105.0 / 95.6.  100k ratings at K = L = 10
// with 2 / 4 / 8 / 16 slots: 26.5 / 32.4, 40.9 / 42.8, 68.0 / 64.9, 119.9 / 115.9 -- with several slots the four-launch
// form shares the index stream among them)
// Data whose segments are cut into pieces pays a combine launch in the separate form (five launches): there the two
// launches win a little further out (log-normal popularity, separate / two, scripts/fused_split_sweep.py: 400k ratings
// K = L = 10 38.4 / 31.3 us, 700k 43.8 / 39.8; 300k K = L = 20 45.1 / 41.4, 600k 54.0 / 65.5; 1M x 100k x 20k K = L = 10
// 77.3 / 92.6) -- up to 18M.
constexpr long long kFusedWorkMax = 14000000, kFusedWorkMaxSplit = 18000000, kFusedRatingsMax = 1500000;

// ---- big problems of small tiles: the triple passes and the T + S stage in one launch (pass_dense.hpp) ------------
// Everything but the size: one restart per launch, the small-tile T + S body at 256 threads (its split of a unit's
// pairs among the slab copies is what the merged kernel mirrors), eight-lane groups on the gathered side, whole
// segments on both sides (no work lists), every workgroup of the pair stage a single 64-pair unit.
bool pass_dense_possible(const mmsbm_hip_ctx *c) {
  return c->launch_slots == 1 && c->code_k == 1 && c->code_l <= 1 && c->n_chunks > 0 && c->pp.pass_dense_shape_ok() &&
         c->lay.pair_work.items.empty() && c->lay.user_work.items.empty() && c->lay.pair_work.splits.empty() &&
         c->lay.user_work.splits.empty();
}
// ... and the size from which it pays, ratings x (K + L, padded): above the two-launch form's range (kFusedWorkMax), so
// that no shape goes from two launches to this form (measured per iteration: EXPERIMENTS.md, section C)
constexpr long long kPassDenseWorkMin = 20000000;
static_assert(kPassDenseWorkMin > kFusedWorkMaxSplit, "no shape changes from two launches to three");

bool use_fused(const mmsbm_hip_ctx *c) {
  // (fused_possible again: options set after create() -- "mfma", "direct" ... -- change what it depends on)
  const bool cut = !c->lay.pair_work.splits.empty() || !c->lay.user_work.splits.empty();
  if (c->pass_dense == 1 && !c->fused_forced && pass_dense_possible(c)) return false;  // (option "pass_dense" = 1 asks for that form)
  return c->fused && fused_possible(c) &&
         (c->fused_forced || c->n_obs * c->launch_slots * (c->kp + c->lp) <= (cut ? kFusedWorkMaxSplit : kFusedWorkMax));
}
// the next COMMITTED iteration takes the three-launch form (update_coefficients, commit off, needs the raw numerators
// of the separate launches and keeps them)
bool use_pass_dense(const mmsbm_hip_ctx *c) {
  if (c->pass_dense == 0 || use_fused(c) || !pass_dense_possible(c)) return false;
  return c->pass_dense == 1 || c->n_obs * (c->kp + c->lp) >= kPassDenseWorkMin;
}

void launch_iteration(mmsbm_hip_ctx *c, bool commit) {
  if (use_fused(c)) {
    stage_fused_pairs(c);  // (writes A of the current parameters on its way)
    stage_fused_tail(c, commit);
    if (commit) c->cur ^= 1;
    mark_a(c, !commit);
    return;
  }
  ensure_a(c);
  if (commit && use_pass_dense(c)) {
    stage_pass_dense(c);
  } else {
    stage_seg(c, commit, true, true, c->stream);
    stage_dense(c);
  }
  stage_eta_p(c, commit);
  if (commit) {
    stage_matvec_a(c, c->cur ^ 1, c->cur ^ 1);
    c->cur ^= 1;
    mark_a(c, true);
  }
}

// n committed iterations: graph replays of two iterations each when enabled, the rest eager
void run_iterations(mmsbm_hip_ctx *c, int n) {
  if (c->graph_mode && !c->profiling) {
    while (n >= 2) {
      const int slot = c->cur;
      if (!c->graph_exec[slot]) {
        if (!use_fused(c)) ensure_a(c);  // (outside the capture: a replay must not repeat it)
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
      // (a replay runs none of launch_iteration's host code: the bookkeeping of "atab[cur] holds A of the current
      // parameters" has to be repeated here -- true after the four-launch form, false after the two-launch one)
      mark_a(c, !use_fused(c));
      n -= 2;
    }
  }
  for (; n > 0; --n) launch_iteration(c, true);
}

void require_params(const mmsbm_hip_ctx *c) {  // the selected slot
  if (!c) throw std::invalid_argument("null context");
  if (!c->have[c->sel]) throw std::invalid_argument("set_params has not been called");
}
void require_all_params(const mmsbm_hip_ctx *c) {  // every slot: the iteration advances all of them
  if (!c) throw std::invalid_argument("null context");
  for (int s = 0; s < c->n_slots; ++s)
    if (!c->have[s])
      throw std::invalid_argument(c->n_slots == 1 ? std::string("set_params has not been called")
                                                  : "set_params has not been called for slot " +
                                                        std::to_string(s));
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

// host (rows, d) row-major  <->  device RowTab (rows, dp) zero-padded, main + tail parts, staged
// through pinned memory in the one-slot layout (main rows, then tail rows): one contiguous copy when
// the context has one slot, a strided (2-D) copy per part when the slots' rows are interleaved
bool tab_is_packed(const RowTab &t, int rows) {
  return t.rs_m == t.mw && t.rs_t == t.tw && (t.tw == 0 || t.tail == t.main + static_cast<size_t>(rows) * t.mw);
}
void copy_rows(mmsbm_hip_ctx *c, const RowTab &t, double *stage, int rows, bool to_device) {
  const size_t e = sizeof(double);
  hipStream_t xs = c->xfer ? c->xfer : c->stream;
  if (rows == 0) return;
  if (tab_is_packed(t, rows)) {
    if (to_device)
      HIP_CHECK(hipMemcpyAsync(t.main, stage, e * rows * (t.mw + t.tw), hipMemcpyHostToDevice, xs));
    else
      HIP_CHECK(hipMemcpyAsync(stage, t.main, e * rows * (t.mw + t.tw), hipMemcpyDeviceToHost, xs));
    return;
  }
  double *stage_t = stage + static_cast<size_t>(rows) * t.mw;
  if (to_device) {
    HIP_CHECK(hipMemcpy2DAsync(t.main, e * t.rs_m, stage, e * t.mw, e * t.mw, rows, hipMemcpyHostToDevice, xs));
    if (t.tw > 0)
      HIP_CHECK(hipMemcpy2DAsync(t.tail, e * t.rs_t, stage_t, e * t.tw, e * t.tw, rows, hipMemcpyHostToDevice, xs));
  } else {
    HIP_CHECK(hipMemcpy2DAsync(stage, e * t.mw, t.main, e * t.rs_m, e * t.mw, rows, hipMemcpyDeviceToHost, xs));
    if (t.tw > 0)
      HIP_CHECK(hipMemcpy2DAsync(stage_t, e * t.tw, t.tail, e * t.rs_t, e * t.tw, rows, hipMemcpyDeviceToHost, xs));
  }
}
void zero_rows(mmsbm_hip_ctx *c, const RowTab &t, int rows) {
  const size_t e = sizeof(double);
  if (rows == 0) return;
  if (tab_is_packed(t, rows)) {
    HIP_CHECK(hipMemsetAsync(t.main, 0, e * rows * (t.mw + t.tw), c->stream));
    return;
  }
  HIP_CHECK(hipMemset2DAsync(t.main, e * t.rs_m, 0, e * t.mw, rows, c->stream));
  if (t.tw > 0) HIP_CHECK(hipMemset2DAsync(t.tail, e * t.rs_t, 0, e * t.tw, rows, c->stream));
}
void upload_rows(mmsbm_hip_ctx *c, const RowTab &t, const double *host, int rows, int d) {
  const int dp = t.mw + t.tw, mw = t.mw, tw = t.tw;
  double *stage = c->pin.take(static_cast<size_t>(rows) * dp);
  double *tail = stage + static_cast<size_t>(rows) * mw;
  const int wm = std::min(d, mw), wt = std::max(0, d - mw);
  for_row_blocks(rows, dp, [=](int a, int b) {
    for (int r = a; r < b; ++r) {
      const double *src = host + static_cast<size_t>(r) * d;
      double *m = stage + static_cast<size_t>(r) * mw;
      std::memcpy(m, src, sizeof(double) * wm);
      for (int j = wm; j < mw; ++j) m[j] = 0.0;
      if (tw > 0) {
        double *tl = tail + static_cast<size_t>(r) * tw;
        std::memcpy(tl, src + mw, sizeof(double) * wt);
        for (int j = wt; j < tw; ++j) tl[j] = 0.0;
      }
    }
  });
  copy_rows(c, t, stage, rows, true);
}
// enqueue the device -> pinned copy; unpack_rows after the stream has been synchronised
double *download_rows(mmsbm_hip_ctx *c, const RowTab &t, int rows) {
  const int dp = t.mw + t.tw;
  double *stage = c->pin.take(static_cast<size_t>(rows) * dp);
  copy_rows(c, t, stage, rows, false);
  return stage;
}
void unpack_rows(double *host, const double *stage, const RowTab &t, int rows, int d) {
  const int dp = t.mw + t.tw, mw = t.mw, tw = t.tw;
  const double *tail = stage + static_cast<size_t>(rows) * mw;
  const int wm = std::min(d, mw), wt = std::max(0, d - mw);
  for_row_blocks(rows, dp, [=](int a, int b) {
    for (int r = a; r < b; ++r) {
      double *dst = host + static_cast<size_t>(r) * d;
      std::memcpy(dst, stage + static_cast<size_t>(r) * mw, sizeof(double) * wm);
      if (tw > 0 && wt > 0) std::memcpy(dst + mw, tail + static_cast<size_t>(r) * tw, sizeof(double) * wt);
    }
  });
}
size_t rows_doubles(const mmsbm_hip_ctx *c) {  // staging for theta + eta + p + pT of one slot
  return static_cast<size_t>(c->n_users) * c->kp + static_cast<size_t>(c->n_items) * c->lp +
         2 * static_cast<size_t>(c->n_ratings) * c->kp * c->lp;
}

// device p layout [R][kp][lp] (internal k, l)  <->  host pr (K, L, R) external
void p_host_to_dev(const mmsbm_hip_ctx *c, const double *pr, double *p, double *pt) {
  const int R = c->n_ratings, K = c->k, L = c->l, kp = c->kp, lp = c->lp;
  std::fill(p, p + static_cast<size_t>(R) * kp * lp, 0.0);
  std::fill(pt, pt + static_cast<size_t>(R) * kp * lp, 0.0);
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < L; ++l)
      for (int r = 0; r < R; ++r) {
        // internal (k,l) == external (l,k) when swapped
        const size_t h = c->swapped ? (static_cast<size_t>(l) * c->ext_l + k) * R + r
                                    : (static_cast<size_t>(k) * c->ext_l + l) * R + r;
        const double v = pr[h];
        p[(static_cast<size_t>(r) * kp + k) * lp + l] = v;
        pt[(static_cast<size_t>(r) * lp + l) * kp + k] = v;
      }
}
void p_dev_to_host(const mmsbm_hip_ctx *c, const double *p, double *pr) {
  const int R = c->n_ratings, K = c->k, L = c->l, kp = c->kp, lp = c->lp;
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < L; ++l)
      for (int r = 0; r < R; ++r) {
        const size_t h = c->swapped ? (static_cast<size_t>(l) * c->ext_l + k) * R + r
                                    : (static_cast<size_t>(k) * c->ext_l + l) * R + r;
        pr[h] = p[(static_cast<size_t>(r) * kp + k) * lp + l];
      }
}

// (theta, eta, p) tables of one slot -> host arrays in host layout; any output may be null
void fetch_params(mmsbm_hip_ctx *c, const RowTab &tt, const RowTab &et, const double *p_dev,
                  double *theta, double *eta, double *pr) {
  hipStream_t xs = c->xfer ? c->xfer : c->stream;
  HIP_CHECK(hipStreamSynchronize(xs));
  c->pin.reset(rows_doubles(c));
  const size_t klr = static_cast<size_t>(c->n_ratings) * c->kp * c->lp;
  const double *st = theta ? download_rows(c, tt, c->n_users) : nullptr;
  const double *se = eta ? download_rows(c, et, c->n_items) : nullptr;
  double *sp = nullptr;
  if (pr) {
    sp = c->pin.take(klr);
    HIP_CHECK(hipMemcpyAsync(sp, p_dev, sizeof(double) * klr, hipMemcpyDeviceToHost, xs));
  }
  HIP_CHECK(hipStreamSynchronize(xs));
  if (theta) unpack_rows(theta, st, tt, c->n_users, c->k);
  if (eta) unpack_rows(eta, se, et, c->n_items, c->l);
  if (pr) p_dev_to_host(c, sp, pr);
}

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

// ---- building a context: the steps of mmsbm_hip_create, in the order it calls them ---------------------------------------

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
      c->fs_pairs = true;
    }
  }
  if (!c->fs_pairs) { c->lay.mv_chunks = plain_chunks; c->lay.mv_chunk_off = plain_off; }
  c->n_chunks = static_cast<int>(c->lay.mv_chunks.size());  // (either list)
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
  c->fs_users = true;
}
// Small problems with uneven degrees (round 4): their segments are cut into pieces by build_range_worklists(); give
// every workgroup of the two-launch form WHOLE segments (layout.hpp: FusedLists) so that the pieces' partial rows meet
// in its LDS instead of in a combine launch.
void build_fused_lists(mmsbm_hip_ctx *c, const CreateKnobs &knobs, CreateLaps &lap) {
  const bool cut_p = !c->lay.pair_work.splits.empty(), cut_u = !c->lay.user_work.splits.empty();
  if (c->n_obs > kFusedRatingsMax || !fused_shape_ok(c) || knobs.no_fused_split || !(cut_p || cut_u)) return;
  if (cut_p) build_fused_pair_lists(c);
  if (cut_u) build_fused_user_lists(c, knobs);
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


// ---- the sessions' guards: one per question ------------------------------------------------------------------------
// The open session of one kind (`held`: where the context keeps it; `kind`: "recommend", "predict" ...), or
// "<kind>_begin has not been called"; with `what` (the entry asking) also at least one slot added to it, or
// "<what> before any <kind>_add"
template <class S>
S &require_open(mmsbm_hip_ctx *ctx, std::unique_ptr<S> mmsbm_hip_ctx::*held, const char *kind, const char *what = nullptr) {
  if (!ctx) throw std::invalid_argument("null context");
  S *s = (ctx->*held).get();
  if (!s) throw std::invalid_argument(std::string(kind) + "_begin has not been called");
  if (what && s->slots == 0) throw std::invalid_argument(std::string(what) + " before any " + kind + "_add");
  return *s;
}

// The four *_end entries: wait for the session's work, drop it.  `kind`: refuse when none is open (heldout_end)
template <class S>
int end_session(mmsbm_hip_ctx *ctx, std::unique_ptr<S> mmsbm_hip_ctx::*held, const char *kind = nullptr) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (kind) require_open(ctx, held, kind);
    use_device(ctx);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    (ctx->*held).reset();
  });
}

// ids[0 .. n) in [0, top), or "<prefix> id out of range at row m"
void require_ids(const int32_t *ids, int64_t n, int32_t top, const std::string &prefix) {
  for (int64_t m = 0; m < n; ++m)
    if (ids[m] < 0 || ids[m] >= top) throw std::invalid_argument(prefix + " id out of range at row " + std::to_string(m));
}

// The n of a top-N query of `who` ("recommend", "similar"), which returns `noun` ("items", "rows")
void require_n(int32_t n, const char *who, const char *noun) {
  if (n < 1) throw std::invalid_argument(std::string(who) + ": n must be at least 1");
  if (n > MMSBM_HIP_RECOMMEND_MAX_N)
    throw ApiError(MMSBM_E_UNSUPPORTED, std::string(who) + ": n = " + std::to_string(n) + " is beyond the " +
                                            std::to_string(MMSBM_HIP_RECOMMEND_MAX_N) + " " + noun + " a query returns at most");
}

// ---- the options: one row per name.  get: its value now; set: null for a read-only name, else the value's check and
// what setting it does.  mmsbm_hip_get_option and mmsbm_hip_set_option both walk this table and nothing else.
struct Option {
  const char *name;
  double (*get)(const mmsbm_hip_ctx *);
  void (*set)(mmsbm_hip_ctx *, double);
};
using Ctx = mmsbm_hip_ctx;
// "audience_rows" / "audience_entries" / "explain_rows" / "diverse_rows" / "group_run_blocks": 0 .. 2^31 - 1, whole
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
    {"fused", [](const Ctx *c) -> double { return c->fused; },
     [](Ctx *c, double v) {
       if (v != 0.0 && !fused_possible(c)) throw std::invalid_argument("fused: not available for this shape / data");
       c->fused = c->fused_forced = v != 0.0;
     }},
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
    // workgroups of gtop_fused_kernel (top_pairs.hpp); 0: the library's choice
    {"top_pairs_groups", [](const Ctx *c) -> double { return c->top_groups; },
     [](Ctx *c, double v) {
       if (v < 0 || v > 4096 || v != std::floor(v)) throw std::invalid_argument("top_pairs_groups: 0 .. 4096");
       c->top_groups = static_cast<int>(v);
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
    // the form FAMILY of an iteration at the current slot count: 2 = the two launches of fused_small.hpp, 4 = the separate
    // stages, with or without "pass_dense" -- the launches a committed iteration really takes are launches - pass_dense
    {"launches", [](const Ctx *c) -> double { return use_fused(c) ? 2 : 4; }, nullptr},
    // the triple passes and the T + S stage of a committed iteration in one launch (pass_dense.hpp).  Set: -1 the
    // library's choice by size, 0 off, 1 on wherever the form applies.  Reads 1 when the next committed iteration takes it
    {"pass_dense", [](const Ctx *c) -> double { return use_pass_dense(c) ? 1 : 0; },
     [](Ctx *c, double v) {
       if (v != -1.0 && v != 0.0 && v != 1.0) throw std::invalid_argument("pass_dense: -1, 0 or 1");
       c->pass_dense = static_cast<int>(v);
     }},
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
    {"fused_split", [](const Ctx *c) -> double { return (c->fs_pairs ? 1 : 0) + (c->fs_users ? 2 : 0); }, nullptr},
    // item_sum walks the fixed-width grid of pair ids (upload_item_grid)
    {"item_grid", [](const Ctx *c) -> double { return c->item_grid.count ? 1 : 0; }, nullptr},
    // the index's sorts ran on the device (build_index)
    {"gpu_layout", [](const Ctx *c) -> double { return c->gpu_layout ? 1 : 0; }, nullptr},
};
const Option *find_option(const std::string &name) {
  for (const Option &o : kOptions)
    if (name == o.name) return &o;
  return nullptr;
}
// A successful set drops the captured graphs: they hold the launches of the plan they were captured under
void set_option(mmsbm_hip_ctx *ctx, const std::string &name, double value) {
  const Option *o = find_option(name);
  if (!o || !o->set) throw std::invalid_argument("unknown option: " + name);
  o->set(ctx, value);
  ctx->drop_graphs();
}
}  // namespace


// ======================================================================================
// C ABI
// ======================================================================================
extern "C" {

int mmsbm_hip_abi_version(void) { return MMSBM_HIP_ABI_VERSION; }

#ifndef MMSBM_BUILD_ID
#define MMSBM_BUILD_ID "unknown"
#endif
const char *mmsbm_hip_build_id(void) { return MMSBM_BUILD_ID; }

const char *mmsbm_hip_last_error(void) { return g_last_error.c_str(); }

int mmsbm_hip_device_count(int *count) {
  return guarded([&] {
    if (!count) throw std::invalid_argument("null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
      *count = 0;
      throw ApiError(MMSBM_E_NODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
  });
}

int mmsbm_hip_device_info(int device, char *name, int name_len, int *compute_units,
                          int64_t *global_mem_bytes) {
  return guarded([&] {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (name && name_len > 0) {
      std::snprintf(name, static_cast<size_t>(name_len), "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (global_mem_bytes) *global_mem_bytes = static_cast<int64_t>(prop.totalGlobalMem);
  });
}

int mmsbm_hip_device_pci(int device, char *bus_id, int bus_id_len) {
  return guarded([&] {
    if (!bus_id || bus_id_len < 16) throw std::invalid_argument("bus_id buffer of at least 16 bytes needed");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      throw ApiError(MMSBM_E_NODEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) throw std::invalid_argument("device index out of range");
    HIP_CHECK(hipDeviceGetPCIBusId(bus_id, bus_id_len, device));
  });
}

int mmsbm_hip_device_mem(int device, int64_t *free_bytes, int64_t *total_bytes) {
  return guarded([&] {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      throw ApiError(MMSBM_E_NODEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) throw std::invalid_argument("device index out of range");
    int prev = 0;
    HIP_CHECK(hipGetDevice(&prev));
    HIP_CHECK(hipSetDevice(device));
    size_t f = 0, t = 0;
    const hipError_t e = hipMemGetInfo(&f, &t);
    (void)hipSetDevice(prev);
    if (e != hipSuccess) throw ApiError(MMSBM_E_HIP, std::string("hipMemGetInfo: ") + hipGetErrorString(e));
    if (free_bytes) *free_bytes = static_cast<int64_t>(f);
    if (total_bytes) *total_bytes = static_cast<int64_t>(t);
  });
}

int mmsbm_hip_create(int device, int64_t n_obs, int32_t n_users, int32_t n_items,
                     int32_t n_ratings, int32_t k_groups, int32_t l_groups,
                     const int32_t *user, const int32_t *item, const int32_t *rating,
                     int swap_sides, mmsbm_hip_ctx **out) {
  return guarded([&] {
    if (!out) throw std::invalid_argument("null out");
    *out = nullptr;
    if (k_groups <= 0 || l_groups <= 0) throw std::invalid_argument("K and L must be positive");
    if (static_cast<int64_t>(k_groups) * l_groups > (int64_t(1) << 26))
      throw ApiError(MMSBM_E_UNSUPPORTED, "K x L beyond 2^26 entries per rating tile");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      throw ApiError(MMSBM_E_NODEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) throw std::invalid_argument("device index out of range");

    const CreateKnobs knobs = read_create_knobs();
    CreateLaps lap{knobs.timing};
    std::unique_ptr<mmsbm_hip_ctx> c(new mmsbm_hip_ctx());
    plan_sides(c.get(), device, n_obs, n_users, n_items, n_ratings, k_groups, l_groups, swap_sides);
    const int32_t *iu = c->swapped ? item : user, *ii = c->swapped ? user : item;  // the id columns of the internal sides
    const PairPlan shape = plan_pair_shape(c->kp, c->lp, knobs.force_wide);
    lap("checks");
    open_device(c.get());
    const bool gpu_layout = build_index(c.get(), knobs, iu, ii, rating, lap);
    c->gpu_layout = gpu_layout;
    const std::vector<mmsbm::Chunk> units64 =
        apply_pair_plan(c.get(), plan_pair_forms(shape, c->lay.n_pairs, c->n_cus, knobs.no_mfma, knobs.mfma_chunk));
    build_range_worklists(c.get(), knobs, gpu_layout);
    lap("xcd-local work lists");
    build_fused_lists(c.get(), knobs, lap);
    // small problems (where eight rows in flight pay, plan_sides): two launches per iteration instead of four
    c->fused = n_obs <= kFusedRatingsMax && fused_possible(c.get()) && !knobs.no_fused;
    upload_index(c.get(), knobs, gpu_layout, units64, iu, ii, rating);
    lap("index uploads");
    alloc_state(c.get(), 1);
    c->lik_part.alloc(4096);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    lap("state allocation");
    *out = c.release();
  });
}

int mmsbm_hip_destroy(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (g_launch_log_on) launch_log().flush();
    delete ctx;
  });
}

int mmsbm_hip_dims(const mmsbm_hip_ctx *ctx, int64_t dims[8]) {
  return guarded([&] {
    if (!ctx || !dims) throw std::invalid_argument("null argument");
    dims[0] = ctx->n_obs; dims[1] = ctx->ext_users; dims[2] = ctx->ext_items;
    dims[3] = ctx->n_ratings; dims[4] = ctx->ext_k; dims[5] = ctx->ext_l;
    dims[6] = ctx->n_pairs; dims[7] = ctx->swapped ? 1 : 0;
  });
}

int mmsbm_hip_degrees(const mmsbm_hip_ctx *ctx, int64_t *d_user, int64_t *d_item) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    const mmsbm::Layout &L = ctx->lay;
    int64_t *du = ctx->swapped ? d_item : d_user;  // internal users
    int64_t *di = ctx->swapped ? d_user : d_item;  // internal items
    if (du)
      for (int u = 0; u < L.n_users; ++u)
        du[u] = std::max<int64_t>(L.user_off[u + 1] - L.user_off[u], 1);
    if (di)
      for (int i = 0; i < L.n_items; ++i) di[i] = std::max<int64_t>(L.item_deg[i], 1);
  });
}

// which: 0 .. 15 as mmsbm_hip_layout_array, 16 item_grid, 17 lik_units, 18 mv_chunk_off.  What has a device buffer is
// read back from it (the device-built pair_user / user_pair exist nowhere else); rating_off, chunk_off and chunks are
// host-only members of the context.
int mmsbm_hip_index_array(mmsbm_hip_ctx *ctx, int which, int32_t *out, int64_t capacity, int64_t *count) {
  return guarded([&] {
    if (!ctx || !count) throw std::invalid_argument("null argument");
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
  });
}

int mmsbm_hip_set_params(mmsbm_hip_ctx *ctx, const double *theta, const double *eta,
                         const double *pr) {
  return guarded([&] {
    if (!ctx || !theta || !eta || !pr) throw std::invalid_argument("null argument");
    use_device(ctx);
    OneSlot one(ctx);
    const double *it = ctx->swapped ? eta : theta;  // internal theta rows = internal users
    const double *ie = ctx->swapped ? theta : eta;
    const int cur = ctx->cur, sl = ctx->sel;
    HIP_CHECK(hipStreamSynchronize(ctx->stream));  // nothing in flight still reads the staging area
    ctx->pin.reset(rows_doubles(ctx));
    upload_rows(ctx, theta_tab(ctx, cur), it, ctx->n_users, ctx->k);
    upload_rows(ctx, eta_tab(ctx, cur), ie, ctx->n_items, ctx->l);
    const size_t klr = static_cast<size_t>(ctx->n_ratings) * ctx->kp * ctx->lp;
    double *p = ctx->pin.take(klr), *pt = ctx->pin.take(klr);
    p_host_to_dev(ctx, pr, p, pt);
    HIP_CHECK(hipMemcpyAsync(ctx->p[cur].at(sl), p, sizeof(double) * klr, hipMemcpyHostToDevice,
                             ctx->stream));
    HIP_CHECK(hipMemcpyAsync(ctx->pt[cur].at(sl), pt, sizeof(double) * klr, hipMemcpyHostToDevice,
                             ctx->stream));
    stage_matvec_a(ctx, cur, cur);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the staging area is free again
    ctx->have[sl] = 1;
    ctx->a_ok[sl] = 1;
  });
}

int mmsbm_hip_init_params(mmsbm_hip_ctx *ctx, const uint64_t pcg64_state[4], const double *pr) {
  return guarded([&] {
    if (!ctx || !pcg64_state || !pr) throw std::invalid_argument("null argument");
    use_device(ctx);
    OneSlot one(ctx);
    const int cur = ctx->cur, sl = ctx->sel;
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const size_t klr = static_cast<size_t>(ctx->n_ratings) * ctx->kp * ctx->lp;
    ctx->pin.reset(2 * klr);
    double *p = ctx->pin.take(klr), *pt = ctx->pin.take(klr);
    p_host_to_dev(ctx, pr, p, pt);
    HIP_CHECK(hipMemcpyAsync(ctx->p[cur].at(sl), p, sizeof(double) * klr, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(ctx->pt[cur].at(sl), pt, sizeof(double) * klr, hipMemcpyHostToDevice, ctx->stream));
    zero_rows(ctx, theta_tab(ctx, cur), ctx->n_users);  // padding columns
    zero_rows(ctx, eta_tab(ctx, cur), ctx->n_items);
    init_rows_launch(ctx, pcg64_state);
    stage_matvec_a(ctx, cur, cur);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->have[sl] = 1;
    ctx->a_ok[sl] = 1;
  });
}

int mmsbm_hip_pcg64_doubles(const uint64_t pcg64_state[4], uint64_t offset, int64_t n, double *out) {
  return guarded([&] {
    if (!pcg64_state || (n > 0 && !out) || n < 0) throw std::invalid_argument("bad argument");
    pcg64::Stream g{pcg64::make128(pcg64_state[0], pcg64_state[1]), pcg64::make128(pcg64_state[2], pcg64_state[3])};
    pcg64::advance(g, offset);
    for (int64_t j = 0; j < n; ++j) out[j] = pcg64::next_double(g);
  });
}

int mmsbm_hip_get_params(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr) {
  return guarded([&] {
    require_params(ctx);
    use_device(ctx);
    OneSlot one(ctx);
    double *it = ctx->swapped ? eta : theta;
    double *ie = ctx->swapped ? theta : eta;
    const int cur = ctx->cur, sl = ctx->sel;
    fetch_params(ctx, theta_tab(ctx, cur), eta_tab(ctx, cur),
                 ctx->p[cur].at(sl), it, ie, pr);
  });
}

int mmsbm_hip_set_slots(mmsbm_hip_ctx *ctx, int n_slots) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (n_slots < 1 || n_slots > 65535) throw std::invalid_argument("n_slots must be in [1, 65535]");
    use_device(ctx);
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
  });
}

int mmsbm_hip_select_slot(mmsbm_hip_ctx *ctx, int slot) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (slot < 0 || slot >= ctx->n_slots)
      throw std::invalid_argument("slot " + std::to_string(slot) + " out of range (the context has " +
                                  std::to_string(ctx->n_slots) + ")");
    ctx->sel = slot;
  });
}

int mmsbm_hip_slots(const mmsbm_hip_ctx *ctx, int *n_slots, int *selected,
                    int64_t *bytes_per_slot) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (n_slots) *n_slots = ctx->n_slots;
    if (selected) *selected = ctx->sel;
    if (bytes_per_slot) {
      size_t d = ctx->ctab.stride + ctx->ttab.stride + ctx->partial.stride + ctx->npr.stride +
                 ctx->pair_parts.stride + ctx->user_parts.stride;
      for (int b = 0; b < 2; ++b)
        d += ctx->theta[b].stride + ctx->eta[b].stride + ctx->p[b].stride + ctx->pt[b].stride +
             ctx->atab[b].stride;
      *bytes_per_slot = static_cast<int64_t>(d * sizeof(double));
    }
  });
}

int mmsbm_hip_em_iterate(mmsbm_hip_ctx *ctx, int n_iters) {
  return guarded([&] {
    require_all_params(ctx);
    if (n_iters < 0) throw std::invalid_argument("n_iters must be >= 0");
    use_device(ctx);
    run_iterations(ctx, n_iters);
  });
}

int mmsbm_hip_synchronize(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    use_device(ctx);
    // Short waits are polled (hipStreamQuery returns within a microsecond or two of the last kernel;
    // a blocking wait is woken by an interrupt tens of microseconds later, which is several percent
    // of a 2 ms run of 20 iterations); after 50 ms the thread blocks like any other waiter.
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t e = hipStreamQuery(ctx->stream);
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) HIP_CHECK(e);
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  });
}

int mmsbm_hip_update_coefficients(mmsbm_hip_ctx *ctx, double *n_theta, double *n_eta,
                                  double *n_pr) {
  return guarded([&] {
    require_params(ctx);
    use_device(ctx);
    OneSlot one(ctx);
    launch_iteration(ctx, false);
    const int nxt = ctx->cur ^ 1, sl = ctx->sel;
    double *it = ctx->swapped ? n_eta : n_theta;
    double *ie = ctx->swapped ? n_theta : n_eta;
    fetch_params(ctx, theta_tab(ctx, nxt), eta_tab(ctx, nxt),
                 ctx->npr.at(sl), it, ie, n_pr);
  });
}

namespace {
double likelihood_finish(mmsbm_hip_ctx *ctx, int nb) {  // workgroup sums added in workgroup order
  std::vector<double> part(nb);
  HIP_CHECK(hipMemcpyAsync(part.data(), ctx->lik_part.ptr, sizeof(double) * nb, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  double tot = 0.0;
  for (double v : part) tot += v;
  return tot;
}
}  // namespace

int mmsbm_hip_likelihood(mmsbm_hip_ctx *ctx, double *out) {
  return guarded([&] {
    require_params(ctx);
    if (!out) throw std::invalid_argument("null out");
    use_device(ctx);
    OneSlot one(ctx);
    *out = likelihood_finish(ctx, likelihood_enqueue(ctx));
  });
}

int mmsbm_hip_result(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr, double *likelihood) {
  return guarded([&] {
    require_params(ctx);
    if (!likelihood) throw std::invalid_argument("null likelihood");
    use_device(ctx);
    OneSlot one(ctx);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the parameters are final
    const int nb = likelihood_enqueue(ctx);        // the likelihood kernels run ...
    struct Xfer {                                   // ... while the tables travel on the copy stream and are unpacked
      mmsbm_hip_ctx *c;
      explicit Xfer(mmsbm_hip_ctx *x) : c(x) { c->xfer = c->copy_stream; }
      ~Xfer() { c->xfer = nullptr; }
    };
    {
      Xfer on(ctx);
      double *it = ctx->swapped ? eta : theta;
      double *ie = ctx->swapped ? theta : eta;
      fetch_params(ctx, theta_tab(ctx, ctx->cur), eta_tab(ctx, ctx->cur),
                   ctx->p[ctx->cur].at(ctx->sel), it, ie, pr);
    }
    *likelihood = likelihood_finish(ctx, nb);
  });
}

int mmsbm_hip_compute_omegas(mmsbm_hip_ctx *ctx, double *out, int64_t capacity_elems) {
  return guarded([&] {
    require_params(ctx);
    if (!out) throw std::invalid_argument("null out");
    use_device(ctx);
    const int64_t kl = static_cast<int64_t>(ctx->k) * ctx->l;
    const int64_t n_elems = ctx->n_obs * kl;
    if (n_elems > capacity_elems)
      throw ApiError(MMSBM_E_TOOLARGE, "omega tensor larger than the caller's buffer");
    if (n_elems > (int64_t(1) << 31))  // 16 GiB: the factorised path exists so nobody needs this
      throw ApiError(MMSBM_E_TOOLARGE, "omega tensor above the 2^31-element cap");
    if (n_elems == 0) return;
    DevBuf<double> dev;
    dev.alloc(static_cast<size_t>(n_elems));
    OneSlot one(ctx);
    omegas_launch(ctx, dev.ptr, n_elems);
    HIP_CHECK(hipMemcpyAsync(out, dev.ptr, sizeof(double) * n_elems, hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  });
}

namespace {
// ---- prod_dist / predict through B = p_r eta_i over every (item, rating) combination ---------------
// Worth it when the rows to score are not far fewer than the items (B costs I R K L multiply-adds, a row
// then R K instead of R K L) and B fits comfortably: otherwise the per-row kernels run.
bool rows_fast_ok(const mmsbm_hip_ctx *c, int64_t n_rows) {
  if (!c->predict_fast || n_rows <= 0) return false;
  const uint64_t combos = static_cast<uint64_t>(c->n_items) * static_cast<uint64_t>(c->n_ratings);
  if (combos >= (uint64_t(1) << 31) - 2048 || n_rows * 4 < c->n_items) return false;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
  return combos * static_cast<uint64_t>(c->kp) * sizeof(double) <= (free_b + c->btab.count * sizeof(double)) / 2;
}
void ensure_pair_grid(mmsbm_hip_ctx *c) {  // q = r * I + i, chunks of the pair stage's size per rating
  const size_t combos = static_cast<size_t>(c->n_items) * c->n_ratings;
  if (c->grid_item.count != combos || c->grid_n_chunks == 0) {
    std::vector<int32_t> item(combos);
    std::vector<mmsbm::Chunk> chunks;
    for (int r = 0; r < c->n_ratings; ++r) {
      const int32_t base = static_cast<int32_t>(static_cast<size_t>(r) * c->n_items);
      for (int i = 0; i < c->n_items; ++i) item[static_cast<size_t>(base) + i] = i;
      for (int i = 0; i < c->n_items; i += c->pp.chunk_pairs)
        chunks.push_back(mmsbm::Chunk{r, base + i, base + std::min(i + c->pp.chunk_pairs, c->n_items), 0});
    }
    c->grid_item.upload(item, c->stream);
    c->grid_chunks.upload(chunks, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));  // (host vectors are locals)
    c->grid_n_chunks = static_cast<int>(chunks.size());
  }
  if (c->btab.count < combos * c->kp) c->btab.alloc(combos * c->kp);
}
// eligibility + the table's memory; false (and no error left behind) sends the caller to the per-row kernels
bool rows_fast_prepare(mmsbm_hip_ctx *c, int64_t n_rows) {
  if (!rows_fast_ok(c, n_rows)) return false;
  try {
    ensure_pair_grid(c);
  } catch (const ApiError &) {  // out of memory after all (another context took it): not an error of this call
    (void)hipGetLastError();
    c->btab.release();
    return false;
  }
  return true;
}
}  // namespace

int mmsbm_hip_prod_dist(mmsbm_hip_ctx *ctx, int64_t n_pairs, const int32_t *user,
                        const int32_t *item, double *out) {
  return guarded([&] {
    require_params(ctx);
    if (n_pairs < 0) throw std::invalid_argument("negative n_pairs");
    if (n_pairs == 0) return;
    if (!user || !item || !out) throw std::invalid_argument("null argument");
    for (int64_t m = 0; m < n_pairs; ++m)
      if (user[m] < 0 || user[m] >= ctx->ext_users || item[m] < 0 || item[m] >= ctx->ext_items)
        throw std::invalid_argument("prod_dist: id out of range at row " + std::to_string(m));
    use_device(ctx);
    const int64_t n_elems = n_pairs * ctx->n_ratings;
    if ((n_elems + kBlock - 1) / kBlock > (int64_t(1) << 31) - 1)
      throw ApiError(MMSBM_E_TOOLARGE, "prod_dist: too many pairs for one launch");
    DevBuf<int32_t> du, di;
    DevBuf<double> dout;
    du.alloc(n_pairs); di.alloc(n_pairs); dout.alloc(n_elems);
    const int32_t *iu = ctx->swapped ? item : user;
    const int32_t *ii = ctx->swapped ? user : item;
    HIP_CHECK(hipMemcpyAsync(du.ptr, iu, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(di.ptr, ii, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
    OneSlot one(ctx);
    if (rows_fast_prepare(ctx, n_pairs)) rows_launch(ctx, 0, du.ptr, di.ptr, nullptr, nullptr, dout.ptr, nullptr, n_pairs, 1);
    else prod_dist_launch(ctx, du.ptr, di.ptr, dout.ptr, n_pairs);
    HIP_CHECK(hipMemcpyAsync(out, dout.ptr, sizeof(double) * n_elems, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->btab.release();  // (the B table is scratch: restart slots are sized from the free memory)
  });
}

namespace {
void score_launch(mmsbm_hip_ctx *ctx, bool finish, double *stats) {
  const int n_stats = score_stats_count();
  PredictSession &ps = *ctx->ps;
  const bool fast = !finish && rows_fast_prepare(ctx, ps.rows);
  const int per_block = fast ? kBlock / group_lanes(ctx->code_k) : kBlock;
  const int nb = static_cast<int>((ps.rows + per_block - 1) / per_block);
  if (ps.part.count < static_cast<size_t>(nb) * n_stats) ps.part.alloc(static_cast<size_t>(nb) * n_stats);
  if (nb > 0 && fast)
    rows_launch(ctx, 1, ps.u.ptr, ps.i.ptr, ps.r.ptr, ps.w.ptr, ps.sum.ptr, ps.part.ptr, ps.rows, ps.slots == 0 ? 1 : 0);
  else if (nb > 0)
    score_rows_launch(ctx, finish);
  std::vector<double> part(static_cast<size_t>(nb) * n_stats);
  if (nb > 0)
    HIP_CHECK(hipMemcpyAsync(part.data(), ps.part.ptr, sizeof(double) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (int j = 0; j < n_stats; ++j) stats[j] = 0.0;
  for (int b = 0; b < nb; ++b)
    for (int j = 0; j < n_stats; ++j) stats[j] += part[static_cast<size_t>(b) * n_stats + j];
}
}  // namespace

int mmsbm_hip_predict_begin(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user,
                            const int32_t *item, const int32_t *rating,
                            const double *rating_weights) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (n_rows < 0) throw std::invalid_argument("negative n_rows");
    if (!rating_weights || (n_rows > 0 && (!user || !item || !rating)))
      throw std::invalid_argument("null argument");
    if (n_rows > (int64_t(1) << 31) - kBlock)
      throw ApiError(MMSBM_E_TOOLARGE, "predict: too many rows for one launch");
    for (int64_t m = 0; m < n_rows; ++m)
      if (user[m] < 0 || user[m] >= ctx->ext_users || item[m] < 0 || item[m] >= ctx->ext_items ||
          rating[m] < 0 || rating[m] >= ctx->n_ratings)
        throw std::invalid_argument("predict: id out of range at row " + std::to_string(m));
    use_device(ctx);
    ctx->ps.reset();  // (arguments are fine: from here on the previous session is gone)
    auto ps = std::make_unique<PredictSession>();
    const int32_t *iu = ctx->swapped ? item : user;
    const int32_t *ii = ctx->swapped ? user : item;
    hipStream_t s = ctx->stream;
    ps->u.alloc(n_rows); ps->i.alloc(n_rows); ps->r.alloc(n_rows);
    ps->sum.alloc(static_cast<size_t>(n_rows) * ctx->n_ratings);
    ps->w.alloc(ctx->n_ratings);
    if (n_rows > 0) {
      HIP_CHECK(hipMemcpyAsync(ps->u.ptr, iu, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(ps->i.ptr, ii, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(ps->r.ptr, rating, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipMemcpyAsync(ps->w.ptr, rating_weights, sizeof(double) * ctx->n_ratings, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));  // the caller's buffers are free again
    ps->rows = n_rows;
    ctx->ps = std::move(ps);
  });
}

int mmsbm_hip_predict_add(mmsbm_hip_ctx *ctx, double stats[6]) {
  return guarded([&] {
    require_params(ctx);
    if (!stats) throw std::invalid_argument("null stats");
    PredictSession &ps = require_open(ctx, &mmsbm_hip_ctx::ps, "predict");
    use_device(ctx);
    OneSlot one(ctx);
    score_launch(ctx, false, stats);
    ps.slots++;
  });
}

int mmsbm_hip_predict_finish(mmsbm_hip_ctx *ctx, double *mean_dist, double stats[6]) {
  return guarded([&] {
    if (!ctx || !stats) throw std::invalid_argument("null argument");
    const PredictSession &ps = require_open(ctx, &mmsbm_hip_ctx::ps, "predict", "predict_finish");
    use_device(ctx);
    OneSlot one(ctx);
    // the session is over on every way out of here, and its buffers go back: restart slots are sized from the free memory
    struct Drop { mmsbm_hip_ctx *c; ~Drop() { c->ps.reset(); } } drop{ctx};
    score_launch(ctx, true, stats);
    ctx->btab.release();
    if (mean_dist && ps.rows > 0) {
      HIP_CHECK(hipMemcpyAsync(mean_dist, ps.sum.ptr, sizeof(double) * ps.rows * ctx->n_ratings, hipMemcpyDeviceToHost,
                               ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
  });
}

namespace {
// A CSR argument of `rows` ranges (none when off is null): off[0] == 0, never decreasing, a total below 2^31 and
// val[0 .. total) in [0, top).  Messages "<who>: <off_name>[0] must be 0", "<who>: <off_name> decrease at <row> b",
// "<who>: more than 2^31 - 1 <vals>", "<who>: <val_name> out of range at entry e".
void check_csr(const int64_t *off, const int32_t *val, int64_t rows, int32_t top, const char *who,
               const char *off_name, const char *row, const char *vals, const char *val_name) {
  if (!off || rows == 0) return;
  const std::string w = std::string(who) + ": ";
  if (off[0] != 0) throw std::invalid_argument(w + off_name + "[0] must be 0");
  for (int64_t b = 0; b < rows; ++b)
    if (off[b + 1] < off[b])
      throw std::invalid_argument(w + off_name + " decrease at " + row + " " + std::to_string(b));
  const int64_t total = off[rows];
  if (total > INT32_MAX) throw std::invalid_argument(w + "more than 2^31 - 1 " + vals);
  if (total > 0 && !val) throw std::invalid_argument("null argument");
  for (int64_t e = 0; e < total; ++e)
    if (val[e] < 0 || val[e] >= top)
      throw std::invalid_argument(w + val_name + " out of range at entry " + std::to_string(e));
}

// Both fold-in entries: new users (user[m] in [0, n_new), K groups) or, items_side, new items (item[m], L groups)
int fold_entry(mmsbm_hip_ctx *ctx, bool items_side, int64_t n_rows, const int32_t *user, const int32_t *item,
               const int32_t *rating, int32_t n_new, int32_t n_iters, double tol, const double *x0, double *x,
               int32_t *iters) {
  return guarded([&] {
    require_params(ctx);
    const std::string what = items_side ? "fold_in_items" : "fold_in";
    if (n_rows < 0 || n_rows > INT32_MAX) throw std::invalid_argument(what + ": n_rows outside [0, 2^31)");
    if (n_new < 0) throw std::invalid_argument(what + ": negative n_new");
    if (n_iters < 0) throw std::invalid_argument(what + ": negative n_iters");
    const int groups = items_side ? ctx->ext_l : ctx->ext_k;
    if (groups > MMSBM_HIP_FOLD_IN_MAX_K)
      throw ApiError(MMSBM_E_UNSUPPORTED, what + (items_side ? ": L = " : ": K = ") + std::to_string(groups) +
                                              " is beyond the " + std::to_string(MMSBM_HIP_FOLD_IN_MAX_K) +
                                              " groups it is built for");
    if (n_rows > 0 && (!user || !item || !rating)) throw std::invalid_argument("null argument");
    if (n_new > 0 && !x) throw std::invalid_argument("null argument");
    const int32_t n_users = items_side ? ctx->ext_users : n_new, n_items = items_side ? n_new : ctx->ext_items;
    for (int64_t m = 0; m < n_rows; ++m) {
      if (user[m] < 0 || user[m] >= n_users)
        throw std::invalid_argument(what + ": user id out of range at row " + std::to_string(m));
      if (item[m] < 0 || item[m] >= n_items)
        throw std::invalid_argument(what + ": item id out of range at row " + std::to_string(m));
      if (rating[m] < 0 || rating[m] >= ctx->n_ratings)
        throw std::invalid_argument(what + ": rating id out of range at row " + std::to_string(m));
    }
    use_device(ctx);
    OneSlot one(ctx);
    fold_in(ctx, items_side, n_rows, user, item, rating, n_new, n_iters, tol, x0, x, iters);
  });
}
}  // namespace

int mmsbm_hip_recommend_begin(mmsbm_hip_ctx *ctx, const double *rating_weights, int exclude_train) {
  return guarded([&] {
    if (!ctx || !rating_weights) throw std::invalid_argument("null argument");
    for (int r = 0; r < ctx->n_ratings; ++r)  // (a NaN score has no place in the order; +-inf is not a score)
      if (!std::isfinite(rating_weights[r]))
        throw std::invalid_argument("recommend: rating weight " + std::to_string(r) + " is not finite");
    recommend_begin(ctx, rating_weights, exclude_train);
  });
}

int mmsbm_hip_recommend_add(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    if (require_open(ctx, &mmsbm_hip_ctx::rc, "recommend").items != ctx->ext_items)
      throw std::invalid_argument("recommend_add after recommend_add_items: the added items hold no row of this slot");
    OneSlot one(ctx);
    recommend_add(ctx);
  });
}

int mmsbm_hip_recommend_query(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n, int32_t *items,
                              double *scores, int32_t *counts) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend: user");
    recommend_query(ctx, n_users, users, n, items, scores, counts);
  });
}

int mmsbm_hip_recommend_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::rc); }

int mmsbm_hip_recommend_query_theta(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                    const int64_t *seen_offsets, const int32_t *seen_items, int32_t n,
                                    int32_t *items, double *scores, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_theta");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!theta || !items)) throw std::invalid_argument("null argument");
    check_csr(seen_offsets, seen_items, n_users, rc.items, "recommend", "seen_offsets", "user", "seen items",
              "seen item");
    recommend_query_theta(ctx, n_users, theta, seen_offsets, seen_items, n, items, scores, counts);
  });
}

int mmsbm_hip_recommend_positions(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users,
                                  const int64_t *offsets, const int32_t *items, int32_t *positions,
                                  int32_t *candidates) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_positions");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    if (n_users > 0 && (!users || !offsets)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend_positions: user");
    check_csr(offsets, items, n_users, rc.items, "recommend_positions", "offsets", "user", "items", "item id");
    if (n_users > 0 && offsets[n_users] > 0 && !positions) throw std::invalid_argument("null argument");
    recommend_positions(ctx, n_users, users, offsets, items, positions, candidates);
  });
}

int mmsbm_hip_recommend_add_items(mmsbm_hip_ctx *ctx, int32_t n_new, const double *eta,
                                  const int64_t *seen_offsets, const int32_t *seen_users) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_add_items");
    if (rc.items != ctx->ext_items)
      throw std::invalid_argument("recommend_add_items: the session already holds added items");
    if (n_new < 0) throw std::invalid_argument("recommend_add_items: negative n_new");
    if (static_cast<int64_t>(ctx->ext_items) + n_new > INT32_MAX)
      throw std::invalid_argument("recommend_add_items: more than 2^31 - 1 items in the catalogue");
    if (n_new > 0 && !eta) throw std::invalid_argument("null argument");
    check_csr(seen_offsets, seen_users, n_new, ctx->ext_users, "recommend_add_items", "seen_offsets", "item",
              "seen users", "seen user");
    recommend_add_items(ctx, n_new, eta, seen_offsets, seen_users);
  });
}

int mmsbm_hip_recommend_top_pairs(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t m,
                                  int32_t *out_users, int32_t *out_items, double *out_scores, int32_t *count) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_top_pairs");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    if (m < 1) throw std::invalid_argument("top_pairs: m must be at least 1");
    if (m > MMSBM_HIP_TOP_PAIRS_MAX_M)
      throw ApiError(MMSBM_E_UNSUPPORTED, "top_pairs: m = " + std::to_string(m) + " is beyond the " +
                                              std::to_string(MMSBM_HIP_TOP_PAIRS_MAX_M) + " pairs a query returns at most");
    if (!out_users || !out_items || !out_scores || !count) throw std::invalid_argument("null argument");
    // the request in id order (ties go by user id; the kernel walks the users in this order), every training user
    // when `users` is null; a repeated id would put its pairs into the order twice
    std::vector<int32_t> ids;
    if (users) {
      require_ids(users, n_users, ctx->ext_users, "top_pairs: user");
      ids.assign(users, users + n_users);
      std::sort(ids.begin(), ids.end());
      const auto twice = std::adjacent_find(ids.begin(), ids.end());
      if (twice != ids.end()) throw std::invalid_argument("top_pairs: user id " + std::to_string(*twice) + " is repeated");
    } else {
      ids.resize(static_cast<size_t>(ctx->ext_users));
      for (int32_t u = 0; u < ctx->ext_users; ++u) ids[static_cast<size_t>(u)] = u;
    }
    recommend_top_pairs(ctx, static_cast<int64_t>(ids.size()), ids.data(), m, out_users, out_items, out_scores, count);
  });
}

int mmsbm_hip_recommend_query_items(mmsbm_hip_ctx *ctx, int64_t n_items, const int32_t *items, int32_t n,
                                    int32_t *users, double *scores, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_items");
    if (n_items < 0) throw std::invalid_argument("negative n_items");
    require_n(n, "recommend", "items");
    if (n_items > 0 && (!items || !users)) throw std::invalid_argument("null argument");
    require_ids(items, n_items, rc.items, "recommend_query_items: item");
    recommend_query_items(ctx, n_items, items, n, users, scores, counts);
  });
}

int mmsbm_hip_recommend_audience(mmsbm_hip_ctx *ctx, int64_t n_items, const int32_t *items, double min_score,
                                 int64_t capacity, int64_t *offsets, int32_t *users, double *scores) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_audience");
    if (n_items < 0) throw std::invalid_argument("negative n_items");
    if (!std::isfinite(min_score)) throw std::invalid_argument("audience: min_score is not finite");
    if (!offsets || (n_items > 0 && !items) || (users && !scores)) throw std::invalid_argument("null argument");
    if (users && capacity < 0) throw std::invalid_argument("audience: negative capacity");
    require_ids(items, n_items, rc.items, "audience: item");
    recommend_audience(ctx, n_items, items, min_score, capacity, offsets, users, scores);
  });
}

namespace {
// A candidate list of `who`: v[0 .. n) strictly ascending (so distinct) ids in [0, top)
void require_candidates(const int32_t *v, int64_t first, int64_t n, int32_t top, const char *who) {
  for (int64_t e = 0; e < n; ++e) {
    if (v[e] < 0 || v[e] >= top)
      throw std::invalid_argument(std::string(who) + ": candidate item id out of range at entry " + std::to_string(first + e));
    if (e > 0 && v[e] <= v[e - 1])
      throw std::invalid_argument(std::string(who) + ": candidate items must be ascending and distinct (entry " +
                                  std::to_string(first + e) + ")");
  }
}
// n_cand / cand_items of the two *_within entries (cand_items null: the whole catalogue, n_cand ignored)
void require_subset(const int32_t *cand_items, int32_t n_cand, int32_t top, const char *who) {
  if (!cand_items) return;
  if (n_cand < 0 || n_cand > top)
    throw std::invalid_argument(std::string(who) + ": n_cand outside [0, items of the catalogue]");
  require_candidates(cand_items, 0, n_cand, top, who);
}
}  // namespace

int mmsbm_hip_recommend_query_within(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                     const int32_t *cand_items, const int64_t *excl_offsets,
                                     const int32_t *excl_items, int32_t n, int32_t *items, double *scores,
                                     int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_within");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend: user");
    require_subset(cand_items, n_cand, rc.items, "recommend_query_within");
    check_csr(excl_offsets, excl_items, n_users, rc.items, "recommend_query_within", "excl_offsets", "user",
              "excluded items", "excluded item");
    recommend_query_within(ctx, n_users, users, cand_items, n_cand, n_users > 0 ? excl_offsets : nullptr, excl_items, n,
                           items, scores, counts);
  });
}

int mmsbm_hip_recommend_query_theta_within(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                           const int64_t *seen_offsets, const int32_t *seen_items, int32_t n_cand,
                                           const int32_t *cand_items, int32_t n, int32_t *items, double *scores,
                                           int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_theta_within");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!theta || !items)) throw std::invalid_argument("null argument");
    require_subset(cand_items, n_cand, rc.items, "recommend_query_theta_within");
    check_csr(seen_offsets, seen_items, n_users, rc.items, "recommend", "seen_offsets", "user", "seen items",
              "seen item");
    recommend_query_theta_within(ctx, n_users, theta, seen_offsets, seen_items, cand_items, n_cand, n, items, scores,
                                 counts);
  });
}

int mmsbm_hip_recommend_rank(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, const int64_t *offsets,
                             const int32_t *cand_items, int32_t n, int32_t *items, double *scores, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_rank");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!users || !offsets || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend_rank: user");
    check_csr(offsets, cand_items, n_users, rc.items, "recommend_rank", "offsets", "user", "candidate items",
              "candidate item id");
    for (int64_t b = 0; b < n_users; ++b)
      require_candidates(cand_items + offsets[b], offsets[b], offsets[b + 1] - offsets[b], rc.items, "recommend_rank");
    recommend_rank(ctx, n_users, users, offsets, cand_items, n, items, scores, counts);
  });
}

int mmsbm_hip_similar_begin(mmsbm_hip_ctx *ctx, int side) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (side != 0 && side != 1) throw std::invalid_argument("similar: side must be 0 (items) or 1 (users)");
    similar_begin(ctx, side);
  });
}

int mmsbm_hip_similar_add(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    require_open(ctx, &mmsbm_hip_ctx::sm, "similar");
    OneSlot one(ctx);
    similar_add(ctx);
  });
}

int mmsbm_hip_similar_query(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *ids, int32_t n, int32_t *out_ids,
                            double *distance, int32_t *counts) {
  return guarded([&] {
    const SimSession &sm = require_open(ctx, &mmsbm_hip_ctx::sm, "similar", "similar_query");
    if (n_rows < 0) throw std::invalid_argument("negative n_rows");
    require_n(n, "similar", "rows");
    if (n_rows > 0 && (!ids || !out_ids)) throw std::invalid_argument("null argument");
    require_ids(ids, n_rows, sm.rows, sm.side == 0 ? "similar: item" : "similar: user");
    similar_query(ctx, n_rows, ids, n, out_ids, distance, counts);
  });
}

int mmsbm_hip_similar_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::sm); }

int mmsbm_hip_similar_pairs(mmsbm_hip_ctx *ctx, int64_t n_pairs, const int32_t *a, const int32_t *b, double *distance) {
  return guarded([&] {
    const SimSession &sm = require_open(ctx, &mmsbm_hip_ctx::sm, "similar", "similar_pairs");
    if (n_pairs < 0) throw std::invalid_argument("negative n_pairs");
    if (n_pairs > 0 && (!a || !b || !distance)) throw std::invalid_argument("null argument");
    const char *who = sm.side == 0 ? "similar_pairs: item" : "similar_pairs: user";
    require_ids(a, n_pairs, sm.rows, who);
    require_ids(b, n_pairs, sm.rows, who);
    similar_pairs(ctx, n_pairs, a, b, distance);
  });
}

int mmsbm_hip_recommend_diverse(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                const int32_t *cand_items, const int64_t *excl_offsets, const int32_t *excl_items,
                                int32_t n, int32_t pool, double trade_off, int32_t *items, double *scores,
                                double *distances, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_diverse");
    const SimSession &sm = require_open(ctx, &mmsbm_hip_ctx::sm, "similar", "recommend_diverse");
    if (sm.side != 0) throw std::invalid_argument("recommend_diverse: the similarity session is over the users");
    if (sm.slots != rc.slots)
      throw std::invalid_argument("recommend_diverse: the recommend session holds " + std::to_string(rc.slots) +
                                  " slots, the similarity session " + std::to_string(sm.slots));
    if (rc.items != sm.rows)
      throw std::invalid_argument("recommend_diverse: the recommend session's catalogue holds added items");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    if (n < 1) throw std::invalid_argument("recommend_diverse: n must be at least 1");
    if (pool < n) throw std::invalid_argument("recommend_diverse: pool must be at least n");
    if (!std::isfinite(trade_off) || trade_off < 0.0)
      throw std::invalid_argument("recommend_diverse: trade_off must be finite and at least 0");
    require_n(pool, "recommend_diverse", "pool entries");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend_diverse: user");
    require_subset(cand_items, n_cand, rc.items, "recommend_diverse");
    check_csr(excl_offsets, excl_items, n_users, rc.items, "recommend_diverse", "excl_offsets", "user", "excluded items",
              "excluded item");
    recommend_diverse(ctx, n_users, users, cand_items, n_cand, n_users > 0 ? excl_offsets : nullptr, excl_items, n, pool,
                      trade_off, items, scores, distances, counts);
  });
}

int mmsbm_hip_recommend_query_groups(mmsbm_hip_ctx *ctx, int64_t n_groups, const int64_t *offsets,
                                     const int32_t *members, int mode, double bar, int32_t n_cand,
                                     const int32_t *cand_items, int32_t n, int32_t *items, double *scores,
                                     int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_groups");
    if (n_groups < 0) throw std::invalid_argument("negative n_groups");
    if (mode != MMSBM_HIP_GROUP_MIN && mode != MMSBM_HIP_GROUP_MAX && mode != MMSBM_HIP_GROUP_COUNT &&
        mode != MMSBM_HIP_GROUP_MEAN)
      throw std::invalid_argument("recommend_query_groups: unknown mode " + std::to_string(mode));
    if (mode == MMSBM_HIP_GROUP_COUNT && !std::isfinite(bar))
      throw std::invalid_argument("recommend_query_groups: bar must be finite");
    require_n(n, "recommend_query_groups", "items");
    if (n_groups > 0 && (!offsets || !items)) throw std::invalid_argument("null argument");
    check_csr(offsets, members, n_groups, ctx->ext_users, "recommend_query_groups", "offsets", "group", "members",
              "member");
    // distinct within a group: last[u] = the last group that named user u
    std::vector<int64_t> last(static_cast<size_t>(ctx->ext_users), -1);
    for (int64_t g = 0; g < n_groups; ++g)
      for (int64_t e = offsets[g]; e < offsets[g + 1]; ++e) {
        if (last[static_cast<size_t>(members[e])] == g)
          throw std::invalid_argument("recommend_query_groups: member repeated in group " + std::to_string(g) +
                                      " at entry " + std::to_string(e));
        last[static_cast<size_t>(members[e])] = g;
      }
    require_subset(cand_items, n_cand, rc.items, "recommend_query_groups");
    recommend_query_groups(ctx, n_groups, offsets, members, mode, bar, cand_items, n_cand, n, items, scores, counts);
  });
}

int mmsbm_hip_recommend_query_ensemble(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int mode, double risk,
                                       int32_t n_cand, const int32_t *cand_items, const int64_t *excl_offsets,
                                       const int32_t *excl_items, int32_t n, int32_t *items, double *scores,
                                       int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_ensemble");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    if (mode != MMSBM_HIP_ENSEMBLE_MIN && mode != MMSBM_HIP_ENSEMBLE_MAX && mode != MMSBM_HIP_ENSEMBLE_LCB)
      throw std::invalid_argument("recommend_query_ensemble: unknown mode " + std::to_string(mode));
    if (mode == MMSBM_HIP_ENSEMBLE_LCB && !std::isfinite(risk))
      throw std::invalid_argument("recommend_query_ensemble: risk must be finite");
    require_n(n, "recommend_query_ensemble", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend_query_ensemble: user");
    require_subset(cand_items, n_cand, rc.items, "recommend_query_ensemble");
    check_csr(excl_offsets, excl_items, n_users, rc.items, "recommend_query_ensemble", "excl_offsets", "user",
              "excluded items", "excluded item");
    recommend_query_ensemble(ctx, n_users, users, mode, risk, cand_items, n_cand, n_users > 0 ? excl_offsets : nullptr,
                             excl_items, n, items, scores, counts);
  });
}

int mmsbm_hip_recommend_pair_spread(mmsbm_hip_ctx *ctx, int64_t n_pairs, const int32_t *users, const int32_t *items,
                                    double *stats, double *per_slot) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_pair_spread");
    if (n_pairs < 0) throw std::invalid_argument("negative n_pairs");
    if (n_pairs > 0 && (!users || !items || !stats)) throw std::invalid_argument("null argument");
    require_ids(users, n_pairs, ctx->ext_users, "recommend_pair_spread: user");
    require_ids(items, n_pairs, rc.items, "recommend_pair_spread: item");
    recommend_pair_spread(ctx, n_pairs, users, items, stats, per_slot);
  });
}

int mmsbm_hip_inform_begin(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    inform_begin(ctx);
  });
}

int mmsbm_hip_inform_add(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    require_open(ctx, &mmsbm_hip_ctx::inf, "inform");
    OneSlot one(ctx);
    inform_add(ctx);
  });
}

int mmsbm_hip_inform_query(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                           const int32_t *cand_items, const int64_t *excl_offsets, const int32_t *excl_items,
                           int exclude_train, int32_t n, int32_t *items, double *gains, int32_t *counts) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::inf, "inform", "inform_query");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "inform", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "inform: user");
    require_subset(cand_items, n_cand, ctx->ext_items, "inform_query");
    check_csr(excl_offsets, excl_items, n_users, ctx->ext_items, "inform_query", "excl_offsets", "user",
              "excluded items", "excluded item");
    inform_query(ctx, n_users, users, cand_items, n_cand, n_users > 0 ? excl_offsets : nullptr, excl_items,
                 exclude_train != 0, n, items, gains, counts);
  });
}

int mmsbm_hip_inform_query_theta(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                                 const int32_t *seen_items, int32_t n_cand, const int32_t *cand_items, int32_t n,
                                 int32_t *items, double *gains, int32_t *counts) {
  return guarded([&] {
    const InfSession &inf = require_open(ctx, &mmsbm_hip_ctx::inf, "inform", "inform_query_theta");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "inform", "items");
    if (n_users > 0 && (!theta || !items)) throw std::invalid_argument("null argument");
    // (a NaN gain has no place in the order, and the entropy of a negative weight is not one)
    const size_t n_theta = static_cast<size_t>(inf.slots) * static_cast<size_t>(n_users) * ctx->ext_k;
    for (size_t e = 0; e < n_theta; ++e)
      if (!std::isfinite(theta[e]) || theta[e] < 0.0)
        throw std::invalid_argument("inform: theta entry " + std::to_string(e) + " is not a finite number >= 0");
    require_subset(cand_items, n_cand, ctx->ext_items, "inform_query_theta");
    check_csr(seen_offsets, seen_items, n_users, ctx->ext_items, "inform", "seen_offsets", "user", "seen items",
              "seen item");
    inform_query_theta(ctx, n_users, theta, seen_offsets, seen_items, cand_items, n_cand, n, items, gains, counts);
  });
}

int mmsbm_hip_inform_mean_theta(mmsbm_hip_ctx *ctx, double *out) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::inf, "inform", "inform_mean_theta");
    if (!out) throw std::invalid_argument("null out");
    inform_mean_theta(ctx, out);
  });
}

int mmsbm_hip_inform_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::inf); }

int mmsbm_hip_overlap_begin(mmsbm_hip_ctx *ctx, int side) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (side != 0 && side != 1) throw std::invalid_argument("overlap: side must be 0 (items) or 1 (users)");
    overlap_begin(ctx, side);
  });
}

int mmsbm_hip_overlap_add(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    require_open(ctx, &mmsbm_hip_ctx::ov, "overlap");
    OneSlot one(ctx);
    overlap_add(ctx);
  });
}

int mmsbm_hip_overlap_query(mmsbm_hip_ctx *ctx, double *out) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::ov, "overlap", "overlap_query");
    if (!out) throw std::invalid_argument("null out");
    overlap_query(ctx, out);
  });
}

int mmsbm_hip_overlap_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::ov); }

int mmsbm_hip_explain_begin(mmsbm_hip_ctx *ctx, const double *rating_weights) {
  return guarded([&] {
    if (!ctx || !rating_weights) throw std::invalid_argument("null argument");
    for (int r = 0; r < ctx->n_ratings; ++r)
      if (!std::isfinite(rating_weights[r]))
        throw std::invalid_argument("explain: rating weight " + std::to_string(r) + " is not finite");
    if (ctx->ext_k > MMSBM_HIP_FOLD_IN_MAX_K)
      throw ApiError(MMSBM_E_UNSUPPORTED, "explain: K = " + std::to_string(ctx->ext_k) + " is beyond the " +
                                              std::to_string(MMSBM_HIP_FOLD_IN_MAX_K) + " groups it is built for");
    explain_begin(ctx, rating_weights);
  });
}

int mmsbm_hip_explain_add(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    require_open(ctx, &mmsbm_hip_ctx::ex, "explain");
    OneSlot one(ctx);
    explain_add(ctx);
  });
}

int mmsbm_hip_explain_query(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, const int64_t *offsets,
                            const int32_t *items, int32_t n, int32_t *hist_items, int32_t *hist_ratings,
                            double *contribution, int32_t *counts, double *explained, double *score, int32_t *degree) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::ex, "explain", "explain_query");
    if (n_users < 0) throw std::invalid_argument("negative n_users");
    require_n(n, "explain", "rows");
    if (n_users > 0 && (!users || !offsets)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "explain: user");
    check_csr(offsets, items, n_users, ctx->ext_items, "explain", "offsets", "user", "pairs", "item id");
    if (n_users > 0 && offsets[n_users] > 0 && !hist_items) throw std::invalid_argument("null argument");
    if (n_users > 0 && offsets[n_users] * static_cast<int64_t>(n) > INT32_MAX)
      throw std::invalid_argument("explain: more than 2^31 - 1 entries in one query");
    explain_query(ctx, n_users, users, offsets, items, n, hist_items, hist_ratings, contribution, counts, explained,
                  score, degree);
  });
}

int mmsbm_hip_explain_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::ex); }

int mmsbm_hip_heldout_begin(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user, const int32_t *item,
                            const int32_t *rating) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (n_rows < 0) throw std::invalid_argument("heldout: negative n_rows");
    if (n_rows > INT32_MAX) throw ApiError(MMSBM_E_UNSUPPORTED, "heldout: n_rows must be below 2^31");
    if (n_rows > 0 && (!user || !item || !rating)) throw std::invalid_argument("null argument");
    for (int64_t m = 0; m < n_rows; ++m)
      if (user[m] < 0 || user[m] >= ctx->ext_users || item[m] < 0 || item[m] >= ctx->ext_items || rating[m] < 0 ||
          rating[m] >= ctx->n_ratings)
        throw std::invalid_argument("heldout: id out of range at row " + std::to_string(m));
    heldout_begin(ctx, n_rows, user, item, rating);
  });
}

int mmsbm_hip_heldout_eval(mmsbm_hip_ctx *ctx, double *loglik) {
  return guarded([&] {
    require_all_params(ctx);
    if (!loglik) throw std::invalid_argument("null loglik");
    require_open(ctx, &mmsbm_hip_ctx::ho, "heldout");
    heldout_eval(ctx, 0, ctx->n_slots, false, loglik);
  });
}

int mmsbm_hip_heldout_add(mmsbm_hip_ctx *ctx, double *loglik) {
  return guarded([&] {
    require_params(ctx);
    if (!loglik) throw std::invalid_argument("null loglik");
    require_open(ctx, &mmsbm_hip_ctx::ho, "heldout");
    heldout_eval(ctx, ctx->sel, 1, true, loglik);
  });
}

int mmsbm_hip_heldout_mean(mmsbm_hip_ctx *ctx, double *mean_p, double *loglik) {
  return guarded([&] {
    if (!ctx || !loglik) throw std::invalid_argument("null argument");
    require_open(ctx, &mmsbm_hip_ctx::ho, "heldout", "heldout_mean");
    heldout_mean(ctx, mean_p, loglik);
  });
}

int mmsbm_hip_heldout_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::ho, "heldout"); }

namespace {
// the snapshot tables as theta_tab / eta_tab see the parameters of slot `slot`
RowTab snap_theta_tab(const mmsbm_hip_ctx *c, int slot) {
  return gather_tab(c, c->snap_theta.ptr, static_cast<size_t>(c->n_users), slot);
}
}  // namespace

int mmsbm_hip_snapshot_save(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    use_device(ctx);
    mmsbm_hip_ctx *c = ctx;
    const int cur = c->cur, sl = c->sel;
    const size_t klr = static_cast<size_t>(c->n_ratings) * c->kp * c->lp;
    if (c->snap_have.empty()) {
      const size_t doubles = c->theta[cur].count + c->eta[cur].count + c->p[cur].count;
      require_free_mem(doubles * sizeof(double), "snapshot: a copy of every slot's parameters");
      try {
        c->snap_theta.alloc(c->theta[cur].count);
        c->snap_eta.alloc_slots(static_cast<size_t>(c->n_items) * c->lp, c->n_slots);
        c->snap_p.alloc_slots(klr, c->n_slots);
      } catch (...) {
        c->drop_snapshots();
        throw;
      }
      c->snap_have.assign(static_cast<size_t>(c->n_slots), 0);
    }
    hipStream_t s = c->stream;
    const size_t e = sizeof(double);
    const RowTab src = gather_tab(c, c->theta[cur].ptr, static_cast<size_t>(c->n_users), sl), dst = snap_theta_tab(c, sl);
    if (c->n_users > 0) {  // the slot's columns of the interleaved rows: main parts, then tail parts
      HIP_CHECK(hipMemcpy2DAsync(dst.main, e * dst.rs_m, src.main, e * src.rs_m, e * src.mw, c->n_users,
                                 hipMemcpyDeviceToDevice, s));
      if (src.tw > 0)
        HIP_CHECK(hipMemcpy2DAsync(dst.tail, e * dst.rs_t, src.tail, e * src.rs_t, e * src.tw, c->n_users,
                                   hipMemcpyDeviceToDevice, s));
    }
    HIP_CHECK(hipMemcpyAsync(c->snap_eta.at(sl), c->eta[cur].at(sl), e * static_cast<size_t>(c->n_items) * c->lp,
                             hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->snap_p.at(sl), c->p[cur].at(sl), e * klr, hipMemcpyDeviceToDevice, s));
    c->snap_have[sl] = 1;
  });
}

int mmsbm_hip_snapshot_get(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (ctx->snap_have.empty() || !ctx->snap_have[ctx->sel])
      throw std::invalid_argument("snapshot_get: nothing saved for the selected slot");
    use_device(ctx);
    double *it = ctx->swapped ? eta : theta;
    double *ie = ctx->swapped ? theta : eta;
    const int sl = ctx->sel;
    fetch_params(ctx, snap_theta_tab(ctx, sl), plain_tab(ctx->snap_eta.at(sl), ctx->lp), ctx->snap_p.at(sl), it, ie, pr);
  });
}

int mmsbm_hip_fold_in(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user, const int32_t *item,
                      const int32_t *rating, int32_t n_new, int32_t n_iters, double tol,
                      const double *theta0, double *theta, int32_t *iters) {
  return fold_entry(ctx, false, n_rows, user, item, rating, n_new, n_iters, tol, theta0, theta, iters);
}

int mmsbm_hip_fold_in_items(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user, const int32_t *item,
                            const int32_t *rating, int32_t n_new, int32_t n_iters, double tol,
                            const double *eta0, double *eta, int32_t *iters) {
  return fold_entry(ctx, true, n_rows, user, item, rating, n_new, n_iters, tol, eta0, eta, iters);
}

int mmsbm_hip_time_iterations(mmsbm_hip_ctx *ctx, int n_iters, float *elapsed_ms) {
  return guarded([&] {
    require_all_params(ctx);
    if (!elapsed_ms || n_iters < 0) throw std::invalid_argument("bad argument");
    use_device(ctx);
    EventPair ev;
    ev.start(ctx->stream);
    run_iterations(ctx, n_iters);
    ev.stop(ctx->stream);
    ev.wait();
    *elapsed_ms = ev.ms();
  });
}

int mmsbm_hip_kernel_count(void) { return K_COUNT; }

const char *mmsbm_hip_kernel_name(int index) {
  return (index >= 0 && index < K_COUNT) ? kKernelNames[index] : "";
}

int mmsbm_hip_profile_iterations(mmsbm_hip_ctx *ctx, int n_iters, float *mean_us,
                                 int *launches_per_iter) {
  return guarded([&] {
    require_all_params(ctx);
    if (!mean_us || n_iters <= 0) throw std::invalid_argument("bad argument");
    use_device(ctx);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->profiling = true;
    try {
      for (int it = 0; it < n_iters; ++it) launch_iteration(ctx, true);
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
    } catch (...) {
      ctx->profiling = false;
      throw;
    }
    ctx->profiling = false;
    collect_profile(ctx, mean_us, launches_per_iter, n_iters);
  });
}

int mmsbm_hip_kernel_bytes(const mmsbm_hip_ctx *ctx, int index, int64_t *bytes_read,
                           int64_t *bytes_written) {
  return guarded([&] {
    if (!ctx || !bytes_read || !bytes_written) throw std::invalid_argument("null argument");
    const int64_t N = ctx->n_obs, U = ctx->n_users, I = ctx->n_items, R = ctx->n_ratings;
    const int64_t K = ctx->k, L = ctx->l, Q = ctx->n_pairs;
    const int64_t C = static_cast<int64_t>(ctx->lay.mv_chunks.size());
    int64_t rd = 0, wr = 0;
    const bool merged = use_pass_dense(ctx);  // K_SEG is the merged launch of pass_dense.hpp, K_DENSE has no launch
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
        if (merged) break;
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
  });
}

int mmsbm_hip_time_stage(mmsbm_hip_ctx *ctx, int stage, int reps, float *mean_us) {
  return guarded([&] {
    require_all_params(ctx);
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
    if ((stage == K_FUSED_PAIRS || stage == K_FUSED_TAIL) && !fused_possible(ctx))
      throw std::invalid_argument("time_stage: the two-launch kernels do not apply to this shape / data");
    use_device(ctx);
    ensure_a(ctx);
    // (with the triple passes and the T + S stage in one launch, stage K_SEG is that launch and K_DENSE has none: 0 us)
    const bool merged = use_pass_dense(ctx);
    if (merged && stage == K_DENSE) {
      *mean_us = 0.f;
      return;
    }
    auto one = [&] {
      switch (stage) {
        case K_SEG:
          if (merged) stage_pass_dense(ctx);
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
  });
}

int mmsbm_hip_set_option(mmsbm_hip_ctx *ctx, const char *name, double value) {
  return guarded([&] {
    if (!ctx || !name) throw std::invalid_argument("null argument");
    set_option(ctx, name, value);
  });
}

int mmsbm_hip_get_option(const mmsbm_hip_ctx *ctx, const char *name, double *value) {
  return guarded([&] {
    if (!ctx || !name || !value) throw std::invalid_argument("null argument");
    const Option *o = find_option(name);
    if (!o) throw std::invalid_argument(std::string("unknown option: ") + name);
    *value = o->get(ctx);
  });
}

int mmsbm_hip_set_graph_mode(mmsbm_hip_ctx *ctx, int enabled) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    set_option(ctx, "graph", enabled != 0);
  });
}

#ifdef MMSBM_STAMPS
// diagnostic build: copy the phase stamps of the last pair-stage launch (blocks x 16 words)
int mmsbm_hip_debug_stamps(unsigned long long *out, int n_words) {
  return guarded([&] {
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * n_words));
  });
}
#endif

// ---- host-only layout helpers (no device needed; used by the CPU tests) --------------------
struct mmsbm_hip_layout {
  mmsbm::Layout lay;
};

int mmsbm_hip_layout_build(int64_t n_obs, int32_t n_users, int32_t n_items, int32_t n_ratings,
                           const int32_t *user, const int32_t *item, const int32_t *rating,
                           int32_t target_chunks, mmsbm_hip_layout **out) {
  return guarded([&] {
    if (!out) throw std::invalid_argument("null out");
    *out = nullptr;
    std::unique_ptr<mmsbm_hip_layout> h(new mmsbm_hip_layout());
    mmsbm::build_layout(n_obs, n_users, n_items, n_ratings, user, item, rating, target_chunks,
                        h->lay);
    *out = h.release();
  });
}

int mmsbm_hip_layout_free(mmsbm_hip_layout *h) {
  delete h;
  return MMSBM_OK;
}

// which: 0 pair_off 1 pair_user 2 pair_item 3 rating_off 4 user_off 5 user_pair 6 item_off
//        7 item_pairs 8 item_deg 9 chunk_off; 4-int records: 10 chunks 11 mv_chunks
//        12 pair work items 13 user work items 14 pair splits 15 user splits
int mmsbm_hip_layout_array(const mmsbm_hip_layout *h, int which, int32_t *out, int64_t capacity,
                           int64_t *count) {
  return guarded([&] {
    if (!h || !count) throw std::invalid_argument("null argument");
    const mmsbm::Layout &L = h->lay;
    const std::vector<int32_t> *v = nullptr;
    switch (which) {
      case 0: v = &L.pair_off; break;
      case 1: v = &L.pair_user; break;
      case 2: v = &L.pair_item; break;
      case 3: v = &L.rating_off; break;
      case 4: v = &L.user_off; break;
      case 5: v = &L.user_pair; break;
      case 6: v = &L.item_off; break;
      case 7: v = &L.item_pairs; break;
      case 8: v = &L.item_deg; break;
      case 9: v = &L.chunk_off; break;
      case 10: case 11: case 12: case 13: case 14: case 15: break;
      default: throw std::invalid_argument("unknown layout array");
    }
    if (which >= 10) {  // arrays of 4-int records
      const void *src = nullptr;
      size_t n = 0;
      switch (which) {
        case 10: src = L.chunks.data(); n = L.chunks.size(); break;
        case 11: src = L.mv_chunks.data(); n = L.mv_chunks.size(); break;
        case 12: src = L.pair_work.items.data(); n = L.pair_work.items.size(); break;
        case 13: src = L.user_work.items.data(); n = L.user_work.items.size(); break;
        case 14: src = L.pair_work.splits.data(); n = L.pair_work.splits.size(); break;
        default: src = L.user_work.splits.data(); n = L.user_work.splits.size(); break;
      }
      *count = static_cast<int64_t>(n) * 4;
      if (out && n) {
        if (capacity < *count) throw ApiError(MMSBM_E_TOOLARGE, "buffer too small");
        std::memcpy(out, src, sizeof(int32_t) * *count);
      }
      return;
    }
    *count = static_cast<int64_t>(v->size());
    if (out) {
      if (capacity < *count) throw ApiError(MMSBM_E_TOOLARGE, "buffer too small");
      std::memcpy(out, v->data(), sizeof(int32_t) * v->size());
    }
  });
}

// side 0: pair segments (the 64-pair units rebuilt with at most cap_items work items each), 1: user segments
// (workgroups of at most cap_items items).  which: 0 units, 1 items, 2 splits (4-int records), 3 the unit list as
// chunks (side 0 only), 4 { max partial rows of a workgroup, built (0 / 1) } (2 ints)
int mmsbm_hip_layout_fused(const mmsbm_hip_layout *h, int side, int32_t cap_items, int which, int32_t *out,
                           int64_t capacity, int64_t *count) {
  return guarded([&] {
    if (!h || !count) throw std::invalid_argument("null argument");
    if ((side != 0 && side != 1) || cap_items < 1 || which < 0 || which > 4) throw std::invalid_argument("bad argument");
    mmsbm::Layout lay = h->lay;  // (the capped unit list replaces mv_chunks: work on a copy)
    mmsbm::FusedLists fl;
    bool built = true;
    if (side == 0) {
      const mmsbm::SegPieces sp = mmsbm::segment_pieces(lay.pair_off, lay.pair_work);
      built = mmsbm::build_mv_chunks_capped(lay, sp, mmsbm::kMvChunkPairs, cap_items);
      if (built) fl = mmsbm::build_fused_pairs(lay, sp);
    } else {
      fl = mmsbm::build_fused_users(mmsbm::segment_pieces(lay.user_off, lay.user_work), cap_items);
    }
    const int32_t info[2] = {fl.max_parts, built ? 1 : 0};
    const void *src = nullptr;
    size_t n = 0;
    switch (which) {
      case 0: src = fl.units.data(); n = fl.units.size() * 4; break;
      case 1: src = fl.items.data(); n = fl.items.size() * 4; break;
      case 2: src = fl.splits.data(); n = fl.splits.size() * 4; break;
      case 3: src = lay.mv_chunks.data(); n = side == 0 ? lay.mv_chunks.size() * 4 : 0; break;
      default: src = info; n = 2; break;
    }
    *count = static_cast<int64_t>(n);
    if (out && n) {
      if (capacity < *count) throw ApiError(MMSBM_E_TOOLARGE, "buffer too small");
      std::memcpy(out, src, sizeof(int32_t) * n);
    }
  });
}

int mmsbm_hip_selftest_throw(int kind) {
  return guarded([&] {
    struct NotStd { int x; };
    switch (kind) {
      case 0: return;
      case 1: throw std::invalid_argument("selftest: invalid argument");
      case 2: throw std::runtime_error("selftest: runtime error");
      case 3: throw std::bad_alloc();
      case 4: throw 42;
      default: throw NotStd{kind};
    }
  });
}

}  // extern "C"
