// tu_once.hip -- translation unit of the once-per-run kernels (once_kernels.hpp, lik_fact.hpp): the likelihood in its
// forms, prod_dist / predict / score, compute_omegas, the random start -- with the host code that chooses among them and
// the host side of their entries (uploads, the predict session, the B table of the fast path, results back)
#include "prelude.hpp"
#include "pcg64.hpp"
#include "once_kernels.hpp"
#include "lik_fact.hpp"

namespace {

// likelihood_fast_kernel: tile + its logarithms in LDS?  (always with several lanes per triple)
bool lik_fast_tile_lds(const mmsbm_hip_ctx *c) {
  return c->lp > 20 || c->lik_g > 1 ||
         2 * static_cast<size_t>(c->kp) * c->lp * sizeof(double) > kScalarTileBytes;
}
bool lik_fast_usable(const mmsbm_hip_ctx *c) {
  const size_t lds = lik_fast_tile_lds(c) ? 2 * static_cast<size_t>(c->kp) * c->lp * sizeof(double) : 0;
  return c->lik_mode >= 1 && c->lp <= 160 && c->n_lik_units > 0 && lds <= kLdsMax - 4096;
}
// likelihood of the selected slot through the logarithm tables; returns the number of partial sums
int likelihood_fast(mmsbm_hip_ctx *c) {
  ensure_a(c);  // (s_n = theta_n . A[q_n])
  const int cur = c->cur, sl = c->sel;
  const size_t nt = static_cast<size_t>(c->n_users) * c->kp, ne = static_cast<size_t>(c->n_items) * c->lp;
  const size_t np = static_cast<size_t>(c->n_ratings) * c->kp * c->lp;
  if (c->lg_theta.count < nt) c->lg_theta.alloc(nt);
  if (c->lg_eta.count < ne) c->lg_eta.alloc(ne);
  if (c->lg_p.count < np) c->lg_p.alloc(np);
  auto logs = [&](const double *in, double *out, size_t n) {
    if (n == 0) return;
    LAUNCH(log_table_kernel, static_cast<unsigned>((n + kBlock - 1) / kBlock), kBlock, 0, c->stream, in, out, n);
  };
  const RowTab th = theta_tab(c, cur);
  const RowTab lth{c->lg_theta.ptr, c->lg_theta.ptr + static_cast<size_t>(c->n_users) * th.mw, th.mw, th.tw,
                   th.mw, th.tw, 0, 0};  // main + tail like theta, one slot
  if (nt > 0)
    LAUNCH(log_rows_kernel, static_cast<unsigned>((nt + kBlock - 1) / kBlock), kBlock, 0, c->stream, th, lth,
           static_cast<size_t>(c->n_users), c->kp);
  logs(c->eta[cur].at(sl), c->lg_eta.ptr, ne);
  logs(c->p[cur].at(sl), c->lg_p.ptr, np);
  const int nb = c->n_lik_units;
  if (c->lik_part.count < static_cast<size_t>(nb)) c->lik_part.alloc(nb);
  // lanes per triple and columns per lane: at most ~20 columns (40 + 40 registers) per lane
  int G = c->lp <= 20 ? 1 : (c->lp <= 40 ? 2 : 4);
  if (c->lik_g > 0) G = c->lik_g;  // tuning override
  while (G < 8 && (c->lp + G - 1) / G > 20) G *= 2;
  const int LW = ((c->lp + G - 1) / G + 3) / 4 * 4;
  const bool tl = lik_fast_tile_lds(c);
  const size_t lds = tl ? 2 * static_cast<size_t>(c->kp) * c->lp * sizeof(double) : 0;
#define LIK_GO(LW_, G_, TL_)                                                                      \
  allow_big_lds(likelihood_fast_kernel<LW_, G_, TL_>, lds);                                       \
  LAUNCH((likelihood_fast_kernel<LW_, G_, TL_>), nb, kLikThreads, lds, c->stream,                 \
         c->lik_units.ptr, c->pair_off.ptr, c->pair_user.ptr, c->pair_item.ptr, th, lth, a_tab(c, cur), \
         c->eta[cur].at(sl), c->lg_eta.ptr, c->p[cur].at(sl), c->lg_p.ptr, c->lik_part.ptr, c->k, \
         c->l, c->kp, c->lp)
#define LIK_LW(G_, TL_)                                                                           \
  do {                                                                                            \
    switch (LW) {                                                                                 \
      case 4: LIK_GO(4, G_, TL_); break;                                                          \
      case 8: LIK_GO(8, G_, TL_); break;                                                          \
      case 12: LIK_GO(12, G_, TL_); break;                                                        \
      case 16: LIK_GO(16, G_, TL_); break;                                                        \
      default: LIK_GO(20, G_, TL_); break;                                                        \
    }                                                                                             \
  } while (0)
  if (G == 1) {
    if (tl) LIK_LW(1, true); else LIK_LW(1, false);
  } else if (G == 2) {
    LIK_LW(2, true);
  } else if (G == 4) {
    LIK_LW(4, true);
  } else {
    LIK_LW(8, true);
  }
#undef LIK_LW
#undef LIK_GO
  return nb;
}

// ---- the likelihood pair by pair (lik_fact.hpp): logarithm tables, then one wave per (item, rating) pair.
// For rows of more than 32 groups (one column per lane: narrower rows would leave most of a wave idle), tiles
// that fit the LDS beside their logarithms, and data with a few triples per pair (the pair's eta p products
// are shared by four triples at a time).  Returns the number of partial sums.
bool lik_pairs_usable(const mmsbm_hip_ctx *c) {
  return c->lik_mode == 2 && c->lp > 32 && c->lp <= 192 && c->kp <= 192 && c->n_lik_units > 0 && c->n_pairs > 0 &&
         (2 * static_cast<size_t>(c->kp) * c->lp + c->kp) * sizeof(double) <= kLdsMax - 4096 &&
         c->n_obs * 2 >= static_cast<int64_t>(c->n_pairs) * 5;
}
int likelihood_pairs(mmsbm_hip_ctx *c) {
  ensure_a(c);  // (s_t = theta_t . A[q])
  const int cur = c->cur, sl = c->sel;
  hipStream_t st = c->stream;
  const size_t nt = static_cast<size_t>(c->n_users) * c->kp, ne = static_cast<size_t>(c->n_items) * c->lp;
  const size_t np = static_cast<size_t>(c->n_ratings) * c->kp * c->lp;
  if (c->lg_theta.count < 2 * nt) c->lg_theta.alloc(2 * nt);  // here: (theta, log theta) pairs, plain rows
  if (c->lg_eta.count < ne) c->lg_eta.alloc(ne);
  if (c->lg_p.count < np) c->lg_p.alloc(np);
  auto blocks = [](size_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); };
  const RowTab th = theta_tab(c, cur);
  double2 *tl = reinterpret_cast<double2 *>(c->lg_theta.ptr);
  const double *eta = c->eta[cur].at(sl), *p = c->p[cur].at(sl);
  if (nt > 0) LAUNCH(theta_log_pairs_kernel, blocks(nt), kBlock, 0, st, th, tl, static_cast<size_t>(c->n_users), c->kp);
  if (ne > 0) LAUNCH(log_table_kernel, blocks(ne), kBlock, 0, st, eta, c->lg_eta.ptr, ne);
  LAUNCH(log_table_kernel, blocks(np), kBlock, 0, st, p, c->lg_p.ptr, np);
  const int nb = c->n_lik_units;
  if (c->lik_part.count < static_cast<size_t>(nb)) c->lik_part.alloc(static_cast<size_t>(nb));
  const size_t lds = (2 * static_cast<size_t>(c->kp) * c->lp + c->kp) * sizeof(double);
#define WAVE_GO(LW_)                                                                                 \
  do {                                                                                               \
    allow_big_lds(lik_wave_kernel<LW_>, lds);                                                        \
    LAUNCH(lik_wave_kernel<LW_>, nb, kLikWaveThreads, lds, st,                                       \
           c->lik_units.ptr, c->pair_off.ptr, c->pair_user.ptr, c->pair_item.ptr, tl, a_tab(c, cur), \
           eta, c->lg_eta.ptr, p, c->lg_p.ptr, c->lik_part.ptr, c->k, c->l, c->kp, c->lp);           \
  } while (0)
  if (c->lp <= 64) WAVE_GO(1); else if (c->lp <= 128) WAVE_GO(2); else WAVE_GO(3);
#undef WAVE_GO
  return nb;
}

// ---- rows of up to 32 groups: a lane per triple, the tile through scalar loads (lik_fact.hpp: lik_lane_kernel) ----
constexpr int kLikLaneThreads = 128;
bool lik_lanes_usable(const mmsbm_hip_ctx *c) {
  return c->lik_mode == 2 && c->kp <= 32 && c->lp <= 32 && c->n_lik_units > 0 && c->n_pairs > 0;
}
int likelihood_lanes(mmsbm_hip_ctx *c) {
  ensure_a(c);  // (s_n = theta_n . A[q_n])
  const int cur = c->cur, sl = c->sel;
  hipStream_t st = c->stream;
  const size_t nt = static_cast<size_t>(c->n_users) * c->kp, ne = static_cast<size_t>(c->n_items) * c->lp;
  const size_t np = static_cast<size_t>(c->n_ratings) * c->kp * c->lp;
  if (c->lg_theta.count < 2 * nt) c->lg_theta.alloc(2 * nt);  // (value, logarithm) pairs, plain rows
  if (c->lg_eta.count < 2 * ne) c->lg_eta.alloc(2 * ne);
  if (c->lg_p.count < 2 * np + 16) c->lg_p.alloc(2 * np + 16);   // (+ 16: lik_lane_kernel's scalar loads run one chunk ahead)
  auto blocks = [](size_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); };
  double2 *tl = reinterpret_cast<double2 *>(c->lg_theta.ptr), *el = reinterpret_cast<double2 *>(c->lg_eta.ptr);
  double2 *ptl = reinterpret_cast<double2 *>(c->lg_p.ptr);
  if (nt > 0) LAUNCH(theta_log_pairs_kernel, blocks(nt), kBlock, 0, st, theta_tab(c, cur), tl, static_cast<size_t>(c->n_users), c->kp);
  if (ne > 0) LAUNCH(theta_log_pairs_kernel, blocks(ne), kBlock, 0, st, eta_tab(c, cur), el, static_cast<size_t>(c->n_items), c->lp);
  LAUNCH(theta_log_pairs_kernel, blocks(np), kBlock, 0, st, plain_tab(c->pt[cur].at(sl), c->kp), ptl,
         static_cast<size_t>(c->n_ratings) * c->lp, c->kp);   // pT: [R][lp][kp]
  const int nb = c->n_lik_units;
  if (c->lik_part.count < static_cast<size_t>(nb)) c->lik_part.alloc(static_cast<size_t>(nb));
#define LANE_GO(KP_)                                                                                          \
  LAUNCH((lik_lane_kernel<KP_, kLikLaneThreads>), nb, kLikLaneThreads, 0, st,                                 \
         c->lik_units.ptr, c->pair_off.ptr, c->pair_user.ptr, c->pair_item.ptr, tl, a_tab(c, cur), el, ptl,  \
         c->lik_part.ptr, c->k, c->l, c->lp)
  switch (c->kp) {
    case 4: LANE_GO(4); break;
    case 8: LANE_GO(8); break;
    case 12: LANE_GO(12); break;
    case 16: LANE_GO(16); break;
    case 20: LANE_GO(20); break;
    case 24: LANE_GO(24); break;
    case 28: LANE_GO(28); break;
    default: LANE_GO(32); break;
  }
#undef LANE_GO
  return nb;
}

}  // namespace

namespace mmsbm_hip_impl {

// likelihood of the selected slot (the caller holds a OneSlot): kernels onto the context's stream, no wait;
// returns the number of partial sums likelihood_finish adds up
int likelihood_enqueue(mmsbm_hip_ctx *ctx) {
  const int cur = ctx->cur, sl = ctx->sel;
  int nb;
  if (lik_pairs_usable(ctx)) {
    nb = likelihood_pairs(ctx);
  } else if (lik_lanes_usable(ctx)) {
    nb = likelihood_lanes(ctx);
  } else if (lik_fast_usable(ctx)) {
    nb = likelihood_fast(ctx);
  } else {
    const size_t lik_lds = static_cast<size_t>(ctx->kp + ctx->lp) * kLikThreads * sizeof(double);
    if (lik_lds <= kLdsMax - 2048 && ctx->n_lik_units > 0) {
      nb = ctx->n_lik_units;
      allow_big_lds(likelihood_units_kernel, lik_lds);
      if (ctx->lik_part.count < static_cast<size_t>(nb)) ctx->lik_part.alloc(nb);
      LAUNCH(likelihood_units_kernel, nb, kLikThreads, lik_lds, ctx->stream,
             ctx->lik_units.ptr, ctx->pair_off.ptr, ctx->pair_user.ptr, ctx->pair_item.ptr,
             theta_tab(ctx, cur), ctx->eta[cur].at(sl), ctx->p[cur].at(sl), ctx->lik_part.ptr, ctx->k,
             ctx->l, ctx->kp, ctx->lp);
    } else {
      nb = static_cast<int>(std::min<int64_t>((ctx->n_obs + kBlock - 1) / kBlock, 4096));
      nb = std::max(nb, 1);
      LAUNCH(likelihood_kernel, nb, kBlock, 0, ctx->stream,
             ctx->orig_u.ptr, ctx->orig_i.ptr, ctx->orig_r.ptr, theta_tab(ctx, cur),
             ctx->eta[cur].at(sl), ctx->p[cur].at(sl), ctx->lik_part.ptr, ctx->n_obs, ctx->k, ctx->l,
             ctx->kp, ctx->lp);
    }
  }
  HIP_CHECK(hipGetLastError());
  return nb;
}

double likelihood_finish(mmsbm_hip_ctx *ctx, int nb) {  // workgroup sums added in workgroup order
  std::vector<double> part(nb);
  HIP_CHECK(hipMemcpyAsync(part.data(), ctx->lik_part.ptr, sizeof(double) * nb, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  double tot = 0.0;
  for (double v : part) tot += v;
  return tot;
}

// theta0 / eta0 of the selected slot drawn on the device from the restart's PCG64 stream (pcg64.hpp)
void init_rows_launch(mmsbm_hip_ctx *ctx, const uint64_t pcg64_state[4]) {
  const int cur = ctx->cur;
  // the reference draws theta (external users x K) first, then eta; internally the two sides
  // may be swapped, the stream offsets are not
  const uint64_t n_theta_ext = static_cast<uint64_t>(ctx->ext_users) * ctx->ext_k;
  const uint64_t off_users = ctx->swapped ? n_theta_ext : 0;  // internal users' table
  const uint64_t off_items = ctx->swapped ? 0 : n_theta_ext;
  const RowTab tt = theta_tab(ctx, cur), et = eta_tab(ctx, cur);
  auto blocks = [](uint64_t total) {
    return static_cast<unsigned>((total + uint64_t(kBlock) * kDrawsPerThread - 1) / (uint64_t(kBlock) * kDrawsPerThread));
  };
  const uint64_t nu = static_cast<uint64_t>(ctx->n_users) * ctx->k, ni = static_cast<uint64_t>(ctx->n_items) * ctx->l;
  if (nu > 0)
    LAUNCH(init_rows_kernel, blocks(nu), kBlock, 0, ctx->stream, tt, ctx->user_off.ptr, nullptr, ctx->n_users, ctx->k,
           pcg64_state[0], pcg64_state[1], pcg64_state[2], pcg64_state[3], off_users);
  if (ni > 0)
    LAUNCH(init_rows_kernel, blocks(ni), kBlock, 0, ctx->stream, et, nullptr, ctx->item_deg.ptr, ctx->n_items, ctx->l,
           pcg64_state[0], pcg64_state[1], pcg64_state[2], pcg64_state[3], off_items);
  HIP_CHECK(hipGetLastError());
}

namespace {

// B for the selected slot (the caller holds a OneSlot and rows_fast_prepare said yes), then one group of
// lanes per row.
// mode 0: dist[m][r] = P[m, r];  mode 1: dist += P, block_out = the restart's six sums per workgroup
int rows_launch(mmsbm_hip_ctx *c, int mode, const int32_t *pu, const int32_t *pi, const int32_t *preal,
                const double *weights, double *dist, double *block_out, int64_t n_rows, int first) {
  stage_matvec_a(c, c->cur, c->cur, true);
  const int per = kBlock / group_lanes(c->code_k);
  const int nb = static_cast<int>((n_rows + per - 1) / per);
  const size_t rstride = static_cast<size_t>(c->n_items) * c->kp;
#define CALL(G, V)                                                                                           \
  do {                                                                                                       \
    if (mode == 0)                                                                                           \
      LAUNCH((predict_rows_kernel<G, V, 0>), nb, kBlock, 0, c->stream, pu, pi, preal, theta_tab(c, c->cur), c->btab.ptr, \
             rstride, weights, dist, block_out, n_rows, c->n_ratings, c->kp, first);                         \
    else                                                                                                     \
      LAUNCH((predict_rows_kernel<G, V, 1>), nb, kBlock, 0, c->stream, pu, pi, preal, theta_tab(c, c->cur), c->btab.ptr, \
             rstride, weights, dist, block_out, n_rows, c->n_ratings, c->kp, first);                         \
  } while (0)
  DISPATCH_GV(c->code_k, CALL);
#undef CALL
  HIP_CHECK(hipGetLastError());
  return nb;
}

// the per-row scoring kernels (fewer rows than items, or predict_fast = 0) and the final pass over the mean; the six sums
// per workgroup go to the session's `part`.  Returns the number of workgroups.
int score_rows_launch(mmsbm_hip_ctx *ctx, bool finish) {
  const PredictSession &ps = *ctx->ps;
  const int nb = static_cast<int>((ps.rows + kBlock - 1) / kBlock);
  if (nb <= 0) return 0;
  const int cur = ctx->cur, sl = ctx->sel;
  if (finish)
    LAUNCH(predict_score_kernel<true>, nb, kBlock, 0, ctx->stream,
           ps.u.ptr, ps.i.ptr, ps.r.ptr, theta_tab(ctx, cur), ctx->eta[cur].at(sl),
           ctx->p[cur].at(sl), ps.w.ptr, ps.sum.ptr, ps.part.ptr, ps.rows,
           ctx->n_ratings, ctx->k, ctx->l, ctx->kp, ctx->lp, 0, static_cast<double>(ps.slots));
  else
    LAUNCH(predict_score_kernel<false>, nb, kBlock, 0, ctx->stream,
           ps.u.ptr, ps.i.ptr, ps.r.ptr, theta_tab(ctx, cur), ctx->eta[cur].at(sl),
           ctx->p[cur].at(sl), ps.w.ptr, ps.sum.ptr, ps.part.ptr, ps.rows,
           ctx->n_ratings, ctx->k, ctx->l, ctx->kp, ctx->lp, ps.slots == 0 ? 1 : 0, 1.0);
  HIP_CHECK(hipGetLastError());
  return nb;
}
// omega[n,k,l] of the selected slot into dev_out (n_elems = N K L), in the caller's (external) orientation
void omegas_launch(mmsbm_hip_ctx *ctx, double *dev_out, int64_t n_elems) {
  const int cur = ctx->cur, sl = ctx->sel;
  // internal (k,l) -> external position: not swapped [k][l] strides (L,1); swapped the
  // external tensor is [l_int][k_int] so strides are (1, K_int)
  const int sk = ctx->swapped ? 1 : ctx->l;
  const int sl_stride = ctx->swapped ? ctx->k : 1;
  const int64_t nb = (n_elems + kBlock - 1) / kBlock;
  LAUNCH(omegas_kernel, static_cast<unsigned>(nb), kBlock, 0, ctx->stream,
         ctx->orig_u.ptr, ctx->orig_i.ptr, ctx->orig_r.ptr, theta_tab(ctx, cur),
         ctx->eta[cur].at(sl), ctx->p[cur].at(sl), dev_out, n_elems, ctx->k, ctx->l, ctx->kp,
         ctx->lp, sk, sl_stride);
  HIP_CHECK(hipGetLastError());
}

// P[m, r] of the selected slot for n_pairs (user, item) rows, a thread per element (few rows, or predict_fast = 0)
void prod_dist_launch(mmsbm_hip_ctx *ctx, const int32_t *du, const int32_t *di, double *dout, int64_t n_pairs) {
  const int cur = ctx->cur, sl = ctx->sel;
  const int64_t n_elems = n_pairs * ctx->n_ratings;
  const int64_t nb = (n_elems + kBlock - 1) / kBlock;
  LAUNCH(prod_dist_kernel, static_cast<unsigned>(nb), kBlock, 0, ctx->stream,
         du, di, theta_tab(ctx, cur), ctx->eta[cur].at(sl), ctx->p[cur].at(sl), dout,
         n_pairs, ctx->n_ratings, ctx->k, ctx->l, ctx->kp, ctx->lp);
  HIP_CHECK(hipGetLastError());
}

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

// the open session's rows scored under the selected slot (finish: its mean), the six sums of the workgroups added up
void score_launch(mmsbm_hip_ctx *ctx, bool finish, double *stats) {
  const int n_stats = kScoreStats;
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

void compute_omegas(mmsbm_hip_ctx *ctx, double *out, int64_t n_elems) {
  DevBuf<double> dev;
  dev.alloc(static_cast<size_t>(n_elems));
  omegas_launch(ctx, dev.ptr, n_elems);
  HIP_CHECK(hipMemcpyAsync(out, dev.ptr, sizeof(double) * n_elems, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void prod_dist(mmsbm_hip_ctx *ctx, int64_t n_pairs, const int32_t *user, const int32_t *item, double *out) {
  const int64_t n_elems = n_pairs * ctx->n_ratings;
  if ((n_elems + kBlock - 1) / kBlock > (int64_t(1) << 31) - 1)
    throw ApiError(MMSBM_E_TOOLARGE, "prod_dist: too many pairs for one launch");
  DevBuf<int32_t> du, di;
  DevBuf<double> dout;
  du.alloc(n_pairs); di.alloc(n_pairs); dout.alloc(n_elems);
  const auto [iu, ii] = internal_sides(ctx, user, item);
  HIP_CHECK(hipMemcpyAsync(du.ptr, iu, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(di.ptr, ii, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, ctx->stream));
  if (rows_fast_prepare(ctx, n_pairs)) rows_launch(ctx, 0, du.ptr, di.ptr, nullptr, nullptr, dout.ptr, nullptr, n_pairs, 1);
  else prod_dist_launch(ctx, du.ptr, di.ptr, dout.ptr, n_pairs);
  HIP_CHECK(hipMemcpyAsync(out, dout.ptr, sizeof(double) * n_elems, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->btab.release();  // (the B table is scratch: restart slots are sized from the free memory)
}

void predict_begin(mmsbm_hip_ctx *ctx, int64_t n_rows, const int32_t *user, const int32_t *item, const int32_t *rating,
                   const double *rating_weights) {
  ctx->ps.reset();  // (arguments are fine: from here on the previous session is gone)
  auto ps = std::make_unique<PredictSession>();
  const auto [iu, ii] = internal_sides(ctx, user, item);
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
}

void predict_add(mmsbm_hip_ctx *ctx, double *stats) {
  score_launch(ctx, false, stats);
  ctx->ps->slots++;
}

void predict_finish(mmsbm_hip_ctx *ctx, double *mean_dist, double *stats) {
  // the session is over on every way out of here, and its buffers go back: restart slots are sized from the free memory
  struct Drop { mmsbm_hip_ctx *c; ~Drop() { c->ps.reset(); } } drop{ctx};
  const PredictSession &ps = *ctx->ps;
  score_launch(ctx, true, stats);
  ctx->btab.release();
  if (mean_dist && ps.rows > 0) {
    HIP_CHECK(hipMemcpyAsync(mean_dist, ps.sum.ptr, sizeof(double) * ps.rows * ctx->n_ratings, hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
}

}  // namespace mmsbm_hip_impl
