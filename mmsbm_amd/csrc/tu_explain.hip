// tu_explain.hip -- translation unit of the explanation of a recommendation (explain.hpp): the session's host side --
// the training rows of every external user, the per-slot copies, the batches of a query.  The slots' tables are folded by
// the serving frame (serve_frame.hpp: fold_weights, fold_rows); recommend.hpp's candidate list and fold_in.hpp's v are
// shared as device code.
// Also the host side of the leave-one-out reliability of the training rows (loo.hpp), which rests on the same identity
// and shares the same two headers.
#include "prelude.hpp"
#include "serve_frame.hpp"
#include "recommend.hpp"
#include "fold_in.hpp"
#include "explain.hpp"
#include "loo.hpp"

namespace mmsbm_hip_impl {

namespace {

constexpr size_t kExpBatchBytes = size_t(256) << 20;  // the c rows of one batch (S x K doubles per training row)

}  // namespace

void explain_begin(mmsbm_hip_ctx *c, const double *weights) {
  use_device(c);
  c->ex.reset();  // (from here on the previous session is gone)
  auto ex = std::make_unique<ExpSession>();
  hipStream_t s = c->stream;
  ex->w.alloc(c->n_ratings);
  HIP_CHECK(hipMemcpyAsync(ex->w.ptr, weights, sizeof(double) * c->n_ratings, hipMemcpyHostToDevice, s));
  // every external user's training rows in the order they were given: from the id columns in their original order
  std::vector<int32_t> eu, ei, rt;
  train_id_columns(c, eu, ei, &rt);
  const size_t n = eu.size();
  std::vector<int32_t> item(n), rating(n);
  ex->off_h = group_by_key<int64_t>(eu.data(), static_cast<int64_t>(n), c->ext_users, [&](int64_t m, int64_t at) {
    item[at] = ei[m];
    rating[at] = rt[m];
  });
  require_free_mem((ex->off_h.size() * 2 + n * 2) * sizeof(int32_t), "explain: the users' training rows");
  ex->off.upload(ex->off_h, s);
  ex->item.upload(item, s);
  ex->rating.upload(rating, s);
  HIP_CHECK(hipStreamSynchronize(s));  // (host vectors are locals)
  c->ex = std::move(ex);
}

void explain_add(mmsbm_hip_ctx *c) {  // the selected slot (the caller holds a OneSlot)
  use_device(c);
  ExpSession &ex = *c->ex;
  const int U = c->ext_users, I = c->ext_items, K = c->ext_k, L = c->ext_l, R = c->n_ratings, S = ex.slots;
  const size_t ts = static_cast<size_t>(U) * K, gs = static_cast<size_t>(I) * K, kl = static_cast<size_t>(K) * L;
  const size_t ps = static_cast<size_t>(R) * kl, es = static_cast<size_t>(I) * L;
  require_free_mem(((S + 1) * (ts + gs + ps + es) + kl) * sizeof(double), "explain: the slots' tables");
  hipStream_t st = c->stream;
  DevBuf<double> nt, ng, np, ne, wk;  // the four tables grow by one slot; W is needed for G only
  double *to = grow_by_slot(ex.th, ts, S, st, nt), *go = grow_by_slot(ex.g, gs, S, st, ng);
  double *po = grow_by_slot(ex.p, ps, S, st, np), *eo = grow_by_slot(ex.eta, es, S, st, ne);
  wk.alloc(kl);
  const ExtSlot e = ext_slot(c);
  fold_weights(st, e.p, ex.w.ptr, wk.ptr, K, L, R, e.rs, e.ks, e.ls);
  fold_rows(c, false, nullptr, 0, 0, to, K);   // theta as it is
  fold_rows(c, true, wk.ptr, 1, L, go, K);     // G[i, k] = sum_l eta[i, l] W[k, l]: recommend_add's y where K <= L
  fold_rows(c, true, nullptr, 0, 0, eo, L);    // eta as it is
  if (ps > 0)
    LAUNCH(exp_p_kernel, static_cast<unsigned>((ps + kBlock - 1) / kBlock), kBlock, 0, st, e.p, e.rs, e.ks, e.ls, K, L,
           R, po);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  ex.th.swap(nt);
  ex.g.swap(ng);
  ex.p.swap(np);
  ex.eta.swap(ne);
  ex.slots = S + 1;
}

// Occurrence b of the request is user users[b] with the candidate items items[offsets[b] .. offsets[b + 1]).  A batch
// is a run of consecutive occurrences whose training rows stay within the budget ("explain_rows", or what keeps the c
// rows within kExpBatchBytes); an occurrence beyond the budget is a batch of its own.  An occurrence without pairs takes
// no part.  How the occurrences fall into batches changes no output: a row's c depends on the row and its user alone.
void explain_query(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int64_t *offsets, const int32_t *items,
                   int n, int32_t *hist_items, int32_t *hist_ratings, double *contribution, int32_t *counts,
                   double *explained, double *score, int32_t *degree) {
  use_device(c);
  const ExpSession &ex = *c->ex;
  c->last_ms[T_EXPLAIN] = 0.f;
  const int U = c->ext_users, I = c->ext_items, K = c->ext_k, L = c->ext_l, R = c->n_ratings, S = ex.slots;
  const int64_t total = n_users > 0 ? offsets[n_users] : 0;  // (checked: below 2^31)
  if (total == 0) return;
  // the occurrences that hold pairs, their first rows counted over the whole request, and each pair's occurrence
  std::vector<int32_t> au;
  std::vector<int64_t> goff{0}, pfirst;
  std::vector<int32_t> pocc(static_cast<size_t>(total));
  for (int64_t b = 0; b < n_users; ++b) {
    if (offsets[b + 1] == offsets[b]) continue;
    const int32_t u = users[b];
    std::fill(pocc.begin() + offsets[b], pocc.begin() + offsets[b + 1], static_cast<int32_t>(au.size()));
    au.push_back(u);
    pfirst.push_back(offsets[b]);
    goff.push_back(goff.back() + (ex.off_h[u + 1] - ex.off_h[u]));
  }
  pfirst.push_back(total);
  const int64_t na = static_cast<int64_t>(au.size());
  const size_t fk = static_cast<size_t>(S) * K;
  int64_t budget = c->exp_rows > 0 ? c->exp_rows : static_cast<int64_t>(kExpBatchBytes / (fk * sizeof(double)));
  budget = std::max<int64_t>(budget, 1);
  std::vector<int64_t> cut{0};
  int64_t max_rows = 1;
  for (int64_t a = 0; a < na; ++a) {
    const int64_t b = cut.back();
    if (a > b && goff[a + 1] - goff[b] > budget) cut.push_back(a);
    max_rows = std::max(max_rows, goff[a + 1] - goff[cut.back()]);
  }
  cut.push_back(na);
  const size_t ld = static_cast<size_t>(max_rows), outs = static_cast<size_t>(total) * n;
  require_free_mem(fk * ld * sizeof(double) + outs * 16 + static_cast<size_t>(total) * 32 + static_cast<size_t>(na) * 12 + 8,
                   "explain: a batch of users");
  hipStream_t st = c->stream;
  DevBuf<int32_t> du, docc, dit, ohi, ohr, ocn, odg;
  DevBuf<int64_t> doff;
  DevBuf<double> dc, oco, oex, osc;
  du.upload(au, st);
  doff.upload(goff, st);
  docc.alloc(static_cast<size_t>(total));
  dit.alloc(static_cast<size_t>(total));
  dc.alloc(fk * ld);
  ohi.alloc(outs); ohr.alloc(outs); oco.alloc(outs);
  ocn.alloc(static_cast<size_t>(total)); odg.alloc(static_cast<size_t>(total));
  oex.alloc(static_cast<size_t>(total)); osc.alloc(static_cast<size_t>(total));
  // a pair's occurrence counted inside its batch
  for (size_t bi = 0; bi + 1 < cut.size(); ++bi)
    for (int64_t q = pfirst[cut[bi]]; q < pfirst[cut[bi + 1]]; ++q) pocc[q] -= static_cast<int32_t>(cut[bi]);
  HIP_CHECK(hipMemcpyAsync(docc.ptr, pocc.data(), sizeof(int32_t) * total, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(dit.ptr, items, sizeof(int32_t) * total, hipMemcpyHostToDevice, st));
  int cap = 1;
  while (cap < n + kExpWave * kExpPerLane) cap <<= 1;
  const size_t lds = static_cast<size_t>(cap) * (sizeof(double) + sizeof(ExpKey));
  EventPair ev;  // device time of the query's kernels (option "explain_ms")
  ev.start(st);
  for (size_t bi = 0; bi + 1 < cut.size(); ++bi) {  // (batches follow each other on the stream: no host wait in between)
    const int64_t a0 = cut[bi], a1 = cut[bi + 1], base = goff[a0], rows = goff[a1] - base;
    const int64_t q0 = pfirst[a0], nq = pfirst[a1] - q0;
    const int nb = static_cast<int>(a1 - a0);
    if (rows > 0)
      LAUNCH(exp_row_kernel, dim3(static_cast<unsigned>((rows + kBlock - 1) / kBlock), static_cast<unsigned>(S)), kBlock, 0,
             st, du.ptr + a0, doff.ptr + a0, base, nb, rows, ex.off.ptr, ex.item.ptr, ex.rating.ptr, ex.th.ptr, ex.p.ptr,
             ex.eta.ptr, U, I, K, L, R, dc.ptr, ld);
    LAUNCH(exp_pair_kernel, static_cast<unsigned>(nq), kExpWave, lds, st, du.ptr + a0, doff.ptr + a0, base, docc.ptr + q0,
           dit.ptr + q0, ex.off.ptr, ex.item.ptr, ex.rating.ptr, dc.ptr, ld, ex.th.ptr, ex.g.ptr, U, I, K, S, n, cap,
           ohi.ptr + q0 * n, ohr.ptr + q0 * n, oco.ptr + q0 * n, ocn.ptr + q0, oex.ptr + q0, osc.ptr + q0, odg.ptr + q0);
    HIP_CHECK(hipGetLastError());
  }
  ev.stop(st);
  auto fetch = [&](void *dst, const void *src, size_t bytes) {
    if (dst) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  };
  fetch(hist_items, ohi.ptr, sizeof(int32_t) * outs);
  fetch(hist_ratings, ohr.ptr, sizeof(int32_t) * outs);
  fetch(contribution, oco.ptr, sizeof(double) * outs);
  fetch(counts, ocn.ptr, sizeof(int32_t) * total);
  fetch(degree, odg.ptr, sizeof(int32_t) * total);
  fetch(explained, oex.ptr, sizeof(double) * total);
  fetch(score, osc.ptr, sizeof(double) * total);
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_EXPLAIN] = ev.ms();
}

// ---- leave-one-out reliability of the training rows (loo.hpp) ---------------------------------------------------------
namespace {

// One side's segments onto the device: the rows of every key (a user, or an item) in ascending position in the training
// table, and their chunks of kLooChunk rows
void loo_upload_side(LooSession::Side &sd, const std::vector<int32_t> &key, int segments, int groups, hipStream_t s) {
  const int64_t n = static_cast<int64_t>(key.size());
  std::vector<int32_t> rows(key.size());
  sd.off_h = group_by_key<int64_t>(key.data(), n, segments,
                                   [&](int64_t m, int64_t at) { rows[at] = static_cast<int32_t>(m); });
  std::vector<int64_t> chunk_off(static_cast<size_t>(segments) + 1, 0);
  for (int g = 0; g < segments; ++g)
    chunk_off[g + 1] = chunk_off[g] + (sd.off_h[g + 1] - sd.off_h[g] + kLooChunk - 1) / kLooChunk;
  sd.chunks = chunk_off.back();
  std::vector<int32_t> chunk_seg(static_cast<size_t>(sd.chunks));
  for (int g = 0; g < segments; ++g)
    std::fill(chunk_seg.begin() + chunk_off[g], chunk_seg.begin() + chunk_off[g + 1], g);
  sd.off.upload(sd.off_h, s);
  sd.chunk_off.upload(chunk_off, s);
  sd.rows.upload(rows, s);
  sd.chunk_seg.upload(chunk_seg, s);
  sd.num.alloc(static_cast<size_t>(segments) * groups);
  sd.part.alloc(static_cast<size_t>(sd.chunks) * std::max(groups, 2));
  sd.bar.alloc(static_cast<size_t>(groups));
  sd.surprise.alloc(static_cast<size_t>(segments) * 2);
  HIP_CHECK(hipStreamSynchronize(s));  // (host vectors are locals)
}

LooSide loo_side(const LooSession::Side &sd) {
  return LooSide{sd.off.ptr, sd.rows.ptr, sd.chunk_seg.ptr, sd.chunk_off.ptr, sd.chunks,
                 static_cast<int>(sd.off_h.size()) - 1};
}

unsigned loo_blocks(int64_t n, int per_block) { return static_cast<unsigned>((n + per_block - 1) / per_block); }

// The four columns and the sides' mean surprises of the slots added so far (once per set of added slots)
void loo_finish(mmsbm_hip_ctx *c, LooSession &lo, hipStream_t st) {
  if (lo.finished) return;
  const int64_t n = c->n_obs;
  if (n > 0)
    LAUNCH(loo_finish_kernel, loo_blocks(n, kBlock), kBlock, 0, st, lo.rel_sum.ptr, lo.fit_sum.ptr, n,
           static_cast<double>(lo.slots), lo.rel.ptr, lo.fitted.ptr, lo.sur.ptr, lo.fsur.ptr);
  for (LooSession::Side *sd : {&lo.by_user, &lo.by_item}) {
    const LooSide v = loo_side(*sd);
    if (v.chunks > 0)
      LAUNCH(loo_agg_kernel, loo_blocks(v.chunks, kBlock), kBlock, 0, st, v, lo.sur.ptr, lo.fsur.ptr, sd->part.ptr);
    if (v.segments > 0)
      LAUNCH(loo_comb_kernel, loo_blocks(static_cast<int64_t>(v.segments) * 2, kBlock), kBlock, 0, st, v, 2, 1,
             sd->part.ptr, sd->surprise.ptr);
  }
  HIP_CHECK(hipGetLastError());
  lo.finished = true;
}

}  // namespace

void loo_begin(mmsbm_hip_ctx *c) {
  use_device(c);
  c->loo.reset();  // (from here on the previous session is gone)
  auto lo = std::make_unique<LooSession>();
  hipStream_t s = c->stream;
  const int U = c->ext_users, I = c->ext_items, K = c->ext_k, L = c->ext_l;
  const size_t n = static_cast<size_t>(c->n_obs);
  const size_t chunks = 2 * (n / kLooChunk) + U + I;  // (at most)
  require_free_mem(n * (5 * sizeof(int32_t) + 7 * sizeof(double)) + chunks * (4 + 8 * std::max({K, L, 2})) +
                       (static_cast<size_t>(U) * (K + 4) + static_cast<size_t>(I) * (L + 4)) * sizeof(double),
                   "loo: the training rows, their sums and the sides' numerators");
  std::vector<int32_t> eu, ei, rt;
  train_id_columns(c, eu, ei, &rt);
  loo_upload_side(lo->by_user, eu, U, K, s);
  loo_upload_side(lo->by_item, ei, I, L, s);
  lo->user.upload(eu, s);
  lo->item.upload(ei, s);
  lo->rating.upload(rt, s);
  for (DevBuf<double> *b : {&lo->fit, &lo->rel_sum, &lo->fit_sum, &lo->rel, &lo->fitted, &lo->sur, &lo->fsur}) b->alloc(n);
  if (n > 0) {  // (the running sums start at +0.0)
    HIP_CHECK(hipMemsetAsync(lo->rel_sum.ptr, 0, sizeof(double) * n, s));
    HIP_CHECK(hipMemsetAsync(lo->fit_sum.ptr, 0, sizeof(double) * n, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));  // (host vectors are locals)
  c->loo = std::move(lo);
}

void loo_add(mmsbm_hip_ctx *c) {  // the selected slot (the caller holds a OneSlot)
  use_device(c);
  LooSession &lo = *c->loo;
  hipStream_t st = c->stream;
  const int U = c->ext_users, I = c->ext_items, K = c->ext_k, L = c->ext_l;
  const int64_t n = c->n_obs;
  const ExtSlot e = ext_slot(c);
  int W = loo_lanes(std::max(K, L));  // (wide rows: fewer rows per workgroup, so that their LDS stays below 96 KB)
  while (W < kBlock && sizeof(double) * (kBlock / W) * (3 * K + 2 * L) > (size_t(96) << 10)) W <<= 1;
  const int rows_per = kBlock / W, R = c->n_ratings;
  // p of every rating goes into LDS where it fits beside the groups' rows (the row pass needs most); the values and the
  // order of the operations are the same either way
  const size_t p_lds = sizeof(double) * loo_p_doubles(K, L, R);
  const size_t fit_rows = sizeof(double) * rows_per * (2 * K + L), row_rows = sizeof(double) * rows_per * (3 * K + 2 * L);
  const int plds = p_lds + row_rows <= kLooLdsP ? 1 : 0;
  const size_t fit_lds = fit_rows + (plds ? p_lds : 0), row_lds = row_rows + (plds ? p_lds : 0), sum_lds = plds ? p_lds : 0;
  const LooArgs a{e.users, e.items, e.p, e.rs, e.ks, e.ls, K, L, R, lo.user.ptr, lo.item.ptr, lo.rating.ptr, n};
  allow_big_lds(loo_fit_kernel<false>, fit_lds);  // (with p on chip everything stays within the plain budget)
  allow_big_lds(loo_row_kernel<false>, row_lds);
  EventPair all, sums, rows;  // device time of the add, of its sums pass and of its row pass (options "loo_*_ms")
  all.start(st);
  sums.start(st);
  LAUNCH(loo_mean_kernel, static_cast<unsigned>(K), kBlock, 0, st, e.users, U, lo.by_user.bar.ptr);
  LAUNCH(loo_mean_kernel, static_cast<unsigned>(L), kBlock, 0, st, e.items, I, lo.by_item.bar.ptr);
  const unsigned row_blocks = loo_blocks(n, rows_per * kLooRounds);
  if (n > 0 && plds) LAUNCH(loo_fit_kernel<true>, row_blocks, kBlock, fit_lds, st, a, W, lo.fit.ptr, lo.fit_sum.ptr);
  if (n > 0 && !plds) LAUNCH(loo_fit_kernel<false>, row_blocks, kBlock, fit_lds, st, a, W, lo.fit.ptr, lo.fit_sum.ptr);
  for (int side = 0; side < 2; ++side) {
    LooSession::Side &sd = side ? lo.by_item : lo.by_user;
    const LooSide v = loo_side(sd);
    const int G = side ? L : K, Ws = loo_lanes(G);
    const unsigned chunk_blocks = loo_blocks(v.chunks, kBlock / Ws);
    if (v.chunks > 0 && plds)
      LAUNCH(loo_sum_kernel<true>, chunk_blocks, kBlock, sum_lds, st, a, v, side, Ws, lo.fit.ptr, sd.part.ptr);
    if (v.chunks > 0 && !plds)
      LAUNCH(loo_sum_kernel<false>, chunk_blocks, kBlock, sum_lds, st, a, v, side, Ws, lo.fit.ptr, sd.part.ptr);
    if (v.segments > 0)
      LAUNCH(loo_comb_kernel, loo_blocks(static_cast<int64_t>(v.segments) * G, kBlock), kBlock, 0, st, v, G, 0,
             sd.part.ptr, sd.num.ptr);
  }
  sums.stop(st);
  rows.start(st);
  if (n > 0 && plds)
    LAUNCH(loo_row_kernel<true>, row_blocks, kBlock, row_lds, st, a, W, lo.fit.ptr, lo.by_user.num.ptr, lo.by_item.num.ptr,
           lo.by_user.bar.ptr, lo.by_item.bar.ptr, lo.by_user.off.ptr, lo.by_item.off.ptr, lo.rel_sum.ptr);
  if (n > 0 && !plds)
    LAUNCH(loo_row_kernel<false>, row_blocks, kBlock, row_lds, st, a, W, lo.fit.ptr, lo.by_user.num.ptr, lo.by_item.num.ptr,
           lo.by_user.bar.ptr, lo.by_item.bar.ptr, lo.by_user.off.ptr, lo.by_item.off.ptr, lo.rel_sum.ptr);
  rows.stop(st);
  all.stop(st);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  lo.slots += 1;
  lo.finished = false;
  c->last_ms[T_LOO] = all.ms();
  c->last_ms[T_LOO_SUMS] = sums.ms();
  c->last_ms[T_LOO_ROWS] = rows.ms();
}

void loo_rows(mmsbm_hip_ctx *c, int64_t n_rows, const int64_t *rows, double *fitted, double *reliability) {
  use_device(c);
  LooSession &lo = *c->loo;
  hipStream_t st = c->stream;
  const int64_t n = rows ? n_rows : c->n_obs;
  DevBuf<int64_t> dr;
  DevBuf<double> of, orl;
  if (rows && n > 0) {
    require_free_mem(static_cast<size_t>(n) * 24, "loo: the requested rows");
    dr.alloc(static_cast<size_t>(n));
    of.alloc(static_cast<size_t>(n));
    orl.alloc(static_cast<size_t>(n));
    HIP_CHECK(hipMemcpyAsync(dr.ptr, rows, sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
  }
  EventPair ev;
  ev.start(st);
  loo_finish(c, lo, st);
  if (rows && n > 0)
    LAUNCH(loo_gather_kernel, loo_blocks(n, kBlock), kBlock, 0, st, dr.ptr, n, lo.fitted.ptr, lo.rel.ptr, of.ptr, orl.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  if (n > 0) {
    if (fitted)
      HIP_CHECK(hipMemcpyAsync(fitted, rows ? of.ptr : lo.fitted.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (reliability)
      HIP_CHECK(hipMemcpyAsync(reliability, rows ? orl.ptr : lo.rel.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  }
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_LOO] = ev.ms();
}

void loo_sides(mmsbm_hip_ctx *c, double *user_surprise, double *user_fitted_surprise, double *item_surprise,
               double *item_fitted_surprise) {
  use_device(c);
  LooSession &lo = *c->loo;
  hipStream_t st = c->stream;
  EventPair ev;
  ev.start(st);
  loo_finish(c, lo, st);
  ev.stop(st);
  std::vector<double> us(static_cast<size_t>(c->ext_users) * 2), is(static_cast<size_t>(c->ext_items) * 2);
  HIP_CHECK(hipMemcpyAsync(us.data(), lo.by_user.surprise.ptr, sizeof(double) * us.size(), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(is.data(), lo.by_item.surprise.ptr, sizeof(double) * is.size(), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  for (size_t u = 0; u < us.size() / 2; ++u) {
    if (user_surprise) user_surprise[u] = us[2 * u];
    if (user_fitted_surprise) user_fitted_surprise[u] = us[2 * u + 1];
  }
  for (size_t i = 0; i < is.size() / 2; ++i) {
    if (item_surprise) item_surprise[i] = is[2 * i];
    if (item_fitted_surprise) item_fitted_surprise[i] = is[2 * i + 1];
  }
  c->last_ms[T_LOO] = ev.ms();
}

void loo_lowest(mmsbm_hip_ctx *c, int m, const uint8_t *user_flags, const uint8_t *item_flags, int64_t *rows,
                double *reliability, int32_t *count) {
  use_device(c);
  LooSession &lo = *c->loo;
  hipStream_t st = c->stream;
  const int64_t n = c->n_obs;
  // ranges of rows: one wave each, at most 256 of them (the split changes no answer)
  const int64_t per = std::max<int64_t>(4096, (n + 255) / 256);
  const int parts = static_cast<int>(std::max<int64_t>(1, (n + per - 1) / per));
  int cap = 1;
  while (cap < m + kLooWave * kLooPerLane) cap <<= 1;
  const size_t lds = static_cast<size_t>(cap) * (sizeof(double) + sizeof(int64_t));
  const size_t list = static_cast<size_t>(parts + 1) * m;
  require_free_mem(list * 16 + (parts + 1) * 4 + (user_flags ? c->ext_users : 0) + (item_flags ? c->ext_items : 0),
                   "loo: the ranges' lists and the flags");
  DevBuf<uint8_t> uf, itf;
  DevBuf<double> ls;
  DevBuf<int64_t> lk;
  DevBuf<int32_t> ln;
  ls.alloc(list);
  lk.alloc(list);
  ln.alloc(static_cast<size_t>(parts) + 1);
  if (user_flags) {
    uf.alloc(static_cast<size_t>(c->ext_users));
    HIP_CHECK(hipMemcpyAsync(uf.ptr, user_flags, static_cast<size_t>(c->ext_users), hipMemcpyHostToDevice, st));
  }
  if (item_flags) {
    itf.alloc(static_cast<size_t>(c->ext_items));
    HIP_CHECK(hipMemcpyAsync(itf.ptr, item_flags, static_cast<size_t>(c->ext_items), hipMemcpyHostToDevice, st));
  }
  const uint8_t *no_flags = nullptr;
  const double *no_s = nullptr;
  const int64_t *no_k = nullptr;
  const int32_t *no_n = nullptr;
  EventPair ev;
  ev.start(st);
  loo_finish(c, lo, st);
  LAUNCH(loo_low_kernel<false>, static_cast<unsigned>(parts), kLooWave, lds, st, lo.rel.ptr, lo.user.ptr, lo.item.ptr,
         user_flags ? uf.ptr : no_flags, item_flags ? itf.ptr : no_flags, n, per, no_s, no_k, no_n, 0, m, cap, ls.ptr,
         lk.ptr, ln.ptr);
  // the ranges' lists into the one behind them
  double *fs = ls.ptr + static_cast<size_t>(parts) * m;
  int64_t *fk = lk.ptr + static_cast<size_t>(parts) * m;
  LAUNCH(loo_low_kernel<true>, 1u, kLooWave, lds, st, lo.rel.ptr, lo.user.ptr, lo.item.ptr, no_flags, no_flags, n, per,
         static_cast<const double *>(ls.ptr), static_cast<const int64_t *>(lk.ptr),
         static_cast<const int32_t *>(ln.ptr), parts, m, cap, fs, fk, ln.ptr + parts);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  int32_t got = 0;
  HIP_CHECK(hipMemcpyAsync(&got, ln.ptr + parts, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(rows, fk, sizeof(int64_t) * m, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(reliability, fs, sizeof(double) * m, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < m; ++k) {  // the list held -reliability (the selection's order); behind the last one (-1, +inf)
    rows[k] = k < got ? rows[k] : -1;
    reliability[k] = k < got ? -reliability[k] : INFINITY;
  }
  if (count) *count = got;
  c->last_ms[T_LOO] = ev.ms();
}

}  // namespace mmsbm_hip_impl
