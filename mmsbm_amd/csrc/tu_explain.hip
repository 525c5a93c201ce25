// tu_explain.hip -- translation unit of the explanation of a recommendation (explain.hpp): the session's host side --
// the training rows of every external user, the per-slot copies, the batches of a query.  It launches rec_w_kernel and
// rec_fold_kernel of recommend.hpp for the slots' tables and shares that header's candidate list and fold_in.hpp's v.
#include "prelude.hpp"
#include "recommend.hpp"
#include "fold_in.hpp"
#include "explain.hpp"

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
  LAUNCH(rec_w_kernel, static_cast<unsigned>((kl + kBlock - 1) / kBlock), kBlock, 0, st, e.p, ex.w.ptr, wk.ptr, K, L, R,
         e.rs, e.ks, e.ls);
  auto fold = [&](const RowTab &src, int d, const double *m, int mt, int mj, double *out, int rows, int rank) {
    const size_t n = static_cast<size_t>(rows) * rank;
    if (n == 0) return;
    LAUNCH(rec_fold_kernel, static_cast<unsigned>((n + kBlock - 1) / kBlock), kBlock, 0, st, src, d, m, mt, mj, out,
           rows, rank);
  };
  fold(e.users, K, nullptr, 0, 0, to, U, K);   // theta as it is
  fold(e.items, L, wk.ptr, 1, L, go, I, K);    // G[i, k] = sum_l eta[i, l] W[k, l]: recommend_add's y where K <= L
  fold(e.items, L, nullptr, 0, 0, eo, I, L);   // eta as it is
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

}  // namespace mmsbm_hip_impl
