// tu_serve_frame.hip -- translation unit of the serving frame's out-of-line half (serve_frame.hpp): the one unit that
// launches the kernels several query families share, so that each of them has one launch site and one copy in the library
//   recommend.hpp  rec_w_kernel and rec_fold_kernel (the sessions' per-slot folds), rec_score_kernel and
//                  rec_exclude_kernel (the score tiles and the seen exclusion), rec_select_kernel (the selection stage)
//   catalogue.hpp  cat_gather_kernel and cat_cols_kernel (the candidates' compact table), cat_exclude_kernel (the
//                  exclusions by column: the seen lists within a candidate list, the query's own excluded items)
// and the host helpers every serving unit calls: the memory check, the training rows' id columns and lists, the uploads
// of a request's lists and of a caller's rows, the blank answer and the read-back of a top-N query.
#include "prelude.hpp"
#include "serve_frame.hpp"
#include "recommend.hpp"
#include "catalogue.hpp"

namespace mmsbm_hip_impl {

void require_free_mem(size_t bytes, const std::string &what) {
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (bytes + kFreeMargin > free_b)
    throw ApiError(MMSBM_E_TOOLARGE, what + " needs " + std::to_string(bytes >> 20) + " MB of device memory, " +
                                         std::to_string(free_b >> 20) + " MB free");
}

void train_id_columns(mmsbm_hip_ctx *c, std::vector<int32_t> &user, std::vector<int32_t> &item,
                      std::vector<int32_t> *rating) {
  hipStream_t s = c->stream;
  const size_t n = static_cast<size_t>(c->n_obs);
  user.resize(n);
  item.resize(n);
  if (rating) rating->resize(n);
  if (n > 0) {
    HIP_CHECK(hipMemcpyAsync(user.data(), c->orig_u.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(item.data(), c->orig_i.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    if (rating) HIP_CHECK(hipMemcpyAsync(rating->data(), c->orig_r.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  if (c->swapped) user.swap(item);  // (internal users = external items)
}

std::vector<int32_t> upload_train_lists(mmsbm_hip_ctx *c, DevBuf<int32_t> &d_off, DevBuf<int32_t> &d_item, const char *what) {
  std::vector<int32_t> eu, ei;
  train_id_columns(c, eu, ei, nullptr);
  std::vector<int32_t> item(eu.size(), 0);
  std::vector<int32_t> off = group_by_key<int32_t>(eu.data(), static_cast<int64_t>(eu.size()), c->ext_users,
                                                   [&](int64_t m, int32_t at) { item[at] = ei[m]; });
  sort_unique_groups(off, item);  // (duplicate pairs dropped)
  if (what) require_free_mem((off.size() + item.size()) * sizeof(int32_t), what);
  d_off.upload(off, c->stream);
  d_item.upload(item, c->stream);
  HIP_CHECK(hipStreamSynchronize(c->stream));  // (host vectors are locals)
  return off;
}

void DevCsr::upload(const RowCsr &lists, int64_t n_rows, hipStream_t st) {
  const int64_t n = entries(lists, n_rows);
  off_h.assign(lists.offsets, lists.offsets + n_rows + 1);
  off.upload(off_h, st);
  val.alloc(static_cast<size_t>(n));
  if (n > 0) HIP_CHECK(hipMemcpyAsync(val.ptr, lists.values, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
}

CallerRows::CallerRows(mmsbm_hip_ctx *c, int S, const ThetaQuery &q) : ids(static_cast<size_t>(q.n_users)), cand(q.cand) {
  const size_t tk = static_cast<size_t>(q.n_users) * c->ext_k;
  th.alloc(S * tk);
  if (S * tk > 0) HIP_CHECK(hipMemcpyAsync(th.ptr, q.theta, sizeof(double) * S * tk, hipMemcpyHostToDevice, c->stream));
  for (int64_t b = 0; b < q.n_users; ++b) ids[static_cast<size_t>(b)] = static_cast<int32_t>(b);
  if (q.seen.offsets && q.n_users > 0) seen.upload(q.seen, q.n_users, c->stream);
}

void fold_weights(hipStream_t st, const double *p, const double *w, double *out, int K, int L, int R, size_t rs, int ks, int ls) {
  LAUNCH(rec_w_kernel, static_cast<unsigned>((K * L + kBlock - 1) / kBlock), kBlock, 0, st, p, w, out, K, L, R, rs, ks, ls);
}

namespace {

void fold_launch(hipStream_t st, const RowTab &src, int d, const double *m, int mt, int mj, double *out, int rows, int rank) {
  const size_t n = static_cast<size_t>(rows) * rank;
  if (n == 0) return;
  LAUNCH(rec_fold_kernel, static_cast<unsigned>((n + kBlock - 1) / kBlock), kBlock, 0, st, src, d, m, mt, mj, out, rows,
         rank);
}

}  // namespace

void fold_rows(hipStream_t st, double *src, int d, const double *m, int mt, int mj, double *out, int rows, int rank) {
  fold_launch(st, plain_tab(src, d), d, m, mt, mj, out, rows, rank);
}

void fold_rows(mmsbm_hip_ctx *c, bool items_side, const double *m, int mt, int mj, double *out, int rank) {
  const ExtSlot e = ext_slot(c);
  if (items_side) fold_launch(c->stream, e.items, c->ext_l, m, mt, mj, out, c->ext_items, rank);
  else fold_launch(c->stream, e.users, c->ext_k, m, mt, mj, out, c->ext_users, rank);
}

void exclude_seen(hipStream_t st, const int32_t *ids, int nb, SeenLists seen, double *sc, size_t ld) {
  if (seen.off) LAUNCH(rec_exclude_kernel, nb, kBlock, 0, st, ids, seen.off, seen.items, sc, ld);
}

void exclude_seen_cols(hipStream_t st, const int32_t *ids, int nb, SeenLists seen, const int32_t *col_of, double *sc,
                       size_t ld) {
  if (seen.off) LAUNCH(cat_exclude_kernel, nb, kBlock, 0, st, ids, 0, seen.off, seen.items, col_of, sc, ld);
}

void score_tiles(mmsbm_hip_ctx *c, const double *a, size_t as, const double *b, size_t bs, int n_cols, const int32_t *ids,
                 int nb, SeenLists seen, double *sc) {
  if (n_cols == 0) return;
  LAUNCH(rec_score_kernel, tile_grid(n_cols, nb), kBlock, 0, c->stream, a, as, b, bs, ids, nb, n_cols, c->rc->rank,
         c->rc->slots, sc, static_cast<size_t>(n_cols));
  exclude_seen(c->stream, ids, nb, seen, sc, static_cast<size_t>(n_cols));
}

void rec_score_batch(mmsbm_hip_ctx *c, const double *x, size_t xs, const int32_t *ub, int nb, SeenLists seen, double *sc) {
  const RecSession &rc = *c->rc;
  score_tiles(c, x, xs, rc.y.ptr, static_cast<size_t>(rc.items) * rc.rank, rc.items, ub, nb, seen, sc);
}

void own_exclude_batch(hipStream_t st, const DevCsr &own, int64_t b0, int nb, const int32_t *col_of, double *sc, size_t ld) {
  LAUNCH(cat_exclude_kernel, nb, kBlock, 0, st, nullptr, static_cast<int>(b0), own.off.ptr, own.val.ptr, col_of, sc, ld);
}

void top_n_blank(int64_t n_rows, int n, const TopNOut &out) {
  for (int64_t b = 0; b < n_rows; ++b) {
    if (out.counts) out.counts[b] = 0;
    for (int k = 0; k < n; ++k) {
      out.items[static_cast<size_t>(b) * n + k] = -1;
      if (out.scores) out.scores[static_cast<size_t>(b) * n + k] = -INFINITY;
    }
  }
}

void SelectStage::run(hipStream_t st, const SelectPlan &p, const double *sc, int nb, int n, double *os, int32_t *oi,
                      int32_t *on) const {
  const auto [cap, lds] = select_list(n);
  const int I = p.cols;
  if (p.parts > 1) {
    LAUNCH(rec_select_kernel<false>, dim3(p.parts, nb), kRecWave, lds, st, sc, static_cast<size_t>(I), I, p.per, nullptr,
           nullptr, nullptr, 0, n, cap, cs.ptr, ci.ptr, cn.ptr);
    LAUNCH(rec_select_kernel<true>, dim3(1, nb), kRecWave, lds, st, nullptr, 0, I, 0, cs.ptr, ci.ptr, cn.ptr, p.parts, n,
           cap, os, oi, on);
  } else {
    LAUNCH(rec_select_kernel<false>, dim3(1, nb), kRecWave, lds, st, sc, static_cast<size_t>(I), I, I, nullptr, nullptr,
           nullptr, 0, n, cap, os, oi, on);
  }
}

void top_n_copy_out(mmsbm_hip_ctx *c, const TopNDev &dev, EventPair &ev, int64_t n_users, int n, TimedCall timed,
                    const TopNOut &out, const int32_t *cand, const double *dev_second, double *second) {
  hipStream_t st = c->stream;
  const size_t outs = static_cast<size_t>(n_users) * n;
  std::vector<double> hs(outs), h2(dev_second ? outs : 0);
  std::vector<int32_t> hi(outs), hn(static_cast<size_t>(n_users));
  HIP_CHECK(hipMemcpyAsync(hs.data(), dev.os, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
  if (dev_second) HIP_CHECK(hipMemcpyAsync(h2.data(), dev_second, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hi.data(), dev.oi, sizeof(int32_t) * outs, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hn.data(), dev.on, sizeof(int32_t) * n_users, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[timed] = ev.ms();
  for (int64_t b = 0; b < n_users; ++b) {
    const size_t o = static_cast<size_t>(b) * n;
    const int cnt = hn[static_cast<size_t>(b)];
    if (out.counts) out.counts[b] = cnt;
    for (int k = 0; k < cnt; ++k) {
      out.items[o + k] = item_of(cand, hi[o + k]);
      if (out.scores) out.scores[o + k] = hs[o + k];
      if (dev_second && second) second[o + k] = h2[o + k];
    }
  }
}

void cat_table(mmsbm_hip_ctx *c, const Subset &cand, CatTable &t) {
  const RecSession &rc = *c->rc;
  const int NI = rc.items, rank = rc.rank, S = rc.slots, C = cand.n;
  const size_t ycs = static_cast<size_t>(C) * rank;
  hipStream_t st = c->stream;
  t.cand.alloc(static_cast<size_t>(C));
  t.col.alloc(static_cast<size_t>(NI));
  t.y.alloc(S * ycs);
  HIP_CHECK(hipMemcpyAsync(t.cand.ptr, cand.items, sizeof(int32_t) * C, hipMemcpyHostToDevice, st));
  EventPair ev;
  ev.start(st);
  LAUNCH(cat_gather_kernel, static_cast<unsigned>((S * ycs + kBlock - 1) / kBlock), kBlock, 0, st, rc.y.ptr,
         static_cast<size_t>(NI) * rank, t.cand.ptr, C, rank, S, t.y.ptr);
  LAUNCH(cat_cols_kernel, static_cast<unsigned>((NI + kBlock - 1) / kBlock), kBlock, 0, st, t.cand.ptr, C, NI, t.col.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  HIP_CHECK(hipStreamSynchronize(st));
  t.ms = ev.ms();
}

void within_prepare(mmsbm_hip_ctx *c, const UserQuery &q, WithinPrep &w) {
  const RecSession &rc = *c->rc;
  const int NI = rc.items, rank = rc.rank;
  const int64_t n_users = q.users.n;
  w.C = q.cand.columns(NI);
  w.has_cand = q.cand.items != nullptr;
  w.has_own = q.excl.offsets != nullptr;
  const size_t ycs = static_cast<size_t>(w.C) * rank;
  if (w.has_cand || w.has_own)
    require_free_mem(CatTable::bytes(rc, q.cand) + (static_cast<size_t>(n_users) + 1 + DevCsr::entries(q.excl, n_users)) * 4,
                     "recommend: the candidates' rows and the query's excluded items");
  if (w.has_own) w.own.upload(q.excl, n_users, c->stream);
  if (w.has_cand) cat_table(c, q.cand, w.ct);
  w.y = w.has_cand ? w.ct.y.ptr : rc.y.ptr;
  w.ys = w.has_cand ? ycs : static_cast<size_t>(NI) * rank;
}

}  // namespace mmsbm_hip_impl
