// tu_recommend.hip -- translation unit of the recommend session and the queries that are its score tiles, exclusions and
// selection as they are, in the frame of serve_frame.hpp (the kernels those share are launched by tu_serve_frame.hip):
//   recommend.hpp  the recommend session: training items per user, the per-slot fold, scores, selection; launched here:
//                  the positions
//   catalogue.hpp  queries within a part of the catalogue: a compact item table, the query's own exclusions (both the
//                  frame's); launched here: the ranking of per-row candidate lists
//   quota.hpp      per-category caps: a mask over the batch buffer between the exclusions and the same selection
//   shelves.hpp    category-level recommendation: the batch buffer reduced per (row, category) to a value buffer, the same
//                  selection over it, then the chosen categories' items
#include "prelude.hpp"
#include "serve_frame.hpp"
#include "recommend.hpp"
#include "catalogue.hpp"
#include "quota.hpp"
#include "shelves.hpp"

namespace mmsbm_hip_impl {

void recommend_begin(mmsbm_hip_ctx *c, const double *weights, int exclude_train) {
  use_device(c);
  c->rc.reset();  // (from here on the previous session is gone)
  auto rc = std::make_unique<RecSession>();
  hipStream_t s = c->stream;
  rc->w.alloc(c->n_ratings);
  HIP_CHECK(hipMemcpyAsync(rc->w.ptr, weights, sizeof(double) * c->n_ratings, hipMemcpyHostToDevice, s));
  rc->excl = exclude_train != 0;
  rc->w_min = *std::min_element(weights, weights + c->n_ratings);  // (the temperature floor of explore.hpp)
  rc->w_max = *std::max_element(weights, weights + c->n_ratings);
  if (rc->excl) rc->seen_off_h = upload_train_lists(c, rc->seen_off, rc->seen, nullptr);  // (also the candidate counts of recommend_positions)
  HIP_CHECK(hipStreamSynchronize(s));
  rc->rank = std::min(c->ext_k, c->ext_l);
  rc->users = c->ext_users;
  rc->items = c->ext_items;
  c->rc = std::move(rc);
}

void recommend_add(mmsbm_hip_ctx *c) {  // the selected slot (the caller holds a OneSlot)
  use_device(c);
  RecSession &rc = *c->rc;
  const int U = c->ext_users, I = c->ext_items, K = c->ext_k, L = c->ext_l, R = c->n_ratings, rank = rc.rank;
  const int S = rc.slots;
  const size_t xs = static_cast<size_t>(U) * rank, ys = static_cast<size_t>(I) * rank;
  require_free_mem(((S + 1) * (xs + ys + static_cast<size_t>(K) * L)) * sizeof(double), "recommend: the slots' factors");
  hipStream_t st = c->stream;
  // the three tables grow by one slot (W of every slot is kept: recommend_query_theta folds the caller's rows with it)
  DevBuf<double> nx, ny, nw;
  double *xo = grow_by_slot(rc.x, xs, S, st, nx), *yo = grow_by_slot(rc.y, ys, S, st, ny);
  double *wo = grow_by_slot(rc.wk, static_cast<size_t>(K) * L, S, st, nw);
  const ExtSlot e = ext_slot(c);
  fold_weights(st, e.p, rc.w.ptr, wo, K, L, R, e.rs, e.ks, e.ls);
  if (K <= L) {  // x = theta, y = eta W^T: y[i, k] = sum_l eta[i, l] W[k, l]
    fold_rows(c, false, nullptr, 0, 0, xo, rank);
    fold_rows(c, true, wo, 1, L, yo, rank);
  } else {       // x = theta W: x[u, l] = sum_k theta[u, k] W[k, l], y = eta
    fold_rows(c, false, wo, L, 1, xo, rank);
    fold_rows(c, true, nullptr, 0, 0, yo, rank);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  rc.x.swap(nx);
  rc.y.swap(ny);
  rc.wk.swap(nw);
  rc.slots = S + 1;
}

void recommend_add_items(mmsbm_hip_ctx *c, int32_t n_new, const double *eta, const int64_t *seen_off,
                         const int32_t *seen_users) {
  use_device(c);
  if (n_new == 0) return;
  RecSession &rc = *c->rc;
  const int U = c->ext_users, I = c->ext_items, K = c->ext_k, L = c->ext_l, rank = rc.rank, S = rc.slots;
  const int NI = I + n_new;
  const size_t ys = static_cast<size_t>(I) * rank, nys = static_cast<size_t>(NI) * rank;
  const size_t el = static_cast<size_t>(n_new) * L, kl = static_cast<size_t>(K) * L;
  require_free_mem(S * (nys + el) * sizeof(double), "recommend: the added items' factors");
  hipStream_t st = c->stream;
  // every slot's table grows from I to I + n_new rows: the training rows copied as they are, the new rows folded with
  // the slot's W exactly as recommend_add folds the slot's own eta (y = eta W^T when K <= L, else y = eta)
  DevBuf<double> ny, de;
  DevBuf<int32_t> so, si;
  ny.alloc(S * nys);
  de.alloc(S * el);
  HIP_CHECK(hipMemcpyAsync(de.ptr, eta, sizeof(double) * S * el, hipMemcpyHostToDevice, st));
  for (int s = 0; s < S; ++s) {
    if (ys > 0)
      HIP_CHECK(hipMemcpyAsync(ny.ptr + s * nys, rc.y.ptr + s * ys, sizeof(double) * ys, hipMemcpyDeviceToDevice, st));
    const double *m = K <= L ? rc.wk.ptr + s * kl : nullptr;
    fold_rows(st, de.ptr + s * el, L, m, 1, L, ny.ptr + s * nys + ys, n_new, rank);  // (n_new > 0: a launch)
  }
  HIP_CHECK(hipGetLastError());
  // the seen pairs: user u also leaves out the new items whose list names it.  A user's list stays ascending and
  // distinct: its training items (< I) first, then its new items (>= I), sorted and de-duplicated.
  const int64_t n_seen = seen_off ? seen_off[n_new] : 0;  // (checked: below 2^31)
  if (n_seen > 0) {
    std::vector<int32_t> old_off = rc.excl ? rc.seen_off_h : std::vector<int32_t>(static_cast<size_t>(U) + 1, 0);
    std::vector<int32_t> old(static_cast<size_t>(old_off[U]));
    if (!old.empty())
      HIP_CHECK(hipMemcpyAsync(old.data(), rc.seen.ptr, sizeof(int32_t) * old.size(), hipMemcpyDeviceToHost, st));
    // the new pairs (user seen_users[e], item I + j for e in item j's range) grouped by user
    std::vector<int32_t> pit(static_cast<size_t>(n_seen)), nit(static_cast<size_t>(n_seen));
    for (int32_t j = 0; j < n_new; ++j) std::fill(pit.begin() + seen_off[j], pit.begin() + seen_off[j + 1], I + j);
    std::vector<int32_t> noff = group_by_key<int32_t>(seen_users, n_seen, U, [&](int64_t e, int32_t at) { nit[at] = pit[e]; });
    sort_unique_groups(noff, nit);
    HIP_CHECK(hipStreamSynchronize(st));
    std::vector<int32_t> off(static_cast<size_t>(U) + 1, 0), item;
    item.reserve(old.size() + static_cast<size_t>(n_seen));
    for (int u = 0; u < U; ++u) {
      off[u] = static_cast<int32_t>(item.size());
      item.insert(item.end(), old.begin() + old_off[u], old.begin() + old_off[u + 1]);
      item.insert(item.end(), nit.begin() + noff[u], nit.begin() + noff[u + 1]);
    }
    off[U] = static_cast<int32_t>(item.size());
    so.upload(off, st);
    si.upload(item, st);
    HIP_CHECK(hipStreamSynchronize(st));  // (host vectors are locals)
    rc.seen_off.swap(so);
    rc.seen.swap(si);
    rc.seen_off_h = off;
    rc.excl = true;
  }
  HIP_CHECK(hipStreamSynchronize(st));
  rc.y.swap(ny);
  rc.items = NI;
  rc.by_item_off.release();  // (the item -> users lists follow the session's lists and catalogue: built again on use)
  rc.by_item.release();
  rc.by_item_built = false;
}

namespace {

// A recommend query: the users (host ids, rows of x: `slots` tables of xs doubles, [row][rank]) scored against the
// session's items; seen (indexed by those ids): the items left out.
void rec_run(mmsbm_hip_ctx *c, const double *x, size_t xs, const UserRows &users, SeenLists seen, int n, const TopNOut &out) {
  top_n_run(c, c->rc->items, users.n, users.ids, n, "recommend: a batch of users",
            [&](const int32_t *ub, int nb, int64_t, double *sc) { rec_score_batch(c, x, xs, ub, nb, seen, sc); },
            T_RECOMMEND, out);
}

// The capped categories of a query on the device (quota.hpp): the plan of serve_plan.hpp, held for as long as the mask
// lives (the copies are asynchronous), and the launches that apply it to a batch buffer
struct QuotaMask {
  QuotaPlan plan;
  DevBuf<int32_t> off, col, cap, wave_first, wave_info;
  void upload(QuotaPlan &&p, hipStream_t st) {
    plan = std::move(p);
    off.upload(plan.off, st);
    col.upload(plan.col, st);
    cap.upload(plan.cap, st);
    wave_first.upload(plan.wave_first, st);
    wave_info.upload(plan.wave_info, st);
  }
  // sc [nb][ld]: every row masked, each category by the form its (m, q) selects
  void apply(hipStream_t st, int nb, double *sc, size_t ld) const {
    const int waves = static_cast<int>(plan.wave_first.size());
    if (waves > 0)
      LAUNCH(quota_short_kernel, dim3(static_cast<unsigned>((waves + kQuotaWaves - 1) / kQuotaWaves), nb), kBlock, 0, st,
             wave_first.ptr, wave_info.ptr, waves, off.ptr, col.ptr, cap.ptr, sc, ld);
    if (plan.n_long() > 0) {
      const auto [places, lds] = select_list(plan.long_cap);
      LAUNCH(quota_long_kernel, dim3(static_cast<unsigned>(plan.n_long()), nb), kRecWave, lds, st, off.ptr, col.ptr, cap.ptr,
             plan.n_short, places, sc, ld);
    }
  }
};

// rec_run of the query q: within its candidates, without its own excluded items, and with the capped categories
// `cats` (null: none; quota.hpp), planned against the candidates (serve_plan.hpp).  Without candidates, own lists and a
// category that can change the answer: rec_run.
void rec_run_within(mmsbm_hip_ctx *c, const double *x, size_t xs, const UserQuery &q, SeenLists seen, int n,
                    const TopNOut &out, const Categories *cats = nullptr) {
  QuotaMask mask;
  if (cats && cats->n > 0 && q.users.n > 0 && q.cand.columns(c->rc->items) > 0) {
    QuotaPlan plan = plan_quota(q.cand.items, q.cand.n, cats->n, cats->offsets, cats->items, cats->caps, n);
    if (plan.kept() > 0) {
      require_free_mem(plan.bytes(), "recommend: the capped categories");
      mask.upload(std::move(plan), c->stream);
    }
  }
  const bool masked = mask.plan.kept() > 0;
  if (!q.cand.items && !q.excl.offsets && !masked) {
    rec_run(c, x, xs, q.users, seen, n, out);
    return;
  }
  top_n_blank(q.users.n, n, out);
  rec_within_run(c, q, seen, n, rec_tiles(c, x, xs), T_RECOMMEND, out,
                 [&](const WithinPrep &w, const int32_t *, int nb, double *sc) {  // behind the exclusions: the caps
                   if (masked) mask.apply(c->stream, nb, sc, static_cast<size_t>(w.C));
                 },
                 masked);
}

// ... of a caller's theta rows, folded first
void rec_theta_run(mmsbm_hip_ctx *c, const ThetaQuery &t, int n, const TopNOut &out, const Categories *cats = nullptr) {
  rec_theta_fold(c, t, [&](const double *x, size_t xs, const UserQuery &q, SeenLists seen) {
    rec_run_within(c, x, xs, q, seen, n, out, cats);
  });
}

// ---- category-level recommendation (shelves.hpp) -------------------------------------------------------------------------
// The categories of a shelves query on the device: the plan of serve_plan.hpp, held for as long as the query runs (the
// copies are asynchronous)
struct ShelfCats {
  ShelfPlan plan;
  DevBuf<int32_t> off, col, slot, of_slot, wave_first, wave_info;
  void upload(ShelfPlan &&p, hipStream_t st) {
    plan = std::move(p);
    off.upload(plan.off, st);
    col.upload(plan.col, st);
    slot.upload(plan.slot, st);
    of_slot.upload(plan.of_slot, st);
    wave_first.upload(plan.wave_first, st);
    wave_info.upload(plan.wave_info, st);
  }
  // val [nb][kept] (and avail, or null) from the batch buffer sc [nb][ld]: each category by the form its size selects
  void values(hipStream_t st, int nb, const double *sc, size_t ld, int depth, int min_items, double *val,
              int32_t *avail) const {
    const int waves = static_cast<int>(plan.wave_first.size());
    const size_t G = static_cast<size_t>(plan.kept());
    if (waves > 0)
      LAUNCH(shelf_value_short_kernel, dim3(static_cast<unsigned>((waves + kQuotaWaves - 1) / kQuotaWaves), nb), kBlock, 0,
             st, wave_first.ptr, wave_info.ptr, waves, off.ptr, col.ptr, slot.ptr, depth, min_items, sc, ld, val, avail, G);
    if (plan.n_long() > 0) {
      const auto [places, lds] = select_list(depth);
      LAUNCH(shelf_value_long_kernel, dim3(static_cast<unsigned>(plan.n_long()), nb), kRecWave, lds, st, off.ptr, col.ptr,
             slot.ptr, plan.n_short, depth, min_items, places, sc, ld, val, avail, G);
    }
  }
};

// Every row of a shelves answer as "no shelf" (the last three: null when per_shelf = 0)
void shelves_blank(int64_t n_users, const ShelfAsk &ask, const ShelfOut &out) {
  const size_t ns = static_cast<size_t>(ask.n_shelves), ps = static_cast<size_t>(ask.per_shelf);
  for (size_t b = 0; b < static_cast<size_t>(n_users); ++b) {
    out.shelf_counts[b] = 0;
    for (size_t k = 0; k < ns; ++k) {
      out.shelf_cats[b * ns + k] = -1;
      out.shelf_values[b * ns + k] = -INFINITY;
      out.shelf_available[b * ns + k] = 0;
      if (ps > 0) out.item_counts[b * ns + k] = 0;
      for (size_t e = 0; e < ps; ++e) {
        out.items[(b * ns + k) * ps + e] = -1;
        out.scores[(b * ns + k) * ps + e] = -INFINITY;
      }
    }
  }
}

// The start of both shelves entries, before any launch: every row blanked and the host plan made.  False: no row, no
// candidate or no category with a column -- every row stays empty and nothing is launched.
bool shelves_begin(mmsbm_hip_ctx *c, int64_t n_users, const Subset &cand, const Categories &cats, const ShelfAsk &ask,
                   const ShelfOut &out, ShelfPlan &plan) {
  shelves_blank(n_users, ask, out);
  c->last_ms[T_RECOMMEND] = 0.f;
  if (n_users == 0 || cats.n == 0 || cand.columns(c->rc->items) == 0) return false;
  plan = plan_shelves(cand.items, cand.n, cats.n, cats.offsets, cats.items);
  return plan.kept() > 0;
}

// A shelves query: the rows of q (host ids, rows of x) within its subset and own lists as rec_within_device's, the
// categories of `plan`.  The batches are a BatchFrame over the C item columns, the selection a stage over the G value columns:
// per batch the score tiles and the exclusions (within_fill: the launches of recommend_query_within), the value kernels,
// the selection over the value buffer and the chosen shelves' items, all before the next batch overwrites the scores;
// every row's result stays on the device until the end.  `plan`: shelves_begin's, with at least one category.
void rec_shelves_run(mmsbm_hip_ctx *c, const double *x, size_t xs, const UserQuery &q, SeenLists seen, ShelfPlan &&plan,
                     const ShelfAsk &ask, const ShelfOut &out) {
  const int64_t n_users = q.users.n;
  ShelfCats sh;
  require_free_mem(plan.bytes(), "recommend_shelves: the categories");
  sh.upload(std::move(plan), c->stream);
  hipStream_t st = c->stream;
  const int G = sh.plan.kept(), ns = ask.n_shelves, ps = ask.per_shelf;
  WithinPrep w;
  within_prepare(c, q, w);
  const int C = w.C;
  BatchFrame fr(C, n_users);  // (the item buffer decides the batch: G <= C)
  const SelectPlan sp = select_plan(c, G, fr.bu, ns);
  const size_t rows_ns = static_cast<size_t>(n_users) * ns, outs = rows_ns * ps;
  const size_t vals = static_cast<size_t>(fr.bu) * G;
  require_free_mem(fr.bytes() + vals * (ps == 0 ? 12 : 8) + sp.bytes() + rows_ns * 20 + outs * 12 +
                       static_cast<size_t>(n_users) * 4,
                   "recommend_shelves: a batch of users");
  const SelectStage sel(sp);
  DevBuf<int32_t> oi, on, oa, av, ic, in;
  DevBuf<double> val, os, is;
  val.alloc(vals);
  if (ps == 0) av.alloc(vals);
  os.alloc(rows_ns); oi.alloc(rows_ns); oa.alloc(rows_ns); on.alloc(n_users);
  if (ps > 0) {
    is.alloc(outs); ic.alloc(outs); in.alloc(rows_ns);
  }
  const auto tiles = rec_tiles(c, x, xs);
  const std::pair<int, size_t> list = select_list(std::max(ps, 1));  // shelf_items_kernel's places and their LDS bytes
  fr.run(st, q.users.ids, [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
    int32_t *obi = oi.ptr + b0 * ns, *obn = on.ptr + b0, *oba = oa.ptr + b0 * ns;
    within_fill(c, w, tiles, seen, ub, nb, b0, sc);
    sh.values(st, nb, sc, static_cast<size_t>(C), ask.depth, ask.min_items, val.ptr, av.ptr);
    sel.run(st, sp, val.ptr, nb, ns, os.ptr + b0 * ns, obi, obn);
    if (ps > 0)
      LAUNCH(shelf_items_kernel, dim3(static_cast<unsigned>(ns), nb), kRecWave, list.second, st, obi, obn, sh.of_slot.ptr,
             sh.off.ptr, sh.col.ptr, ps, list.first, sc, static_cast<size_t>(C), ic.ptr + b0 * ns * ps, is.ptr + b0 * ns * ps, in.ptr + b0 * ns,
             oba);
    else
      LAUNCH(shelf_avail_kernel, nb, kRecWave, 0, st, obi, obn, ns, av.ptr, static_cast<size_t>(G), oba);
  });
  std::vector<double> hs(rows_ns), his(outs);
  std::vector<int32_t> hi(rows_ns), ha(rows_ns), hn(static_cast<size_t>(n_users)), hic(outs), hin(ps > 0 ? rows_ns : 0);
  HIP_CHECK(hipMemcpyAsync(hs.data(), os.ptr, sizeof(double) * rows_ns, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hi.data(), oi.ptr, sizeof(int32_t) * rows_ns, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(ha.data(), oa.ptr, sizeof(int32_t) * rows_ns, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hn.data(), on.ptr, sizeof(int32_t) * n_users, hipMemcpyDeviceToHost, st));
  if (ps > 0) {
    HIP_CHECK(hipMemcpyAsync(his.data(), is.ptr, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hic.data(), ic.ptr, sizeof(int32_t) * outs, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hin.data(), in.ptr, sizeof(int32_t) * rows_ns, hipMemcpyDeviceToHost, st));
  }
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_RECOMMEND] = fr.ev.ms() + w.ct.ms;
  for (size_t b = 0; b < static_cast<size_t>(n_users); ++b) {
    const int cnt = hn[b];
    out.shelf_counts[b] = cnt;
    for (size_t k = 0; k < static_cast<size_t>(cnt); ++k) {
      const size_t o = b * ns + k;
      out.shelf_cats[o] = sh.plan.cat[static_cast<size_t>(sh.plan.of_slot[static_cast<size_t>(hi[o])])];
      out.shelf_values[o] = hs[o];
      out.shelf_available[o] = ha[o];
      if (ps == 0) continue;
      out.item_counts[o] = hin[o];
      for (size_t e = 0; e < static_cast<size_t>(hin[o]); ++e) {
        out.items[o * ps + e] = item_of(q.cand.items, hic[o * ps + e]);
        out.scores[o * ps + e] = his[o * ps + e];
      }
    }
  }
}

}  // namespace

void recommend_query(mmsbm_hip_ctx *c, const UserRows &users, int n, const TopNOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  rec_run(c, rc.x.ptr, rc.x_stride(), users, rc.seen_lists(), n, out);
}

void recommend_query_within(mmsbm_hip_ctx *c, const UserQuery &q, int n, const TopNOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  rec_run_within(c, rc.x.ptr, rc.x_stride(), q, rc.seen_lists(), n, out);
}

void recommend_query_theta(mmsbm_hip_ctx *c, const ThetaQuery &q, int n, const TopNOut &out) {
  use_device(c);
  rec_theta_run(c, q, n, out);
}

void recommend_query_quota(mmsbm_hip_ctx *c, const UserQuery &q, const Categories &cats, int n, const TopNOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  rec_run_within(c, rc.x.ptr, rc.x_stride(), q, rc.seen_lists(), n, out, &cats);
}

void recommend_query_theta_quota(mmsbm_hip_ctx *c, const ThetaQuery &q, const Categories &cats, int n, const TopNOut &out) {
  use_device(c);
  rec_theta_run(c, q, n, out, &cats);
}

void recommend_query_shelves(mmsbm_hip_ctx *c, const UserQuery &q, const Categories &cats, const ShelfAsk &ask,
                             const ShelfOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  ShelfPlan plan;
  if (!shelves_begin(c, q.users.n, q.cand, cats, ask, out, plan)) return;
  rec_shelves_run(c, rc.x.ptr, rc.x_stride(), q, rc.seen_lists(), std::move(plan), ask, out);
}

void recommend_query_theta_shelves(mmsbm_hip_ctx *c, const ThetaQuery &t, const Categories &cats, const ShelfAsk &ask,
                                   const ShelfOut &out) {
  use_device(c);
  ShelfPlan plan;
  if (!shelves_begin(c, t.n_users, t.cand, cats, ask, out, plan)) return;
  rec_theta_fold(c, t, [&](const double *x, size_t xs, const UserQuery &q, SeenLists seen) {
    rec_shelves_run(c, x, xs, q, seen, std::move(plan), ask, out);
  });
}

void recommend_rank(mmsbm_hip_ctx *c, const UserRows &users, const RowCsr &cands, int n, const TopNOut &out) {
  const int64_t n_users = users.n;
  use_device(c);
  const RecSession &rc = *c->rc;
  top_n_blank(n_users, n, out);
  c->last_ms[T_RECOMMEND] = 0.f;
  if (n_users == 0) return;
  hipStream_t st = c->stream;
  const auto [cap, lds] = select_list(n);
  const size_t outs = static_cast<size_t>(n_users) * n;
  require_free_mem(outs * 12 + (2 * static_cast<size_t>(n_users) + 1 + static_cast<size_t>(cands.offsets[n_users])) * 4 +
                       static_cast<size_t>(n_users) * 4,
                   "recommend_rank: the users' lists and results");
  DevBuf<int32_t> du, oi, on;
  DevBuf<double> os;
  DevCsr lists;  // every request row's candidates
  du.alloc(static_cast<size_t>(n_users));
  lists.upload(cands, n_users, st);
  os.alloc(outs); oi.alloc(outs); on.alloc(static_cast<size_t>(n_users));
  HIP_CHECK(hipMemcpyAsync(du.ptr, users.ids, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  const SeenLists seen = rc.seen_lists();
  EventPair ev;  // device time of the query's kernel (option "recommend_ms")
  ev.start(st);
  LAUNCH(cat_rank_kernel, static_cast<unsigned>(n_users), kRecWave, lds, st, rc.x.ptr, rc.x_stride(), rc.y.ptr,
         static_cast<size_t>(rc.items) * rc.rank, rc.rank, rc.slots, du.ptr, lists.off.ptr, lists.val.ptr, seen.off,
         seen.items, n, cap, os.ptr, oi.ptr, on.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  top_n_copy_out(c, TopNDev{os.ptr, oi.ptr, on.ptr}, ev, n_users, n, T_RECOMMEND, out);
}

void recommend_positions(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int64_t *offsets,
                         const int32_t *items, int32_t *positions, int32_t *candidates) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int I = rc.items;
  const int64_t total = n_users > 0 ? offsets[n_users] : 0;  // (checked: below 2^31)
  for (int64_t b = 0; b < n_users && candidates; ++b) {
    const int32_t u = users[b];
    candidates[b] = rc.excl ? I - (rc.seen_off_h[u + 1] - rc.seen_off_h[u]) : I;
  }
  // only the users that hold test items are scored: the others' ranges are empty, so the ranges of the rows kept
  // follow each other and toff[k] = offsets[row k] (toff[na] = total)
  std::vector<int32_t> hu, toff;
  for (int64_t b = 0; b < n_users; ++b)
    if (offsets[b + 1] > offsets[b]) {
      hu.push_back(users[b]);
      toff.push_back(static_cast<int32_t>(offsets[b]));
    }
  toff.push_back(static_cast<int32_t>(total));
  const int64_t na = static_cast<int64_t>(hu.size());
  if (na == 0) {
    c->last_ms[T_POSITIONS] = 0.f;
    return;
  }
  hipStream_t st = c->stream;
  const int64_t bu = rec_batch_users(I, na);
  // items split across workgroups until about 8 counting workgroups per CU are in flight; the counts are integers,
  // so the split cannot change a position
  const auto [parts, per] = item_parts(I, bu, 8LL * c->n_cus, kPosMinPerPart);
  int64_t most = 0;  // test entries of the largest batch
  for (int64_t b0 = 0; b0 < na; b0 += bu) most = std::max<int64_t>(most, toff[std::min(na, b0 + bu)] - toff[b0]);
  require_free_mem(static_cast<size_t>(bu) * I * sizeof(double) + static_cast<size_t>(most) * parts * 4 +
                       static_cast<size_t>(total) * 8 + static_cast<size_t>(na) * 8,
                   "recommend: the positions of a batch of users");
  DevBuf<int32_t> du, dto, dit, dpos, pc;
  DevBuf<double> sc;
  du.upload(hu, st);
  dto.upload(toff, st);
  dit.alloc(static_cast<size_t>(total));
  dpos.alloc(static_cast<size_t>(total));
  pc.alloc(static_cast<size_t>(most) * parts);
  sc.alloc(static_cast<size_t>(bu) * I);
  HIP_CHECK(hipMemcpyAsync(dit.ptr, items, sizeof(int32_t) * total, hipMemcpyHostToDevice, st));
  EventPair ev;  // device time of the call's kernels (option "position_ms")
  ev.start(st);
  for (int64_t b0 = 0; b0 < na; b0 += bu) {  // (batches follow each other on the stream)
    const int nb = static_cast<int>(std::min(bu, na - b0));
    rec_score_batch(c, rc.x.ptr, rc.x_stride(), du.ptr + b0, nb, rc.seen_lists(), sc.ptr);
    LAUNCH(rec_position_kernel, dim3(parts, nb), kBlock, 0, st, sc.ptr, static_cast<size_t>(I), I, per, dto.ptr + b0,
           dit.ptr, pc.ptr);
    LAUNCH(rec_position_sum_kernel, nb, kBlock, 0, st, sc.ptr, static_cast<size_t>(I), dto.ptr + b0, dit.ptr, pc.ptr,
           parts, dpos.ptr);
    HIP_CHECK(hipGetLastError());
  }
  ev.stop(st);
  HIP_CHECK(hipMemcpyAsync(positions, dpos.ptr, sizeof(int32_t) * total, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_POSITIONS] = ev.ms();
}

}  // namespace mmsbm_hip_impl
