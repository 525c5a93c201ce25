// tu_recommend.hip -- translation unit of the serving queries: the host side of the sessions and queries whose kernels
// live in the headers below.  Every batched query runs in one frame (BatchFrame: the ids, the batch buffer, the loop, the
// event pair) and selects through one stage (SelectStage: the split's scratch and launches); a top-N query is the two
// together (top_n_device) and ends in one read-back (top_n_copy_out).  The round-based queries keep their round loops and
// share the loop over a round's batches (for_batches), the tile grid and the seen exclusion (tile_grid, exclude_seen).
// The integer planning of the queries is serve_plan.hpp.
//   recommend.hpp  the recommend session: training items per user, the per-slot fold, scores, selection, positions
//   similar.hpp    nearest items / users: a session of its own, the same batches and selection
//   top_pairs.hpp  the m best pairs of the whole model: a query of the recommend session with kernels of its own
//   pairs_bulk.hpp the m best pairs beyond 1,024: a radix select of the bar over the score tiles, count-then-write, then
//                  the sorts of tu_pairs_bulk.hip; the host steps are pairs_bulk_plan.hpp
//   overlap.hpp    the overlap of the restarts' groups: a session that copies a slot's rows with rec_fold_kernel
//   audience.hpp   item-side queries: the n best users of an item, and an item's audience above a bar (fused kernel)
//   catalogue.hpp  queries within a part of the catalogue: a compact item table, the query's own exclusions, ranking
//   diverse.hpp    diversified top-N: the pool kept on the device, then a greedy kernel; reads the similarity session
//   inform.hpp     the most informative items of a user: a session of its own behind a score kernel of its own
//   group.hpp      group queries: the members' score tiles reduced per group, then the same selection
//   ensemble.hpp   ensemble-aware queries: the restarts' scores reduced per pair (min, max, mean - risk std), then the
//                  same selection; the spread of given pairs
//   quota.hpp      per-category caps: a mask over the batch buffer between the exclusions and the same selection
//   allocate.hpp   capacity-aware allocation: rounds of the user-side and the item-side batches with a threshold epilogue
//                  on the score tile, the same exclusions and selection; the lists and the keys stay on the device
//   shelves.hpp    category-level recommendation: the batch buffer reduced per (row, category) to a value buffer, the same
//                  selection over it, then the chosen categories' items
//   explore.hpp    randomised top-N with propensities: the batch buffer moved to a second one and perturbed with Gumbel
//                  noise from a counter-based PCG64 stream, the same selection over the keys, then each position's
//                  probability from the unperturbed scores; the propensities of given lists
//   assortment.hpp greedy assortment selection: rounds of a gain pass over the score tiles against a per-user state, an
//                  arg-max over the catalogue and a state update, chained on the stream behind a stop flag
//   assign.hpp     welfare-maximising assignment: rounds of a forward auction over the compacted active users -- the
//                  score tile less a price per column, the same exclusions and selection with n = 2, the bids sorted
//                  (tu_pairs_bulk.hip) and merged into the items' slots by one wave per item
#include "prelude.hpp"
#include "recommend.hpp"
#include "similar.hpp"
#include "overlap.hpp"
#include "top_pairs.hpp"
#include "audience.hpp"
#include "pairs_bulk.hpp"
#include "catalogue.hpp"
#include "diverse.hpp"
#include "inform.hpp"
#include "group.hpp"
#include "ensemble.hpp"
#include "quota.hpp"
#include "allocate.hpp"
#include "shelves.hpp"
#include "explore.hpp"
#include "assortment.hpp"
#include "assign.hpp"

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

namespace {

// Every external user's distinct training items, ascending, onto the device (off [U + 1], item); returns the offsets.
// `what`: the memory is checked under that name first (null: no check).  The stream has passed the copies on return.
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

// A query's lists by request row on the device: host int64 offsets [n_rows + 1] narrowed to int32 (checked: below
// 2^31) and the values behind them.  Holds the narrowed offsets for as long as it lives: the copies are asynchronous.
// Never uploaded: both pointers null ("no list").
struct DevCsr {
  DevBuf<int32_t> off, val;
  std::vector<int32_t> off_h;
  static int64_t entries(const int64_t *offsets, int64_t n_rows) { return offsets && n_rows > 0 ? offsets[n_rows] : 0; }
  void upload(const int64_t *offsets, const int32_t *values, int64_t n_rows, hipStream_t st) {
    const int64_t n = entries(offsets, n_rows);
    off_h.assign(offsets, offsets + n_rows + 1);
    off.upload(off_h, st);
    val.alloc(static_cast<size_t>(n));
    if (n > 0) HIP_CHECK(hipMemcpyAsync(val.ptr, values, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
  }
  SeenLists lists() const { return {off.ptr, val.ptr}; }
};

// The rows a caller brings instead of the session's users: theta [S][n_users][K] on the device as it is, the identity
// ids 0 .. n_users - 1 (request row b is row b of every slot's block) and the caller's seen lists by row (null: none).
// The caller has checked the memory.
struct CallerRows {
  DevBuf<double> th;
  std::vector<int32_t> ids;
  DevCsr seen;
  CallerRows(mmsbm_hip_ctx *c, int S, int64_t n_users, const double *theta, const int64_t *seen_offsets,
             const int32_t *seen_items)
      : ids(static_cast<size_t>(n_users)) {
    const size_t tk = static_cast<size_t>(n_users) * c->ext_k;
    th.alloc(S * tk);
    if (S * tk > 0) HIP_CHECK(hipMemcpyAsync(th.ptr, theta, sizeof(double) * S * tk, hipMemcpyHostToDevice, c->stream));
    for (int64_t b = 0; b < n_users; ++b) ids[static_cast<size_t>(b)] = static_cast<int32_t>(b);
    if (seen_offsets && n_users > 0) seen.upload(seen_offsets, seen_items, n_users, c->stream);
  }
};

}  // namespace

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
  LAUNCH(rec_w_kernel, static_cast<unsigned>((K * L + kBlock - 1) / kBlock), kBlock, 0, st, e.p, rc.w.ptr, wo, K, L, R,
         e.rs, e.ks, e.ls);
  auto fold = [&](const RowTab &src, int d, const double *m, int mt, int mj, double *out, int rows) {
    const size_t n = static_cast<size_t>(rows) * rank;
    if (n == 0) return;
    LAUNCH(rec_fold_kernel, static_cast<unsigned>((n + kBlock - 1) / kBlock), kBlock, 0, st, src, d, m, mt, mj, out,
           rows, rank);
  };
  if (K <= L) {  // x = theta, y = eta W^T: y[i, k] = sum_l eta[i, l] W[k, l]
    fold(e.users, K, nullptr, 0, 0, xo, U);
    fold(e.items, L, wo, 1, L, yo, I);
  } else {       // x = theta W: x[u, l] = sum_k theta[u, k] W[k, l], y = eta
    fold(e.users, K, wo, L, 1, xo, U);
    fold(e.items, L, nullptr, 0, 0, yo, I);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  rc.x.swap(nx);
  rc.y.swap(ny);
  rc.wk.swap(nw);
  rc.slots = S + 1;
}

void recommend_add_items(mmsbm_hip_ctx *c, int32_t n_new, const double *eta, const int64_t *seen_offsets,
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
  const size_t nr = static_cast<size_t>(n_new) * rank;
  for (int s = 0; s < S; ++s) {
    if (ys > 0)
      HIP_CHECK(hipMemcpyAsync(ny.ptr + s * nys, rc.y.ptr + s * ys, sizeof(double) * ys, hipMemcpyDeviceToDevice, st));
    const double *m = K <= L ? rc.wk.ptr + s * kl : nullptr;
    LAUNCH(rec_fold_kernel, static_cast<unsigned>((nr + kBlock - 1) / kBlock), kBlock, 0, st,
           plain_tab(de.ptr + s * el, L), L, m, 1, L, ny.ptr + s * nys + ys, n_new, rank);
  }
  HIP_CHECK(hipGetLastError());
  // the seen pairs: user u also leaves out the new items whose list names it.  A user's list stays ascending and
  // distinct: its training items (< I) first, then its new items (>= I), sorted and de-duplicated.
  const int64_t n_seen = seen_offsets ? seen_offsets[n_new] : 0;  // (checked: below 2^31)
  if (n_seen > 0) {
    std::vector<int32_t> old_off = rc.excl ? rc.seen_off_h : std::vector<int32_t>(static_cast<size_t>(U) + 1, 0);
    std::vector<int32_t> old(static_cast<size_t>(old_off[U]));
    if (!old.empty())
      HIP_CHECK(hipMemcpyAsync(old.data(), rc.seen.ptr, sizeof(int32_t) * old.size(), hipMemcpyDeviceToHost, st));
    // the new pairs (user seen_users[e], item I + j for e in item j's range) grouped by user
    std::vector<int32_t> pit(static_cast<size_t>(n_seen)), nit(static_cast<size_t>(n_seen));
    for (int32_t j = 0; j < n_new; ++j) std::fill(pit.begin() + seen_offsets[j], pit.begin() + seen_offsets[j + 1], I + j);
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

// The grid of a kernel that writes a batch buffer in tiles: `cols` columns x `nb` rows, `tile` of each to a workgroup
dim3 tile_grid(int cols, int nb, int tile = kRecTile) {
  return dim3(static_cast<unsigned>((cols + tile - 1) / tile), static_cast<unsigned>((nb + tile - 1) / tile));
}

// -inf over the columns of sc [nb][ld] that `seen` (indexed by the rows' ids, device) leaves out; no lists: nothing
void exclude_seen(hipStream_t st, const int32_t *ids, int nb, SeenLists seen, double *sc, size_t ld) {
  if (seen.off) LAUNCH(rec_exclude_kernel, nb, kBlock, 0, st, ids, seen.off, seen.items, sc, ld);
}

// sc [nb][n_cols]: the scores of the rows ids[0 .. nb) (device) of table a (`slots` tables as doubles apart, [row][rank])
// against the rows 0 .. n_cols - 1 of table b; seen (indexed by those ids): the columns set to -inf.  fma is commutative
// in its factors, so the sides exchanged give (u, i) the same score bit for bit.
void score_tiles(mmsbm_hip_ctx *c, const double *a, size_t as, const double *b, size_t bs, int n_cols, const int32_t *ids,
                 int nb, SeenLists seen, double *sc) {
  if (n_cols == 0) return;
  LAUNCH(rec_score_kernel, tile_grid(n_cols, nb), kBlock, 0, c->stream, a, as, b, bs, ids, nb, n_cols, c->rc->rank,
         c->rc->slots, sc, static_cast<size_t>(n_cols));
  exclude_seen(c->stream, ids, nb, seen, sc, static_cast<size_t>(n_cols));
}

// ... of one batch of users ub (rows of x) against the session's catalogue.  Shared by the selection and the positions.
void rec_score_batch(mmsbm_hip_ctx *c, const double *x, size_t xs, const int32_t *ub, int nb, SeenLists seen, double *sc) {
  const RecSession &rc = *c->rc;
  score_tiles(c, x, xs, rc.y.ptr, static_cast<size_t>(rc.items) * rc.rank, rc.items, ub, nb, seen, sc);
}

// The query's own excluded items (catalogue.hpp) of the batch that begins at request row b0: own's lists are by
// request row; col_of (device): every item's column of sc, or null where the columns are the items
void own_exclude_batch(hipStream_t st, const DevCsr &own, int64_t b0, int nb, const int32_t *col_of, double *sc, size_t ld) {
  LAUNCH(cat_exclude_kernel, nb, kBlock, 0, st, nullptr, static_cast<int>(b0), own.off.ptr, own.val.ptr, col_of, sc, ld);
}

// Every row of a top-N answer as "no candidate": counts 0, ids -1, values -inf
void top_n_blank(int64_t n_rows, int n, int32_t *items, double *scores, int32_t *counts) {
  for (int64_t b = 0; b < n_rows; ++b) {
    if (counts) counts[b] = 0;
    for (int k = 0; k < n; ++k) {
      items[static_cast<size_t>(b) * n + k] = -1;
      if (scores) scores[static_cast<size_t>(b) * n + k] = -INFINITY;
    }
  }
}

// What top_n_device leaves on the device: row b's os / oi [b * n + k], k < on[b] (the entries behind are not written)
struct TopNDev {
  const double *os;
  int32_t *oi;        // (a following stage may map them in place: div_ids_kernel)
  const int32_t *on;
};

// The stages a query may add to its batches and does not: after the exclusions (rec_within_device), after the selection
// (top_n_device)
struct NoFillStage {
  template <class Prep>
  void operator()(const Prep &, const int32_t *, int, double *) const {}
};
struct NoBatchStage {
  void operator()(const TopNDev &, int, int64_t) const {}
};

// The selection of a query's batches (serve_plan.hpp: SelectPlan): the items split across waves until about 32 selecting
// waves per CU are in flight (the selection waits on its loads)
SelectPlan select_plan(const mmsbm_hip_ctx *c, int cols, int64_t rows, int n) {
  return SelectPlan(cols, rows, n, kRecMinPerPart, 32LL * c->n_cus);
}

// The selection stage: the scratch cs / ci / cn of the parts' lists -- sized for one plan, or for two that run in turn
// over one scratch (recommend_allocate's two passes) -- and the launches of one batch
struct SelectStage {
  DevBuf<double> cs;
  DevBuf<int32_t> ci, cn;
  static size_t bytes(const SelectPlan &a, const SelectPlan &b = SelectPlan{}) {
    return std::max(a.entries, b.entries) * 12 + std::max(a.lists, b.lists) * 4;
  }
  explicit SelectStage(const SelectPlan &a, const SelectPlan &b = SelectPlan{}) {
    const size_t entries = std::max(a.entries, b.entries);
    if (entries == 0) return;  // (one part: it selects straight into the result)
    cs.alloc(entries);
    ci.alloc(entries);
    cn.alloc(std::max(a.lists, b.lists));
  }
  // the n best of every row of sc [nb][p.cols] to os / oi [row * n + k], k < on[row]; the lists of the parts, where the
  // columns are split, are then merged
  void run(hipStream_t st, const SelectPlan &p, const double *sc, int nb, int n, double *os, int32_t *oi, int32_t *on) const {
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
};

// The batches of a request of n rows, bu at a time: body(b0, nb) for each in turn (they follow each other on the stream:
// no host wait in between)
template <class Body>
void for_batches(int64_t n, int64_t bu, Body &&body) {
  for (int64_t b0 = 0; b0 < n; b0 += bu) body(b0, static_cast<int>(std::min(bu, n - b0)));
}

// The frame of a batched query over a buffer of `cols` columns: the request's ids on the device, the buffer sc [bu][cols]
// of one batch (rec_batch_users), and the event pair around the query's kernels
struct BatchFrame {
  const int cols;
  const int64_t n_rows, bu;
  DevBuf<int32_t> ids;
  DevBuf<double> sc;
  EventPair ev;
  BatchFrame(int cols_, int64_t n_rows_) : cols(cols_), n_rows(n_rows_), bu(rec_batch_users(cols_, n_rows_)) {}
  size_t bytes() const { return static_cast<size_t>(bu) * cols * sizeof(double) + static_cast<size_t>(n_rows) * 4; }
  // the ids (host) uploaded and the buffer allocated, then `body(ub, nb, b0, sc)` for every batch -- request rows
  // b0 .. b0 + nb, whose device ids are ub -- between the event pair's two records (recorded; not waited for)
  template <class Body>
  void run(hipStream_t st, const int32_t *host_ids, Body &&body) {
    ids.alloc(static_cast<size_t>(n_rows));
    sc.alloc(static_cast<size_t>(bu) * cols);
    HIP_CHECK(hipMemcpyAsync(ids.ptr, host_ids, sizeof(int32_t) * n_rows, hipMemcpyHostToDevice, st));
    ev.start(st);
    for_batches(n_rows, bu, [&](int64_t b0, int nb) {
      body(ids.ptr + b0, nb, b0, sc.ptr);
      HIP_CHECK(hipGetLastError());
    });
    ev.stop(st);
  }
};

// The batches of a top-N query over a buffer of `I` columns: rows ids[0 .. n_rows) (host ids); `fill(ub, nb, b0, sc)`
// enqueues the kernels that write the values sc [nb][I] of the batch of request rows b0 .. b0 + nb, whose device ids
// are ub (-inf: no candidate), then the N best of every row are selected (and merged when the columns are split across
// waves).  `what` names the query in MMSBM_E_TOOLARGE.  Every row's result stays on the device: `then(dev, ev)` is
// called once the last batch is enqueued, with the result and the event pair around the query's kernels (recorded; not
// waited for; options "recommend_ms", "similar_ms", "diverse_ms", ...) -- it copies the result out (top_n_copy_out) or
// enqueues a stage that reads it there (diverse.hpp); `extra` bytes of device memory are what it will allocate.
// n_users > 0.  `each(batch, nb, b0)` (default: nothing) is called once a batch's selection is enqueued, with that
// batch's part of the result: a stage that needs what `fill` left of the batch before the next batch overwrites it
// (explore.hpp).
template <class Fill, class Then, class Each = NoBatchStage>
void top_n_device(mmsbm_hip_ctx *c, int I, int64_t n_users, const int32_t *users, int n, const char *what, size_t extra,
                  Fill &&fill, Then &&then, Each &&each = Each{}) {
  hipStream_t st = c->stream;
  BatchFrame fr(I, n_users);
  const SelectPlan sp = select_plan(c, I, fr.bu, n);
  const size_t outs = static_cast<size_t>(n_users) * n;
  require_free_mem(fr.bytes() + sp.bytes() + outs * 12 + static_cast<size_t>(n_users) * 4 + extra, what);
  const SelectStage sel(sp);
  DevBuf<int32_t> oi, on;
  DevBuf<double> os;
  os.alloc(outs); oi.alloc(outs); on.alloc(n_users);  // every user's result stays on the device until the end
  fr.run(st, users, [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
    double *obs = os.ptr + b0 * n;
    int32_t *obi = oi.ptr + b0 * n, *obn = on.ptr + b0;
    fill(ub, nb, b0, sc);
    sel.run(st, sp, sc, nb, n, obs, obi, obn);
    each(TopNDev{obs, obi, obn}, nb, b0);
  });
  then(TopNDev{os.ptr, oi.ptr, on.ptr}, fr.ev);
}

// A column of a query's buffer as an item id: the candidate list's entry, or (null: the columns are the items) itself
inline int32_t item_of(const int32_t *cand, int32_t col) { return cand ? cand[col] : col; }

// The result of top_n_device to the host (rows blanked by top_n_blank), and the device time of its kernels to `timed`.
// cand (host; null: none): the ids are columns of that list and leave as its items.  dev_second / second (null: none): a
// second value per place, [row * n + k] on the device as dev.os, to the host as the scores (explore.hpp's propensities).
void top_n_copy_out(mmsbm_hip_ctx *c, const TopNDev &dev, EventPair &ev, int64_t n_users, int n, TimedCall timed,
                    int32_t *items, double *scores, int32_t *counts, const int32_t *cand = nullptr,
                    const double *dev_second = nullptr, double *second = nullptr) {
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
    if (counts) counts[b] = cnt;
    for (int k = 0; k < cnt; ++k) {
      items[o + k] = item_of(cand, hi[o + k]);
      if (scores) scores[o + k] = hs[o + k];
      if (dev_second && second) second[o + k] = h2[o + k];
    }
  }
}

// top_n_device with the result copied to the host; `timed`: the timer that takes the device time of the query's kernels
template <class Fill>
void top_n_run(mmsbm_hip_ctx *c, int I, int64_t n_users, const int32_t *users, int n, const char *what, Fill &&fill,
               TimedCall timed, int32_t *items, double *scores, int32_t *counts) {
  top_n_blank(n_users, n, items, scores, counts);
  if (n_users == 0) return;
  top_n_device(c, I, n_users, users, n, what, 0, fill, [&](const TopNDev &dev, EventPair &ev) {
    top_n_copy_out(c, dev, ev, n_users, n, timed, items, scores, counts);
  });
}

// A recommend query: users users[0 .. n_users) (host ids, rows of x: `slots` tables of xs doubles, [row][rank]),
// scored against the session's items; seen (indexed by those ids): the items left out.
void rec_run(mmsbm_hip_ctx *c, const double *x, size_t xs, int64_t n_users, const int32_t *users, SeenLists seen, int n,
             int32_t *items, double *scores, int32_t *counts) {
  top_n_run(c, c->rc->items, n_users, users, n, "recommend: a batch of users",
            [&](const int32_t *ub, int nb, int64_t, double *sc) { rec_score_batch(c, x, xs, ub, nb, seen, sc); },
            T_RECOMMEND, items, scores, counts);
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

// The compact item table of a candidate subset (catalogue.hpp): the candidates on the device, every catalogue item's
// column and the candidates' rows of the session's item table, and the device time of the two kernels that make them
struct CatTable {
  DevBuf<int32_t> cand, col;  // [C]; [items of the catalogue]
  DevBuf<double> y;           // [slot][C][rank]
  float ms = 0.f;
  // the device memory of the table of cand[0 .. C) (null: no table)
  static size_t bytes(const RecSession &rc, const int32_t *cand, int C) {
    return cand ? static_cast<size_t>(rc.slots) * C * rc.rank * sizeof(double) + (static_cast<size_t>(C) + rc.items) * 4 : 0;
  }
};

// cand[0 .. C) (host; ascending, distinct ids of the session's catalogue) -> t (the memory was found free by the caller)
void cat_table(mmsbm_hip_ctx *c, const int32_t *cand, int C, CatTable &t) {
  const RecSession &rc = *c->rc;
  const int NI = rc.items, rank = rc.rank, S = rc.slots;
  const size_t ycs = static_cast<size_t>(C) * rank;
  hipStream_t st = c->stream;
  t.cand.alloc(static_cast<size_t>(C));
  t.col.alloc(static_cast<size_t>(NI));
  t.y.alloc(S * ycs);
  HIP_CHECK(hipMemcpyAsync(t.cand.ptr, cand, sizeof(int32_t) * C, hipMemcpyHostToDevice, st));
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

// What a query within the candidates holds on the device beside its batches: the query's own excluded items by request
// row and the candidates' compact table (cat_table), and from them the item table y (slots ys doubles apart) of C rows
// that the batches' tiles read
struct WithinPrep {
  DevCsr own;
  CatTable ct;
  bool has_cand = false, has_own = false;
  const double *y = nullptr;
  size_t ys = 0;
  int C = 0;
  const int32_t *dcand() const { return has_cand ? ct.cand.ptr : nullptr; }
};

// cand / n_cand / xoff / xit as rec_within_device's: the memory is checked, the lists uploaded, the compact table made
void within_prepare(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *cand, int n_cand, const int64_t *xoff,
                    const int32_t *xit, WithinPrep &w) {
  const RecSession &rc = *c->rc;
  const int NI = rc.items, rank = rc.rank;
  w.C = cand ? n_cand : NI;
  w.has_cand = cand != nullptr;
  w.has_own = xoff != nullptr;
  const size_t ycs = static_cast<size_t>(w.C) * rank;
  if (cand || xoff)
    require_free_mem(CatTable::bytes(rc, cand, w.C) + (static_cast<size_t>(n_users) + 1 + DevCsr::entries(xoff, n_users)) * 4,
                     "recommend: the candidates' rows and the query's excluded items");
  if (xoff) w.own.upload(xoff, xit, n_users, c->stream);
  if (cand) cat_table(c, cand, w.C, w.ct);
  w.y = cand ? w.ct.y.ptr : rc.y.ptr;
  w.ys = cand ? ycs : static_cast<size_t>(NI) * rank;
}

// The values sc [nb][C] of the batch of request rows b0 .. b0 + nb (device ids ub): `tiles`, then -inf over what `seen`
// leaves out for the rows' ids and over the query's own excluded items.  The one copy of these launches: the `fill` of
// rec_within_device and the batches of rec_shelves_run and recommend_list_propensity call it.
template <class Tiles>
void within_fill(mmsbm_hip_ctx *c, const WithinPrep &w, Tiles &&tiles, SeenLists seen, const int32_t *ub, int nb,
                 int64_t b0, double *sc) {
  hipStream_t st = c->stream;
  const int C = w.C;
  tiles(w.y, w.ys, C, ub, nb, sc);
  if (!w.has_cand)
    exclude_seen(st, ub, nb, seen, sc, static_cast<size_t>(C));
  else if (seen.off)
    LAUNCH(cat_exclude_kernel, nb, kBlock, 0, st, ub, 0, seen.off, seen.items, w.ct.col.ptr, sc, static_cast<size_t>(C));
  if (w.has_own) own_exclude_batch(st, w.own, b0, nb, w.ct.col.ptr, sc, static_cast<size_t>(C));
}

// The device side of a recommend query within the candidates cand[0 .. n_cand) (host; ascending, distinct ids of the
// session's catalogue; null: the whole catalogue), and with the query's own excluded items: row b of the request also
// leaves out xit[xoff[b] .. xoff[b + 1]) (host, any order, repeats allowed; null: none).  catalogue.hpp.
// `tiles(y, ys, C, ub, nb, sc)` enqueues the kernel that writes the values sc [nb][C] of the batch's rows ub (device ids)
// against the C rows of the item table y (slots ys doubles apart: the catalogue's, or the candidates' compact table) --
// the score tiles of recommend_query (rec_tiles), the aggregate over the restarts (ensemble.hpp); seen (indexed by user
// id): the items left out after it.  The result stays on the device (top_n_device): `then(dev, ev, dcand, prep_ms)` gets
// it -- as COLUMNS of the candidate list when there is one --, the candidate list on the device (or null) and the device
// time of the compact table and the columns.  n_users > 0 and at least one column.  quota: the capped categories
// (uploaded; in the buffer's columns), applied after the exclusions; null: none.  `after(w, ub, nb, sc)` (default:
// nothing) enqueues a stage of the query's own over the batch buffer behind them, before the selection; `each`:
// top_n_device's (explore.hpp uses both).
template <class Tiles, class Then, class After = NoFillStage, class Each = NoBatchStage>
void rec_within_device(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, SeenLists seen, const int32_t *cand,
                       int n_cand, const int64_t *xoff, const int32_t *xit, int n, size_t extra, Tiles &&tiles,
                       Then &&then, const QuotaMask *quota = nullptr, After &&after = After{}, Each &&each = Each{}) {
  WithinPrep w;
  within_prepare(c, n_users, cand, n_cand, xoff, xit, w);
  top_n_device(c, w.C, n_users, users, n,
               cand || xoff || quota ? "recommend: a batch of users within the candidates" : "recommend: a batch of users", extra,
               [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
                 within_fill(c, w, tiles, seen, ub, nb, b0, sc);
                 if (quota) quota->apply(c->stream, nb, sc, static_cast<size_t>(w.C));
                 after(w, ub, nb, sc);
               },
               [&](const TopNDev &dev, EventPair &ev) { then(dev, ev, w.dcand(), w.ct.ms); }, each);
}

// rec_within_device's `tiles` of recommend_query: the scores of the rows of x (`slots` tables xs doubles apart)
auto rec_tiles(mmsbm_hip_ctx *c, const double *x, size_t xs) {
  return [=](const double *y, size_t ys, int C, const int32_t *ub, int nb, double *sc) {
    score_tiles(c, x, xs, y, ys, C, ub, nb, SeenLists{}, sc);
  };
}

// rec_within_device with the result copied to the host (top_n_blank done by the caller), the columns as item ids; the device time of the query's kernels goes to `timed`.  No column or no row: every row stays empty.
template <class Tiles>
void rec_within_run(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, SeenLists seen, const int32_t *cand,
                    int n_cand, const int64_t *xoff, const int32_t *xit, int n, Tiles &&tiles, TimedCall timed,
                    int32_t *items, double *scores, int32_t *counts, const QuotaMask *quota = nullptr) {
  c->last_ms[timed] = 0.f;
  if ((cand ? n_cand : c->rc->items) == 0 || n_users == 0) return;
  rec_within_device(c, n_users, users, seen, cand, n_cand, xoff, xit, n, 0, tiles,
                    [&](const TopNDev &dev, EventPair &ev, const int32_t *, float prep_ms) {
                      top_n_copy_out(c, dev, ev, n_users, n, timed, items, scores, counts, cand);
                      c->last_ms[timed] += prep_ms;
                    },
                    quota);
}

// The capped categories of a query (quota.hpp): cat_items[cat_off[g] .. cat_off[g + 1]) (host; catalogue ids, each
// category strictly ascending, the categories disjoint) with cap caps[g], planned against the candidates (serve_plan.hpp)
struct QuotaCats {
  int64_t n_cats = 0;
  const int64_t *off = nullptr;
  const int32_t *items = nullptr, *caps = nullptr;
};

// rec_run within the candidates, without the query's own excluded items and with the capped categories `cats` (null:
// none).  Without candidates, own lists and a category that can change the answer: rec_run.
void rec_run_within(mmsbm_hip_ctx *c, const double *x, size_t xs, int64_t n_users, const int32_t *users, SeenLists seen,
                    const int32_t *cand, int n_cand, const int64_t *xoff, const int32_t *xit, int n, int32_t *items,
                    double *scores, int32_t *counts, const QuotaCats *cats = nullptr) {
  QuotaMask mask;
  if (cats && cats->n_cats > 0 && n_users > 0 && (cand ? n_cand : c->rc->items) > 0) {
    QuotaPlan plan = plan_quota(cand, n_cand, cats->n_cats, cats->off, cats->items, cats->caps, n);
    if (plan.kept() > 0) {
      require_free_mem(plan.bytes(), "recommend: the capped categories");
      mask.upload(std::move(plan), c->stream);
    }
  }
  const bool masked = mask.plan.kept() > 0;
  if (!cand && !xoff && !masked) {
    rec_run(c, x, xs, n_users, users, seen, n, items, scores, counts);
    return;
  }
  top_n_blank(n_users, n, items, scores, counts);
  rec_within_run(c, n_users, users, seen, cand, n_cand, xoff, xit, n, rec_tiles(c, x, xs), T_RECOMMEND, items, scores,
                 counts, masked ? &mask : nullptr);
}

// The caller's theta rows [S][n_users][K] folded exactly as recommend_add folds a slot's own theta (x = theta, or
// theta W when K > L), then `run(x, xs, ids, seen)` over the rows 0 .. n_users - 1 with the caller's seen lists
template <class Run>
void rec_theta_fold(mmsbm_hip_ctx *c, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                    const int32_t *seen_items, Run &&run) {
  const int K = c->ext_k, L = c->ext_l, rank = c->rc->rank, S = c->rc->slots;
  const size_t tk = static_cast<size_t>(n_users) * K, xs = static_cast<size_t>(n_users) * rank;
  require_free_mem(S * (tk + xs) * sizeof(double) +
                       (static_cast<size_t>(n_users) + 1 + DevCsr::entries(seen_offsets, n_users)) * 4,
                   "recommend: the caller's theta rows");
  hipStream_t st = c->stream;
  CallerRows rows(c, S, n_users, theta, seen_offsets, seen_items);
  DevBuf<double> x;
  x.alloc(S * xs);
  const size_t kl = static_cast<size_t>(K) * L;
  for (int s = 0; s < S && xs > 0; ++s) {
    const RowTab src = plain_tab(rows.th.ptr + s * tk, K);
    const double *m = K <= L ? nullptr : c->rc->wk.ptr + s * kl;
    LAUNCH(rec_fold_kernel, static_cast<unsigned>((xs + kBlock - 1) / kBlock), kBlock, 0, st, src, K, m, L, 1,
           x.ptr + s * xs, static_cast<int>(n_users), rank);
  }
  HIP_CHECK(hipGetLastError());
  run(x.ptr, xs, rows.ids.data(), rows.seen.lists());
}

// ... then rec_run_within
void rec_theta_run(mmsbm_hip_ctx *c, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                   const int32_t *seen_items, const int32_t *cand, int n_cand, int n, int32_t *items, double *scores,
                   int32_t *counts, const QuotaCats *cats = nullptr) {
  rec_theta_fold(c, n_users, theta, seen_offsets, seen_items,
                 [&](const double *x, size_t xs, const int32_t *ids, SeenLists seen) {
                   rec_run_within(c, x, xs, n_users, ids, seen, cand, n_cand, nullptr, nullptr, n, items, scores, counts,
                                  cats);
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
bool shelves_begin(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *cand, int n_cand, int64_t n_cats,
                   const int64_t *cat_offsets, const int32_t *cat_items, const ShelfAsk &ask, const ShelfOut &out,
                   ShelfPlan &plan) {
  shelves_blank(n_users, ask, out);
  c->last_ms[T_RECOMMEND] = 0.f;
  if (n_users == 0 || n_cats == 0 || (cand ? n_cand : c->rc->items) == 0) return false;
  plan = plan_shelves(cand, n_cand, n_cats, cat_offsets, cat_items);
  return plan.kept() > 0;
}

// A shelves query: rows users[0 .. n_users) (host ids, rows of x) within cand / xoff / xit as rec_within_device's, the
// categories cats.  The batches are a BatchFrame over the C item columns, the selection a stage over the G value columns:
// per batch the score tiles and the exclusions (within_fill: the launches of recommend_query_within), the value kernels,
// the selection over the value buffer and the chosen shelves' items, all before the next batch overwrites the scores;
// every row's result stays on the device until the end.  `plan`: shelves_begin's, with at least one category.
void rec_shelves_run(mmsbm_hip_ctx *c, const double *x, size_t xs, int64_t n_users, const int32_t *users, SeenLists seen,
                     const int32_t *cand, int n_cand, const int64_t *xoff, const int32_t *xit, ShelfPlan &&plan,
                     const ShelfAsk &ask, const ShelfOut &out) {
  ShelfCats sh;
  require_free_mem(plan.bytes(), "recommend_shelves: the categories");
  sh.upload(std::move(plan), c->stream);
  hipStream_t st = c->stream;
  const int G = sh.plan.kept(), ns = ask.n_shelves, ps = ask.per_shelf;
  WithinPrep w;
  within_prepare(c, n_users, cand, n_cand, xoff, xit, w);
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
  fr.run(st, users, [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
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
        out.items[o * ps + e] = item_of(cand, hic[o * ps + e]);
        out.scores[o * ps + e] = his[o * ps + e];
      }
    }
  }
}

}  // namespace

void recommend_query(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int n, int32_t *items, double *scores,
                     int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  rec_run(c, rc.x.ptr, rc.x_stride(), n_users, users, rc.seen_lists(), n, items, scores, counts);
}

void recommend_query_theta(mmsbm_hip_ctx *c, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                           const int32_t *seen_items, int n, int32_t *items, double *scores, int32_t *counts) {
  use_device(c);
  rec_theta_run(c, n_users, theta, seen_offsets, seen_items, nullptr, 0, n, items, scores, counts);
}

void recommend_query_within(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int32_t *cand, int n_cand,
                            const int64_t *excl_offsets, const int32_t *excl_items, int n, int32_t *items,
                            double *scores, int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  rec_run_within(c, rc.x.ptr, rc.x_stride(), n_users, users, rc.seen_lists(), cand, n_cand, excl_offsets, excl_items, n,
                 items, scores, counts);
}

void recommend_query_theta_within(mmsbm_hip_ctx *c, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                                  const int32_t *seen_items, const int32_t *cand, int n_cand, int n, int32_t *items,
                                  double *scores, int32_t *counts) {
  use_device(c);
  rec_theta_run(c, n_users, theta, seen_offsets, seen_items, cand, n_cand, n, items, scores, counts);
}

void recommend_query_quota(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int32_t *cand, int n_cand,
                           const int64_t *excl_offsets, const int32_t *excl_items, int64_t n_cats,
                           const int64_t *cat_offsets, const int32_t *cat_items, const int32_t *cat_caps, int n,
                           int32_t *items, double *scores, int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const QuotaCats cats{n_cats, cat_offsets, cat_items, cat_caps};
  rec_run_within(c, rc.x.ptr, rc.x_stride(), n_users, users, rc.seen_lists(), cand, n_cand, excl_offsets, excl_items, n,
                 items, scores, counts, &cats);
}

void recommend_query_theta_quota(mmsbm_hip_ctx *c, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                                 const int32_t *seen_items, const int32_t *cand, int n_cand, int64_t n_cats,
                                 const int64_t *cat_offsets, const int32_t *cat_items, const int32_t *cat_caps, int n,
                                 int32_t *items, double *scores, int32_t *counts) {
  use_device(c);
  const QuotaCats cats{n_cats, cat_offsets, cat_items, cat_caps};
  rec_theta_run(c, n_users, theta, seen_offsets, seen_items, cand, n_cand, n, items, scores, counts, &cats);
}

void recommend_query_shelves(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int32_t *cand, int n_cand,
                             const int64_t *excl_offsets, const int32_t *excl_items, int64_t n_cats,
                             const int64_t *cat_offsets, const int32_t *cat_items, const ShelfAsk &ask,
                             const ShelfOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  ShelfPlan plan;
  if (!shelves_begin(c, n_users, cand, n_cand, n_cats, cat_offsets, cat_items, ask, out, plan)) return;
  rec_shelves_run(c, rc.x.ptr, rc.x_stride(), n_users, users, rc.seen_lists(), cand, n_cand, excl_offsets, excl_items,
                  std::move(plan), ask, out);
}

void recommend_query_theta_shelves(mmsbm_hip_ctx *c, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                                   const int32_t *seen_items, const int32_t *cand, int n_cand, int64_t n_cats,
                                   const int64_t *cat_offsets, const int32_t *cat_items, const ShelfAsk &ask,
                                   const ShelfOut &out) {
  use_device(c);
  ShelfPlan plan;
  if (!shelves_begin(c, n_users, cand, n_cand, n_cats, cat_offsets, cat_items, ask, out, plan)) return;
  rec_theta_fold(c, n_users, theta, seen_offsets, seen_items,
                 [&](const double *x, size_t xs, const int32_t *ids, SeenLists seen) {
                   rec_shelves_run(c, x, xs, n_users, ids, seen, cand, n_cand, nullptr, nullptr, std::move(plan), ask,
                                   out);
                 });
}

// ---- randomised top-N with propensities (explore.hpp) ---------------------------------------------------------------------
namespace {

// The PCG64 stream of a call: its four words and the jump table on the device (the host copy is held: the upload is
// asynchronous)
struct ExploreStream {
  uint64_t st[4];
  std::vector<uint64_t> tab_h;
  DevBuf<uint64_t> tab;
  ExploreStream(const uint64_t state[4], hipStream_t stream) : tab_h(64 * 4) {
    std::copy(state, state + 4, st);
    explore_jump_table(st, tab_h.data());
    tab.upload(tab_h, stream);
  }
};

}  // namespace

// recommend_query_within's batches with two stages of its own around the unchanged selection: behind the exclusions the
// row maxima and the perturbation (the scores move to `raw`, the keys take their place), behind the selection the
// propensities from `raw` -- per batch, before the next one overwrites it (top_n_device's `each`).
void recommend_query_explore(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int32_t *cand, int n_cand,
                             const int64_t *xoff, const int32_t *xit, int n, double temperature,
                             const uint64_t state[4], int32_t *items, double *scores, double *propensity,
                             int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  top_n_blank(n_users, n, items, scores, counts);
  const size_t outs = static_cast<size_t>(n_users) * n;
  for (size_t e = 0; propensity && e < outs; ++e) propensity[e] = 0.0;
  c->last_ms[T_RECOMMEND] = 0.f;
  const int C = cand ? n_cand : rc.items;
  if (C == 0 || n_users == 0) return;  // (no column to score: every row is empty)
  hipStream_t st = c->stream;
  const int64_t bu = rec_batch_users(C, n_users);  // (the batches top_n_device will form)
  const size_t ld = static_cast<size_t>(C);
  require_free_mem(static_cast<size_t>(bu) * ld * sizeof(double) + static_cast<size_t>(bu) * 24 + outs * 16 + 2048,
                   "recommend_explore: the unperturbed scores of a batch of users");
  ExploreStream rng(state, st);
  DevBuf<double> raw, mx, ps, pp;
  DevBuf<uint64_t> base;
  raw.alloc(static_cast<size_t>(bu) * ld);
  mx.alloc(static_cast<size_t>(bu));
  base.alloc(static_cast<size_t>(bu) * 2);
  ps.alloc(outs);
  pp.alloc(outs);
  const unsigned spans = static_cast<unsigned>((C + kExpSpan - 1) / kExpSpan);
  rec_within_device(
      c, n_users, users, rc.seen_lists(), cand, n_cand, xoff, xit, n, 0, rec_tiles(c, rc.x.ptr, rc.x_stride()),
      [&](const TopNDev &dev, EventPair &ev, const int32_t *, float prep_ms) {  // the scores are `raw`'s, not the keys
        top_n_copy_out(c, TopNDev{ps.ptr, dev.oi, dev.on}, ev, n_users, n, T_RECOMMEND, items, scores, counts, cand, pp.ptr,
                       propensity);
        c->last_ms[T_RECOMMEND] += prep_ms;
      },
      nullptr,
      [&](const WithinPrep &w, const int32_t *ub, int nb, double *sc) {
        LAUNCH(explore_norm_kernel, nb, kBlock, 0, st, sc, ld, C, ub, rng.tab.ptr, rng.st[0], rng.st[1], mx.ptr, base.ptr);
        LAUNCH(explore_perturb_kernel, dim3(spans, static_cast<unsigned>(nb)), kBlock, 0, st, sc, raw.ptr, ld, C, w.dcand(),
               rng.tab.ptr, base.ptr, rng.st[2], rng.st[3], temperature);
      },
      [&](const TopNDev &batch, int nb, int64_t b0) {
        LAUNCH(explore_finish_kernel, nb, kRecWave, 0, st, raw.ptr, ld, C, mx.ptr, temperature, batch.oi, batch.on, n,
               ps.ptr + b0 * n, pp.ptr + b0 * n);
      });
}

// The propensities of caller-given lists: recommend_query_within's score tiles and exclusions per batch (within_fill),
// the row maxima, then explore_list_kernel over the batch buffer itself -- no noise, no selection.
void recommend_list_propensity(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int32_t *cand, int n_cand,
                               const int64_t *xoff, const int32_t *xit, double temperature, const int64_t *list_offsets,
                               const int32_t *list_items, double *scores, double *propensity) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const size_t total = static_cast<size_t>(DevCsr::entries(list_offsets, n_users));  // (checked: below 2^31)
  for (size_t e = 0; e < total; ++e) {
    if (scores) scores[e] = -INFINITY;
    propensity[e] = 0.0;
  }
  c->last_ms[T_RECOMMEND] = 0.f;
  const int C = cand ? n_cand : rc.items;
  if (C == 0 || total == 0) return;  // (no candidate anywhere, or nothing asked)
  hipStream_t st = c->stream;
  WithinPrep w;
  within_prepare(c, n_users, cand, n_cand, xoff, xit, w);
  BatchFrame fr(C, n_users);
  const size_t ld = static_cast<size_t>(C);
  require_free_mem(fr.bytes() + static_cast<size_t>(fr.bu) * 8 + (static_cast<size_t>(n_users) + 1) * 4 + total * 20,
                   "recommend_list_propensity: a batch of users and the lists");
  DevBuf<double> mx, os, op;
  DevCsr lists;
  mx.alloc(static_cast<size_t>(fr.bu));
  os.alloc(total);
  op.alloc(total);
  lists.upload(list_offsets, list_items, n_users, st);
  const auto tiles = rec_tiles(c, rc.x.ptr, rc.x_stride());
  const int32_t *col_of = w.has_cand ? w.ct.col.ptr : nullptr;
  fr.run(st, users, [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
    within_fill(c, w, tiles, rc.seen_lists(), ub, nb, b0, sc);
    LAUNCH(explore_norm_kernel, nb, kBlock, 0, st, sc, ld, C, ub, nullptr, uint64_t(0), uint64_t(0), mx.ptr, nullptr);
    LAUNCH(explore_list_kernel, nb, kRecWave, 0, st, sc, ld, C, mx.ptr, temperature, lists.off.ptr + b0, lists.val.ptr, col_of,
           os.ptr, op.ptr);
  });
  if (scores) HIP_CHECK(hipMemcpyAsync(scores, os.ptr, sizeof(double) * total, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(propensity, op.ptr, sizeof(double) * total, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_RECOMMEND] = fr.ev.ms() + w.ct.ms;
}

void explore_noise(mmsbm_hip_ctx *c, const uint64_t state[4], int64_t n_pairs, const int32_t *users, const int32_t *items,
                   double *r, double *g) {
  use_device(c);
  if (n_pairs == 0) return;
  hipStream_t st = c->stream;
  const int64_t per = std::min<int64_t>(n_pairs, int64_t(1) << 24);  // pairs per launch (24 bytes each)
  require_free_mem(static_cast<size_t>(per) * 24 + 2048, "explore_noise: a batch of pairs");
  ExploreStream rng(state, st);
  DevBuf<int32_t> du, di;
  DevBuf<double> dr, dg;
  du.alloc(static_cast<size_t>(per));
  di.alloc(static_cast<size_t>(per));
  dr.alloc(static_cast<size_t>(per));
  dg.alloc(static_cast<size_t>(per));
  for (int64_t p0 = 0; p0 < n_pairs; p0 += per) {
    const int64_t np = std::min(per, n_pairs - p0);
    HIP_CHECK(hipMemcpyAsync(du.ptr, users + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(di.ptr, items + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    LAUNCH(explore_noise_kernel, static_cast<unsigned>((np + kBlock - 1) / kBlock), kBlock, 0, st, rng.tab.ptr, rng.st[0],
           rng.st[1], rng.st[2], rng.st[3], du.ptr, di.ptr, np, dr.ptr, dg.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(r + p0, dr.ptr, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(g + p0, dg.ptr, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }
}

void recommend_rank(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int64_t *offsets,
                    const int32_t *cand, int n, int32_t *items, double *scores, int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  top_n_blank(n_users, n, items, scores, counts);
  c->last_ms[T_RECOMMEND] = 0.f;
  if (n_users == 0) return;
  hipStream_t st = c->stream;
  const auto [cap, lds] = select_list(n);
  const size_t outs = static_cast<size_t>(n_users) * n;
  require_free_mem(outs * 12 + (2 * static_cast<size_t>(n_users) + 1 + static_cast<size_t>(offsets[n_users])) * 4 +
                       static_cast<size_t>(n_users) * 4,
                   "recommend_rank: the users' lists and results");
  DevBuf<int32_t> du, oi, on;
  DevBuf<double> os;
  DevCsr lists;  // every request row's candidates
  du.alloc(static_cast<size_t>(n_users));
  lists.upload(offsets, cand, n_users, st);
  os.alloc(outs); oi.alloc(outs); on.alloc(static_cast<size_t>(n_users));
  HIP_CHECK(hipMemcpyAsync(du.ptr, users, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  const SeenLists seen = rc.seen_lists();
  EventPair ev;  // device time of the query's kernel (option "recommend_ms")
  ev.start(st);
  LAUNCH(cat_rank_kernel, static_cast<unsigned>(n_users), kRecWave, lds, st, rc.x.ptr, rc.x_stride(), rc.y.ptr,
         static_cast<size_t>(rc.items) * rc.rank, rc.rank, rc.slots, du.ptr, lists.off.ptr, lists.val.ptr, seen.off,
         seen.items, n, cap, os.ptr, oi.ptr, on.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  top_n_copy_out(c, TopNDev{os.ptr, oi.ptr, on.ptr}, ev, n_users, n, T_RECOMMEND, items, scores, counts);
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

// The m best pairs over users[0 .. n_users) (host ids, ascending and distinct) x the session's catalogue
// (top_pairs.hpp).  The launches of a query: one fused launch and the merge levels of G lists -- whatever U and I.
void recommend_top_pairs(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int m, int32_t *out_users,
                         int32_t *out_items, double *out_scores, int32_t *count) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int I = rc.items, rank = rc.rank;
  for (int k = 0; k < m; ++k) {
    out_users[k] = -1;
    out_items[k] = -1;
    out_scores[k] = -INFINITY;
  }
  *count = 0;
  c->last_ms[T_TOP_PAIRS] = 0.f;
  if (n_users == 0 || I == 0) return;
  hipStream_t st = c->stream;
  const int64_t tiles = ((n_users + kRecTile - 1) / kRecTile) * ((static_cast<int64_t>(I) + kRecTile - 1) / kRecTile);
  // G: two workgroups per CU (what the LDS of gtop_fused_kernel allows), one resident set that walks all tiles
  const int G = static_cast<int>(std::min<int64_t>(c->top_groups > 0 ? c->top_groups : 2 * c->n_cus, tiles));
  const size_t per_list = static_cast<size_t>(m) * (sizeof(double) + sizeof(uint64_t)) + sizeof(int32_t);
  const int G1 = (G + kTopFan - 1) / kTopFan;  // lists after the first merge level
  require_free_mem((static_cast<size_t>(G) + G1) * per_list + static_cast<size_t>(n_users) * 4, "top_pairs: the workgroups' lists");
  DevBuf<int32_t> du, na, nb2;
  DevBuf<double> sa, sb;
  DevBuf<uint64_t> ka, kb;
  du.alloc(n_users);
  sa.alloc(static_cast<size_t>(G) * m); ka.alloc(static_cast<size_t>(G) * m); na.alloc(G);
  sb.alloc(static_cast<size_t>(G1) * m); kb.alloc(static_cast<size_t>(G1) * m); nb2.alloc(G1);
  HIP_CHECK(hipMemcpyAsync(du.ptr, users, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  EventPair ev;  // device time of the query's kernels (option "top_pairs_ms")
  ev.start(st);
  const SeenLists seen = rc.seen_lists();
  LAUNCH(gtop_fused_kernel, G, kBlock, 0, st, rc.x.ptr, rc.x_stride(), rc.y.ptr, static_cast<size_t>(I) * rank, du.ptr,
         static_cast<int>(n_users), I, rank, rc.slots, seen.off, seen.items, m, sa.ptr, ka.ptr, na.ptr);
  // merge levels: a -> b -> a ... until one list is left (G = 1: one level, so that the merge is always part of a query)
  double *is = sa.ptr, *os = sb.ptr;
  uint64_t *ik = ka.ptr, *ok = kb.ptr;
  int32_t *in = na.ptr, *on = nb2.ptr;
  int lists = G;
  do {
    const int out_lists = (lists + kTopFan - 1) / kTopFan;
    LAUNCH(gtop_merge_kernel, out_lists, kBlock, 0, st, is, ik, in, lists, kTopFan, m, os, ok, on);
    std::swap(is, os);
    std::swap(ik, ok);
    std::swap(in, on);
    lists = out_lists;
  } while (lists > 1);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  std::vector<double> hs(static_cast<size_t>(m));
  std::vector<uint64_t> hk(static_cast<size_t>(m));
  int32_t hn = 0;
  HIP_CHECK(hipMemcpyAsync(hs.data(), is, sizeof(double) * m, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(hk.data(), ik, sizeof(uint64_t) * m, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(&hn, in, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_TOP_PAIRS] = ev.ms();
  *count = hn;
  for (int k = 0; k < hn; ++k) {
    out_users[k] = static_cast<int32_t>(hk[static_cast<size_t>(k)] >> 32);
    out_items[k] = static_cast<int32_t>(hk[static_cast<size_t>(k)] & 0xffffffffu);
    out_scores[k] = hs[static_cast<size_t>(k)];
  }
}

// ---- the m best pairs beyond a workgroup's list (pairs_bulk.hpp) ---------------------------------------------------------
// users ascending and distinct.  out_* null: phase 1 alone (mmsbm_hip_recommend_pair_bar).  counts: above, ties,
// candidates.  The host steps between the launches are pairs_bulk_plan.hpp's.
void recommend_top_pairs_bulk(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int64_t m, int32_t *out_users,
                              int32_t *out_items, double *out_scores, int64_t *count, double *bar, int64_t counts[3]) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int I = rc.items, rank = rc.rank, S = rc.slots;
  const bool fill = out_users != nullptr;
  if (fill) {
    for (int64_t k = 0; k < m; ++k) {
      out_users[k] = -1;
      out_items[k] = -1;
      out_scores[k] = -INFINITY;
    }
    *count = 0;
  }
  *bar = -INFINITY;
  counts[0] = counts[1] = counts[2] = 0;
  c->last_ms[T_TOP_PAIRS_BULK] = 0.f;
  c->pb_passes = 0;
  c->pb_collected = 0;
  int64_t cand = n_users * static_cast<int64_t>(I);
  if (rc.excl)
    for (int64_t b = 0; b < n_users; ++b) cand -= rc.seen_off_h[static_cast<size_t>(users[b]) + 1] - rc.seen_off_h[static_cast<size_t>(users[b])];
  counts[2] = cand;
  if (cand <= 0) return;
  const PbPlan plan = plan_pairs_bulk(n_users, I, cand, m, c->n_cus, c->pb_groups, c->pb_bits, c->pb_collect);
  require_free_mem(fill ? plan.bytes() : plan.bytes() - plan.out_bytes, "top_pairs_bulk: the entries, the histograms and the counts");
  hipStream_t st = c->stream;
  const int nb = static_cast<int>(n_users), G = plan.groups;
  const size_t xs = rc.x_stride(), ys = static_cast<size_t>(I) * rank;
  const SeenLists seen = rc.seen_lists();
  DevBuf<int32_t> du, tie_row, cut_item;
  DevBuf<unsigned long long> hist, n_buf;
  DevBuf<long long> grp;  // [4][G]: above, ties, admitted, bases
  DevBuf<double> d_bar;
  du.alloc(n_users);
  tie_row.alloc(n_users);
  cut_item.alloc(1);
  hist.alloc(2 * static_cast<size_t>(plan.bins));
  n_buf.alloc(1);
  grp.alloc(4 * static_cast<size_t>(G));
  d_bar.alloc(1);
  HIP_CHECK(hipMemcpyAsync(du.ptr, users, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  EventPair ev;  // device time of the whole query, the host steps between its launches included (option "pairs_bulk_ms")
  ev.start(st);
  // ---- phase 1: the m-th accumulator ----
  PbState sel = pb_begin(cand, plan.m_out);
  std::vector<unsigned long long> hh(2 * static_cast<size_t>(plan.bins));
  std::vector<int64_t> h(static_cast<size_t>(plan.bins));
  const unsigned seen_grid = static_cast<unsigned>(std::min<int64_t>((n_users + 3) / 4, 64LL * std::max(c->n_cus, 1)));
  for (int pass = 0; sel.done_bits < 64 && !pb_collect_now(sel, plan.collect); ++pass) {
    const PbDigit dg = pb_digit(plan.bits, pass);
    const int bins = 1 << dg.width;
    const PbulkDigit d{sel.prefix, sel.done_bits == 0 ? 1 : 0, sel.done_bits == 0 ? 0 : 64 - sel.done_bits, dg.shift,
                       static_cast<uint32_t>(bins - 1)};
    HIP_CHECK(hipMemsetAsync(hist.ptr, 0, sizeof(unsigned long long) * 2 * plan.bins, st));
    LAUNCH(pbulk_tile_kernel<false>, G, kBlock, sizeof(uint32_t) * bins, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank,
           S, d, hist.ptr, nullptr, nullptr, nullptr, 0ull, nullptr);
    if (seen.off)
      LAUNCH(pbulk_seen_kernel, seen_grid, kBlock, sizeof(uint32_t) * bins, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, rank,
             S, d, seen.off, seen.items, hist.ptr + plan.bins);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hh.data(), hist.ptr, sizeof(unsigned long long) * 2 * plan.bins, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < bins; ++b) {
      h[b] = static_cast<int64_t>(hh[b]) - static_cast<int64_t>(hh[static_cast<size_t>(plan.bins) + b]);
      if (h[b] < 0) throw std::runtime_error("top_pairs_bulk: more seen pairs than pairs in a bin");
    }
    if (!pb_advance(sel, dg, h.data())) throw std::runtime_error("top_pairs_bulk: the histogram holds fewer than m candidates");
    ++c->pb_passes;
  }
  uint64_t key_m = sel.prefix;
  if (sel.done_bits < 64) {  // a small bin: its candidates' keys, sorted; the key of rank k
    const size_t n = static_cast<size_t>(sel.in_bin);
    DevBuf<uint64_t> buf, sorted;
    buf.alloc(n);
    sorted.alloc(n);
    const PbulkDigit d{sel.prefix, sel.done_bits == 0 ? 1 : 0, sel.done_bits == 0 ? 0 : 64 - sel.done_bits, 0, 0u};
    HIP_CHECK(hipMemsetAsync(n_buf.ptr, 0, sizeof(unsigned long long), st));
    LAUNCH(pbulk_tile_kernel<true>, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, d, nullptr, seen.off,
           seen.items, buf.ptr, static_cast<unsigned long long>(n), n_buf.ptr);
    HIP_CHECK(hipGetLastError());
    unsigned long long got = 0;
    HIP_CHECK(hipMemcpyAsync(&got, n_buf.ptr, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (got != n) throw std::runtime_error("top_pairs_bulk: the collected bin does not hold what its histogram counted");
    pairs_bulk_sort_desc(c, buf.ptr, sorted.ptr, n);
    HIP_CHECK(hipMemcpyAsync(&key_m, sorted.ptr + (sel.k - 1), sizeof key_m, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    c->pb_collected = sel.in_bin;
  }
  const double acc_m = pb_value(key_m);
  // ---- the bar, the counts above and at it, the ties per user ----
  long long *g_above = grp.ptr, *g_tie = grp.ptr + G, *g_adm = grp.ptr + 2 * static_cast<size_t>(G), *g_base = grp.ptr + 3 * static_cast<size_t>(G);
  HIP_CHECK(hipMemsetAsync(tie_row.ptr, 0, sizeof(int32_t) * n_users, st));
  LAUNCH(pbulk_count_kernel, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, acc_m, seen.off,
         seen.items, g_above, g_tie, tie_row.ptr, d_bar.ptr);
  HIP_CHECK(hipGetLastError());
  std::vector<long long> hg(2 * static_cast<size_t>(G));
  std::vector<int32_t> ties(static_cast<size_t>(n_users));
  HIP_CHECK(hipMemcpyAsync(hg.data(), grp.ptr, sizeof(long long) * 2 * G, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(ties.data(), tie_row.ptr, sizeof(int32_t) * n_users, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(bar, d_bar.ptr, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  int64_t above = 0, at_bar = 0;
  for (int g = 0; g < G; ++g) {
    above += hg[g];
    at_bar += hg[static_cast<size_t>(G) + g];
  }
  counts[0] = above;
  counts[1] = at_bar;
  if (!(above < plan.m_out && plan.m_out <= above + at_bar))
    throw std::runtime_error("top_pairs_bulk: the bar does not hold the m-th pair");
  if (fill) {
    // ---- phase 2: the pairs above the bar and the ties the order admits ----
    const int64_t quota = plan.m_out - above;
    const PbCut cut = pb_tie_cut(ties.data(), n_users, quota);
    const int32_t none = -1;
    HIP_CHECK(hipMemcpyAsync(cut_item.ptr, &none, sizeof none, hipMemcpyHostToDevice, st));
    if (cut.part > 0)
      LAUNCH(pbulk_cut_kernel, 1, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, static_cast<int>(users[cut.row]), I, rank, S,
             acc_m, static_cast<long long>(cut.part), seen.off, seen.items, cut_item.ptr);
    std::vector<long long> adm(static_cast<size_t>(G)), base(static_cast<size_t>(G));
    if (quota == at_bar) {  // every tie is in: the count's numbers
      for (int g = 0; g < G; ++g) adm[g] = hg[g] + hg[static_cast<size_t>(G) + g];
    } else {
      LAUNCH(pbulk_emit_kernel<false>, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, acc_m, seen.off,
             seen.items, static_cast<long long>(cut.row), cut_item.ptr, g_adm, nullptr, nullptr, nullptr, 0ll);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(adm.data(), g_adm, sizeof(long long) * G, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
    }
    long long run = 0;
    for (int g = 0; g < G; ++g) {
      base[g] = run;
      run += adm[g];
    }
    if (run != plan.m_out) throw std::runtime_error("top_pairs_bulk: the admitted pairs are not min(m, candidates)");
    const size_t n = static_cast<size_t>(plan.m_out);
    DevBuf<uint64_t> ok, fk;
    DevBuf<double> os, fs;
    ok.alloc(n); os.alloc(n); fk.alloc(n); fs.alloc(n);
    HIP_CHECK(hipMemcpyAsync(g_base, base.data(), sizeof(long long) * G, hipMemcpyHostToDevice, st));
    LAUNCH(pbulk_emit_kernel<true>, G, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, du.ptr, nb, I, rank, S, acc_m, seen.off,
           seen.items, static_cast<long long>(cut.row), cut_item.ptr, g_adm, g_base, ok.ptr, os.ptr, static_cast<long long>(n));
    HIP_CHECK(hipGetLastError());
    // ---- phase 3: the order ----
    pairs_bulk_order(c, ok.ptr, os.ptr, n, fk.ptr, fs.ptr);
    std::vector<uint64_t> hk(n);
    HIP_CHECK(hipMemcpyAsync(hk.data(), fk.ptr, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(out_scores, fs.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (size_t k = 0; k < n; ++k) {
      out_users[k] = static_cast<int32_t>(hk[k] >> 32);
      out_items[k] = static_cast<int32_t>(hk[k] & 0xffffffffu);
    }
    *count = plan.m_out;
  }
  ev.stop(st);
  ev.wait();
  c->last_ms[T_TOP_PAIRS_BULK] = ev.ms();
}

// ---- item-side queries (audience.hpp) -----------------------------------------------------------------------------------
namespace {

// The item -> users lists of the session: the transpose of seen_off / seen, so each item's users are ascending and
// distinct by construction.  Built by the first item-side query, dropped by recommend_add_items.
void rec_item_lists(mmsbm_hip_ctx *c) {
  RecSession &rc = *c->rc;
  if (!rc.excl || rc.by_item_built) return;
  const int U = c->ext_users, NI = rc.items;
  hipStream_t st = c->stream;
  const size_t n = static_cast<size_t>(rc.seen_off_h[U]);
  std::vector<int32_t> seen(n);
  if (n > 0) HIP_CHECK(hipMemcpyAsync(seen.data(), rc.seen.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  std::vector<int32_t> off(static_cast<size_t>(NI) + 1, 0), user(n);
  for (size_t e = 0; e < n; ++e) ++off[static_cast<size_t>(seen[e]) + 1];
  for (int i = 0; i < NI; ++i) off[i + 1] += off[i];
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (int u = 0; u < U; ++u)  // (users ascending: so is every item's list)
    for (int32_t e = rc.seen_off_h[u]; e < rc.seen_off_h[u + 1]; ++e) user[static_cast<size_t>(at[seen[e]]++)] = u;
  require_free_mem((off.size() + n) * sizeof(int32_t), "recommend: the items' excluded users");
  DevBuf<int32_t> d_off, d_user;
  d_off.upload(off, st);
  d_user.upload(user, st);
  HIP_CHECK(hipStreamSynchronize(st));  // (host vectors are locals)
  rc.by_item_off.swap(d_off);
  rc.by_item.swap(d_user);
  rc.by_item_built = true;
}

}  // namespace

void recommend_query_items(mmsbm_hip_ctx *c, int64_t n_items, const int32_t *items, int n, int32_t *users,
                           double *scores, int32_t *counts) {
  use_device(c);
  rec_item_lists(c);
  const RecSession &rc = *c->rc;
  const SeenLists ex{rc.excl ? rc.by_item_off.ptr : nullptr, rc.by_item.ptr};  // (by item id: the users left out)
  top_n_run(c, rc.users, n_items, items, n, "recommend: a batch of items",
            [&](const int32_t *ib, int nb, int64_t, double *sc) {  // rec_score_batch with the sides exchanged
              score_tiles(c, rc.y.ptr, static_cast<size_t>(rc.items) * rc.rank, rc.x.ptr, rc.x_stride(), rc.users, ib, nb, ex, sc);
            },
            T_RECOMMEND, users, scores, counts);
}

// ---- capacity-aware allocation (allocate.hpp) ----------------------------------------------------------------------------
// The rounds of deferred acceptance: per round the batches of recommend_query (user pass) and of recommend_query_items
// over the capped items (item pass), both with alloc_score_kernel in place of rec_score_kernel; P, sigma and tau stay on
// the device, and the host reads one int per round.  users: distinct ids (checked by the C ABI); plan: the caps.
void recommend_allocate(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int n, const AllocPlan &plan,
                        int max_rounds, int32_t *items, double *scores, int32_t *counts, int32_t *rounds,
                        int32_t *converged) {
  use_device(c);
  top_n_blank(n_users, n, items, scores, counts);
  *rounds = 0;
  *converged = 1;
  c->last_ms[T_ALLOCATE] = 0.f;
  c->alloc_rounds = 0;
  if (n_users == 0) return;
  rec_item_lists(c);
  const RecSession &rc = *c->rc;
  const int U = rc.users, NI = rc.items, rank = rc.rank;
  const int64_t NC = plan.capped();
  hipStream_t st = c->stream;
  const size_t xs = rc.x_stride(), ys = static_cast<size_t>(NI) * rank;
  // user pass: batches of bu users over NI columns; item pass: batches of plan.bi capped items over U columns
  const int64_t bu = rec_batch_users(NI, n_users), bi = plan.bi;
  const int nsel = plan.most_n;
  const SelectPlan up = select_plan(c, NI, bu, n), ip = NC > 0 ? select_plan(c, U, bi, nsel) : SelectPlan{};
  const size_t buf = std::max(static_cast<size_t>(bu) * NI, static_cast<size_t>(bi) * U);
  const size_t outs = static_cast<size_t>(n_users) * n, lists = static_cast<size_t>(bi) * nsel;
  require_free_mem(buf * sizeof(double) + SelectStage::bytes(up, ip) + outs * 12 + static_cast<size_t>(n_users) * 8 +
                       lists * 12 + static_cast<size_t>(bi) * 4 + (static_cast<size_t>(NI) + U) * 12 +
                       static_cast<size_t>(NC) * 9 + 4,
                   "recommend_allocate: a batch of scores, the users' lists and the items' keys");
  // tau by item: -inf (everything is acceptable), +inf for a closed item (nothing is); sigma by user: +inf outside the
  // request (nothing stands in front of it), written for the request's users by every round
  std::vector<double> tau_h(static_cast<size_t>(NI), -INFINITY), sig_h(static_cast<size_t>(U), INFINITY);
  for (int32_t i : plan.closed) tau_h[static_cast<size_t>(i)] = INFINITY;
  const std::vector<int32_t> tau_uh(static_cast<size_t>(NI), -1), sig_ih(static_cast<size_t>(U), -1);
  DevBuf<double> sc, ps, ls, tau_s, sig_s;
  DevBuf<int32_t> du, pi, pn, lu, ln, tau_u, sig_i, d_item, d_cap, d_total;
  DevBuf<unsigned char> d_changed;
  sc.alloc(buf);
  const SelectStage sel(up, ip);  // (the two passes follow each other: one scratch)
  ps.alloc(outs); pi.alloc(outs); pn.alloc(static_cast<size_t>(n_users));
  du.alloc(static_cast<size_t>(n_users));
  HIP_CHECK(hipMemcpyAsync(du.ptr, users, sizeof(int32_t) * n_users, hipMemcpyHostToDevice, st));
  tau_s.upload(tau_h, st); tau_u.upload(tau_uh, st);
  if (NC > 0) {
    ls.alloc(lists); lu.alloc(lists); ln.alloc(static_cast<size_t>(bi));
    sig_s.upload(sig_h, st); sig_i.upload(sig_ih, st);
    d_item.upload(plan.item, st); d_cap.upload(plan.cap, st);
    d_changed.alloc(static_cast<size_t>(NC));
    d_total.alloc(1);
  }
  const SeenLists seen = rc.seen_lists();
  const SeenLists by_item{rc.excl ? rc.by_item_off.ptr : nullptr, rc.by_item.ptr};
  const unsigned row_blocks = static_cast<unsigned>((n_users + kBlock - 1) / kBlock);
  EventPair ev;  // device time of the whole call (option "allocate_ms"): the host's reads between the rounds included
  ev.start(st);
  int round = 0;
  bool done = false;
  while (!done) {
    ++round;
    for_batches(n_users, bu, [&](int64_t b0, int nb) {  // the user pass
      const int32_t *ub = du.ptr + b0;
      LAUNCH(alloc_score_kernel, tile_grid(NI, nb), kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, ub, nb, NI, rank, rc.slots,
             nullptr, nullptr, tau_s.ptr, tau_u.ptr, sc.ptr, static_cast<size_t>(NI));
      exclude_seen(st, ub, nb, seen, sc.ptr, static_cast<size_t>(NI));
      sel.run(st, up, sc.ptr, nb, n, ps.ptr + b0 * n, pi.ptr + b0 * n, pn.ptr + b0);
    });
    HIP_CHECK(hipGetLastError());
    if (NC == 0) break;  // (no cap binds: the answer is the user pass)
    LAUNCH(alloc_sigma_kernel, row_blocks, kBlock, 0, st, du.ptr, static_cast<int>(n_users), n, ps.ptr, pi.ptr, pn.ptr,
           sig_s.ptr, sig_i.ptr);
    for_batches(NC, bi, [&](int64_t r0, int nb) {  // the item pass: the sides exchanged
      const int32_t *ib = d_item.ptr + r0;
      const int bn = plan.batch_n[static_cast<size_t>(r0 / bi)];
      LAUNCH(alloc_score_kernel, tile_grid(U, nb), kBlock, 0, st, rc.y.ptr, ys, rc.x.ptr, xs, ib, nb, U, rank, rc.slots,
             tau_s.ptr, tau_u.ptr, sig_s.ptr, sig_i.ptr, sc.ptr, static_cast<size_t>(U));
      exclude_seen(st, ib, nb, by_item, sc.ptr, static_cast<size_t>(U));
      sel.run(st, ip, sc.ptr, nb, bn, ls.ptr, lu.ptr, ln.ptr);
      LAUNCH(alloc_tau_kernel, static_cast<unsigned>((nb + kBlock - 1) / kBlock), kBlock, 0, st, ib, d_cap.ptr + r0, nb, bn,
             ls.ptr, lu.ptr, ln.ptr, tau_s.ptr, tau_u.ptr, d_changed.ptr + r0);
    });
    LAUNCH(alloc_changed_kernel, 1, kBlock, 0, st, d_changed.ptr, static_cast<int>(NC), d_total.ptr);
    HIP_CHECK(hipGetLastError());
    int32_t changed = 0;
    HIP_CHECK(hipMemcpyAsync(&changed, d_total.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));  // (the round's only wait)
    if (changed == 0) {
      done = true;
    } else if (round == max_rounds) {
      *converged = 0;
      done = true;
    }
  }
  LAUNCH(alloc_cut_kernel, row_blocks, kBlock, 0, st, du.ptr, static_cast<int>(n_users), n, tau_s.ptr, tau_u.ptr, ps.ptr,
         pi.ptr, pn.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  top_n_copy_out(c, TopNDev{ps.ptr, pi.ptr, pn.ptr}, ev, n_users, n, T_ALLOCATE, items, scores, counts);
  *rounds = round;
  c->alloc_rounds = round;
}

// ---- welfare-maximising assignment (assign.hpp) -------------------------------------------------------------------------
// The rounds of the forward auction over the compacted list of active rows, then the certificate pass over all rows; the
// row state, the slots and the prices stay on the device, and the host reads one int per round: the next round's active
// rows.  users: distinct ids (checked by the C ABI), any order -- the device works in id order.
void recommend_assign(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const AssignPlan &plan, double reserve,
                      double eps, int max_rounds, const AssignOut &out) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const int NI = rc.items, rank = rc.rank;
  for (int64_t b = 0; b < n_users; ++b) {
    out.items[b] = -1;
    out.scores[b] = -INFINITY;
    out.paid[b] = 0.0;
    out.pi[b] = reserve;
  }
  for (int i = 0; i < NI; ++i) {
    const int32_t q = plan.cap[static_cast<size_t>(i)];
    out.price[i] = q == 0 ? INFINITY : 0.0;
    out.price_sum[i] = 0.0;
    out.load[i] = 0;
  }
  *out.rounds = 0;
  *out.converged = 1;
  c->last_ms[T_ASSIGN] = 0.f;
  c->asg_rounds = 0;
  c->asg_bids = 0;
  if (n_users == 0 || NI == 0) return;
  hipStream_t st = c->stream;
  const size_t xs = rc.x_stride(), ys = static_cast<size_t>(NI) * rank;
  const size_t nu = static_cast<size_t>(n_users), n_slots = plan.slots();
  // the request in id order: row r is request row at[r]
  std::vector<int64_t> at(nu);
  for (size_t b = 0; b < nu; ++b) at[b] = static_cast<int64_t>(b);
  std::sort(at.begin(), at.end(), [&](int64_t a, int64_t b) { return users[a] < users[b]; });
  std::vector<int32_t> ids(nu);
  for (size_t r = 0; r < nu; ++r) ids[r] = users[at[r]];
  const int64_t bu = rec_batch_users(NI, n_users);
  const SelectPlan sp = select_plan(c, NI, bu, 2);
  const int nblk = static_cast<int>((n_users + kBlock - 1) / kBlock);
  const size_t sort_bytes = assign_sort_bytes(nu);
  require_free_mem(static_cast<size_t>(bu) * NI * sizeof(double) + sp.bytes() +
                       nu * (2 * 8 + 2 * 4 + 2 * 12 + 4 + 3 * 4 + 2 * 8 + 2 * 4) + n_slots * 12 +
                       static_cast<size_t>(NI) * (3 * 8 + 2 * 4) + static_cast<size_t>(nblk) * 8 + sort_bytes + 4,
                   "recommend_assign: a batch of scores, the users' state, the bids and the items' slots");
  std::vector<double> p1_h(static_cast<size_t>(NI)), p2_h(static_cast<size_t>(NI));
  for (int i = 0; i < NI; ++i) {
    const int32_t q = plan.cap[static_cast<size_t>(i)];
    p1_h[static_cast<size_t>(i)] = q == 0 ? INFINITY : 0.0;
    p2_h[static_cast<size_t>(i)] = q < 0 || q >= 2 ? 0.0 : INFINITY;
  }
  DevBuf<double> sc, vs, row_paid, row_score, price, p1, p2, bid, bid_score, psum;
  DevBuf<int32_t> du, vi, vn, row_item, dropped, holder, d_cap, d_off, act_r, act_u, bid_item, blk_cnt, blk_base,
      d_total;
  DevBuf<uint32_t> place, ord;
  DevBuf<char> tmp;
  sc.alloc(static_cast<size_t>(bu) * NI);
  const SelectStage sel(sp);
  vs.alloc(2 * nu); vi.alloc(2 * nu); vn.alloc(nu);
  du.upload(ids, st);
  act_u.upload(ids, st);  // the first round: every row is active
  std::vector<int32_t> iota(nu);
  for (size_t r = 0; r < nu; ++r) iota[r] = static_cast<int32_t>(r);
  act_r.upload(iota, st);
  // nobody holds anything, every slot is free at price 0 (+0.0 and -1 are one byte repeated)
  const std::vector<double> ninf_d(nu, -INFINITY);
  row_item.alloc(nu); dropped.alloc(nu); row_paid.alloc(nu); row_score.upload(ninf_d, st);
  price.alloc(n_slots); holder.alloc(n_slots); psum.alloc(static_cast<size_t>(NI));
  HIP_CHECK(hipMemsetAsync(row_item.ptr, 0xFF, sizeof(int32_t) * nu, st));
  HIP_CHECK(hipMemsetAsync(dropped.ptr, 0, sizeof(int32_t) * nu, st));
  HIP_CHECK(hipMemsetAsync(row_paid.ptr, 0, sizeof(double) * nu, st));
  if (n_slots > 0) {
    HIP_CHECK(hipMemsetAsync(price.ptr, 0, sizeof(double) * n_slots, st));
    HIP_CHECK(hipMemsetAsync(holder.ptr, 0xFF, sizeof(int32_t) * n_slots, st));
  }
  p1.upload(p1_h, st); p2.upload(p2_h, st);
  d_cap.upload(plan.cap, st); d_off.upload(plan.slot_off, st);
  bid.alloc(nu); bid_score.alloc(nu); bid_item.alloc(nu); place.alloc(nu); ord.alloc(nu);
  blk_cnt.alloc(static_cast<size_t>(nblk)); blk_base.alloc(static_cast<size_t>(nblk)); d_total.alloc(1);
  tmp.alloc(sort_bytes);
  HIP_CHECK(hipStreamSynchronize(st));  // (the uploads' host vectors are temporaries)
  const SeenLists seen = rc.seen_lists();
  const size_t accept_lds = static_cast<size_t>(plan.lds_places()) * (sizeof(double) + sizeof(int32_t));
  // the values of the rows ids[0 .. n_rows) (device) at the prices p1, the exclusions, and the n best of every row to
  // vs / vi / vn, batch by batch
  auto value_pass = [&](const int32_t *ids, int64_t n_rows, int n) {
    for_batches(n_rows, bu, [&](int64_t b0, int nb) {
      const int32_t *ub = ids + b0;
      LAUNCH(assign_value_kernel, tile_grid(NI, nb), kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys, ub, nb, NI, rank, rc.slots,
             p1.ptr, sc.ptr, static_cast<size_t>(NI));
      exclude_seen(st, ub, nb, seen, sc.ptr, static_cast<size_t>(NI));
      sel.run(st, sp, sc.ptr, nb, n, vs.ptr + b0 * n, vi.ptr + b0 * n, vn.ptr + b0);
    });
  };
  EventPair ev;  // device time of the whole call (option "assign_ms"): the host's reads between the rounds included
  ev.start(st);
  int round = 0;
  int64_t na = n_users, active_sum = 0;
  while (na > 0) {
    if (round == max_rounds) {
      *out.converged = 0;
      break;
    }
    ++round;
    active_sum += na;
    value_pass(act_u.ptr, na, 2);
    const int n_act = static_cast<int>(na);
    LAUNCH(assign_bid_kernel, static_cast<unsigned>((na + kBlock - 1) / kBlock), kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, ys,
           rank, rc.slots, act_u.ptr, act_r.ptr, n_act, vs.ptr, vi.ptr, vn.ptr, p1.ptr, p2.ptr, reserve, eps, bid_item.ptr,
           bid.ptr, bid_score.ptr, place.ptr, dropped.ptr);
    assign_sort_bids(st, tmp.ptr, sort_bytes, bid_item.ptr, bid.ptr, place.ptr, ord.ptr, static_cast<size_t>(na));
    LAUNCH(assign_accept_kernel, static_cast<unsigned>(NI), kRecWave, accept_lds, st, d_cap.ptr, d_off.ptr, plan.lds_places(),
           bid_item.ptr, bid.ptr, bid_score.ptr, ord.ptr, n_act, act_r.ptr, price.ptr, holder.ptr, p1.ptr, p2.ptr,
           row_item.ptr, row_paid.ptr, row_score.ptr);
    LAUNCH(assign_count_kernel, static_cast<unsigned>(nblk), kBlock, 0, st, row_item.ptr, dropped.ptr,
           static_cast<int>(n_users), blk_cnt.ptr);
    LAUNCH(assign_scan_kernel, 1, kBlock, 0, st, blk_cnt.ptr, nblk, blk_base.ptr, d_total.ptr);
    LAUNCH(assign_list_kernel, static_cast<unsigned>(nblk), kBlock, 0, st, row_item.ptr, dropped.ptr, du.ptr,
           static_cast<int>(n_users), blk_base.ptr, act_r.ptr, act_u.ptr);
    HIP_CHECK(hipGetLastError());
    int32_t next = 0;
    HIP_CHECK(hipMemcpyAsync(&next, d_total.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));  // (the round's only wait)
    na = next;
  }
  // the certificate: every row's best value at the final prices
  value_pass(du.ptr, n_users, 1);
  LAUNCH(assign_price_sum_kernel, static_cast<unsigned>((NI + kBlock - 1) / kBlock), kBlock, 0, st, d_off.ptr, price.ptr, NI,
         psum.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  std::vector<int32_t> h_item(nu), h_drop(nu), h_vn(nu);
  std::vector<double> h_paid(nu), h_score(nu), h_vs(nu);
  HIP_CHECK(hipMemcpyAsync(h_item.data(), row_item.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_drop.data(), dropped.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_vn.data(), vn.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_paid.data(), row_paid.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_score.data(), row_score.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_vs.data(), vs.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(out.price_sum, psum.ptr, sizeof(double) * NI, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(out.price, p1.ptr, sizeof(double) * NI, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_ASSIGN] = ev.ms();
  int64_t n_dropped = 0;
  for (size_t r = 0; r < nu; ++r) {
    const size_t b = static_cast<size_t>(at[r]);
    const double best = h_vn[r] > 0 ? h_vs[r] : -INFINITY;
    out.pi[b] = best > reserve ? best : reserve;
    n_dropped += h_drop[r] != 0;
    if (h_item[r] < 0) continue;
    out.items[b] = h_item[r];
    out.scores[b] = h_score[r];
    out.paid[b] = h_paid[r];
    ++out.load[h_item[r]];
  }
  *out.rounds = round;
  c->asg_rounds = round;
  c->asg_bids = active_sum - n_dropped;  // every active row of a round bids or drops out, and drops out once
}

void recommend_audience(mmsbm_hip_ctx *c, int64_t n_items, const int32_t *items, double min_score, int64_t capacity,
                        int64_t *offsets, int32_t *users, double *scores) {
  use_device(c);
  rec_item_lists(c);
  const RecSession &rc = *c->rc;
  std::fill(offsets, offsets + n_items + 1, int64_t(0));
  c->last_ms[T_AUDIENCE] = 0.f;
  const int U = c->ext_users, rank = rc.rank, S = rc.slots;
  if (n_items == 0 || U == 0) return;
  hipStream_t st = c->stream;
  const int64_t n_ut = (static_cast<int64_t>(U) + kRecTile - 1) / kRecTile;
  const int64_t rb = aud_count_rows(U, c->aud_rows, n_items);  // items per COUNT batch
  const size_t table = static_cast<size_t>(rb) * n_ut;
  require_free_mem(table * 4 + static_cast<size_t>(n_items) * 8 + static_cast<size_t>(rb) * 8,
                   "audience: the counts of a batch of items");
  DevBuf<int32_t> di, cnt, tot;
  di.alloc(n_items);
  cnt.alloc(table);
  tot.alloc(n_items);
  HIP_CHECK(hipMemcpyAsync(di.ptr, items, sizeof(int32_t) * n_items, hipMemcpyHostToDevice, st));
  const int32_t *ex_off = rc.excl ? rc.by_item_off.ptr : nullptr, *ex = rc.by_item.ptr;
  const size_t xs = static_cast<size_t>(rc.items) * rank, ys = rc.x_stride();
  // tiles are dealt to at most 8 workgroups per CU (what the staging tiles' LDS allows twice over)
  auto groups = [&](int nb) {
    return static_cast<unsigned>(std::min<int64_t>(n_ut * ((nb + kRecTile - 1) / kRecTile), 8LL * c->n_cus));
  };
  // COUNT + offsets of rows [r0, r0 + nb): cnt [user tile][nb], tot[r0 ...]
  auto count_batch = [&](int64_t r0, int nb) {
    LAUNCH(aud_tile_kernel<false>, groups(nb), kBlock, 0, st, rc.y.ptr, xs, rc.x.ptr, ys, di.ptr + r0, nb, U, rank, S,
           ex_off, ex, min_score, cnt.ptr, static_cast<size_t>(nb), nullptr, int64_t(0), nullptr, nullptr, int64_t(0));
    LAUNCH(aud_offsets_kernel, static_cast<unsigned>((nb + kBlock - 1) / kBlock), kBlock, 0, st, cnt.ptr,
           static_cast<size_t>(nb), static_cast<int>(n_ut), nb, tot.ptr + r0);
  };
  float ms = 0.f;  // device time of the call's kernels (option "audience_ms")
  std::vector<int32_t> ht(static_cast<size_t>(n_items));
  {
    EventPair ev;
    ev.start(st);
    for (int64_t r0 = 0; r0 < n_items; r0 += rb) count_batch(r0, static_cast<int>(std::min(rb, n_items - r0)));
    HIP_CHECK(hipGetLastError());
    ev.stop(st);
    HIP_CHECK(hipMemcpyAsync(ht.data(), tot.ptr, sizeof(int32_t) * n_items, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ms += ev.ms();
  }
  int64_t largest = 0;
  for (int64_t b = 0; b < n_items; ++b) {
    offsets[b + 1] = offsets[b] + ht[static_cast<size_t>(b)];
    largest = std::max<int64_t>(largest, ht[static_cast<size_t>(b)]);
  }
  c->last_ms[T_AUDIENCE] = ms;
  const int64_t total = offsets[n_items];
  if (!users || total == 0) return;
  if (capacity < total)
    throw ApiError(MMSBM_E_TOOLARGE, "audience: " + std::to_string(total) + " entries, room for " + std::to_string(capacity));
  // WRITE: runs of rows whose entries stay under the cap (a larger row goes alone), inside the COUNT batches; a batch's
  // counts are formed again unless the request was one batch, whose offsets are still there
  const int64_t cap = c->aud_entries > 0 ? c->aud_entries : kAudEntries;
  const int64_t out_cap = std::min(total, std::max(cap, largest));
  require_free_mem(static_cast<size_t>(out_cap) * 12 + static_cast<size_t>(rb) * 8, "audience: the entries of a batch of items");
  DevBuf<int32_t> ou;
  DevBuf<double> os;
  DevBuf<int64_t> rbase;
  ou.alloc(static_cast<size_t>(out_cap));
  os.alloc(static_cast<size_t>(out_cap));
  rbase.alloc(static_cast<size_t>(rb));
  const bool one_batch = rb >= n_items;
  std::vector<int64_t> hb(static_cast<size_t>(rb));
  for (int64_t r0 = 0; r0 < n_items; r0 += rb) {
    const int nb = static_cast<int>(std::min(rb, n_items - r0));
    if (offsets[r0 + nb] == offsets[r0]) continue;
    for (int j = 0; j < nb; ++j) hb[static_cast<size_t>(j)] = offsets[r0 + j] - offsets[r0];
    HIP_CHECK(hipMemcpyAsync(rbase.ptr, hb.data(), sizeof(int64_t) * nb, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));  // (hb is written again for the next batch)
    if (!one_batch) {
      EventPair ev;
      ev.start(st);
      count_batch(r0, nb);
      ev.stop(st);
      HIP_CHECK(hipStreamSynchronize(st));
      ms += ev.ms();
    }
    for (const AudRun &run : aud_write_runs(ht.data() + r0, nb, cap)) {
      if (run.entries == 0) continue;
      const int s0 = run.first;
      EventPair ev;
      ev.start(st);
      LAUNCH(aud_tile_kernel<true>, groups(run.rows), kBlock, 0, st, rc.y.ptr, xs, rc.x.ptr, ys, di.ptr + r0 + s0, run.rows,
             U, rank, S, ex_off, ex, min_score, cnt.ptr + s0, static_cast<size_t>(nb), rbase.ptr + s0,
             hb[static_cast<size_t>(s0)], ou.ptr, os.ptr, out_cap);
      HIP_CHECK(hipGetLastError());
      ev.stop(st);
      const int64_t o = offsets[r0 + s0];
      HIP_CHECK(hipMemcpyAsync(users + o, ou.ptr, sizeof(int32_t) * run.entries, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipMemcpyAsync(scores + o, os.ptr, sizeof(double) * run.entries, hipMemcpyDeviceToHost, st));
      HIP_CHECK(hipStreamSynchronize(st));
      ms += ev.ms();
    }
  }
  c->last_ms[T_AUDIENCE] = ms;
}

// ---- group queries (group.hpp) ------------------------------------------------------------------------------------------
// plan (plan_groups: the member blocks, the batches' runs and fragments), memory check, uploads, top_n_run, scatter
void recommend_query_groups(mmsbm_hip_ctx *c, int64_t n_groups, const int64_t *offsets, const int32_t *members, int mode,
                            double bar, const int32_t *cand, int n_cand, int n, int32_t *items, double *scores,
                            int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  top_n_blank(n_groups, n, items, scores, counts);
  c->last_ms[T_GROUP] = 0.f;
  const int NI = rc.items, rank = rc.rank, S = rc.slots;
  const int C = cand ? n_cand : NI;
  const bool tiles = mode != MMSBM_HIP_GROUP_MEAN;
  const GroupPlan p = plan_groups(offsets, members, n_groups, C, c->n_cus, c->grp_run, tiles);
  const int64_t G = p.groups();
  if (G == 0 || C == 0) return;  // (no row or no column to score: every row is empty)
  if (p.too_large())
    throw ApiError(MMSBM_E_TOOLARGE, "recommend_query_groups: " + std::to_string(p.n_blocks) + " blocks of member rows in one query");
  const size_t ycs = static_cast<size_t>(C) * rank, bs = static_cast<size_t>(G) * rank;
  require_free_mem(CatTable::bytes(rc, cand, C) +
                       (p.rows.size() + 3 * p.info.size() + p.run_off.size() + 2 * p.cut_off.size() + 2 * static_cast<size_t>(G) + 1) * 4 +
                       (tiles ? static_cast<size_t>(p.most_frag) * C : S * bs) * sizeof(double),
                   "recommend_query_groups: the member rows, the groups' lists and the candidates' rows");
  hipStream_t st = c->stream;
  DevBuf<int32_t> d_rows, d_info, d_grp, d_out, d_run, d_cut_grp, d_cut_off, d_gblk, d_size;
  DevBuf<double> xbar, part;
  CatTable ct;
  d_rows.upload(p.rows, st);
  d_info.upload(p.info, st);
  d_grp.upload(p.grp, st);
  if (tiles) {
    d_out.upload(p.out, st);
    d_run.upload(p.run_off, st);
    if (p.most_frag > 0) {
      d_cut_grp.upload(p.cut_grp, st);
      d_cut_off.upload(p.cut_off, st);
      part.alloc(static_cast<size_t>(p.most_frag) * C);
    }
  } else {
    d_gblk.upload(p.gblk, st);
    d_size.upload(p.gsize, st);
    xbar.alloc(S * bs);
  }
  if (cand) cat_table(c, cand, C, ct);
  const double *y = cand ? ct.y.ptr : rc.y.ptr;
  const size_t ys = cand ? ycs : static_cast<size_t>(NI) * rank, xs = rc.x_stride();
  const SeenLists seen = rc.seen_lists();
  const int32_t *col_of = cand ? ct.col.ptr : nullptr;
  std::vector<int32_t> ti(static_cast<size_t>(G) * n), tc(static_cast<size_t>(G));
  std::vector<double> ts(static_cast<size_t>(G) * n);
  top_n_run(c, C, G, p.ids.data(), n, "recommend_query_groups: a batch of groups",
            [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
              const int g0 = static_cast<int>(b0);
              const unsigned it = static_cast<unsigned>(p.item_tiles);
              if (tiles) {
                const size_t k = static_cast<size_t>(b0 / p.bu);
                const dim3 g(it, static_cast<unsigned>(p.batch_run[k + 1] - p.batch_run[k]));
                const int32_t *ro = d_run.ptr + p.batch_run[k];
                const int n_cut = p.batch_cut[k + 1] - p.batch_cut[k], p0 = p.cut_off[static_cast<size_t>(p.batch_cut[k])];
                auto tile = [&](auto kernel) {
                  LAUNCH(kernel, g, kBlock, 0, st, rc.x.ptr, xs, y, ys, d_rows.ptr, d_info.ptr, d_out.ptr, ro, g0, p0, C, rank,
                         S, bar, sc, part.ptr, static_cast<size_t>(C));
                };
                if (mode == MMSBM_HIP_GROUP_MIN) tile(grp_tile_kernel<kGrpMin>);
                else if (mode == MMSBM_HIP_GROUP_MAX) tile(grp_tile_kernel<kGrpMax>);
                else tile(grp_tile_kernel<kGrpCount>);
                if (n_cut > 0)
                  LAUNCH(grp_combine_kernel, dim3(static_cast<unsigned>((C + kBlock - 1) / kBlock), static_cast<unsigned>(n_cut)),
                         kBlock, 0, st, part.ptr, d_cut_grp.ptr + p.batch_cut[k], d_cut_off.ptr + p.batch_cut[k], g0, p0, C, mode, S,
                         sc, static_cast<size_t>(C));
              } else {
                const size_t e = static_cast<size_t>(nb) * rank * S;
                LAUNCH(grp_mean_kernel, static_cast<unsigned>((e + kBlock - 1) / kBlock), kBlock, 0, st, rc.x.ptr, xs, rank,
                       S, d_rows.ptr, d_gblk.ptr, d_size.ptr, g0, nb, xbar.ptr, bs);
                score_tiles(c, xbar.ptr, bs, y, ys, C, ub, nb, SeenLists{}, sc);
              }
              if (seen.off) {
                const int blk0 = p.gblk[static_cast<size_t>(g0)];
                LAUNCH(grp_exclude_kernel, static_cast<unsigned>(p.gblk[static_cast<size_t>(g0) + nb] - blk0), kBlock, 0, st,
                       d_rows.ptr, d_info.ptr, d_grp.ptr, blk0, g0, seen.off, seen.items, col_of, sc, static_cast<size_t>(C));
              }
            },
            T_GROUP, ti.data(), ts.data(), tc.data());
  c->last_ms[T_GROUP] += ct.ms;
  for (int64_t r = 0; r < G; ++r) {  // the rows to their places in the request, columns -> item ids
    const size_t o = static_cast<size_t>(p.at[r]) * n, t = static_cast<size_t>(r) * n;
    const int cnt = tc[static_cast<size_t>(r)];
    if (counts) counts[p.at[r]] = cnt;
    for (int k = 0; k < cnt; ++k) {
      items[o + k] = item_of(cand, ti[t + k]);
      if (scores) scores[o + k] = ts[t + k];
    }
  }
}

// ---- greedy assortment selection (assortment.hpp) -------------------------------------------------------------------------
// plan (plan_assortment: the runs of user rows, the batches of item tiles), memory check, uploads; the given items one
// by one (their gain over the state before them, then the state); then n_pick rounds of gain / join / pick / update
// enqueued back to back -- no host wait and no copy between them: once the stop flag is set on the device the launches
// that follow return at once -- and ONE read-back at the end.  users: ascending, distinct.
void recommend_assortment(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int mode, double level,
                          const int32_t *given, int n_given, const int32_t *cand, int n_cand, int n_pick, int32_t *items,
                          double *gains, int32_t *count, int32_t *stop, double *given_gains, int32_t *served_items,
                          double *served_scores) {
  use_device(c);
  const RecSession &rc = *c->rc;
  for (float *t : {&c->last_ms[T_ASSORT], &c->asrt_ms[0], &c->asrt_ms[1], &c->asrt_ms[2]}) *t = 0.f;
  const int NI = rc.items, rank = rc.rank, S = rc.slots;
  const int C = cand ? n_cand : NI;
  for (int k = 0; k < n_pick; ++k) {
    items[k] = -1;
    gains[k] = 0.0;
  }
  for (int g = 0; g < n_given; ++g) given_gains[g] = 0.0;
  *count = 0;
  *stop = n_pick == 0 ? MMSBM_HIP_ASSORT_STOP_C : C == 0 ? MMSBM_HIP_ASSORT_STOP_NO_CANDIDATES : MMSBM_HIP_ASSORT_STOP_NO_GAIN;
  if (n_users == 0) return;  // (nobody to serve: no item gains anything)
  const int nu = static_cast<int>(n_users);
  const AssortPlan p = plan_assortment(n_users, C, c->n_cus, c->asrt_run,
                                       c->asrt_part > 0 ? static_cast<size_t>(c->asrt_part) : kAsrtPartBytes);
  // a given item: its one tile of the catalogue, in the runs of the rounds -- a column's sum is the same additions in the
  // same order whether the item is given or chosen, so a set valued as given items gets the greedy's bits
  const AssortPlan pg = plan_assortment(n_users, kRecTile, c->n_cus, C > 0 ? p.run_blocks : c->asrt_run);
  const bool rounds = n_pick > 0 && C > 0;
  const size_t ycs = static_cast<size_t>(C) * rank;
  const size_t n_res = static_cast<size_t>(n_pick) + static_cast<size_t>(n_given);
  require_free_mem(CatTable::bytes(rc, cand, C) + static_cast<size_t>(nu) * (4 + 8 + 4 + 8) + static_cast<size_t>(C) * 4 + n_res * 12 +
                       (rounds ? p.part_doubles() * sizeof(double) + static_cast<size_t>(p.n_blk()) * 12 : 0) +
                       (n_given > 0 ? pg.part_doubles() * sizeof(double) : 0),
                   "recommend_assortment: the users' state, the runs' partial sums and the candidates' rows");
  hipStream_t st = c->stream;
  // the state: best[u] = level x S undivided (BEST; REACH fills it when a user is covered), nobody served
  std::vector<double> h_best(static_cast<size_t>(nu), mode == kAsrtBest ? level * static_cast<double>(S) : 0.0);
  std::vector<int32_t> h_served(static_cast<size_t>(nu), -1), h_users(users, users + nu);
  std::vector<int32_t> h_taken(static_cast<size_t>(C), 0);
  for (int g = 0; g < n_given; ++g) {  // a given item is never chosen: its column, where it has one
    if (cand) {
      const int32_t *at = std::lower_bound(cand, cand + n_cand, given[g]);
      if (at != cand + n_cand && *at == given[g]) h_taken[static_cast<size_t>(at - cand)] = 1;
    } else {
      h_taken[static_cast<size_t>(given[g])] = 1;
    }
  }
  DevBuf<double> best, score, part, part_g, blk_v, res_gain;
  DevBuf<int32_t> rows, served, taken, blk_i, res_col, flags;
  CatTable ct;
  rows.upload(h_users, st);
  best.upload(h_best, st);
  served.upload(h_served, st);
  taken.upload(h_taken, st);
  score.alloc(static_cast<size_t>(nu));
  res_col.alloc(static_cast<size_t>(n_pick));
  res_gain.alloc(n_res);
  flags.alloc(2);  // the stop flag, the count
  HIP_CHECK(hipMemsetAsync(res_gain.ptr, 0, sizeof(double) * std::max<size_t>(n_res, 1), st));
  HIP_CHECK(hipMemsetAsync(flags.ptr, 0, sizeof(int32_t) * 2, st));
  if (rounds) {
    part.alloc(p.part_doubles());
    blk_v.alloc(static_cast<size_t>(p.n_blk()));
    blk_i.alloc(static_cast<size_t>(p.n_blk()));
    if (cand) cat_table(c, cand, C, ct);
  }
  if (n_given > 0) part_g.alloc(pg.part_doubles());
  const double *y = cand && rounds ? ct.y.ptr : rc.y.ptr;
  const size_t yfs = static_cast<size_t>(NI) * rank, ys = cand && rounds ? ycs : yfs, xs = rc.x_stride();
  const SeenLists seen = rc.seen_lists();
  const int32_t *dcand = cand && rounds ? ct.cand.ptr : nullptr;
  int32_t *d_stop = flags.ptr, *d_count = flags.ptr + 1;
  double *d_given = res_gain.ptr + n_pick;
  const unsigned user_grid = static_cast<unsigned>((nu + kBlock - 1) / kBlock);
  auto gain = [&](const AssortPlan &pl, const double *yy, size_t yys, int ni, int tile0, unsigned tiles, const int32_t *cols,
                  double *out) {
    const dim3 g(tiles, static_cast<unsigned>(pl.runs));
    auto tile = [&](auto kernel) {
      LAUNCH(kernel, g, kBlock, 0, st, rc.x.ptr, xs, yy, yys, rows.ptr, nu, static_cast<int>(pl.run_rows), ni, tile0, rank, S,
             level, best.ptr, served.ptr, seen.off, seen.items, cols, d_stop, out, static_cast<size_t>(pl.ld));
    };
    if (mode == kAsrtBest) tile(asrt_gain_kernel<kAsrtBest>);
    else tile(asrt_gain_kernel<kAsrtReach>);
  };
  auto update = [&](int k, int item) {
    auto go = [&](auto kernel) {
      LAUNCH(kernel, user_grid, kBlock, 0, st, rc.x.ptr, xs, rc.y.ptr, yfs, rows.ptr, nu, rank, S, level, k, item, res_col.ptr,
             dcand, seen.off, seen.items, d_stop, best.ptr, served.ptr);
    };
    if (mode == kAsrtBest) go(asrt_update_kernel<kAsrtBest>);
    else go(asrt_update_kernel<kAsrtReach>);
  };
  // the phases' device times (option "assortment_timing"): one event at every border between two phases of a round
  std::vector<std::unique_ptr<EventPair::Event>> marks;
  auto mark = [&] {
    if (!c->asrt_timing) return;
    marks.push_back(std::make_unique<EventPair::Event>());
    HIP_CHECK(hipEventRecord(marks.back()->e, st));
  };
  EventPair ev;  // device time of the query's kernels (option "assortment_ms")
  ev.start(st);
  for (int g = 0; g < n_given; ++g) {
    gain(pg, rc.y.ptr, yfs, NI, given[g] / kRecTile, 1u, nullptr, part_g.ptr);
    LAUNCH(asrt_given_kernel, 1, kRecWave, 0, st, part_g.ptr, static_cast<size_t>(pg.ld), static_cast<int>(pg.runs),
           given[g] % kRecTile, g, d_given);
    update(-1, given[g]);
  }
  HIP_CHECK(hipGetLastError());
  for (int k = 0; rounds && k < n_pick; ++k) {  // (rounds follow each other on the stream: no host wait in between)
    mark();
    for (int64_t b = 0; b < p.batches; ++b) {
      const auto [col0, n_cols] = p.batch_cols(b, C);
      gain(p, y, ys, C, static_cast<int>(b * p.batch_tiles), static_cast<unsigned>((n_cols + kRecTile - 1) / kRecTile), dcand,
           part.ptr);
      LAUNCH(asrt_join_kernel, static_cast<unsigned>((n_cols + kAsrtJoin - 1) / kAsrtJoin), kBlock, 0, st, part.ptr,
             static_cast<size_t>(p.ld), static_cast<int>(p.runs), static_cast<int>(col0), static_cast<int>(n_cols), taken.ptr,
             p.batch_blk[static_cast<size_t>(b)], d_stop, blk_v.ptr, blk_i.ptr);
    }
    mark();
    LAUNCH(asrt_pick_kernel, 1, kBlock, 0, st, blk_v.ptr, blk_i.ptr, static_cast<int>(p.n_blk()), k, taken.ptr, res_col.ptr,
           res_gain.ptr, d_count, d_stop);
    mark();
    update(k, 0);
    HIP_CHECK(hipGetLastError());
  }
  mark();
  LAUNCH(asrt_finish_kernel, static_cast<unsigned>((std::max<size_t>(n_res, static_cast<size_t>(nu)) + kBlock - 1) / kBlock),
         kBlock, 0, st, res_gain.ptr, static_cast<int>(n_res), mode == kAsrtBest, best.ptr, served.ptr, nu, S, score.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  std::vector<int32_t> h_col(static_cast<size_t>(n_pick)), h_flags(2);
  std::vector<double> h_gain(n_res);
  if (n_pick > 0) HIP_CHECK(hipMemcpyAsync(h_col.data(), res_col.ptr, sizeof(int32_t) * n_pick, hipMemcpyDeviceToHost, st));
  if (n_res > 0) HIP_CHECK(hipMemcpyAsync(h_gain.data(), res_gain.ptr, sizeof(double) * n_res, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(h_flags.data(), flags.ptr, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(served_items, served.ptr, sizeof(int32_t) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(served_scores, score.ptr, sizeof(double) * nu, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_ASSORT] = ev.ms() + ct.ms;
  for (size_t m = 0; m + 1 < marks.size(); ++m) {  // gain + join, pick, update: in turn
    float v = 0.f;
    HIP_CHECK(hipEventElapsedTime(&v, marks[m]->e, marks[m + 1]->e));
    c->asrt_ms[m % 3] += v;
  }
  const int cnt = rounds ? h_flags[1] : 0;
  *count = cnt;
  if (rounds) *stop = h_flags[0];  // (0: all n_pick rounds ran)
  for (int k = 0; k < cnt; ++k) {
    items[k] = item_of(cand, h_col[static_cast<size_t>(k)]);
    gains[k] = h_gain[static_cast<size_t>(k)];
  }
  for (int g = 0; g < n_given; ++g) given_gains[g] = h_gain[static_cast<size_t>(n_pick) + g];
}

// ---- ensemble-aware queries (ensemble.hpp) ------------------------------------------------------------------------------
// rec_run_within with the score tile replaced by the aggregate over the restarts (rec_within_run: the same candidate
// table, the same exclusions, the same batches and selection)
void recommend_query_ensemble(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, int mode, double risk,
                              const int32_t *cand, int n_cand, const int64_t *xoff, const int32_t *xit, int n,
                              int32_t *items, double *scores, int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  top_n_blank(n_users, n, items, scores, counts);
  rec_within_run(c, n_users, users, rc.seen_lists(), cand, n_cand, xoff, xit, n,
                 [&](const double *y, size_t ys, int C, const int32_t *ub, int nb, double *sc) {
                   auto tile = [&](auto kernel) {
                     LAUNCH(kernel, tile_grid(C, nb, kEnsTile), kBlock, 0, c->stream, rc.x.ptr, rc.x_stride(), y, ys, ub, nb, C, rc.rank, rc.slots, risk, sc,
                            static_cast<size_t>(C));
                   };
                   if (mode == MMSBM_HIP_ENSEMBLE_MIN) tile(ens_tile_kernel<kEnsMin>);
                   else if (mode == MMSBM_HIP_ENSEMBLE_MAX) tile(ens_tile_kernel<kEnsMax>);
                   else tile(ens_tile_kernel<kEnsLcb>);
                 },
                 T_ENSEMBLE, items, scores, counts);
}

void recommend_pair_spread(mmsbm_hip_ctx *c, int64_t n_pairs, const int32_t *users, const int32_t *items, double *stats,
                           double *per_slot) {
  use_device(c);
  const RecSession &rc = *c->rc;
  c->last_ms[T_ENSEMBLE] = 0.f;
  if (n_pairs == 0) return;
  const int S = rc.slots;
  hipStream_t st = c->stream;
  const int64_t per = ens_pairs_per_launch(n_pairs, S, per_slot != nullptr);
  require_free_mem(static_cast<size_t>(per) * ens_pair_bytes(S, per_slot != nullptr), "recommend_pair_spread: a batch of pairs");
  DevBuf<int32_t> du, di;
  DevBuf<double> ds, dp;
  du.alloc(static_cast<size_t>(per));
  di.alloc(static_cast<size_t>(per));
  ds.alloc(static_cast<size_t>(per) * 4);
  if (per_slot) dp.alloc(static_cast<size_t>(per) * S);
  float ms = 0.f;  // device time of the call's kernels (option "ensemble_ms")
  for (int64_t p0 = 0; p0 < n_pairs; p0 += per) {
    const int64_t np = std::min(per, n_pairs - p0);
    HIP_CHECK(hipMemcpyAsync(du.ptr, users + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(di.ptr, items + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    EventPair ev;
    ev.start(st);
    LAUNCH(ens_pairs_kernel, static_cast<unsigned>((np + kBlock - 1) / kBlock), kBlock, 0, st, rc.x.ptr, rc.x_stride(),
           rc.y.ptr, static_cast<size_t>(rc.items) * rc.rank, rc.rank, S, du.ptr, di.ptr, np, ds.ptr, dp.ptr);
    HIP_CHECK(hipGetLastError());
    ev.stop(st);
    HIP_CHECK(hipMemcpyAsync(stats + p0 * 4, ds.ptr, sizeof(double) * np * 4, hipMemcpyDeviceToHost, st));
    for (int s = 0; s < S && per_slot; ++s)  // the batch's [S][np] into the caller's [S][n_pairs]
      HIP_CHECK(hipMemcpyAsync(per_slot + static_cast<size_t>(s) * n_pairs + p0, dp.ptr + static_cast<size_t>(s) * np,
                               sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ms += ev.ms();
  }
  c->last_ms[T_ENSEMBLE] = ms;
}

// ---- nearest items / users (similar.hpp) ------------------------------------------------------------------------------
void similar_begin(mmsbm_hip_ctx *c, int side) {
  use_device(c);
  c->sm.reset();  // (from here on the previous session is gone)
  auto sm = std::make_unique<SimSession>();
  sm->side = side;
  sm->rows = side == 0 ? c->ext_items : c->ext_users;
  sm->others = side == 0 ? c->ext_users : c->ext_items;
  sm->width = (side == 0 ? c->ext_k : c->ext_l) * c->n_ratings;
  c->sm = std::move(sm);
}

void similar_add(mmsbm_hip_ctx *c) {  // the selected slot (the caller holds a OneSlot)
  use_device(c);
  SimSession &sm = *c->sm;
  const int R = c->n_ratings, S = sm.slots, W = sm.width, rows = sm.rows;
  const size_t qs = static_cast<size_t>(rows) * W;
  require_free_mem((S + 1) * (qs + W) * sizeof(double), "similar: the slots' profiles");
  hipStream_t st = c->stream;
  DevBuf<double> nq, nm;  // the two tables grow by one slot
  double *qo = grow_by_slot(sm.q, qs, S, st, nq), *mo = grow_by_slot(sm.mf, static_cast<size_t>(W), S, st, nm);
  const ExtSlot e = ext_slot(c);
  // items: profiles over the user groups (g = k) from eta (t = l), masses of theta; users: the other way round
  const bool items = sm.side == 0;
  const int G = items ? c->ext_k : c->ext_l, T = items ? c->ext_l : c->ext_k;
  LAUNCH(sim_mass_kernel, static_cast<unsigned>(G), kBlock, 0, st, items ? e.users : e.items, sm.others, R, mo);
  if (qs > 0)
    LAUNCH(sim_profile_kernel, static_cast<unsigned>((qs + kBlock - 1) / kBlock), kBlock, 0, st,
           items ? e.items : e.users, T, e.p, e.rs, items ? e.ks : e.ls, items ? e.ls : e.ks, qo, rows, G, R);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  sm.q.swap(nq);
  sm.mf.swap(nm);
  sm.slots = S + 1;
}

void similar_query(mmsbm_hip_ctx *c, int64_t n_rows, const int32_t *ids, int n, int32_t *out_ids, double *distance,
                   int32_t *counts) {
  use_device(c);
  const SimSession &sm = *c->sm;
  const int rows = sm.rows, W = sm.width, S = sm.slots;
  const double denom = static_cast<double>(S) * static_cast<double>(sm.others);
  hipStream_t st = c->stream;
  top_n_run(c, rows, n_rows, ids, n, "similar: a batch of query rows",
            [&](const int32_t *ub, int nb, int64_t, double *sc) {
              LAUNCH(sim_dist_kernel, tile_grid(rows, nb, kSimTile), kBlock, 0, st, sm.q.ptr, static_cast<size_t>(rows) * W, sm.mf.ptr, ub, nb, rows,
                     W, S, denom, sc, static_cast<size_t>(rows));
            },
            T_SIMILAR, out_ids, distance, counts);
  // the buffer held -D (the selection's order): the distances, +inf behind the last one (a zero leaves as +0.0)
  for (size_t e = 0; distance && e < static_cast<size_t>(n_rows) * n; ++e) distance[e] = -distance[e];
}

// ---- diversified top-N and the distance of given pairs (diverse.hpp) --------------------------------------------------
void similar_pairs(mmsbm_hip_ctx *c, int64_t n_pairs, const int32_t *a, const int32_t *b, double *distance) {
  use_device(c);
  const SimSession &sm = *c->sm;
  c->last_ms[T_DIVERSE] = 0.f;
  if (n_pairs == 0) return;
  const double denom = static_cast<double>(sm.slots) * static_cast<double>(sm.others);
  hipStream_t st = c->stream;
  const int64_t per = std::min<int64_t>(n_pairs, int64_t(1) << 24);  // pairs per launch (16 bytes each)
  require_free_mem(static_cast<size_t>(per) * 16, "similar_pairs: a batch of pairs");
  DevBuf<int32_t> da, db;
  DevBuf<double> dd;
  da.alloc(static_cast<size_t>(per));
  db.alloc(static_cast<size_t>(per));
  dd.alloc(static_cast<size_t>(per));
  float ms = 0.f;  // device time of the call's kernels (option "diverse_ms")
  for (int64_t p0 = 0; p0 < n_pairs; p0 += per) {
    const int64_t np = std::min(per, n_pairs - p0);
    HIP_CHECK(hipMemcpyAsync(da.ptr, a + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(db.ptr, b + p0, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
    EventPair ev;
    ev.start(st);
    LAUNCH(div_pairs_kernel, static_cast<unsigned>((np + kBlock - 1) / kBlock), kBlock, 0, st, sm.q.ptr,
           static_cast<size_t>(sm.rows) * sm.width, sm.mf.ptr, sm.width, sm.slots, denom, da.ptr, db.ptr, np, dd.ptr);
    HIP_CHECK(hipGetLastError());
    ev.stop(st);
    HIP_CHECK(hipMemcpyAsync(distance + p0, dd.ptr, sizeof(double) * np, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ms += ev.ms();
  }
  c->last_ms[T_DIVERSE] = ms;
}

void recommend_diverse(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int32_t *cand, int n_cand,
                       const int64_t *xoff, const int32_t *xit, int n, int pool, double trade_off, int32_t *items,
                       double *scores, double *distances, int32_t *counts) {
  use_device(c);
  const RecSession &rc = *c->rc;
  const SimSession &sm = *c->sm;
  top_n_blank(n_users, n, items, scores, counts);
  for (size_t e = 0; distances && e < static_cast<size_t>(n_users) * n; ++e) distances[e] = INFINITY;
  c->last_ms[T_DIVERSE] = 0.f;
  if ((cand ? n_cand : rc.items) == 0 || n_users == 0) return;  // (no column to score: every row is empty)
  hipStream_t st = c->stream;
  const double denom = static_cast<double>(sm.slots) * static_cast<double>(sm.others);
  const size_t lds = (static_cast<size_t>(pool) * 21 + 7) / 8 * 8;  // score, m, id, picked flag per place
  size_t free_b = 0, total_b = 0;
  if (c->div_rows <= 0) HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  const int64_t rows_per = div_rows_per_call(c->div_rows, n_users, free_b, div_row_bytes(pool, n));
  const SeenLists seen = rc.seen_lists();
  float ms = 0.f;  // device time of the query's kernels (option "diverse_ms")
  std::vector<int64_t> sub;
  for (int64_t b0 = 0; b0 < n_users; b0 += rows_per) {
    const int64_t nb = std::min(rows_per, n_users - b0);
    if (xoff) {  // the rows' own lists, offsets from the first of them
      sub.resize(static_cast<size_t>(nb) + 1);
      for (int64_t k = 0; k <= nb; ++k) sub[static_cast<size_t>(k)] = xoff[b0 + k] - xoff[b0];
    }
    const size_t outs = static_cast<size_t>(nb) * n;
    rec_within_device(
        c, nb, users + b0, seen, cand, n_cand, xoff ? sub.data() : nullptr, xoff ? xit + xoff[b0] : nullptr, pool,
        outs * 20 + static_cast<size_t>(nb) * 4, rec_tiles(c, rc.x.ptr, rc.x_stride()),
        [&](const TopNDev &dev, EventPair &ev, const int32_t *dcand, float prep_ms) {
          DevBuf<int32_t> ri, rn;
          DevBuf<double> rs, rd;
          ri.alloc(outs); rs.alloc(outs); rd.alloc(outs); rn.alloc(static_cast<size_t>(nb));
          EventPair ev2;
          ev2.start(st);
          if (dcand)  // the pool as columns of the compact table -> item ids
            LAUNCH(div_ids_kernel, static_cast<unsigned>((static_cast<size_t>(nb) * pool + kBlock - 1) / kBlock), kBlock, 0,
                   st, dcand, n_cand, dev.on, static_cast<int>(nb), pool, dev.oi);
          LAUNCH(div_greedy_kernel, static_cast<unsigned>(nb), kDivWave, lds, st, sm.q.ptr,
                 static_cast<size_t>(sm.rows) * sm.width, sm.mf.ptr, sm.width, sm.slots, sm.rows, denom, dev.os, dev.oi, dev.on, pool, n, trade_off, ri.ptr, rs.ptr, rd.ptr, rn.ptr);
          HIP_CHECK(hipGetLastError());
          ev2.stop(st);
          const size_t o = static_cast<size_t>(b0) * n;  // (the kernel wrote the padding too: straight into the caller's rows)
          HIP_CHECK(hipMemcpyAsync(items + o, ri.ptr, sizeof(int32_t) * outs, hipMemcpyDeviceToHost, st));
          if (scores) HIP_CHECK(hipMemcpyAsync(scores + o, rs.ptr, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
          if (distances) HIP_CHECK(hipMemcpyAsync(distances + o, rd.ptr, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
          if (counts) HIP_CHECK(hipMemcpyAsync(counts + b0, rn.ptr, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st));
          HIP_CHECK(hipStreamSynchronize(st));
          ms += ev.ms() + ev2.ms() + prep_ms;
        });
  }
  c->last_ms[T_DIVERSE] = ms;
}

// ---- the most informative items of a user (inform.hpp) ----------------------------------------------------------------
void inform_begin(mmsbm_hip_ctx *c) {
  use_device(c);
  c->inf.reset();  // (from here on the previous session is gone)
  c->inf = std::make_unique<InfSession>();
}

void inform_add(mmsbm_hip_ctx *c) {  // the selected slot (the caller holds a OneSlot)
  use_device(c);
  InfSession &inf = *c->inf;
  const int U = c->ext_users, I = c->ext_items, K = c->ext_k, L = c->ext_l, R = c->n_ratings, S = inf.slots;
  const size_t ths = static_cast<size_t>(U) * K, hs = static_cast<size_t>(I) * K, qs = hs * R;
  require_free_mem((S + 1) * (ths + qs + hs + K) * sizeof(double), "inform: the slots' profiles");
  hipStream_t st = c->stream;
  DevBuf<double> nt, nq, nh, nm;  // the four tables grow by one slot
  double *to = grow_by_slot(inf.th, ths, S, st, nt), *qo = grow_by_slot(inf.q, qs, S, st, nq);
  double *ho = grow_by_slot(inf.h, hs, S, st, nh), *mo = grow_by_slot(inf.mass, static_cast<size_t>(K), S, st, nm);
  const ExtSlot e = ext_slot(c);
  if (ths > 0)  // the users' rows as they are, external sides (rec_fold_kernel without a matrix)
    LAUNCH(rec_fold_kernel, static_cast<unsigned>((ths + kBlock - 1) / kBlock), kBlock, 0, st, e.users, K, nullptr, 0, 0,
           to, U, K);
  LAUNCH(sim_mass_kernel, static_cast<unsigned>(K), kBlock, 0, st, e.users, U, 1, mo);
  if (qs > 0) {
    LAUNCH(sim_profile_kernel, static_cast<unsigned>((qs + kBlock - 1) / kBlock), kBlock, 0, st, e.items, L, e.p, e.rs,
           e.ks, e.ls, qo, I, K, R);
    LAUNCH(inf_entropy_kernel, static_cast<unsigned>((hs + kBlock - 1) / kBlock), kBlock, 0, st, qo, ho, hs, R);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  inf.th.swap(nt);
  inf.q.swap(nq);
  inf.h.swap(nh);
  inf.mass.swap(nm);
  inf.slots = S + 1;
}

namespace {

// An inform query: request rows users[0 .. n_users) (host ids, rows of th: `slots` tables of ts doubles, [row][K])
// against every item.  seen (indexed by those ids): the items left out; cand[0 .. n_cand) (host; ascending, distinct
// item ids; null: every item): the candidate mask; xoff / xit (host, by request row, any order, repeats allowed; null:
// none): the query's own excluded items.
void inf_run(mmsbm_hip_ctx *c, const double *th, size_t ts, int64_t n_users, const int32_t *users, SeenLists seen,
             const int32_t *cand, int n_cand, const int64_t *xoff, const int32_t *xit, int n, int32_t *items,
             double *gains, int32_t *counts) {
  const InfSession &inf = *c->inf;
  const int I = c->ext_items, K = c->ext_k, R = c->n_ratings, S = inf.slots;
  c->last_ms[T_INFORM] = 0.f;
  if (I == 0 || n_users == 0 || (cand && n_cand == 0)) {  // (no column to score: every row is empty)
    top_n_blank(n_users, n, items, gains, counts);
    return;
  }
  hipStream_t st = c->stream;
  require_free_mem((cand ? static_cast<size_t>(I) : 0) +
                       (xoff ? (static_cast<size_t>(n_users) + 1 + DevCsr::entries(xoff, n_users)) * 4 : 0),
                   "inform: the candidate mask and the query's excluded items");
  DevBuf<uint8_t> dmask;
  DevCsr own;
  if (cand) {
    std::vector<uint8_t> hm(static_cast<size_t>(I), 0);
    for (int e = 0; e < n_cand; ++e) hm[static_cast<size_t>(cand[e])] = 1;
    dmask.upload(hm, st);
    HIP_CHECK(hipStreamSynchronize(st));  // (`hm` is a local)
  }
  if (xoff) own.upload(xoff, xit, n_users, st);
  const size_t hs = static_cast<size_t>(I) * K, qs = hs * R;
  top_n_run(c, I, n_users, users, n, "inform: a batch of users",
            [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
              LAUNCH(inf_score_kernel, tile_grid(I, nb, kInfTile), kBlock, 0, st, th, ts, inf.q.ptr, qs, inf.h.ptr, hs, ub, nb, I,
                     K, R, S, dmask.ptr, sc, static_cast<size_t>(I));
              exclude_seen(st, ub, nb, seen, sc, static_cast<size_t>(I));
              if (xoff) own_exclude_batch(st, own, b0, nb, nullptr, sc, static_cast<size_t>(I));
            },
            T_INFORM, items, gains, counts);
}

}  // namespace

void inform_query(mmsbm_hip_ctx *c, int64_t n_users, const int32_t *users, const int32_t *cand, int n_cand,
                  const int64_t *excl_offsets, const int32_t *excl_items, bool exclude_train, int n, int32_t *items,
                  double *gains, int32_t *counts) {
  use_device(c);
  InfSession &inf = *c->inf;
  if (exclude_train && !inf.seen_built) {  // every user's training items, built by the first query that leaves them out
    upload_train_lists(c, inf.seen_off, inf.seen, "inform: the users' training items");
    inf.seen_built = true;
  }
  inf_run(c, inf.th.ptr, static_cast<size_t>(c->ext_users) * c->ext_k, n_users, users,
          SeenLists{exclude_train ? inf.seen_off.ptr : nullptr, inf.seen.ptr}, cand, n_cand, excl_offsets, excl_items, n,
          items, gains, counts);
}

void inform_query_theta(mmsbm_hip_ctx *c, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                        const int32_t *seen_items, const int32_t *cand, int n_cand, int n, int32_t *items,
                        double *gains, int32_t *counts) {
  use_device(c);
  const int S = c->inf->slots;
  const size_t tk = static_cast<size_t>(n_users) * c->ext_k;
  require_free_mem(S * tk * sizeof(double) + (static_cast<size_t>(n_users) + 1 + DevCsr::entries(seen_offsets, n_users)) * 4,
                   "inform: the caller's theta rows");
  CallerRows rows(c, S, n_users, theta, seen_offsets, seen_items);
  inf_run(c, rows.th.ptr, tk, n_users, rows.ids.data(), rows.seen.lists(), cand, n_cand, nullptr, nullptr, n, items, gains,
          counts);
  HIP_CHECK(hipStreamSynchronize(c->stream));  // (the rows and the lists are locals)
}

void inform_mean_theta(mmsbm_hip_ctx *c, double *out) {
  use_device(c);
  const InfSession &inf = *c->inf;
  const size_t n = static_cast<size_t>(inf.slots) * c->ext_k;
  HIP_CHECK(hipMemcpyAsync(out, inf.mass.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  const double users = static_cast<double>(c->ext_users);
  for (size_t e = 0; e < n; ++e) out[e] /= users;  // (the masses were summed on the device: one division each)
}

// ---- the overlap of the restarts' groups (overlap.hpp) ---------------------------------------------------------------
void overlap_begin(mmsbm_hip_ctx *c, int side) {
  use_device(c);
  c->ov.reset();  // (from here on the previous session is gone)
  auto ov = std::make_unique<OvlSession>();
  ov->side = side;
  ov->rows = side == 0 ? c->ext_items : c->ext_users;
  ov->groups = side == 0 ? c->ext_l : c->ext_k;
  c->ov = std::move(ov);
}

void overlap_add(mmsbm_hip_ctx *c) {  // the selected slot (the caller holds a OneSlot)
  use_device(c);
  OvlSession &ov = *c->ov;
  const int S = ov.slots, G = ov.groups, rows = ov.rows;
  const size_t qs = static_cast<size_t>(rows) * G;
  require_free_mem((S + 1) * qs * sizeof(double), "overlap: the slots' membership tables");
  hipStream_t st = c->stream;
  DevBuf<double> nx;  // the table grows by one slot
  double *xo = grow_by_slot(ov.x, qs, S, st, nx);
  const ExtSlot e = ext_slot(c);
  if (qs > 0)  // the slot's rows as they are, external sides (rec_fold_kernel without a matrix)
    LAUNCH(rec_fold_kernel, static_cast<unsigned>((qs + kBlock - 1) / kBlock), kBlock, 0, st,
           ov.side == 0 ? e.items : e.users, G, nullptr, 0, 0, xo, rows, G);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));
  ov.x.swap(nx);
  ov.slots = S + 1;
}

void overlap_query(mmsbm_hip_ctx *c, double *out) {
  use_device(c);
  const OvlSession &ov = *c->ov;
  const int rows = ov.rows, G = ov.groups;
  const size_t F = static_cast<size_t>(ov.slots) * G, nt = (F + kOvlTile - 1) / kOvlTile, pairs = nt * (nt + 1) / 2;
  // B is a constant, so the number of slabs -- and with it the size of the partials -- follows from the rows alone
  const size_t slabs = static_cast<size_t>(std::max(1, (rows + kOvlSlab - 1) / kOvlSlab));
  const size_t tile = static_cast<size_t>(kOvlTile) * kOvlTile, outs = F * F;
  require_free_mem((slabs * pairs * tile + outs) * sizeof(double), "overlap: the slabs' partial results and the result");
  if (slabs * pairs > (size_t(1) << 26))  // (the grid: 2^26 tiles are 2 TB of partial results)
    throw ApiError(MMSBM_E_TOOLARGE, "overlap: " + std::to_string(slabs * pairs) + " partial tiles in one query");
  hipStream_t st = c->stream;
  DevBuf<double> part, res;
  part.alloc(slabs * pairs * tile);
  res.alloc(outs);
  EventPair ev;  // device time of the query's kernels (option "overlap_ms")
  ev.start(st);
  LAUNCH(ovl_gram_kernel, static_cast<unsigned>(slabs * pairs), kBlock, 0, st, ov.x.ptr, static_cast<size_t>(rows) * G,
         rows, G, static_cast<int>(F), static_cast<int>(nt), static_cast<int>(pairs), part.ptr);
  LAUNCH(ovl_combine_kernel, static_cast<unsigned>(pairs * (tile / kBlock)), kBlock, 0, st, part.ptr,
         static_cast<int>(slabs), static_cast<int>(F), static_cast<int>(nt), static_cast<int>(pairs), res.ptr);
  HIP_CHECK(hipGetLastError());
  ev.stop(st);
  HIP_CHECK(hipMemcpyAsync(out, res.ptr, sizeof(double) * outs, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_OVERLAP] = ev.ms();
}

}  // namespace mmsbm_hip_impl
