// serve_frame.hpp -- the frame every serving unit runs its queries in: what tu_recommend.hip, tu_rerank.hip, tu_pairs.hip,
// tu_market.hip and tu_similar.hip (and tu_explain.hip, for the two folds) share, and nothing else is shared between them.
// Every batched query runs in one frame (BatchFrame: the ids, the batch buffer, the loop, the event pair) and selects
// through one stage (SelectStage: the split's scratch and launches); a top-N query is the two together (top_n_device) and
// ends in one read-back (top_n_copy_out).  The round-based queries keep their round loops and share the loop over a
// round's batches (for_batches), the tile grid and the seen exclusion (tile_grid, exclude_seen).  The integer planning of
// the queries is serve_plan.hpp.
// Host side only: this header includes no kernel header and launches nothing.  The functions that are only declared here
// are tu_serve_frame.hip's -- the one unit that launches the kernels several query families share (recommend.hpp: the
// weights, the fold, the score tile, the seen exclusion, the selection; catalogue.hpp: the compact table and the
// exclusions by column) -- and a template that needs such a launch calls one of them.
// Included by the serving units after prelude.hpp.
#pragma once

namespace mmsbm_hip_impl {

// Every external user's distinct training items, ascending, onto the device (off [U + 1], item); returns the offsets.
// `what`: the memory is checked under that name first (null: no check).  The stream has passed the copies on return.
std::vector<int32_t> upload_train_lists(mmsbm_hip_ctx *c, DevBuf<int32_t> &d_off, DevBuf<int32_t> &d_item, const char *what);

// A query's lists by request row on the device: host int64 offsets [n_rows + 1] narrowed to int32 (checked: below
// 2^31) and the values behind them.  Holds the narrowed offsets for as long as it lives: the copies are asynchronous.
// Never uploaded: both pointers null ("no list").
struct DevCsr {
  DevBuf<int32_t> off, val;
  std::vector<int32_t> off_h;
  static int64_t entries(const RowCsr &lists, int64_t n_rows) { return lists.offsets && n_rows > 0 ? lists.offsets[n_rows] : 0; }
  void upload(const RowCsr &lists, int64_t n_rows, hipStream_t st);
  SeenLists lists() const { return {off.ptr, val.ptr}; }
};

// The rows a caller brings instead of the session's users: q.theta [S][n_users][K] on the device as it is, the identity
// ids 0 .. n_users - 1 (request row b is row b of every slot's block) and the caller's seen lists by row (no offsets:
// none).  The caller has checked the memory.  users(): the rows as a query of their own -- q's subset, no own lists.
struct CallerRows {
  DevBuf<double> th;
  std::vector<int32_t> ids;
  DevCsr seen;
  Subset cand;
  CallerRows(mmsbm_hip_ctx *c, int S, const ThetaQuery &q);
  UserQuery users() const { return {{static_cast<int64_t>(ids.size()), ids.data()}, cand, RowCsr{}}; }
};

// W [K][L] of a slot from its p (external sides: ExtSlot's p, rs, ks, ls) and the R rating weights w (device): the one
// launch site of rec_w_kernel (recommend_add, explain_add)
void fold_weights(hipStream_t st, const double *p, const double *w, double *out, int K, int L, int R, size_t rs, int ks, int ls);
// out [rows][rank] from the rows of a table d wide: the rows as they are (m null), or times the matrix m (strides mt, mj).
// The one launch site of rec_fold_kernel, in two forms of the source (RowTab is internal to every unit, so the table is
// named, not passed): a plain table src [rows][d] on the device -- new items' eta, a caller's theta rows --, and the
// selected slot's own rows in external terms (the caller holds a OneSlot; on the context's stream) -- `items_side`: the
// items' rows, L wide, else the users', K wide: the sessions' per-slot folds (recommend, inform, overlap, explain).
// No row or no column: nothing is launched.
void fold_rows(hipStream_t st, double *src, int d, const double *m, int mt, int mj, double *out, int rows, int rank);
void fold_rows(mmsbm_hip_ctx *c, bool items_side, const double *m, int mt, int mj, double *out, int rank);

// The grid of a kernel that writes a batch buffer in tiles: `cols` columns x `nb` rows, `tile` of each to a workgroup
inline dim3 tile_grid(int cols, int nb, int tile = kRecTile) {
  return dim3(static_cast<unsigned>((cols + tile - 1) / tile), static_cast<unsigned>((nb + tile - 1) / tile));
}

// -inf over the columns of sc [nb][ld] that `seen` (indexed by the rows' ids, device) leaves out; no lists: nothing
void exclude_seen(hipStream_t st, const int32_t *ids, int nb, SeenLists seen, double *sc, size_t ld);
// ... where the columns are those of a candidate list: col_of (device) is every item's column of sc (catalogue.hpp)
void exclude_seen_cols(hipStream_t st, const int32_t *ids, int nb, SeenLists seen, const int32_t *col_of, double *sc,
                       size_t ld);

// sc [nb][n_cols]: the scores of the rows ids[0 .. nb) (device) of table a (`slots` tables as doubles apart, [row][rank])
// against the rows 0 .. n_cols - 1 of table b; seen (indexed by those ids): the columns set to -inf.  fma is commutative
// in its factors, so the sides exchanged give (u, i) the same score bit for bit.
void score_tiles(mmsbm_hip_ctx *c, const double *a, size_t as, const double *b, size_t bs, int n_cols, const int32_t *ids,
                 int nb, SeenLists seen, double *sc);

// ... of one batch of users ub (rows of x) against the session's catalogue.  Shared by the selection and the positions.
void rec_score_batch(mmsbm_hip_ctx *c, const double *x, size_t xs, const int32_t *ub, int nb, SeenLists seen, double *sc);

// The query's own excluded items (catalogue.hpp) of the batch that begins at request row b0: own's lists are by
// request row; col_of (device): every item's column of sc, or null where the columns are the items
void own_exclude_batch(hipStream_t st, const DevCsr &own, int64_t b0, int nb, const int32_t *col_of, double *sc, size_t ld);

// Every row of a top-N answer as "no candidate": counts 0, ids -1, values -inf
void top_n_blank(int64_t n_rows, int n, const TopNOut &out);

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
inline SelectPlan select_plan(const mmsbm_hip_ctx *c, int cols, int64_t rows, int n) {
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
  void run(hipStream_t st, const SelectPlan &p, const double *sc, int nb, int n, double *os, int32_t *oi, int32_t *on) const;
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
                    const TopNOut &out, const int32_t *cand = nullptr, const double *dev_second = nullptr,
                    double *second = nullptr);

// top_n_device with the result copied to the host; `timed`: the timer that takes the device time of the query's kernels
template <class Fill>
void top_n_run(mmsbm_hip_ctx *c, int I, int64_t n_users, const int32_t *users, int n, const char *what, Fill &&fill,
               TimedCall timed, const TopNOut &out) {
  top_n_blank(n_users, n, out);
  if (n_users == 0) return;
  top_n_device(c, I, n_users, users, n, what, 0, fill, [&](const TopNDev &dev, EventPair &ev) {
    top_n_copy_out(c, dev, ev, n_users, n, timed, out);
  });
}

// The compact item table of a candidate subset (catalogue.hpp): the candidates on the device, every catalogue item's
// column and the candidates' rows of the session's item table, and the device time of the two kernels that make them
struct CatTable {
  DevBuf<int32_t> cand, col;  // [C]; [items of the catalogue]
  DevBuf<double> y;           // [slot][C][rank]
  float ms = 0.f;
  // the device memory of the table of a subset (the whole catalogue: no table)
  static size_t bytes(const RecSession &rc, const Subset &cand) {
    return cand.items ? static_cast<size_t>(rc.slots) * cand.n * rc.rank * sizeof(double) + (static_cast<size_t>(cand.n) + rc.items) * 4 : 0;
  }
};

// cand (host; its items given: ascending, distinct ids of the session's catalogue) -> t (the memory was found free by
// the caller)
void cat_table(mmsbm_hip_ctx *c, const Subset &cand, CatTable &t);

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

// q's subset and own lists as rec_within_device's: the memory is checked, the lists uploaded, the compact table made
void within_prepare(mmsbm_hip_ctx *c, const UserQuery &q, WithinPrep &w);

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
  else
    exclude_seen_cols(st, ub, nb, seen, w.ct.col.ptr, sc, static_cast<size_t>(C));
  if (w.has_own) own_exclude_batch(st, w.own, b0, nb, w.ct.col.ptr, sc, static_cast<size_t>(C));
}

// The device side of a recommend query q (host): within its candidates (ascending, distinct ids of the session's
// catalogue; no items: the whole catalogue), and with the query's own excluded items: row b of the request also leaves
// out q.excl's list b (any order, repeats allowed; no offsets: none).  catalogue.hpp.
// `tiles(y, ys, C, ub, nb, sc)` enqueues the kernel that writes the values sc [nb][C] of the batch's rows ub (device ids)
// against the C rows of the item table y (slots ys doubles apart: the catalogue's, or the candidates' compact table) --
// the score tiles of recommend_query (rec_tiles), the aggregate over the restarts (ensemble.hpp); seen (indexed by user
// id): the items left out after it.  The result stays on the device (top_n_device): `then(dev, ev, dcand, prep_ms)` gets
// it -- as COLUMNS of the candidate list when there is one --, the candidate list on the device (or null) and the device
// time of the compact table and the columns.  n_users > 0 and at least one column.  `after(w, ub, nb, sc)` (default:
// nothing) enqueues a stage of the query's own over the batch buffer behind the exclusions, before the selection: the
// capped categories of quota.hpp (in the buffer's columns; `capped` says so: the memory check then names the query as one
// within the candidates), the perturbation of explore.hpp; `each`: top_n_device's (explore.hpp uses both).
template <class Tiles, class Then, class After = NoFillStage, class Each = NoBatchStage>
void rec_within_device(mmsbm_hip_ctx *c, const UserQuery &q, SeenLists seen, int n, size_t extra, Tiles &&tiles,
                       Then &&then, After &&after = After{}, Each &&each = Each{}, bool capped = false) {
  WithinPrep w;
  within_prepare(c, q, w);
  top_n_device(c, w.C, q.users.n, q.users.ids, n,
               q.cand.items || q.excl.offsets || capped ? "recommend: a batch of users within the candidates" : "recommend: a batch of users", extra,
               [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
                 within_fill(c, w, tiles, seen, ub, nb, b0, sc);
                 after(w, ub, nb, sc);
               },
               [&](const TopNDev &dev, EventPair &ev) { then(dev, ev, w.dcand(), w.ct.ms); }, each);
}

// rec_within_device's `tiles` of recommend_query: the scores of the rows of x (`slots` tables xs doubles apart)
inline auto rec_tiles(mmsbm_hip_ctx *c, const double *x, size_t xs) {
  return [=](const double *y, size_t ys, int C, const int32_t *ub, int nb, double *sc) {
    score_tiles(c, x, xs, y, ys, C, ub, nb, SeenLists{}, sc);
  };
}

// rec_within_device with the result copied to the host (top_n_blank done by the caller), the columns as item ids; the device time of the query's kernels goes to `timed`.  No column or no row: every row stays empty.
// `after` / `capped`: rec_within_device's.
template <class Tiles, class After = NoFillStage>
void rec_within_run(mmsbm_hip_ctx *c, const UserQuery &q, SeenLists seen, int n, Tiles &&tiles, TimedCall timed,
                    const TopNOut &out, After &&after = After{}, bool capped = false) {
  c->last_ms[timed] = 0.f;
  if (q.cand.columns(c->rc->items) == 0 || q.users.n == 0) return;
  rec_within_device(c, q, seen, n, 0, tiles,
                    [&](const TopNDev &dev, EventPair &ev, const int32_t *, float prep_ms) {
                      top_n_copy_out(c, dev, ev, q.users.n, n, timed, out, q.cand.items);
                      c->last_ms[timed] += prep_ms;
                    },
                    after, NoBatchStage{}, capped);
}

// The caller's theta rows [S][n_users][K] folded exactly as recommend_add folds a slot's own theta (x = theta, or
// theta W when K > L), then `run(x, xs, users, seen)` over the rows 0 .. n_users - 1 as a query of their own
// (CallerRows::users) with the caller's seen lists
template <class Run>
void rec_theta_fold(mmsbm_hip_ctx *c, const ThetaQuery &q, Run &&run) {
  const int K = c->ext_k, L = c->ext_l, rank = c->rc->rank, S = c->rc->slots;
  const int64_t n_users = q.n_users;
  const size_t tk = static_cast<size_t>(n_users) * K, xs = static_cast<size_t>(n_users) * rank;
  require_free_mem(S * (tk + xs) * sizeof(double) +
                       (static_cast<size_t>(n_users) + 1 + DevCsr::entries(q.seen, n_users)) * 4,
                   "recommend: the caller's theta rows");
  hipStream_t st = c->stream;
  CallerRows rows(c, S, q);
  DevBuf<double> x;
  x.alloc(S * xs);
  const size_t kl = static_cast<size_t>(K) * L;
  for (int s = 0; s < S; ++s) {
    const double *m = K <= L ? nullptr : c->rc->wk.ptr + s * kl;
    fold_rows(st, rows.th.ptr + s * tk, K, m, L, 1, x.ptr + s * xs, static_cast<int>(n_users), rank);
  }
  HIP_CHECK(hipGetLastError());
  run(x.ptr, xs, rows.users(), rows.seen.lists());
}

}  // namespace mmsbm_hip_impl
