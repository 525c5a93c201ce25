// tu_similar.hip -- translation unit of the sessions beside the recommend session that are built from a slot's rating
// profiles and group masses or from its rows as they are, and of their queries, in the frame of serve_frame.hpp
//   similar.hpp    nearest items / users: a session of its own, the same batches and selection
//   inform.hpp     the most informative items of a user: a session of its own (similar.hpp's profiles and masses) behind
//                  a score kernel of its own
//   overlap.hpp    the overlap of the restarts' groups: a session that copies a slot's rows (fold_rows)
#include "prelude.hpp"
#include "serve_frame.hpp"
#include "similar.hpp"
#include "inform.hpp"
#include "overlap.hpp"

namespace mmsbm_hip_impl {

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

void similar_query(mmsbm_hip_ctx *c, int64_t n_rows, const int32_t *ids, int n, const TopNOut &out) {
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
            T_SIMILAR, out);
  // the buffer held -D (the selection's order): the distances, +inf behind the last one (a zero leaves as +0.0)
  for (size_t e = 0; out.scores && e < static_cast<size_t>(n_rows) * n; ++e) out.scores[e] = -out.scores[e];
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
  fold_rows(c, false, nullptr, 0, 0, to, K);  // the users' rows as they are, external sides (no matrix)
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

// An inform query: the request rows of q (host ids, rows of th: `slots` tables of ts doubles, [row][K]) against every
// item.  seen (indexed by those ids): the items left out; q's subset: the candidate mask; its own lists (by request row,
// any order, repeats allowed): the query's own excluded items.  out.scores: the gains.
void inf_run(mmsbm_hip_ctx *c, const double *th, size_t ts, const UserQuery &q, SeenLists seen, int n, const TopNOut &out) {
  const InfSession &inf = *c->inf;
  const int I = c->ext_items, K = c->ext_k, R = c->n_ratings, S = inf.slots;
  const int64_t n_users = q.users.n;
  const int32_t *cand = q.cand.items;
  const bool own_lists = q.excl.offsets != nullptr;
  c->last_ms[T_INFORM] = 0.f;
  if (I == 0 || n_users == 0 || q.cand.columns(I) == 0) {  // (no column to score: every row is empty)
    top_n_blank(n_users, n, out);
    return;
  }
  hipStream_t st = c->stream;
  require_free_mem((cand ? static_cast<size_t>(I) : 0) +
                       (own_lists ? (static_cast<size_t>(n_users) + 1 + DevCsr::entries(q.excl, n_users)) * 4 : 0),
                   "inform: the candidate mask and the query's excluded items");
  DevBuf<uint8_t> dmask;
  DevCsr own;
  if (cand) {
    std::vector<uint8_t> hm(static_cast<size_t>(I), 0);
    for (int e = 0; e < q.cand.n; ++e) hm[static_cast<size_t>(cand[e])] = 1;
    dmask.upload(hm, st);
    HIP_CHECK(hipStreamSynchronize(st));  // (`hm` is a local)
  }
  if (own_lists) own.upload(q.excl, n_users, st);
  const size_t hs = static_cast<size_t>(I) * K, qs = hs * R;
  top_n_run(c, I, n_users, q.users.ids, n, "inform: a batch of users",
            [&](const int32_t *ub, int nb, int64_t b0, double *sc) {
              LAUNCH(inf_score_kernel, tile_grid(I, nb, kInfTile), kBlock, 0, st, th, ts, inf.q.ptr, qs, inf.h.ptr, hs, ub, nb, I,
                     K, R, S, dmask.ptr, sc, static_cast<size_t>(I));
              exclude_seen(st, ub, nb, seen, sc, static_cast<size_t>(I));
              if (own_lists) own_exclude_batch(st, own, b0, nb, nullptr, sc, static_cast<size_t>(I));
            },
            T_INFORM, out);
}

}  // namespace

void inform_query(mmsbm_hip_ctx *c, const UserQuery &q, bool exclude_train, int n, const TopNOut &out) {
  use_device(c);
  InfSession &inf = *c->inf;
  if (exclude_train && !inf.seen_built) {  // every user's training items, built by the first query that leaves them out
    upload_train_lists(c, inf.seen_off, inf.seen, "inform: the users' training items");
    inf.seen_built = true;
  }
  inf_run(c, inf.th.ptr, static_cast<size_t>(c->ext_users) * c->ext_k, q,
          SeenLists{exclude_train ? inf.seen_off.ptr : nullptr, inf.seen.ptr}, n, out);
}

void inform_query_theta(mmsbm_hip_ctx *c, const ThetaQuery &q, int n, const TopNOut &out) {
  use_device(c);
  const int S = c->inf->slots;
  const size_t tk = static_cast<size_t>(q.n_users) * c->ext_k;
  require_free_mem(S * tk * sizeof(double) + (static_cast<size_t>(q.n_users) + 1 + DevCsr::entries(q.seen, q.n_users)) * 4,
                   "inform: the caller's theta rows");
  CallerRows rows(c, S, q);
  inf_run(c, rows.th.ptr, tk, rows.users(), rows.seen.lists(), n, out);
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
  fold_rows(c, ov.side == 0, nullptr, 0, 0, xo, G);  // the slot's rows as they are, external sides (no matrix)
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
