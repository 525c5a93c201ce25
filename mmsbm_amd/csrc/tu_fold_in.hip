// tu_fold_in.hip -- translation unit of fold-in (fold_in.hpp), new users and new items alike: the request's rows grouped
// by new user (item), batches within the scratch budget, the jobs of the two forms and their launches
#include "prelude.hpp"
#include "fold_in.hpp"

namespace mmsbm_hip_impl {

namespace {

constexpr size_t kFoldBatchBytes = size_t(128) << 20;  // the v rows of one batch of users (as recommend's score buffer)

template <class T>
void fold_upload(DevBuf<T> &b, const T *h, size_t n, hipStream_t s) {
  if (n > 0) HIP_CHECK(hipMemcpyAsync(b.ptr, h, n * sizeof(T), hipMemcpyHostToDevice, s));
}

}  // namespace

// Both sides of fold-in (mmsbm_hip_fold_in / mmsbm_hip_fold_in_items): the new rows' own ids `own` (user, or item for
// items_side) in [0, n_new), the fitted side's ids `other`.  Users: groups K, fixed rows the external items' eta, p as
// (k, l).  Items: groups L, fixed rows the external users' theta, p read as (l, k) -- v_j[l] = sum_k p[k, l, r_j]
// theta[u_j, k] is fold_v_kernel with the strides and the group counts exchanged.  Everything below is the same for both.
void fold_in(mmsbm_hip_ctx *c, bool items_side, int64_t n_rows, const int32_t *user, const int32_t *item,
             const int32_t *rating, int32_t n_new, int32_t n_iters, double tol, const double *x0, double *x,
             int32_t *iters) {
  use_device(c);
  const int32_t *own = items_side ? item : user, *other = items_side ? user : item;
  const int K = items_side ? c->ext_l : c->ext_k, L = items_side ? c->ext_k : c->ext_l;  // (own, fixed) group counts
  const int code = fold_code(K), G = fold_lanes(code);
  // rows grouped by new user / item ("user" below; a user's rows keep the order of the request)
  std::vector<int32_t> it(static_cast<size_t>(n_rows)), rt(static_cast<size_t>(n_rows));
  const std::vector<int64_t> off = group_by_key<int64_t>(own, n_rows, n_new, [&](int64_t m, int64_t at) {
    it[at] = other[m];
    rt[at] = rating[m];
  });
  const size_t nk = static_cast<size_t>(n_new) * K;
  std::vector<double> th0(nk);
  if (x0) std::copy(x0, x0 + nk, th0.begin());
  else std::fill(th0.begin(), th0.end(), 1.0 / K);
  // batches: consecutive users whose v rows fit kFoldBatchBytes (a user beyond it: a batch of its own)
  const size_t row_b = static_cast<size_t>(K) * sizeof(double);
  std::vector<int32_t> cut{0};
  size_t max_rows = 0, max_users = 0;
  for (int32_t u = 0; u < n_new; ++u) {
    const int32_t b = cut.back();
    const size_t rows = static_cast<size_t>(off[u + 1] - off[b]);
    if (u > b && rows * row_b > kFoldBatchBytes) {
      max_rows = std::max(max_rows, static_cast<size_t>(off[u] - off[b]));
      max_users = std::max(max_users, static_cast<size_t>(u - b));
      cut.push_back(u);
    }
  }
  if (n_new > 0) {
    max_rows = std::max(max_rows, static_cast<size_t>(off[n_new] - off[cut.back()]));
    max_users = std::max(max_users, static_cast<size_t>(n_new - cut.back()));
  }
  cut.push_back(n_new);
  const size_t max_jobs = max_users * (kFoldWave / G) + 1;
  require_free_mem(max_rows * (row_b + 8) + max_users * (2 * row_b + 12) + 2 * max_jobs * sizeof(int2),
                   "fold_in: a batch of users");
  hipStream_t st = c->stream;
  DevBuf<int32_t> di, dr, dn;
  DevBuf<int64_t> doff;
  DevBuf<double> dv, dt0, dt;
  DevBuf<int2> jon, jst;
  di.alloc(max_rows); dr.alloc(max_rows); dv.alloc(max_rows * K);
  doff.alloc(max_users + 1); dt0.alloc(max_users * K); dt.alloc(max_users * K); dn.alloc(max_users);
  jon.alloc(max_jobs); jst.alloc(max_jobs);
  // external (k, l, r) of the slot's p (exchanged for items), the fixed side's external rows: the external items'
  // (internal users when swapped) for users, the external users' (internal items when swapped) for items
  const ExtSlot e = ext_slot(c);
  const int ks = items_side ? e.ls : e.ks, ls = items_side ? e.ks : e.ls;
  const RowTab et = items_side ? e.users : e.items;
  float total_ms = 0.f;
  EventPair ev;
  for (size_t bi = 0; bi + 1 < cut.size(); ++bi) {
    const int32_t u0 = cut[bi], u1 = cut[bi + 1], nb = u1 - u0;
    if (nb == 0) continue;
    const int64_t r0 = off[u0], nr = off[u1] - r0;
    std::vector<int64_t> boff(static_cast<size_t>(nb) + 1);
    for (int32_t b = 0; b <= nb; ++b) boff[b] = off[u0 + b] - r0;
    // the jobs: packed LDS groups (rows on chip) and one wave per streamed user
    const int gpw = kFoldWave / G;
    std::vector<int2> on, str;
    int used = 0, groups = gpw, lds_max = 0;
    for (int32_t b = 0; b < nb; ++b) {
      const int64_t d = boff[b + 1] - boff[b];
      if (d == 0) continue;
      if (fold_onchip(d, K)) {
        const int need = static_cast<int>(d) * K;
        if (groups == gpw || used + need > kFoldWaveLds) {
          on.resize(on.size() + gpw, make_int2(-1, 0));
          used = 0;
          groups = 0;
        }
        on[on.size() - gpw + groups] = make_int2(b, used);
        ++groups;
        used += need;
        lds_max = std::max(lds_max, used);
      } else {
        str.push_back(make_int2(b, 0));
      }
    }
    fold_upload(di, it.data() + r0, static_cast<size_t>(nr), st);
    fold_upload(dr, rt.data() + r0, static_cast<size_t>(nr), st);
    fold_upload(doff, boff.data(), boff.size(), st);
    fold_upload(dt0, th0.data() + static_cast<size_t>(u0) * K, static_cast<size_t>(nb) * K, st);
    fold_upload(jon, on.data(), on.size(), st);
    fold_upload(jst, str.data(), str.size(), st);
    ev.start(st);
    const size_t ve = static_cast<size_t>(nr) * K;
    if (ve > 0)
      LAUNCH(fold_v_kernel, static_cast<unsigned>((ve + kBlock - 1) / kBlock), kBlock, 0, st, et, e.p, e.rs,
             ks, ls, di.ptr, dr.ptr, nr, K, L, dv.ptr);
    const unsigned n_on = static_cast<unsigned>(on.size() / gpw), n_st = static_cast<unsigned>(str.size());
    const size_t lds = static_cast<size_t>(lds_max) * sizeof(double);
#define FOLD_CALL(GG, NT)                                                                                            \
  do {                                                                                                             \
    if (n_on > 0)                                                                                                  \
      LAUNCH((fold_kernel<GG, NT, 1, true>), n_on, kFoldWave, lds, st, jon.ptr, doff.ptr, dv.ptr, dt0.ptr, dt.ptr,  \
             dn.ptr, K, n_iters, tol);                                                                             \
    if (n_st > 0)                                                                                                  \
      LAUNCH((fold_kernel<GG, NT, kFoldWave / GG, false>), n_st, kFoldWave, 0, st, jst.ptr, doff.ptr, dv.ptr,      \
             dt0.ptr, dt.ptr, dn.ptr, K, n_iters, tol);                                                            \
  } while (0)
    DISPATCH_FOLD(code, FOLD_CALL);
#undef FOLD_CALL
    HIP_CHECK(hipGetLastError());
    ev.stop(st);
    std::vector<double> ht(static_cast<size_t>(nb) * K);
    std::vector<int32_t> hn(static_cast<size_t>(nb));
    if (!ht.empty()) HIP_CHECK(hipMemcpyAsync(ht.data(), dt.ptr, ht.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hn.data(), dn.ptr, hn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    total_ms += ev.ms();
    for (int32_t b = 0; b < nb; ++b) {  // a user without rows: theta0 and 0 iterations
      const bool empty = boff[b + 1] == boff[b];
      const double *src = empty ? th0.data() + static_cast<size_t>(u0 + b) * K : ht.data() + static_cast<size_t>(b) * K;
      std::copy(src, src + K, x + static_cast<size_t>(u0 + b) * K);
      if (iters) iters[u0 + b] = empty ? 0 : hn[b];
    }
  }
  c->last_ms[T_FOLD_IN] = total_ms;
}

}  // namespace mmsbm_hip_impl
