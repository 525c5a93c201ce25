// mmsbm_hip.hip -- the C ABI of include/mmsbm_hip.h, and nothing else: every entry is its argument checks, the device
// and (for the single-restart entries) the selected slot, and ONE call into the unit that owns the work -- launch.hpp
// declares those calls.  What stays here: the exception-to-status wrapper with the last-error string, the guards the
// entries share (parameters present, a session open), the device-info entries
// (they have no context), pcg64_doubles and the host-only layout helpers of the CPU tests.  What a request's users,
// subsets, lists, categories and user sets must satisfy is abi_request.hpp's, host-only code, and so are the values a
// request crosses into the units as (UserQuery, ThetaQuery, Subset, RowCsr, Categories; TopNOut, ShelfOut, AssignOut): a
// serving entry opens its session, runs its own checks, builds the value, checks it -- in the order its refusals
// promise -- and makes the call with the value.
//
//   tu_create.hip   building a context, restart slots, the index read-back
//   tu_params.hip   parameters in and out, update_coefficients' fetch, result, snapshots
//   tu_iterate.hip  the EM iteration: its form, its order of launches, graph replay, the timers (the description of the
//                   algorithm is there)
//   tu_once.hip     likelihood, prod_dist / predict, compute_omegas, the random start
//   tu_options.hip  the option table
//   the serving queries, behind serve_frame.hpp (tu_serve_frame.hip: what they share):
//   tu_recommend.hip  the recommend session; within a subset, ranks, positions, quota, shelves
//   tu_rerank.hip     explore, ensemble, groups, diverse      tu_pairs.hip   top_pairs, top_pairs_bulk
//   tu_market.hip     the item side, allocate, assign, assortment
//   tu_similar.hip    similar, inform, overlap
//   tu_fold_in.hip, tu_heldout.hip, tu_explain.hip (explain, leave-one-out)   sessions outside the frame

#include "prelude.hpp"
#include "pcg64.hpp"

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

// ---- parameters present: of the selected slot; of every slot (the iteration advances all of them) -------------------
void require_params(const mmsbm_hip_ctx *c) {
  if (!c) throw std::invalid_argument("null context");
  if (!c->have[c->sel]) throw std::invalid_argument("set_params has not been called");
}
void require_all_params(const mmsbm_hip_ctx *c) {
  if (!c) throw std::invalid_argument("null context");
  for (int s = 0; s < c->n_slots; ++s)
    if (!c->have[s])
      throw std::invalid_argument(c->n_slots == 1 ? std::string("set_params has not been called")
                                                  : "set_params has not been called for slot " +
                                                        std::to_string(s));
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

static_assert(kErrUnsupported == MMSBM_E_UNSUPPORTED && kErrTooLarge == MMSBM_E_TOOLARGE &&
              kQueryMaxN == MMSBM_HIP_RECOMMEND_MAX_N, "abi_request.hpp stands alone: its copies of the header's numbers");

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
    *out = context_create(device, n_obs, n_users, n_items, n_ratings, k_groups, l_groups, user, item, rating, swap_sides);
  });
}

int mmsbm_hip_destroy(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    launch_log_flush();
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

// which: 0 .. 15 as mmsbm_hip_layout_array, 16 item_grid, 17 lik_units, 18 mv_chunk_off
int mmsbm_hip_index_array(mmsbm_hip_ctx *ctx, int which, int32_t *out, int64_t capacity, int64_t *count) {
  return guarded([&] {
    if (!ctx || !count) throw std::invalid_argument("null argument");
    index_array(ctx, which, out, capacity, count);
  });
}

int mmsbm_hip_set_params(mmsbm_hip_ctx *ctx, const double *theta, const double *eta,
                         const double *pr) {
  return guarded([&] {
    if (!ctx || !theta || !eta || !pr) throw std::invalid_argument("null argument");
    use_device(ctx);
    OneSlot one(ctx);
    set_params(ctx, theta, eta, pr);
  });
}

int mmsbm_hip_init_params(mmsbm_hip_ctx *ctx, const uint64_t pcg64_state[4], const double *pr) {
  return guarded([&] {
    if (!ctx || !pcg64_state || !pr) throw std::invalid_argument("null argument");
    use_device(ctx);
    OneSlot one(ctx);
    init_params(ctx, pcg64_state, pr);
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
    get_params(ctx, theta, eta, pr);
  });
}

int mmsbm_hip_set_slots(mmsbm_hip_ctx *ctx, int n_slots) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (n_slots < 1 || n_slots > 65535) throw std::invalid_argument("n_slots must be in [1, 65535]");
    use_device(ctx);
    set_slots(ctx, n_slots);
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
    update_coefficients(ctx, n_theta, n_eta, n_pr);
  });
}

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
    fetch_result(ctx, theta, eta, pr, likelihood);
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
    OneSlot one(ctx);
    compute_omegas(ctx, out, n_elems);
  });
}

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
    OneSlot one(ctx);
    prod_dist(ctx, n_pairs, user, item, out);
  });
}

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
    predict_begin(ctx, n_rows, user, item, rating, rating_weights);
  });
}

int mmsbm_hip_predict_add(mmsbm_hip_ctx *ctx, double stats[6]) {
  return guarded([&] {
    require_params(ctx);
    if (!stats) throw std::invalid_argument("null stats");
    require_open(ctx, &mmsbm_hip_ctx::ps, "predict");
    use_device(ctx);
    OneSlot one(ctx);
    predict_add(ctx, stats);
  });
}

int mmsbm_hip_predict_finish(mmsbm_hip_ctx *ctx, double *mean_dist, double stats[6]) {
  return guarded([&] {
    if (!ctx || !stats) throw std::invalid_argument("null argument");
    require_open(ctx, &mmsbm_hip_ctx::ps, "predict", "predict_finish");
    use_device(ctx);
    OneSlot one(ctx);
    predict_finish(ctx, mean_dist, stats);
  });
}

namespace {
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
    require_rows(n_users);
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend: user");
    recommend_query(ctx, {n_users, users}, n, {items, scores, counts});
  });
}

int mmsbm_hip_recommend_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::rc); }

int mmsbm_hip_recommend_query_theta(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                    const int64_t *seen_offsets, const int32_t *seen_items, int32_t n,
                                    int32_t *items, double *scores, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_theta");
    require_rows(n_users);
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!theta || !items)) throw std::invalid_argument("null argument");
    const ThetaQuery q = theta_query(n_users, theta, seen_offsets, seen_items, 0, nullptr);
    q.check(rc.items, "recommend_query_theta", "recommend");
    recommend_query_theta(ctx, q, n, {items, scores, counts});
  });
}

int mmsbm_hip_recommend_positions(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users,
                                  const int64_t *offsets, const int32_t *items, int32_t *positions,
                                  int32_t *candidates) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_positions");
    require_rows(n_users);
    if (n_users > 0 && (!users || !offsets)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend_positions: user");
    RowCsr{offsets, items, "offsets", "user", "items", "item id"}.check(n_users, rc.items, "recommend_positions");
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
    RowCsr{seen_offsets, seen_users, "seen_offsets", "item", "seen users", "seen user"}.check(n_new, ctx->ext_users,
                                                                                               "recommend_add_items");
    recommend_add_items(ctx, n_new, eta, seen_offsets, seen_users);
  });
}

int mmsbm_hip_recommend_top_pairs(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t m,
                                  int32_t *out_users, int32_t *out_items, double *out_scores, int32_t *count) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_top_pairs");
    require_rows(n_users);
    if (m < 1) throw std::invalid_argument("top_pairs: m must be at least 1");
    if (m > MMSBM_HIP_TOP_PAIRS_MAX_M)
      throw ApiError(MMSBM_E_UNSUPPORTED, "top_pairs: m = " + std::to_string(m) + " is beyond the " +
                                              std::to_string(MMSBM_HIP_TOP_PAIRS_MAX_M) + " pairs a query returns at most");
    if (!out_users || !out_items || !out_scores || !count) throw std::invalid_argument("null argument");
    const std::vector<int32_t> ids = sorted_user_set(users, n_users, ctx->ext_users, "top_pairs");
    recommend_top_pairs(ctx, static_cast<int64_t>(ids.size()), ids.data(), m, out_users, out_items, out_scores, count);
  });
}

namespace {

// The request of top_pairs_bulk / pair_bar checked, and in id order in `ids` (every training user when `users` is null)
void pairs_bulk_request(mmsbm_hip_ctx *ctx, const char *entry, int64_t n_users, const int32_t *users, int64_t m,
                        std::vector<int32_t> &ids) {
  require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", entry);
  require_rows(n_users);
  if (m < 1) throw std::invalid_argument("top_pairs_bulk: m must be at least 1");
  if (m > MMSBM_HIP_TOP_PAIRS_BULK_MAX_M)
    throw ApiError(MMSBM_E_UNSUPPORTED, "top_pairs_bulk: m = " + std::to_string(m) + " is beyond the " +
                                            std::to_string(MMSBM_HIP_TOP_PAIRS_BULK_MAX_M) + " pairs a query returns at most");
  ids = sorted_user_set(users, n_users, ctx->ext_users, "top_pairs_bulk");
}

}  // namespace

int mmsbm_hip_recommend_top_pairs_bulk(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int64_t m,
                                       int32_t *out_users, int32_t *out_items, double *out_scores, int64_t *count,
                                       double *bar, int64_t counts[3]) {
  return guarded([&] {
    std::vector<int32_t> ids;
    pairs_bulk_request(ctx, "recommend_top_pairs_bulk", n_users, users, m, ids);
    if (!out_users || !out_items || !out_scores || !count || !bar || !counts) throw std::invalid_argument("null argument");
    recommend_top_pairs_bulk(ctx, static_cast<int64_t>(ids.size()), ids.data(), m, out_users, out_items, out_scores, count,
                             bar, counts);
  });
}

int mmsbm_hip_recommend_pair_bar(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int64_t m, double *bar,
                                 int64_t counts[3]) {
  return guarded([&] {
    std::vector<int32_t> ids;
    pairs_bulk_request(ctx, "recommend_pair_bar", n_users, users, m, ids);
    if (!bar || !counts) throw std::invalid_argument("null argument");
    recommend_top_pairs_bulk(ctx, static_cast<int64_t>(ids.size()), ids.data(), m, nullptr, nullptr, nullptr, nullptr, bar,
                             counts);
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
    recommend_query_items(ctx, n_items, items, n, {users, scores, counts});
  });
}

int mmsbm_hip_recommend_allocate(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n,
                                 const int32_t *caps, int32_t max_rounds, int32_t *items, double *scores,
                                 int32_t *counts, int32_t *rounds, int32_t *converged) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_allocate");
    require_rows(n_users);
    require_n(n, "recommend_allocate", "items");
    if (max_rounds < 1) throw std::invalid_argument("recommend_allocate: max_rounds must be at least 1");
    if (!caps || !rounds || !converged || (n_users > 0 && !items)) throw std::invalid_argument("null argument");
    std::vector<int32_t> all;
    users = asked_once_user_set(users, n_users, ctx->ext_users, "recommend_allocate", all);
    const AllocPlan plan = plan_allocate(caps, rc.items, n_users, ctx->ext_users, MMSBM_HIP_RECOMMEND_MAX_N);
    if (plan.refused >= 0)
      throw ApiError(MMSBM_E_UNSUPPORTED, refused_cap("recommend_allocate", plan.refused, caps[plan.refused], n_users));
    recommend_allocate(ctx, {n_users, users}, n, plan, max_rounds, {items, scores, counts}, rounds, converged);
  });
}

int mmsbm_hip_recommend_assign(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, const int32_t *caps,
                               double reserve, double epsilon, int32_t max_rounds, int32_t *items, double *scores,
                               double *paid, double *pi, double *price, double *price_sum, int32_t *load,
                               int32_t *rounds, int32_t *converged) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_assign");
    require_rows(n_users);
    if (max_rounds < 1) throw std::invalid_argument("recommend_assign: max_rounds must be at least 1");
    if (!std::isfinite(epsilon) || !(epsilon > 0.0) || epsilon < (rc.w_max - rc.w_min) * 0x1p-40)
      throw std::invalid_argument("recommend_assign: epsilon must be finite, positive and at least (largest - smallest "
                                  "rating weight) x 2^-40");
    if (std::isnan(reserve) || reserve == INFINITY) throw std::invalid_argument("recommend_assign: reserve is NaN or +inf");
    if (!caps || !rounds || !converged || !price || !price_sum || !load || (n_users > 0 && (!items || !scores || !paid || !pi)))
      throw std::invalid_argument("null argument");
    std::vector<int32_t> all;
    users = asked_once_user_set(users, n_users, ctx->ext_users, "recommend_assign", all);
    const AssignPlan plan = plan_assign(caps, rc.items, n_users, MMSBM_HIP_RECOMMEND_MAX_N);
    if (plan.refused >= 0)
      throw ApiError(MMSBM_E_UNSUPPORTED, refused_cap("recommend_assign", plan.refused, caps[plan.refused], n_users,
                                                      " (or the slots are more than 2^31)"));
    recommend_assign(ctx, {n_users, users}, plan, reserve, epsilon, max_rounds,
                     {items, scores, paid, pi, price, price_sum, load, rounds, converged});
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

int mmsbm_hip_recommend_query_within(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                     const int32_t *cand_items, const int64_t *excl_offsets,
                                     const int32_t *excl_items, int32_t n, int32_t *items, double *scores,
                                     int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_within");
    require_rows(n_users);
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "recommend: user", rc.items, "recommend_query_within");
    recommend_query_within(ctx, q, n, {items, scores, counts});
  });
}

int mmsbm_hip_recommend_query_theta_within(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                           const int64_t *seen_offsets, const int32_t *seen_items, int32_t n_cand,
                                           const int32_t *cand_items, int32_t n, int32_t *items, double *scores,
                                           int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_theta_within");
    require_rows(n_users);
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!theta || !items)) throw std::invalid_argument("null argument");
    const ThetaQuery q = theta_query(n_users, theta, seen_offsets, seen_items, n_cand, cand_items);
    q.check(rc.items, "recommend_query_theta_within", "recommend");
    recommend_query_theta(ctx, q, n, {items, scores, counts});
  });
}

int mmsbm_hip_recommend_query_explore(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                      const int32_t *cand_items, const int64_t *excl_offsets,
                                      const int32_t *excl_items, int32_t n, double temperature,
                                      const uint64_t pcg64_state[4], int32_t *items, double *scores,
                                      double *propensity, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_explore");
    require_rows(n_users);
    require_n(n, "recommend_explore", "items");
    require_temperature(temperature, rc.w_min, rc.w_max, "recommend_query_explore");
    if (!pcg64_state || (n_users > 0 && (!users || !items))) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "recommend: user", rc.items, "recommend_query_explore");
    recommend_query_explore(ctx, q, n, temperature, pcg64_state, {items, scores, counts}, propensity);
  });
}

int mmsbm_hip_recommend_list_propensity(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                        const int32_t *cand_items, const int64_t *excl_offsets,
                                        const int32_t *excl_items, double temperature, const int64_t *list_offsets,
                                        const int32_t *list_items, double *scores, double *propensity) {
  return guarded([&] {
    const char *who = "recommend_list_propensity";
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", who);
    require_rows(n_users);
    require_temperature(temperature, rc.w_min, rc.w_max, who);
    if (n_users > 0 && (!users || !list_offsets)) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "recommend: user", rc.items, who);
    const RowCsr lists = listed_items(list_offsets, list_items).of_rows(n_users);
    lists.check(n_users, rc.items, who);
    if (n_users > 0 && list_offsets[n_users] > 0 && !propensity) throw std::invalid_argument("null argument");
    require_lists(lists, n_users, who);
    recommend_list_propensity(ctx, q, temperature, lists, scores, propensity);
  });
}

int mmsbm_hip_explore_noise(mmsbm_hip_ctx *ctx, const uint64_t pcg64_state[4], int64_t n_pairs, const int32_t *users,
                            const int32_t *items, double *r, double *g) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (n_pairs < 0) throw std::invalid_argument("negative n_pairs");
    if (!pcg64_state || (n_pairs > 0 && (!users || !items || !r || !g))) throw std::invalid_argument("null argument");
    for (int64_t p = 0; p < n_pairs; ++p)
      if (users[p] < 0 || items[p] < 0)
        throw std::invalid_argument("explore_noise: negative id at pair " + std::to_string(p));
    explore_noise(ctx, pcg64_state, n_pairs, users, items, r, g);
  });
}

int mmsbm_hip_recommend_query_quota(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                    const int32_t *cand_items, const int64_t *excl_offsets, const int32_t *excl_items,
                                    int64_t n_cats, const int64_t *cat_offsets, const int32_t *cat_items,
                                    const int32_t *cat_caps, int32_t n, int32_t *items, double *scores,
                                    int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_quota");
    require_rows(n_users);
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "recommend: user", rc.items, "recommend_query_quota");
    const Categories cats{n_cats, cat_offsets, cat_items, cat_caps};
    cats.check(rc.items, "recommend_query_quota");
    recommend_query_quota(ctx, q, cats, n, {items, scores, counts});
  });
}

int mmsbm_hip_recommend_query_theta_quota(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                          const int64_t *seen_offsets, const int32_t *seen_items, int32_t n_cand,
                                          const int32_t *cand_items, int64_t n_cats, const int64_t *cat_offsets,
                                          const int32_t *cat_items, const int32_t *cat_caps, int32_t n, int32_t *items,
                                          double *scores, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_theta_quota");
    require_rows(n_users);
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!theta || !items)) throw std::invalid_argument("null argument");
    const ThetaQuery q = theta_query(n_users, theta, seen_offsets, seen_items, n_cand, cand_items);
    q.check(rc.items, "recommend_query_theta_quota", "recommend");
    const Categories cats{n_cats, cat_offsets, cat_items, cat_caps};
    cats.check(rc.items, "recommend_query_theta_quota");
    recommend_query_theta_quota(ctx, q, cats, n, {items, scores, counts});
  });
}

int mmsbm_hip_recommend_query_shelves(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int32_t n_cand,
                                      const int32_t *cand_items, const int64_t *excl_offsets,
                                      const int32_t *excl_items, int64_t n_cats, const int64_t *cat_offsets,
                                      const int32_t *cat_items, int32_t depth, int32_t min_items, int32_t n_shelves,
                                      int32_t per_shelf, int32_t *shelf_cats, double *shelf_values,
                                      int32_t *shelf_available, int32_t *shelf_counts, int32_t *items, double *scores,
                                      int32_t *item_counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_shelves");
    require_rows(n_users);
    const ShelfAsk ask{depth, min_items, n_shelves, per_shelf};
    const ShelfOut out{shelf_cats, shelf_values, shelf_available, shelf_counts, items, scores, item_counts};
    require_shelf_ask(n_users, n_cats, ask, out, "recommend_query_shelves");
    if (n_users > 0 && !users) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "recommend: user", rc.items, "recommend_query_shelves");
    const Categories cats{n_cats, cat_offsets, cat_items, nullptr};
    cats.check(rc.items, "recommend_query_shelves", false);
    recommend_query_shelves(ctx, q, cats, ask, out);
  });
}

int mmsbm_hip_recommend_query_theta_shelves(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta,
                                            const int64_t *seen_offsets, const int32_t *seen_items, int32_t n_cand,
                                            const int32_t *cand_items, int64_t n_cats, const int64_t *cat_offsets,
                                            const int32_t *cat_items, int32_t depth, int32_t min_items,
                                            int32_t n_shelves, int32_t per_shelf, int32_t *shelf_cats,
                                            double *shelf_values, int32_t *shelf_available, int32_t *shelf_counts,
                                            int32_t *items, double *scores, int32_t *item_counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_theta_shelves");
    require_rows(n_users);
    const ShelfAsk ask{depth, min_items, n_shelves, per_shelf};
    const ShelfOut out{shelf_cats, shelf_values, shelf_available, shelf_counts, items, scores, item_counts};
    require_shelf_ask(n_users, n_cats, ask, out, "recommend_query_theta_shelves");
    if (n_users > 0 && !theta) throw std::invalid_argument("null argument");
    const ThetaQuery q = theta_query(n_users, theta, seen_offsets, seen_items, n_cand, cand_items);
    q.check(rc.items, "recommend_query_theta_shelves", "recommend");
    const Categories cats{n_cats, cat_offsets, cat_items, nullptr};
    cats.check(rc.items, "recommend_query_theta_shelves", false);
    recommend_query_theta_shelves(ctx, q, cats, ask, out);
  });
}

int mmsbm_hip_recommend_rank(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, const int64_t *offsets,
                             const int32_t *cand_items, int32_t n, int32_t *items, double *scores, int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_rank");
    require_rows(n_users);
    require_n(n, "recommend", "items");
    if (n_users > 0 && (!users || !offsets || !items)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend_rank: user");
    const RowCsr lists{offsets, cand_items, "offsets", "user", "candidate items", "candidate item id"};
    lists.check(n_users, rc.items, "recommend_rank");
    for (int64_t b = 0; b < n_users; ++b)
      require_candidates(cand_items + offsets[b], offsets[b], offsets[b + 1] - offsets[b], rc.items, "recommend_rank");
    recommend_rank(ctx, {n_users, users}, lists, n, {items, scores, counts});
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
    similar_query(ctx, n_rows, ids, n, {out_ids, distance, counts});
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
    require_rows(n_users);
    if (n < 1) throw std::invalid_argument("recommend_diverse: n must be at least 1");
    if (pool < n) throw std::invalid_argument("recommend_diverse: pool must be at least n");
    if (!std::isfinite(trade_off) || trade_off < 0.0)
      throw std::invalid_argument("recommend_diverse: trade_off must be finite and at least 0");
    require_n(pool, "recommend_diverse", "pool entries");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "recommend_diverse: user", rc.items, "recommend_diverse");
    recommend_diverse(ctx, q, n, pool, trade_off, {items, scores, counts}, distances);
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
    const RowCsr groups{offsets, members, "offsets", "group", "members", "member"};
    groups.check(n_groups, ctx->ext_users, "recommend_query_groups");
    require_distinct_members(offsets, members, n_groups, ctx->ext_users, "recommend_query_groups");
    const Subset cand{n_cand, cand_items};
    cand.check(rc.items, "recommend_query_groups");
    recommend_query_groups(ctx, n_groups, groups, mode, bar, cand, n, {items, scores, counts});
  });
}

int mmsbm_hip_recommend_assortment(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int mode, double level,
                                   int32_t n_given, const int32_t *given_items, int32_t n_cand,
                                   const int32_t *cand_items, int32_t c, int32_t *items, double *gains, int32_t *count,
                                   int32_t *stop, double *given_gains, int32_t *served_items, double *served_scores) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_assortment");
    require_rows(n_users);
    if (n_given < 0) throw std::invalid_argument("recommend_assortment: negative n_given");
    if (mode != MMSBM_HIP_ASSORT_BEST && mode != MMSBM_HIP_ASSORT_REACH)
      throw std::invalid_argument("recommend_assortment: unknown mode " + std::to_string(mode));
    if (!std::isfinite(level))
      throw std::invalid_argument(mode == MMSBM_HIP_ASSORT_BEST ? "recommend_assortment: floor must be finite"
                                                                : "recommend_assortment: bar must be finite");
    if (c < 0) throw std::invalid_argument("recommend_assortment: c must be at least 0");
    if (c > MMSBM_HIP_ASSORT_MAX_C)
      throw ApiError(MMSBM_E_UNSUPPORTED, "recommend_assortment: c = " + std::to_string(c) + " is beyond the " +
                                              std::to_string(MMSBM_HIP_ASSORT_MAX_C) + " items a query takes at most");
    if (!count || !stop || (n_users > 0 && (!users || !served_items || !served_scores)) ||
        (c > 0 && (!items || !gains)) || (n_given > 0 && (!given_items || !given_gains)))
      throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "recommend_assortment: user");
    for (int64_t m = 1; m < n_users; ++m)
      if (users[m] <= users[m - 1])
        throw std::invalid_argument("recommend_assortment: users must be strictly ascending (row " + std::to_string(m) + ")");
    require_ids(given_items, n_given, rc.items, "recommend_assortment: given item");
    const Subset cand{n_cand, cand_items};
    cand.check(rc.items, "recommend_assortment");
    recommend_assortment(ctx, {n_users, users}, mode, level, given_items, n_given, cand, c, items, gains, count, stop,
                         given_gains, served_items, served_scores);
  });
}

int mmsbm_hip_recommend_query_ensemble(mmsbm_hip_ctx *ctx, int64_t n_users, const int32_t *users, int mode, double risk,
                                       int32_t n_cand, const int32_t *cand_items, const int64_t *excl_offsets,
                                       const int32_t *excl_items, int32_t n, int32_t *items, double *scores,
                                       int32_t *counts) {
  return guarded([&] {
    const RecSession &rc = require_open(ctx, &mmsbm_hip_ctx::rc, "recommend", "recommend_query_ensemble");
    require_rows(n_users);
    if (mode != MMSBM_HIP_ENSEMBLE_MIN && mode != MMSBM_HIP_ENSEMBLE_MAX && mode != MMSBM_HIP_ENSEMBLE_LCB)
      throw std::invalid_argument("recommend_query_ensemble: unknown mode " + std::to_string(mode));
    if (mode == MMSBM_HIP_ENSEMBLE_LCB && !std::isfinite(risk))
      throw std::invalid_argument("recommend_query_ensemble: risk must be finite");
    require_n(n, "recommend_query_ensemble", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "recommend_query_ensemble: user", rc.items, "recommend_query_ensemble");
    recommend_query_ensemble(ctx, q, mode, risk, n, {items, scores, counts});
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
    require_rows(n_users);
    require_n(n, "inform", "items");
    if (n_users > 0 && (!users || !items)) throw std::invalid_argument("null argument");
    const UserQuery q = user_query(n_users, users, n_cand, cand_items, excl_offsets, excl_items);
    q.check(ctx->ext_users, "inform: user", ctx->ext_items, "inform_query");
    inform_query(ctx, q, exclude_train != 0, n, {items, gains, counts});
  });
}

int mmsbm_hip_inform_query_theta(mmsbm_hip_ctx *ctx, int64_t n_users, const double *theta, const int64_t *seen_offsets,
                                 const int32_t *seen_items, int32_t n_cand, const int32_t *cand_items, int32_t n,
                                 int32_t *items, double *gains, int32_t *counts) {
  return guarded([&] {
    const InfSession &inf = require_open(ctx, &mmsbm_hip_ctx::inf, "inform", "inform_query_theta");
    require_rows(n_users);
    require_n(n, "inform", "items");
    if (n_users > 0 && (!theta || !items)) throw std::invalid_argument("null argument");
    require_theta_entries(theta, static_cast<size_t>(inf.slots) * static_cast<size_t>(n_users) * ctx->ext_k, "inform");
    const ThetaQuery q = theta_query(n_users, theta, seen_offsets, seen_items, n_cand, cand_items);
    q.check(ctx->ext_items, "inform_query_theta", "inform");
    inform_query_theta(ctx, q, n, {items, gains, counts});
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
    require_rows(n_users);
    require_n(n, "explain", "rows");
    if (n_users > 0 && (!users || !offsets)) throw std::invalid_argument("null argument");
    require_ids(users, n_users, ctx->ext_users, "explain: user");
    RowCsr{offsets, items, "offsets", "user", "pairs", "item id"}.check(n_users, ctx->ext_items, "explain");
    if (n_users > 0 && offsets[n_users] > 0 && !hist_items) throw std::invalid_argument("null argument");
    if (n_users > 0 && offsets[n_users] * static_cast<int64_t>(n) > INT32_MAX)
      throw std::invalid_argument("explain: more than 2^31 - 1 entries in one query");
    explain_query(ctx, n_users, users, offsets, items, n, hist_items, hist_ratings, contribution, counts, explained,
                  score, degree);
  });
}

int mmsbm_hip_explain_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::ex); }

int mmsbm_hip_loo_begin(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (std::max(ctx->ext_k, ctx->ext_l) > MMSBM_HIP_FOLD_IN_MAX_K)
      throw ApiError(MMSBM_E_UNSUPPORTED, "loo: K = " + std::to_string(ctx->ext_k) + ", L = " + std::to_string(ctx->ext_l) +
                                              " is beyond the " + std::to_string(MMSBM_HIP_FOLD_IN_MAX_K) +
                                              " groups it is built for");
    if (ctx->n_obs > INT32_MAX) throw ApiError(MMSBM_E_UNSUPPORTED, "loo: n_obs must be below 2^31");
    loo_begin(ctx);
  });
}

int mmsbm_hip_loo_add(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    require_open(ctx, &mmsbm_hip_ctx::loo, "loo");
    OneSlot one(ctx);
    loo_add(ctx);
  });
}

int mmsbm_hip_loo_rows(mmsbm_hip_ctx *ctx, int64_t n_rows, const int64_t *rows, double *fitted, double *reliability) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::loo, "loo", "loo_rows");
    if (rows && n_rows < 0) throw std::invalid_argument("loo: negative n_rows");
    for (int64_t m = 0; rows && m < n_rows; ++m)
      if (rows[m] < 0 || rows[m] >= ctx->n_obs)
        throw std::invalid_argument("loo: row position out of range at entry " + std::to_string(m));
    loo_rows(ctx, n_rows, rows, fitted, reliability);
  });
}

int mmsbm_hip_loo_sides(mmsbm_hip_ctx *ctx, double *user_surprise, double *user_fitted_surprise,
                        double *item_surprise, double *item_fitted_surprise) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::loo, "loo", "loo_sides");
    loo_sides(ctx, user_surprise, user_fitted_surprise, item_surprise, item_fitted_surprise);
  });
}

int mmsbm_hip_loo_lowest(mmsbm_hip_ctx *ctx, int32_t m, const uint8_t *user_flags, const uint8_t *item_flags,
                         int64_t *rows, double *reliability, int32_t *count) {
  return guarded([&] {
    require_open(ctx, &mmsbm_hip_ctx::loo, "loo", "loo_lowest");
    if (m < 1 || m > MMSBM_HIP_LOO_MAX_M)
      throw std::invalid_argument("loo: m must be in 1 .. " + std::to_string(MMSBM_HIP_LOO_MAX_M));
    if (!rows || !reliability) throw std::invalid_argument("null argument");
    loo_lowest(ctx, m, user_flags, item_flags, rows, reliability, count);
  });
}

int mmsbm_hip_loo_end(mmsbm_hip_ctx *ctx) { return end_session(ctx, &mmsbm_hip_ctx::loo); }

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

int mmsbm_hip_snapshot_save(mmsbm_hip_ctx *ctx) {
  return guarded([&] {
    require_params(ctx);
    use_device(ctx);
    snapshot_save(ctx);
  });
}

int mmsbm_hip_snapshot_get(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr) {
  return guarded([&] {
    if (!ctx) throw std::invalid_argument("null context");
    if (ctx->snap_have.empty() || !ctx->snap_have[ctx->sel])
      throw std::invalid_argument("snapshot_get: nothing saved for the selected slot");
    use_device(ctx);
    snapshot_get(ctx, theta, eta, pr);
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
    *elapsed_ms = time_iterations(ctx, n_iters);
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
    profile_iterations(ctx, n_iters, mean_us, launches_per_iter);
  });
}

int mmsbm_hip_kernel_bytes(const mmsbm_hip_ctx *ctx, int index, int64_t *bytes_read,
                           int64_t *bytes_written) {
  return guarded([&] {
    if (!ctx || !bytes_read || !bytes_written) throw std::invalid_argument("null argument");
    kernel_bytes(ctx, index, bytes_read, bytes_written);
  });
}

// stage: a KernelId; in the diagnostic build (-DMMSBM_ABLATE) bits 8.. name the phases to skip
int mmsbm_hip_time_stage(mmsbm_hip_ctx *ctx, int stage, int reps, float *mean_us) {
  return guarded([&] {
    require_all_params(ctx);
    time_stage(ctx, stage, reps, mean_us);
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
    *value = get_option(ctx, name);
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
