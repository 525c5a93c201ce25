// tu_params.hip -- parameters in and out: host arrays (rows x groups, row-major; p as (K, L, R), external sides) <-> the
// device's tables (rows zero-padded and split into main + tail parts, RowTab; p as [R][kp][lp] with its transpose),
// staged through pinned memory.  Behind set_params / init_params / get_params, update_coefficients, result and the
// snapshots.  Host code only.
#include "prelude.hpp"

namespace mmsbm_hip_impl {

namespace {

// host (rows, d) row-major  <->  device RowTab (rows, dp) zero-padded, main + tail parts, staged
// through pinned memory in the one-slot layout (main rows, then tail rows): one contiguous copy when
// the context has one slot, a strided (2-D) copy per part when the slots' rows are interleaved
bool tab_is_packed(const RowTab &t, int rows) {
  return t.rs_m == t.mw && t.rs_t == t.tw && (t.tw == 0 || t.tail == t.main + static_cast<size_t>(rows) * t.mw);
}
void copy_rows(mmsbm_hip_ctx *c, const RowTab &t, double *stage, int rows, bool to_device) {
  const size_t e = sizeof(double);
  hipStream_t xs = c->xfer ? c->xfer : c->stream;
  if (rows == 0) return;
  if (tab_is_packed(t, rows)) {
    if (to_device)
      HIP_CHECK(hipMemcpyAsync(t.main, stage, e * rows * (t.mw + t.tw), hipMemcpyHostToDevice, xs));
    else
      HIP_CHECK(hipMemcpyAsync(stage, t.main, e * rows * (t.mw + t.tw), hipMemcpyDeviceToHost, xs));
    return;
  }
  double *stage_t = stage + static_cast<size_t>(rows) * t.mw;
  if (to_device) {
    HIP_CHECK(hipMemcpy2DAsync(t.main, e * t.rs_m, stage, e * t.mw, e * t.mw, rows, hipMemcpyHostToDevice, xs));
    if (t.tw > 0)
      HIP_CHECK(hipMemcpy2DAsync(t.tail, e * t.rs_t, stage_t, e * t.tw, e * t.tw, rows, hipMemcpyHostToDevice, xs));
  } else {
    HIP_CHECK(hipMemcpy2DAsync(stage, e * t.mw, t.main, e * t.rs_m, e * t.mw, rows, hipMemcpyDeviceToHost, xs));
    if (t.tw > 0)
      HIP_CHECK(hipMemcpy2DAsync(stage_t, e * t.tw, t.tail, e * t.rs_t, e * t.tw, rows, hipMemcpyDeviceToHost, xs));
  }
}
void zero_rows(mmsbm_hip_ctx *c, const RowTab &t, int rows) {
  const size_t e = sizeof(double);
  if (rows == 0) return;
  if (tab_is_packed(t, rows)) {
    HIP_CHECK(hipMemsetAsync(t.main, 0, e * rows * (t.mw + t.tw), c->stream));
    return;
  }
  HIP_CHECK(hipMemset2DAsync(t.main, e * t.rs_m, 0, e * t.mw, rows, c->stream));
  if (t.tw > 0) HIP_CHECK(hipMemset2DAsync(t.tail, e * t.rs_t, 0, e * t.tw, rows, c->stream));
}
void upload_rows(mmsbm_hip_ctx *c, const RowTab &t, const double *host, int rows, int d) {
  const int dp = t.mw + t.tw, mw = t.mw, tw = t.tw;
  double *stage = c->pin.take(static_cast<size_t>(rows) * dp);
  double *tail = stage + static_cast<size_t>(rows) * mw;
  const int wm = std::min(d, mw), wt = std::max(0, d - mw);
  for_row_blocks(rows, dp, [=](int a, int b) {
    for (int r = a; r < b; ++r) {
      const double *src = host + static_cast<size_t>(r) * d;
      double *m = stage + static_cast<size_t>(r) * mw;
      std::memcpy(m, src, sizeof(double) * wm);
      for (int j = wm; j < mw; ++j) m[j] = 0.0;
      if (tw > 0) {
        double *tl = tail + static_cast<size_t>(r) * tw;
        std::memcpy(tl, src + mw, sizeof(double) * wt);
        for (int j = wt; j < tw; ++j) tl[j] = 0.0;
      }
    }
  });
  copy_rows(c, t, stage, rows, true);
}
// enqueue the device -> pinned copy; unpack_rows after the stream has been synchronised
double *download_rows(mmsbm_hip_ctx *c, const RowTab &t, int rows) {
  const int dp = t.mw + t.tw;
  double *stage = c->pin.take(static_cast<size_t>(rows) * dp);
  copy_rows(c, t, stage, rows, false);
  return stage;
}
void unpack_rows(double *host, const double *stage, const RowTab &t, int rows, int d) {
  const int dp = t.mw + t.tw, mw = t.mw, tw = t.tw;
  const double *tail = stage + static_cast<size_t>(rows) * mw;
  const int wm = std::min(d, mw), wt = std::max(0, d - mw);
  for_row_blocks(rows, dp, [=](int a, int b) {
    for (int r = a; r < b; ++r) {
      double *dst = host + static_cast<size_t>(r) * d;
      std::memcpy(dst, stage + static_cast<size_t>(r) * mw, sizeof(double) * wm);
      if (tw > 0 && wt > 0) std::memcpy(dst + mw, tail + static_cast<size_t>(r) * tw, sizeof(double) * wt);
    }
  });
}
size_t tile_doubles(const mmsbm_hip_ctx *c) { return static_cast<size_t>(c->n_ratings) * c->kp * c->lp; }  // p, or pT
size_t rows_doubles(const mmsbm_hip_ctx *c) {  // staging for theta + eta + p + pT of one slot
  return static_cast<size_t>(c->n_users) * c->kp + static_cast<size_t>(c->n_items) * c->lp + 2 * tile_doubles(c);
}

// device p layout [R][kp][lp] (internal k, l)  <->  host pr (K, L, R) external
void p_host_to_dev(const mmsbm_hip_ctx *c, const double *pr, double *p, double *pt) {
  const int R = c->n_ratings, K = c->k, L = c->l, kp = c->kp, lp = c->lp;
  std::fill(p, p + static_cast<size_t>(R) * kp * lp, 0.0);
  std::fill(pt, pt + static_cast<size_t>(R) * kp * lp, 0.0);
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < L; ++l)
      for (int r = 0; r < R; ++r) {
        // internal (k,l) == external (l,k) when swapped
        const size_t h = c->swapped ? (static_cast<size_t>(l) * c->ext_l + k) * R + r
                                    : (static_cast<size_t>(k) * c->ext_l + l) * R + r;
        const double v = pr[h];
        p[(static_cast<size_t>(r) * kp + k) * lp + l] = v;
        pt[(static_cast<size_t>(r) * lp + l) * kp + k] = v;
      }
}
void p_dev_to_host(const mmsbm_hip_ctx *c, const double *p, double *pr) {
  const int R = c->n_ratings, K = c->k, L = c->l, kp = c->kp, lp = c->lp;
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < L; ++l)
      for (int r = 0; r < R; ++r) {
        const size_t h = c->swapped ? (static_cast<size_t>(l) * c->ext_l + k) * R + r
                                    : (static_cast<size_t>(k) * c->ext_l + l) * R + r;
        pr[h] = p[(static_cast<size_t>(r) * kp + k) * lp + l];
      }
}

// p and pT of the selected slot from the host's pr, onto the context's stream; the staging area (reset by the caller)
// has room for both
void upload_p(mmsbm_hip_ctx *c, const double *pr) {
  const size_t klr = tile_doubles(c);
  double *p = c->pin.take(klr), *pt = c->pin.take(klr);
  p_host_to_dev(c, pr, p, pt);
  HIP_CHECK(hipMemcpyAsync(c->p[c->cur].at(c->sel), p, sizeof(double) * klr, hipMemcpyHostToDevice, c->stream));
  HIP_CHECK(hipMemcpyAsync(c->pt[c->cur].at(c->sel), pt, sizeof(double) * klr, hipMemcpyHostToDevice, c->stream));
}

// The selected slot's tables are filled and enqueued: A of them, wait (the staging area is free again), mark the slot
void params_arrived(mmsbm_hip_ctx *c) {
  stage_matvec_a(c, c->cur, c->cur);
  HIP_CHECK(hipStreamSynchronize(c->stream));
  c->have[c->sel] = 1;
  c->a_ok[c->sel] = 1;
}

// (theta, eta, p) tables of one slot -> host arrays in host layout, the caller's (external) sides; any output may be null
void fetch_params(mmsbm_hip_ctx *c, const RowTab &tt, const RowTab &et, const double *p_dev,
                  double *ext_theta, double *ext_eta, double *pr) {
  const auto [theta, eta] = internal_sides(c, ext_theta, ext_eta);
  hipStream_t xs = c->xfer ? c->xfer : c->stream;
  HIP_CHECK(hipStreamSynchronize(xs));
  c->pin.reset(rows_doubles(c));
  const size_t klr = tile_doubles(c);
  const double *st = theta ? download_rows(c, tt, c->n_users) : nullptr;
  const double *se = eta ? download_rows(c, et, c->n_items) : nullptr;
  double *sp = nullptr;
  if (pr) {
    sp = c->pin.take(klr);
    HIP_CHECK(hipMemcpyAsync(sp, p_dev, sizeof(double) * klr, hipMemcpyDeviceToHost, xs));
  }
  HIP_CHECK(hipStreamSynchronize(xs));
  if (theta) unpack_rows(theta, st, tt, c->n_users, c->k);
  if (eta) unpack_rows(eta, se, et, c->n_items, c->l);
  if (pr) p_dev_to_host(c, sp, pr);
}

// the snapshot tables as theta_tab / eta_tab see the parameters of slot `slot`
RowTab snap_theta_tab(const mmsbm_hip_ctx *c, int slot) {
  return gather_tab(c, c->snap_theta.ptr, static_cast<size_t>(c->n_users), slot);
}

}  // namespace

void set_params(mmsbm_hip_ctx *ctx, const double *theta, const double *eta, const double *pr) {
  const auto [it, ie] = internal_sides(ctx, theta, eta);  // internal theta rows = internal users
  HIP_CHECK(hipStreamSynchronize(ctx->stream));  // nothing in flight still reads the staging area
  ctx->pin.reset(rows_doubles(ctx));
  upload_rows(ctx, theta_tab(ctx, ctx->cur), it, ctx->n_users, ctx->k);
  upload_rows(ctx, eta_tab(ctx, ctx->cur), ie, ctx->n_items, ctx->l);
  upload_p(ctx, pr);
  params_arrived(ctx);
}

void init_params(mmsbm_hip_ctx *ctx, const uint64_t pcg64_state[4], const double *pr) {
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->pin.reset(2 * tile_doubles(ctx));
  upload_p(ctx, pr);
  zero_rows(ctx, theta_tab(ctx, ctx->cur), ctx->n_users);  // padding columns
  zero_rows(ctx, eta_tab(ctx, ctx->cur), ctx->n_items);
  init_rows_launch(ctx, pcg64_state);
  params_arrived(ctx);
}

void get_params(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr) {
  const int cur = ctx->cur;
  fetch_params(ctx, theta_tab(ctx, cur), eta_tab(ctx, cur), ctx->p[cur].at(ctx->sel), theta, eta, pr);
}

void update_coefficients(mmsbm_hip_ctx *ctx, double *n_theta, double *n_eta, double *n_pr) {
  launch_iteration(ctx, false);
  const int nxt = ctx->cur ^ 1;
  fetch_params(ctx, theta_tab(ctx, nxt), eta_tab(ctx, nxt), ctx->npr.at(ctx->sel), n_theta, n_eta, n_pr);
}

void fetch_result(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr, double *likelihood) {
  HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the parameters are final
  const int nb = likelihood_enqueue(ctx);        // the likelihood kernels run ...
  struct Xfer {                                   // ... while the tables travel on the copy stream and are unpacked
    mmsbm_hip_ctx *c;
    explicit Xfer(mmsbm_hip_ctx *x) : c(x) { c->xfer = c->copy_stream; }
    ~Xfer() { c->xfer = nullptr; }
  };
  {
    Xfer on(ctx);
    get_params(ctx, theta, eta, pr);
  }
  *likelihood = likelihood_finish(ctx, nb);
}

void snapshot_save(mmsbm_hip_ctx *c) {
  const int cur = c->cur, sl = c->sel;
  const size_t klr = tile_doubles(c);
  if (c->snap_have.empty()) {
    const size_t doubles = c->theta[cur].count + c->eta[cur].count + c->p[cur].count;
    require_free_mem(doubles * sizeof(double), "snapshot: a copy of every slot's parameters");
    try {
      c->snap_theta.alloc(c->theta[cur].count);
      c->snap_eta.alloc_slots(static_cast<size_t>(c->n_items) * c->lp, c->n_slots);
      c->snap_p.alloc_slots(klr, c->n_slots);
    } catch (...) {
      c->drop_snapshots();
      throw;
    }
    c->snap_have.assign(static_cast<size_t>(c->n_slots), 0);
  }
  hipStream_t s = c->stream;
  const size_t e = sizeof(double);
  const RowTab src = gather_tab(c, c->theta[cur].ptr, static_cast<size_t>(c->n_users), sl), dst = snap_theta_tab(c, sl);
  if (c->n_users > 0) {  // the slot's columns of the interleaved rows: main parts, then tail parts
    HIP_CHECK(hipMemcpy2DAsync(dst.main, e * dst.rs_m, src.main, e * src.rs_m, e * src.mw, c->n_users,
                               hipMemcpyDeviceToDevice, s));
    if (src.tw > 0)
      HIP_CHECK(hipMemcpy2DAsync(dst.tail, e * dst.rs_t, src.tail, e * src.rs_t, e * src.tw, c->n_users,
                                 hipMemcpyDeviceToDevice, s));
  }
  HIP_CHECK(hipMemcpyAsync(c->snap_eta.at(sl), c->eta[cur].at(sl), e * static_cast<size_t>(c->n_items) * c->lp,
                           hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(c->snap_p.at(sl), c->p[cur].at(sl), e * klr, hipMemcpyDeviceToDevice, s));
  c->snap_have[sl] = 1;
}

void snapshot_get(mmsbm_hip_ctx *ctx, double *theta, double *eta, double *pr) {
  const int sl = ctx->sel;
  fetch_params(ctx, snap_theta_tab(ctx, sl), plain_tab(ctx->snap_eta.at(sl), ctx->lp), ctx->snap_p.at(sl), theta, eta, pr);
}

}  // namespace mmsbm_hip_impl
