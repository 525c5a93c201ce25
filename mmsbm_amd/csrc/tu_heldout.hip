// tu_heldout.hip -- translation unit of the held-out log-likelihood (heldout.hpp): the session's rows ordered by rating
// and cut into blocks once, then two launches per evaluation whatever the number of slots
#include "prelude.hpp"
#include "heldout.hpp"

namespace mmsbm_hip_impl {

namespace {

// (G, tile in LDS) for the shape: G lanes per row follow the wider of the two rows (group_code, shapes.hpp); the
// rating's tile is staged where the launch's LDS holds it
struct HoldForm {
  int lanes;
  bool plds;
  size_t lds;
};
HoldForm hold_form(const mmsbm_hip_ctx *c) {
  const int K = c->ext_k, L = c->ext_l;
  const int lanes = group_lanes(group_code(pad_dim(std::max(K, L))));
  const bool plds = hold_lds_doubles(K, L, true) * sizeof(double) <= kLdsMax;
  return HoldForm{lanes, plds, hold_lds_doubles(K, L, plds) * sizeof(double)};
}

template <class Kern>
void hold_launch(Kern kernel, const HoldForm &f, dim3 grid, hipStream_t st, const HoldArgs &a) {
  allow_big_lds(kernel, f.lds);
  LAUNCH(kernel, grid, kBlock, f.lds, st, a);
}

// out[s] = the n_parts block sums of slot s; the caller fetches `out` (hold_fetch) once its timing is closed
void hold_sums(mmsbm_hip_ctx *c, HoldSession &h, int n_slots, int n_parts) {
  LAUNCH(hold_sum_kernel, static_cast<unsigned>(n_slots), kBlock, 0, c->stream, h.part.ptr,
         static_cast<size_t>(std::max(h.n_blocks, 1)), n_parts, h.out.ptr);
  HIP_CHECK(hipGetLastError());
}
void hold_fetch(mmsbm_hip_ctx *c, HoldSession &h, int n_slots, double *loglik) {
  HIP_CHECK(hipMemcpyAsync(loglik, h.out.ptr, sizeof(double) * n_slots, hipMemcpyDeviceToHost, c->stream));
}

void hold_reserve(HoldSession &h, int n_slots) {  // block sums and results for n_slots slots
  if (h.part_slots >= n_slots) return;
  const size_t nb = static_cast<size_t>(std::max(h.n_blocks, 1));
  require_free_mem((nb + 1) * n_slots * sizeof(double), "heldout: the slots' block sums");
  h.part.alloc(nb * n_slots);
  h.out.alloc(n_slots);
  h.part_slots = n_slots;
}

}  // namespace

void heldout_begin(mmsbm_hip_ctx *c, int64_t n_rows, const int32_t *user, const int32_t *item, const int32_t *rating) {
  use_device(c);
  HIP_CHECK(hipStreamSynchronize(c->stream));
  c->ho.reset();  // (arguments are fine: from here on the previous session is gone)
  auto h = std::make_unique<HoldSession>();
  const size_t n = static_cast<size_t>(n_rows);
  // rating-major, a rating's rows in request order; blocks of at most kHoldRows rows of one rating
  std::vector<int32_t> su(n), si(n), so(n);
  const std::vector<int64_t> off = group_by_key<int64_t>(rating, n_rows, c->n_ratings, [&](int64_t m, int64_t at) {
    su[at] = user[m];
    si[at] = item[m];
    so[at] = static_cast<int32_t>(m);
  });
  std::vector<int4> blocks;
  for (int r = 0; r < c->n_ratings; ++r)
    for (int64_t b = off[r]; b < off[r + 1]; b += kHoldRows)
      blocks.push_back(make_int4(r, static_cast<int>(b), static_cast<int>(std::min<int64_t>(kHoldRows, off[r + 1] - b)), 0));
  require_free_mem(n * (3 * sizeof(int32_t) + 2 * sizeof(double)) + blocks.size() * (sizeof(int4) + sizeof(double)),
                   "heldout: the session's rows");
  hipStream_t s = c->stream;
  h->user.upload(su, s);
  h->item.upload(si, s);
  h->orig.upload(so, s);
  h->blocks.upload(blocks, s);
  h->sum.alloc(n);
  h->mean.alloc(n);
  HIP_CHECK(hipMemsetAsync(h->sum.ptr, 0, sizeof(double) * std::max<size_t>(n, 1), s));
  h->rows = n_rows;
  h->n_blocks = static_cast<int>(blocks.size());
  hold_reserve(*h, 1);
  HIP_CHECK(hipStreamSynchronize(s));  // (host vectors are locals)
  c->ho = std::move(h);
}

void heldout_eval(mmsbm_hip_ctx *c, int first, int n_slots, bool add, double *loglik) {
  use_device(c);
  HoldSession &h = *c->ho;
  hold_reserve(h, n_slots);
  hipStream_t st = c->stream;
  const HoldForm f = hold_form(c);
  const ExtSlot e = ext_slot(c, first);
  const HoldArgs a{e.users, e.items, e.p, c->p[c->cur].stride, e.rs, e.ks, e.ls, h.user.ptr, h.item.ptr, h.orig.ptr,
                   h.blocks.ptr, c->ext_k, c->ext_l, h.part.ptr, static_cast<size_t>(std::max(h.n_blocks, 1)),
                   add ? h.sum.ptr : nullptr};
  EventPair ev;
  ev.start(st);
  if (h.n_blocks > 0) {
    const dim3 grid(static_cast<unsigned>(h.n_blocks), static_cast<unsigned>(n_slots), 1);
    if (!f.plds) {  // (a tile beyond the LDS has a side beyond 128 groups: 64 lanes)
      if (f.lanes != 64) throw ApiError(MMSBM_E_INTERNAL, "heldout: no tile-free form for this shape");
      hold_launch(hold_rows_kernel<64, false>, f, grid, st, a);
    } else {
      switch (f.lanes) {
        case 4: hold_launch(hold_rows_kernel<4, true>, f, grid, st, a); break;
        case 8: hold_launch(hold_rows_kernel<8, true>, f, grid, st, a); break;
        case 16: hold_launch(hold_rows_kernel<16, true>, f, grid, st, a); break;
        case 32: hold_launch(hold_rows_kernel<32, true>, f, grid, st, a); break;
        default: hold_launch(hold_rows_kernel<64, true>, f, grid, st, a); break;
      }
    }
    HIP_CHECK(hipGetLastError());
  }
  hold_sums(c, h, n_slots, h.n_blocks);
  ev.stop(st);  // (the two launches: the copy of the results is not part of "heldout_ms")
  hold_fetch(c, h, n_slots, loglik);
  HIP_CHECK(hipStreamSynchronize(st));
  c->last_ms[T_HELDOUT] = ev.ms();
  if (add) h.slots++;
}

void heldout_mean(mmsbm_hip_ctx *c, double *mean_p, double *loglik) {
  use_device(c);
  HoldSession &h = *c->ho;
  hipStream_t st = c->stream;
  const int nb = static_cast<int>((h.rows + kHoldRows - 1) / kHoldRows);  // (<= n_blocks: a block holds at most kHoldRows)
  if (nb > 0) {
    LAUNCH(hold_mean_kernel, static_cast<unsigned>(nb), kBlock, 0, st, h.sum.ptr, h.rows, static_cast<double>(h.slots),
           h.mean.ptr, h.part.ptr);
    HIP_CHECK(hipGetLastError());
  }
  hold_sums(c, h, 1, nb);
  hold_fetch(c, h, 1, loglik);
  if (mean_p && h.rows > 0)
    HIP_CHECK(hipMemcpyAsync(mean_p, h.mean.ptr, sizeof(double) * h.rows, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace mmsbm_hip_impl
