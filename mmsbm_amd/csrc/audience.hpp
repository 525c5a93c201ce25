// audience.hpp -- item-side serving inside an open recommend session (recommend.hpp): who should see an item.
//
//   mmsbm_hip_recommend_query_items   the n best users of each requested item.  No kernel of its own: the session's
//                       item table takes the x side of rec_score_kernel (rows = the requested item ids), the user table
//                       the y side, the batch buffer has U columns, rec_exclude_kernel runs over the item -> users
//                       lists, and top_n_run selects (serve_frame.hpp).  fma(a, b, c) is commutative in a, b, so the
//                       exchanged tables give the bits of recommend_query.
//   mmsbm_hip_recommend_audience      every candidate user of an item whose score reaches a bar, as a CSR, without a
//                       score buffer (the answer holds anything from nothing to U x items entries):
//     aud_tile_kernel<WRITE = false>  COUNT.  A workgroup walks 128 x 128 tiles (item rows x user columns) of the batch;
//                       per tile the 8 x 8 accumulators per thread come from rec_tile_acc (items on the x side) and stay
//                       in registers.  A pair passes if its row and column are inside the request (masked BY INDEX: the
//                       accumulators outside are 0.0 and would pass any bar <= 0), its final score -- the quotient --
//                       is >= min_score, and its user is not in the item's ascending excluded list (binary search, only
//                       for pairs that passed the score test).  The division is not done per pair: gtop_floor_acc
//                       (top_pairs.hpp) gives the smallest accumulator whose quotient reaches the bar, verified, so
//                       acc >= lo IS the decision; where it answers -inf the kernel divides and compares.
//                       Positions come from wave ballots: for a fixed row (ty, a) and fixed c the 16 lanes of the ty group
//                       hold users tx + 16 c in lane order, so the row's 16-bit field of the ballot of "passes" ranks
//                       the lane among the passing users of that c, and the fields' popcounts over c = 0 .. 7 give the
//                       rest: in-tile position = ascending user id, the running total = the tile's count.  No atomics,
//                       no LDS, no barrier.  cnt[tile][row] = the count (int32).
//     aud_offsets_kernel              per row of the batch: cnt -> exclusive offsets in user-tile order, and the row's
//                       total.  Integers, one thread per row: no atomics.
//     aud_tile_kernel<WRITE = true>   the same decision code; a passing pair goes to out[base(row) + offset(row, tile)
//                       + position] as (user id, acc / S).
// Determinism: a pair's decision depends on the pair alone; its place in the output is (row, user tile, rank inside the
// tile), all three functions of the ids, so the result does not depend on the batches, on the order in which tiles
// are walked or on the number of workgroups.
#pragma once

namespace {

// One tile's decisions.  `pass`: bit a * 8 + c set when pair (row b0 + ty * 8 + a, user i0 + tx + 16 c) is in.
// items: the batch's item ids (rows of x); ex_off / ex: the excluded users per item id, ascending, or null.
__device__ __forceinline__ uint64_t aud_decide(const double (&acc)[kRecTm][kRecTm], const int32_t *__restrict__ items,
                                               int nb, int nu, int b0, int i0, int tx, int ty, double min_score,
                                               double lo, double n_slots, const int32_t *__restrict__ ex_off,
                                               const int32_t *__restrict__ ex) {
  uint32_t cols = 0;
#pragma unroll
  for (int c = 0; c < kRecTm; ++c) cols |= (i0 + tx + 16 * c < nu ? 1u : 0u) << c;
  uint64_t pass = 0;
  const bool by_acc = lo > -INFINITY;  // (uniform)
#pragma unroll
  for (int a = 0; a < kRecTm; ++a) {
    if (b0 + ty * kRecTm + a >= nb) continue;
    uint32_t row = 0;
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) {
      const bool ok = by_acc ? acc[a][c] >= lo : acc[a][c] / n_slots >= min_score;
      row |= (ok ? 1u : 0u) << c;
    }
    pass |= static_cast<uint64_t>(row & cols) << (kRecTm * a);
  }
  if (!ex_off) return pass;
  // the excluded list: only for what passed the score test
#pragma unroll
  for (int a = 0; a < kRecTm; ++a) {
    uint32_t rb = static_cast<uint32_t>(pass >> (kRecTm * a)) & 0xffu;
    if (rb == 0) continue;
    const int it = items[b0 + ty * kRecTm + a];
    const int beg = ex_off[it], end = ex_off[it + 1];
    if (beg == end) continue;
    uint32_t drop = 0;
    for (; rb != 0; rb &= rb - 1) {
      const int c = __ffs(static_cast<int>(rb)) - 1, u = i0 + tx + 16 * c;
      int p = beg, q = end;
      while (p < q) {
        const int mid = (p + q) >> 1;
        if (ex[mid] < u) p = mid + 1; else q = mid;
      }
      if (p < end && ex[p] == u) drop |= 1u << c;
    }
    pass &= ~(static_cast<uint64_t>(drop) << (kRecTm * a));
  }
  return pass;
}

// COUNT (WRITE = false): cnt[tile * ld + row] = passing pairs of batch row `row` in user tile `tile`.
// WRITE: cnt holds the exclusive offsets aud_offsets_kernel made of those counts; pair -> out_u / out_s
//        [row_base[row] - base0 + cnt[tile * ld + row] + position] (out_cap entries).
// x / xs: the session's item table (rows = items[0 .. nb)), y / ys: the user table (nu rows); rank, slots as
// rec_score_kernel.  grid: any number of workgroups <= tiles; tile t = row tile t / n_ut, user tile t % n_ut.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void aud_tile_kernel(const double *__restrict__ x, size_t xs,
                                                          const double *__restrict__ y, size_t ys,
                                                          const int32_t *__restrict__ items, int nb, int nu, int rank,
                                                          int slots, const int32_t *__restrict__ ex_off,
                                                          const int32_t *__restrict__ ex, double min_score,
                                                          int32_t *__restrict__ cnt, size_t ld,
                                                          const int64_t *__restrict__ row_base, int64_t base0,
                                                          int32_t *__restrict__ out_u, double *__restrict__ out_s,
                                                          int64_t out_cap) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int field = (tid % kRecWave) / 16 * 16;  // this ty group's 16 bits of a wave ballot
  const double n_slots = static_cast<double>(slots);
  const double lo = gtop_floor_acc(min_score, n_slots);
  const long long n_ut = (nu + kRecTile - 1) / kRecTile, n_rt = (nb + kRecTile - 1) / kRecTile;
  const long long T = n_ut * n_rt;
  for (long long t = blockIdx.x; t < T; t += gridDim.x) {
    const int ut = static_cast<int>(t % n_ut);
    const int b0 = static_cast<int>(t / n_ut) * kRecTile, i0 = ut * kRecTile;
    double acc[kRecTm][kRecTm];
    rec_tile_acc(x, xs, y, ys, items, nb, nu, rank, slots, b0, i0, tx, ty, xt, yt, acc);
    const uint64_t pass = aud_decide(acc, items, nb, nu, b0, i0, tx, ty, min_score, lo, n_slots, ex_off, ex);
#pragma unroll
    for (int a = 0; a < kRecTm; ++a) {
      const int b = b0 + ty * kRecTm + a;
      int run = 0;  // passing users of this row below the current c (the same in the 16 lanes of the ty group)
      int64_t at = 0;
      if (WRITE && b < nb) at = row_base[b] - base0 + cnt[static_cast<size_t>(ut) * ld + b];
#pragma unroll
      for (int c = 0; c < kRecTm; ++c) {
        const bool ok = (pass >> (kRecTm * a + c)) & 1u;
        const uint32_t f = static_cast<uint32_t>(__ballot(ok) >> field) & 0xffffu;
        if (WRITE && ok) {
          const int64_t o = at + run + __popc(f & ((1u << tx) - 1u));
          if (o < out_cap) {  // (always: the counts are this code's own; the buffer's bound all the same)
            out_u[o] = i0 + tx + 16 * c;
            out_s[o] = acc[a][c] / n_slots;
          }
        }
        run += __popc(f);
      }
      if (!WRITE && tx == 0 && b < nb) cnt[static_cast<size_t>(ut) * ld + b] = run;
    }
  }
}

// cnt[tile * ld + row], tile < n_ut: counts -> exclusive offsets in tile order; total[row] = their sum.  One thread
// per row of the batch.
__global__ __launch_bounds__(kBlock) void aud_offsets_kernel(int32_t *__restrict__ cnt, size_t ld, int n_ut, int nb,
                                                             int32_t *__restrict__ total) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= nb) return;
  int run = 0;
  for (int t = 0; t < n_ut; ++t) {
    const size_t e = static_cast<size_t>(t) * ld + b;
    const int v = cnt[e];
    cnt[e] = run;
    run += v;
  }
  total[b] = run;
}

}  // namespace
