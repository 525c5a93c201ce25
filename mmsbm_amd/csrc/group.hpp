// group.hpp -- group recommendation inside an open recommend session (recommend.hpp): what a set of users should get
// together (mmsbm_hip_recommend_query_groups).  The request is the concatenation of the groups' members; a group's
// value for an item aggregates its members' scores:
//   MIN   (least misery)   agg(g, i) = min_m score(m, i)
//   MAX   (most pleasure)  agg(g, i) = max_m score(m, i)
//   COUNT (approval)       agg(g, i) = #{m : score(m, i) >= bar}, as a double
//   MEAN                   agg(g, i) = score of the group's mean row
// The first three are not bilinear in (theta, eta), so no score buffer of members x items is formed for them:
//   grp_tile_kernel<MODE>  one workgroup per (item tile of 128 columns, RUN of consecutive groups).  The host lays every
//                       group's members out in BLOCKS of 8 rows (the last block of a group padded: blk_info says how
//                       many of its rows are members), so the 8 rows a thread of rec_tile_acc holds belong to one
//                       group.  The workgroup walks its run 16 blocks (128 rows) at a time; per step the 8 x 8
//                       accumulators per thread come from rec_tile_acc as they are, the thread folds its block's MEMBER
//                       rows (masked BY INDEX a < members of the block: a padding row repeats a member's id only so that
//                       the load is in bounds, and the rows beyond the run come out as 0.0 -- either would win a MIN
//                       over positive scores, a MAX over negative ones and pass any bar <= 0; the identities are
//                       +inf / -inf / 0) into one value per column and writes it to LDS (16 blocks x 128 columns, in
//                       the x staging tile, which is free between two calls of rec_tile_acc).  Thread t < 128 then
//                       combines column t's 16 values in block order into a carry that lives in a register from one
//                       step to the next, and where a block is the last of its group stores agg[g][i0 + t] -- one
//                       division by S for MIN / MAX: the correctly rounded quotient is monotone, so the quotient of
//                       the smallest accumulator IS the smallest quotient, bit for bit (an accumulator is never -0.0:
//                       the chain starts from +0.0) -- and resets the carry.  Stores run along the items.
//                       COUNT compares the accumulator with gtop_floor_acc(bar, S) (top_pairs.hpp), as aud_decide does;
//                       where that answers -inf it divides and compares.  Counts are small integers: their sum is exact
//                       in any order.  min, max and the count do not depend on the shape of the reduction, so a group's
//                       value does not depend on where the group stands in the request, on the runs or on the batches.
//                       A group longer than a run is cut into FRAGMENTS, one run each, so that one large group fills
//                       the device too: a fragment's blocks carry kGrpPart and its undivided carry goes to a row of a
//                       partial buffer [fragments][items] instead;
//   grp_combine_kernel  joins the fragments' rows of every cut group in fragment order (the same min / max / sum) and
//                       writes agg[g][i], with the one division.  Launched only when a group of the batch was cut.
//   grp_exclude_kernel  -inf at agg[g][item] (or its column in a candidate subset) for every item ANY member of g has
//                       in the session's excluded lists.  One workgroup per block of members; several threads may store
//                       the same -inf to one address: a plain store of one value.
//   grp_mean_kernel     xbar[s][g][j] = (x_s[m_0, j] + x_s[m_1, j] + ...) / |g|: one chain from +0.0 in the request's
//                       member order.  rec_score_kernel then runs over xbar (its users are 0 .. G - 1): no new score
//                       code, and a group of one gets its member's row back (0.0 + x = x, x / 1 = x).
// Selection and merge: rec_select_kernel through top_n_run (serve_frame.hpp), rows = groups.  No atomics.
#pragma once

namespace {

constexpr int kGrpMin = MMSBM_HIP_GROUP_MIN, kGrpMax = MMSBM_HIP_GROUP_MAX, kGrpCount = MMSBM_HIP_GROUP_COUNT;
// (kGrpBlock, kGrpStep, kGrpLast, kGrpPart: serve_plan.hpp -- plan_groups writes what the kernels here read)
static_assert(kGrpStep <= kRecKc && kRecTile <= kRecLdsRow, "the blocks' partial values fit the x staging tile");

template <int MODE>
__device__ __forceinline__ double grp_identity() {
  return MODE == kGrpMin ? INFINITY : MODE == kGrpMax ? -INFINITY : 0.0;
}

template <int MODE>
__device__ __forceinline__ double grp_join(double a, double b) {
  if (MODE == kGrpMin) return b < a ? b : a;
  if (MODE == kGrpMax) return b > a ? b : a;
  return a + b;
}

// rows: the request's member rows, 8 per block (user ids; padding rows repeat a member); blk_info / blk_grp [block]:
// members of the block | kGrpLast on a group's (fragment's) last block | kGrpPart inside a fragment, and the group (row
// of agg, counted from g0) or the fragment (row of part, counted from p0); run_off: the runs' first blocks
// (run_off[r + 1]: one past the last), every run a whole number of groups or one fragment.  y: ni rows (the catalogue, or
// the compact table of a candidate subset).  agg and part have ld columns.  grid (item tiles, runs).
template <int MODE>
__global__ __launch_bounds__(kBlock) void grp_tile_kernel(const double *__restrict__ x, size_t xs,
                                                          const double *__restrict__ y, size_t ys,
                                                          const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ blk_info,
                                                          const int32_t *__restrict__ blk_grp,
                                                          const int32_t *__restrict__ run_off, int g0, int p0, int ni,
                                                          int rank, int slots, double bar, double *__restrict__ agg,
                                                          double *__restrict__ part, size_t ld) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * kRecTile;
  const int rb = run_off[blockIdx.y], re = run_off[blockIdx.y + 1];
  const double n_slots = static_cast<double>(slots);
  const double lo = MODE == kGrpCount ? gtop_floor_acc(bar, n_slots) : 0.0;
  const bool by_acc = lo > -INFINITY;  // (uniform)
  double carry = grp_identity<MODE>();  // column i0 + tid of the group under way (threads < 128)
  for (int t0 = rb; t0 < re; t0 += kGrpStep) {
    const int nblk = min(kGrpStep, re - t0);
    double acc[kRecTm][kRecTm];
    rec_tile_acc(x, xs, y, ys, rows + static_cast<size_t>(t0) * kGrpBlock, nblk * kGrpBlock, ni, rank, slots, 0, i0, tx,
                 ty, xt, yt, acc);
    // this thread's block: rows a < members, by index
    const int members = ty < nblk ? (blk_info[t0 + ty] & (kGrpLast - 1)) : 0;
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) {
      double v = grp_identity<MODE>();
#pragma unroll
      for (int a = 0; a < kRecTm; ++a) {
        if (a >= members) continue;
        if (MODE == kGrpCount)
          v += (by_acc ? acc[a][c] >= lo : acc[a][c] / n_slots >= bar) ? 1.0 : 0.0;
        else
          v = grp_join<MODE>(v, acc[a][c]);
      }
      xt[ty][tx + 16 * c] = v;
    }
    __syncthreads();
    if (tid < kRecTile) {
      const int i = i0 + tid;
      for (int b = 0; b < nblk; ++b) {
        carry = grp_join<MODE>(carry, xt[b][tid]);
        const int info = blk_info[t0 + b];
        if (info & kGrpLast) {
          if (i < ni) {
            if (info & kGrpPart)
              part[static_cast<size_t>(blk_grp[t0 + b] - p0) * ld + i] = carry;
            else
              agg[static_cast<size_t>(blk_grp[t0 + b] - g0) * ld + i] = MODE == kGrpCount ? carry : carry / n_slots;
          }
          carry = grp_identity<MODE>();
        }
      }
    }
    __syncthreads();  // (the next step stages into xt)
  }
}

// Cut group c = blockIdx.y of the batch: agg[(cut_grp[c] - g0) * ld + i] = the rows cut_off[c] .. cut_off[c + 1] of part
// (counted from p0) joined in that order -- min, max or sum by `mode` -- and, but for COUNT, divided by the slots.
// grid (columns / kBlock, cut groups).
__global__ __launch_bounds__(kBlock) void grp_combine_kernel(const double *__restrict__ part,
                                                             const int32_t *__restrict__ cut_grp,
                                                             const int32_t *__restrict__ cut_off, int g0, int p0, int ni,
                                                             int mode, int slots, double *__restrict__ agg, size_t ld) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= ni) return;
  const int c = blockIdx.y;
  double v = mode == kGrpMin ? INFINITY : mode == kGrpMax ? -INFINITY : 0.0;
  for (int f = cut_off[c]; f < cut_off[c + 1]; ++f) {
    const double w = part[static_cast<size_t>(f - p0) * ld + i];
    v = mode == kGrpMin ? grp_join<kGrpMin>(v, w) : mode == kGrpMax ? grp_join<kGrpMax>(v, w) : v + w;
  }
  agg[static_cast<size_t>(cut_grp[c] - g0) * ld + i] = mode == kGrpCount ? v : v / static_cast<double>(slots);
}

// Block blk0 + blockIdx.x of the request (blk_row: every block's group, cut or not): agg[(its group - g0) * ld + col] = -inf for every item its members have in
// seen_off / seen (by user id), col = col_of[item] (skipped when -1), or the item itself without col_of.
__global__ __launch_bounds__(kBlock) void grp_exclude_kernel(const int32_t *__restrict__ rows,
                                                             const int32_t *__restrict__ blk_info,
                                                             const int32_t *__restrict__ blk_row, int blk0, int g0,
                                                             const int32_t *__restrict__ seen_off,
                                                             const int32_t *__restrict__ seen_item,
                                                             const int32_t *__restrict__ col_of,
                                                             double *__restrict__ agg, size_t ld) {
  const int blk = blk0 + blockIdx.x;
  const int members = blk_info[blk] & (kGrpLast - 1);
  double *row = agg + static_cast<size_t>(blk_row[blk] - g0) * ld;
  for (int a = 0; a < members; ++a) {
    const int u = rows[static_cast<size_t>(blk) * kGrpBlock + a];
    for (int e = seen_off[u] + threadIdx.x; e < seen_off[u + 1]; e += kBlock) {
      const int col = col_of ? col_of[seen_item[e]] : seen_item[e];
      if (col >= 0) row[col] = -INFINITY;
    }
  }
}

// xbar[s * bs + g * rank + j] for groups g0 <= g < g0 + ng: the members' rows of table s added in member order from
// +0.0, divided by their number.  grp_blk[g]: the group's first block (its members are the first size[g] rows from
// there); bs: doubles between two slots' tables of xbar.
__global__ __launch_bounds__(kBlock) void grp_mean_kernel(const double *__restrict__ x, size_t xs, int rank, int slots,
                                                          const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ grp_blk,
                                                          const int32_t *__restrict__ size, int g0, int ng,
                                                          double *__restrict__ xbar, size_t bs) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const size_t per = static_cast<size_t>(ng) * rank;
  if (e >= per * slots) return;
  const size_t s = e / per, r = e - s * per;
  const int g = g0 + static_cast<int>(r / rank), j = static_cast<int>(r % rank);
  const int32_t *m = rows + static_cast<size_t>(grp_blk[g]) * kGrpBlock;
  const int cnt = size[g];
  double acc = 0.0;
  for (int k = 0; k < cnt; ++k) acc += x[s * xs + static_cast<size_t>(m[k]) * rank + j];
  xbar[s * bs + static_cast<size_t>(g) * rank + j] = acc / static_cast<double>(cnt);
}

}  // namespace
