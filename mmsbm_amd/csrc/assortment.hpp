// assortment.hpp -- greedy assortment selection inside an open recommend session (recommend.hpp): which c items serve a
// set of users best TOGETHER (mmsbm_hip_recommend_assortment).  With a(u, i) the undivided accumulator of the score
// tile (score = a / S) and a per-user state carried from round to round, a round's gain of candidate i is
//   BEST   (best score)   gain(i) = sum_u max(0, a(u, i) - best[u])          best[u] starts at floor x S
//   REACH  (reach)        gain(i) = #{u not covered : a(u, i) / S >= bar}    as a double
// over the ELIGIBLE pairs (i not in u's excluded list of the session); the item of largest gain is taken (equal gains:
// the smallest item id), the state is advanced with it, and the next round follows on the stream:
//   asrt_gain_kernel<MODE>  one workgroup per (item tile of 128 columns, RUN of user rows).  The rows are the request's
//                       users ascending by id; a run is a whole number of 128-row steps (plan_assortment).  Per step the
//                       8 x 8 accumulators per thread come from rec_tile_acc as they are; rows beyond the request and
//                       columns beyond the table are masked BY INDEX (their accumulators are 0.0, which would beat a
//                       negative best and pass any bar <= 0); each row's state is loaded once per step; a pair whose
//                       term is not zero -- and only such a pair -- then has the user's ascending excluded list searched
//                       (as gtop_fused_kernel does for its survivors) and drops out when the item is in it.  The thread
//                       folds its 8 rows in row order into one value per column, from +0.0, and writes it to LDS (16
//                       blocks x 128 columns, in the x staging tile, free between two calls of rec_tile_acc); thread
//                       t < 128 adds column t's 16 values in block order to a carry that lives in a register across the
//                       steps of the run, and stores it to part[run][column] at the end.  Every addition's place is
//                       fixed by the plan; nothing is subtracted after the fact.  Terms are >= +0.0, so a masked term
//                       (0.0) leaves a sum's bits as they are.
//   asrt_join_kernel    one thread per column: the runs' rows added in run order from +0.0, -inf where the column is
//                       given or chosen already, then the best (value, column) of the workgroup's 256 columns -- larger
//                       value, equal values by the smaller column (columns ascend with the item ids) -- to blk[block].
//   asrt_pick_kernel    one workgroup: the best of the blocks' entries, same order.  -inf: no candidate is left (stop
//                       2); not > 0: no gain (stop 1); else (column, gain sum) is appended to the result, the column is
//                       marked as taken and the count goes up.  The stop flag stays set: every kernel of a later round
//                       reads it first and returns at once (a uniform exit), so the rounds are enqueued without a host
//                       wait in between and nothing is read back until the end.
//   asrt_update_kernel<MODE>  one thread per user row and one item -- round k's pick, read from the result on the
//                       device, or a given item: a(u, i*) by THE chain of rec_tile_acc (f = s * rank + j ascending from
//                       +0.0: the bits the gain kernel compared), the eligibility test, then BEST: best[u] = a and
//                       served[u] = i* where a > best[u] (strictly: the earliest item that reaches a user's best keeps
//                       them); REACH: where u is not covered and reaches the bar, served[u] = i* and best[u] = a.
//   asrt_given_kernel   a given item's gain over the state before it: its column of the runs' rows added in run order
//                       (the gain kernel ran over its one item tile of the catalogue), kept undivided.
//   asrt_finish_kernel  the one division by S of what leaves the device: the rounds' and the given items' gain sums
//                       (BEST) and every served user's accumulator.
// REACH compares the accumulator with gtop_floor_acc(bar, S) (top_pairs.hpp), as COUNT of group.hpp and aud_decide do;
// where that answers -inf it divides and compares.  No atomics.
#pragma once

namespace {

constexpr int kAsrtBest = MMSBM_HIP_ASSORT_BEST, kAsrtReach = MMSBM_HIP_ASSORT_REACH;
constexpr int kAsrtMaxC = MMSBM_HIP_ASSORT_MAX_C;
// (kAsrtNoGain, kAsrtNoCand, the runs and the batches: serve_plan.hpp -- plan_assortment lays out what the kernels walk)
static_assert(kGrpStep <= kRecKc && kRecTile <= kRecLdsRow, "the blocks' partial values fit the x staging tile");
static_assert(kAsrtNoGain == MMSBM_HIP_ASSORT_STOP_NO_GAIN && kAsrtNoCand == MMSBM_HIP_ASSORT_STOP_NO_CANDIDATES &&
                  MMSBM_HIP_ASSORT_STOP_C == 0 && kAsrtJoin == kBlock,
              "the stop flag is the stop reason; a joining workgroup takes one column per thread");

// Is `item` in the ascending list seen[lo .. hi)?
__device__ __forceinline__ bool asrt_seen(const int32_t *__restrict__ seen, int lo, int hi, int item) {
  int p = lo, q = hi;
  while (p < q) {
    const int mid = (p + q) >> 1;
    if (seen[mid] < item) p = mid + 1; else q = mid;
  }
  return p < hi && seen[p] == item;
}

// Does the accumulator reach the bar?  lo: gtop_floor_acc(bar, S), or -inf where the division decides
__device__ __forceinline__ bool asrt_reaches(double acc, double lo, bool by_acc, double n_slots, double bar) {
  return by_acc ? acc >= lo : acc / n_slots >= bar;
}

// rows [n_rows]: the request's users ascending; run blockIdx.y walks the rows [y * run_rows, min(n_rows, + run_rows)),
// run_rows a multiple of 128.  y: ni rows (the catalogue, or the compact table of a candidate subset; cand: the columns'
// item ids, or null where the columns are the items); the launch covers the item tiles from tile0 on, part [runs][ld]
// holds their columns counted from tile0 * 128.  level: the bar (REACH).  best / served [n_rows]: the state.  seen_off /
// seen: the session's excluded items per user id (ascending), or null.  grid (item tiles of the batch, runs).
template <int MODE>
__global__ __launch_bounds__(kBlock) void asrt_gain_kernel(const double *__restrict__ x, size_t xs,
                                                           const double *__restrict__ y, size_t ys,
                                                           const int32_t *__restrict__ rows, int n_rows, int run_rows,
                                                           int ni, int tile0, int rank, int slots, double level,
                                                           const double *__restrict__ best,
                                                           const int32_t *__restrict__ served,
                                                           const int32_t *__restrict__ seen_off,
                                                           const int32_t *__restrict__ seen,
                                                           const int32_t *__restrict__ cand,
                                                           const int32_t *__restrict__ stop, double *__restrict__ part,
                                                           size_t ld) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  if (*stop != 0) return;  // (uniform: the query has stopped)
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = (tile0 + static_cast<int>(blockIdx.x)) * kRecTile;
  const int rb = static_cast<int>(blockIdx.y) * run_rows, re = min(n_rows, rb + run_rows);
  const double n_slots = static_cast<double>(slots);
  const double lo = MODE == kAsrtReach ? gtop_floor_acc(level, n_slots) : 0.0;
  const bool by_acc = lo > -INFINITY;  // (uniform)
  uint32_t cols = 0;  // this thread's columns inside the table, by index
#pragma unroll
  for (int c = 0; c < kRecTm; ++c) cols |= (i0 + tx + 16 * c < ni ? 1u : 0u) << c;
  double carry = 0.0;  // column i0 + tid of the run (threads < 128)
  for (int b0 = rb; b0 < re; b0 += kRecTile) {
    double acc[kRecTm][kRecTm];
    rec_tile_acc(x, xs, y, ys, rows, n_rows, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
    // ---- bit a * 8 + c of `live`: the pairs of this thread whose term is not zero; rows and columns outside the request
    // are masked by index, the state of a row is loaded once ----
    double st[kRecTm];
    uint64_t live = 0;
#pragma unroll
    for (int a = 0; a < kRecTm; ++a) {
      const int r = b0 + ty * kRecTm + a;
      st[a] = 0.0;
      if (r >= re) continue;
      uint32_t row = 0;
      if (MODE == kAsrtBest) {
        st[a] = best[r];
#pragma unroll
        for (int c = 0; c < kRecTm; ++c) row |= (acc[a][c] > st[a] ? 1u : 0u) << c;
      } else if (served[r] < 0) {
#pragma unroll
        for (int c = 0; c < kRecTm; ++c) row |= (asrt_reaches(acc[a][c], lo, by_acc, n_slots, level) ? 1u : 0u) << c;
      }
      live |= static_cast<uint64_t>(row & cols) << (kRecTm * a);
    }
    // ---- eligibility, for the pairs that are left only: the user's ascending excluded list ----
    if (seen_off) {
#pragma unroll
      for (int a = 0; a < kRecTm; ++a) {
        uint32_t rbits = static_cast<uint32_t>(live >> (kRecTm * a)) & 0xffu;
        if (rbits == 0) continue;
        const int u = rows[b0 + ty * kRecTm + a];
        const int s_lo = seen_off[u], s_hi = seen_off[u + 1];
        if (s_lo == s_hi) continue;
        uint32_t gone = 0;
        for (; rbits != 0; rbits &= rbits - 1) {
          const int c = __ffs(static_cast<int>(rbits)) - 1, i = i0 + tx + 16 * c;
          if (asrt_seen(seen, s_lo, s_hi, cand ? cand[i] : i)) gone |= 1u << c;
        }
        live &= ~(static_cast<uint64_t>(gone) << (kRecTm * a));
      }
    }
    // ---- the thread's 8 rows in row order, then the step's 16 blocks in block order ----
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) {
      double v = 0.0;
#pragma unroll
      for (int a = 0; a < kRecTm; ++a) {
        const bool on = (live >> (kRecTm * a + c)) & 1u;
        v += on ? (MODE == kAsrtBest ? acc[a][c] - st[a] : 1.0) : 0.0;
      }
      xt[ty][tx + 16 * c] = v;
    }
    __syncthreads();
    if (tid < kRecTile)
      for (int b = 0; b < kGrpStep; ++b) carry += xt[b][tid];
    __syncthreads();  // (the next step stages into xt)
  }
  if (tid < kRecTile && i0 + tid < ni)
    part[static_cast<size_t>(blockIdx.y) * ld + static_cast<size_t>(i0 + tid - tile0 * kRecTile)] = carry;
}

// The better of two (value, column) entries: the larger value, equal values by the smaller column
__device__ __forceinline__ void asrt_better(double &v, int &i, double w, int j) {
  if (w > v || (w == v && j < i)) {
    v = w;
    i = j;
  }
}

// The best entry of the workgroup's 256 threads, in thread 0.  red_v / red_i: a place per wave.
__device__ __forceinline__ void asrt_reduce(double &v, int &i, double *red_v, int *red_i) {
  for (int o = kRecWave / 2; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, kRecWave);
    const int j = __shfl_xor(i, o, kRecWave);
    asrt_better(v, i, w, j);
  }
  const int lane = threadIdx.x % kRecWave, wave = threadIdx.x / kRecWave;
  if (lane == 0) {
    red_v[wave] = v;
    red_i[wave] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBlock / kRecWave; ++w) asrt_better(v, i, red_v[w], red_i[w]);
}

// Columns col0 .. col0 + n_cols of the table (the batch part [runs][ld] holds): blk_v / blk_i [blk0 + blockIdx.x] = the
// best (gain sum, column) of the workgroup's columns that are not taken, or (-inf, INT_MAX).  grid n_cols / 256.
__global__ __launch_bounds__(kBlock) void asrt_join_kernel(const double *__restrict__ part, size_t ld, int runs, int col0,
                                                           int n_cols, const int32_t *__restrict__ taken, int blk0,
                                                           const int32_t *__restrict__ stop, double *__restrict__ blk_v,
                                                           int32_t *__restrict__ blk_i) {
  __shared__ double red_v[kBlock / kRecWave];
  __shared__ int red_i[kBlock / kRecWave];
  if (*stop != 0) return;  // (uniform)
  const int j = blockIdx.x * kBlock + threadIdx.x;
  double v = -INFINITY;
  int i = INT_MAX;
  if (j < n_cols && taken[col0 + j] == 0) {
    double sum = 0.0;
    for (int r = 0; r < runs; ++r) sum += part[static_cast<size_t>(r) * ld + j];
    v = sum;
    i = col0 + j;
  }
  asrt_reduce(v, i, red_v, red_i);
  if (threadIdx.x == 0) {
    blk_v[blk0 + blockIdx.x] = v;
    blk_i[blk0 + blockIdx.x] = i;
  }
}

// Round k: the best of the n_blk entries of blk_v / blk_i; res_col / res_gain [k] and count[0] = k + 1, or the stop flag.
// One workgroup.
__global__ __launch_bounds__(kBlock) void asrt_pick_kernel(const double *__restrict__ blk_v,
                                                           const int32_t *__restrict__ blk_i, int n_blk, int k,
                                                           int32_t *__restrict__ taken, int32_t *__restrict__ res_col,
                                                           double *__restrict__ res_gain, int32_t *__restrict__ count,
                                                           int32_t *__restrict__ stop) {
  __shared__ double red_v[kBlock / kRecWave];
  __shared__ int red_i[kBlock / kRecWave];
  if (*stop != 0) return;  // (uniform)
  double v = -INFINITY;
  int i = INT_MAX;
  for (int e = threadIdx.x; e < n_blk; e += kBlock) asrt_better(v, i, blk_v[e], blk_i[e]);
  asrt_reduce(v, i, red_v, red_i);
  if (threadIdx.x != 0) return;
  if (i == INT_MAX) {
    *stop = kAsrtNoCand;
  } else if (!(v > 0.0)) {
    *stop = kAsrtNoGain;
  } else {
    res_col[k] = i;
    res_gain[k] = v;
    taken[i] = 1;
    count[0] = k + 1;
  }
}

// The state after one more item: round k's pick (k >= 0: column res_col[k], item cand[column] with a candidate list)
// or the given item `item` (k < 0).  y: the session's catalogue (ys doubles between two slots).  grid n_rows / 256.
template <int MODE>
__global__ __launch_bounds__(kBlock) void asrt_update_kernel(const double *__restrict__ x, size_t xs,
                                                             const double *__restrict__ y, size_t ys,
                                                             const int32_t *__restrict__ rows, int n_rows, int rank,
                                                             int slots, double level, int k, int item,
                                                             const int32_t *__restrict__ res_col,
                                                             const int32_t *__restrict__ cand,
                                                             const int32_t *__restrict__ seen_off,
                                                             const int32_t *__restrict__ seen,
                                                             const int32_t *__restrict__ stop, double *__restrict__ best,
                                                             int32_t *__restrict__ served) {
  if (*stop != 0) return;  // (uniform)
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rows) return;
  if (k >= 0) item = cand ? cand[res_col[k]] : res_col[k];
  const int u = rows[r];
  if (MODE == kAsrtReach && served[r] >= 0) return;
  const double *xu = x + static_cast<size_t>(u) * rank, *yi = y + static_cast<size_t>(item) * rank;
  double acc = 0.0;  // THE chain of rec_tile_acc: f = s * rank + j ascending
  for (int s = 0; s < slots; ++s)
    for (int j = 0; j < rank; ++j) acc = fma(xu[static_cast<size_t>(s) * xs + j], yi[static_cast<size_t>(s) * ys + j], acc);
  const double n_slots = static_cast<double>(slots);
  bool on;
  if (MODE == kAsrtBest) {
    on = acc > best[r];
  } else {
    const double lo = gtop_floor_acc(level, n_slots);
    on = asrt_reaches(acc, lo, lo > -INFINITY, n_slots, level);
  }
  if (on && seen_off) on = !asrt_seen(seen, seen_off[u], seen_off[u + 1], item);
  if (on) {
    best[r] = acc;
    served[r] = item;
  }
}

// given_gain[g] = column `col` of part [runs][ld] added in run order from +0.0 (undivided).  One thread.
__global__ void asrt_given_kernel(const double *__restrict__ part, size_t ld, int runs, int col, int g,
                                  double *__restrict__ given_gain) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = 0.0;
  for (int r = 0; r < runs; ++r) sum += part[static_cast<size_t>(r) * ld + col];
  given_gain[g] = sum;
}

// What leaves the device, divided once by the slots: gains [n_gain] when `divide_gains` (BEST; REACH counts stay), and
// score[r] = best[r] / S of every served row (the others: -inf).
__global__ __launch_bounds__(kBlock) void asrt_finish_kernel(double *__restrict__ gains, int n_gain, bool divide_gains,
                                                             const double *__restrict__ best,
                                                             const int32_t *__restrict__ served, int n_rows, int slots,
                                                             double *__restrict__ score) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  const double n_slots = static_cast<double>(slots);
  if (divide_gains && e < n_gain) gains[e] = gains[e] / n_slots;
  if (e < n_rows) score[e] = served[e] >= 0 ? best[e] / n_slots : -INFINITY;
}

}  // namespace
