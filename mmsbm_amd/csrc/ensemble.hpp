// ensemble.hpp -- ensemble-aware queries of an open recommend session (recommend.hpp): how far the restarts AGREE about
// a pair (mmsbm_hip_recommend_query_ensemble, mmsbm_hip_recommend_pair_spread).  With x_s / y_s the folded factors the
// session holds for slot s,
//   a_s(u, i) = ONE fma chain over j = 0 .. rank - 1 ascending from +0.0 of x_s[u, j] y_s[i, j]
// -- the bits recommend_query returns as the score in a session that holds slot s alone -- and, per pair, without
// contraction (every product and every sum below is rounded on its own, so numpy restates it operation by operation):
//   worst = min_s a_s                       best = max_s a_s
//   d_s = a_s - a_0   (s = 1 .. S - 1)      D = ((+0.0 + d_1) + d_2) + ...      Q = ((+0.0 + d_1 d_1) + d_2 d_2) + ...
//   mean = a_0 + D / S
//   var  = max(S Q - D D, +0.0) / (S S)     std = sqrt(var)                     (population form)
//   lcb  = mean - risk std                  (product rounded, then the subtraction)
// Shifted by a_0, the cancellation in S Q - D D is relative to the spread of the restarts, not to the size of the score:
// restarts that agree give d = 0, std = +0.0 and mean = a_0 exactly, and S = 1 gives recommend_query's bits in every mode.
// None of these is bilinear in the concatenated factors: each restart's chain is closed before the next one starts, so
// rec_tile_acc (whose chain runs across the restarts) cannot form them.
//   ens_tile_kernel<MODE>  the `fill` of top_n_device for this query: the aggregate tile (64 users x 64 items per
//                       workgroup, 4 x 4 outputs per thread: LCB holds four tiles of doubles per thread -- the chain, a_0,
//                       D, Q --, which the 8 x 8 tile of rec_tile_acc does not fit) into the batch buffer
//                       [users][items].  A restart's rank is staged through LDS 16 at a time, its last step short: a
//                       staging step never crosses a restart, and the accumulators are closed into the running values at
//                       the restart's end.  The running minimum / maximum start from +inf / -inf, never from 0.0 (with
//                       signed weights a 0.0 would win a maximum over negative scores); rows beyond nb and columns
//                       beyond ni are never stored.  The item table and its slot stride are arguments: the compact
//                       table of a candidate subset (catalogue.hpp) goes through it as the whole catalogue does.
//   ens_pairs_kernel    one thread per caller-given (user, item) pair: the same chains, so the same bits, and from them
//                       mean, std, worst, best and optionally every a_s.  No row of scores is formed.
// Exclusion, selection and merge: rec_exclude_kernel / cat_exclude_kernel, rec_select_kernel, as they are.  An output's
// operations do not depend on the tile, the batch, the other rows of the call, the candidate set or the side layout.  No
// atomics.
#pragma once

namespace {

constexpr int kEnsMin = MMSBM_HIP_ENSEMBLE_MIN, kEnsMax = MMSBM_HIP_ENSEMBLE_MAX, kEnsLcb = MMSBM_HIP_ENSEMBLE_LCB;
constexpr int kEnsTm = 4;                 // outputs per thread along each side (16 x 16 threads)
constexpr int kEnsTile = 16 * kEnsTm;     // users x items of one workgroup
constexpr int kEnsKc = 16;                // rank entries of ONE restart staged in LDS per step
constexpr int kEnsLdsRow = kEnsTile + 2;  // (padded LDS row, 16-byte aligned rows)

// What the restarts' values a_0, a_1, ... of one pair leave behind: MIN / MAX keep `v` alone, LCB a_0 in `v`, D and Q.
template <int MODE>
struct EnsRun {
  double v, D, Q;
  __device__ __forceinline__ void open() {
    v = MODE == kEnsMin ? INFINITY : MODE == kEnsMax ? -INFINITY : 0.0;
    D = 0.0;
    Q = 0.0;
  }
  // restart s closed with the value a
  __device__ __forceinline__ void close(int s, double a) {
#pragma clang fp contract(off)
    if (MODE == kEnsMin) {
      v = a < v ? a : v;
    } else if (MODE == kEnsMax) {
      v = a > v ? a : v;
    } else if (s == 0) {
      v = a;
    } else {
      const double d = a - v;
      const double dd = d * d;
      D = D + d;
      Q = Q + dd;
    }
  }
};

// mean and std of (a_0, D, Q) over S restarts
__device__ __forceinline__ void ens_mean_std(double a0, double D, double Q, double S, double &mean, double &std_) {
#pragma clang fp contract(off)
  const double q = D / S;
  mean = a0 + q;
  const double sq = S * Q, dd = D * D;
  const double t = sq - dd;
  const double var = (t > 0.0 ? t : 0.0) / (S * S);
  std_ = sqrt(var);
}

__device__ __forceinline__ double ens_lcb(double mean, double std_, double risk) {
#pragma clang fp contract(off)
  const double r = risk * std_;
  return mean - r;
}

// out[b * ld + i] = the MODE aggregate of a_s(users[b], i) over the `slots` restarts, for b < nb, i < ni.
// x / y: `slots` tables [rows][rank] one after the other (x: xs doubles apart, y: ys).  grid (item tiles, user tiles).
template <int MODE>
__global__ __launch_bounds__(kBlock) void ens_tile_kernel(const double *__restrict__ x, size_t xs,
                                                          const double *__restrict__ y, size_t ys,
                                                          const int32_t *__restrict__ users, int nb, int ni, int rank,
                                                          int slots, double risk, double *__restrict__ out, size_t ld) {
  __shared__ double xt[kEnsKc][kEnsLdsRow];
  __shared__ double yt[kEnsKc][kEnsLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * kEnsTile, b0 = blockIdx.y * kEnsTile;
  EnsRun<MODE> run[kEnsTm][kEnsTm];
#pragma unroll
  for (int a = 0; a < kEnsTm; ++a)
#pragma unroll
    for (int c = 0; c < kEnsTm; ++c) run[a][c].open();
  // the rows this thread stages: (kk, r) = (e % 16, e / 16) for e = tid + 256 m; its users' ids are read once
  int32_t xrow[kEnsTile * kEnsKc / kBlock];
#pragma unroll
  for (int m = 0; m < kEnsTile * kEnsKc / kBlock; ++m) {
    const int r = (tid + kBlock * m) / kEnsKc;
    xrow[m] = b0 + r < nb ? users[b0 + r] : 0;
  }
  for (int s = 0; s < slots; ++s) {
    const double *xs_ = x + static_cast<size_t>(s) * xs, *ys_ = y + static_cast<size_t>(s) * ys;
    double acc[kEnsTm][kEnsTm];
#pragma unroll
    for (int a = 0; a < kEnsTm; ++a)
#pragma unroll
      for (int c = 0; c < kEnsTm; ++c) acc[a][c] = 0.0;
    for (int j0 = 0; j0 < rank; j0 += kEnsKc) {
      const int kc = min(kEnsKc, rank - j0);  // (the restart's last step is short: the next restart starts a new one)
#pragma unroll
      for (int m = 0; m < kEnsTile * kEnsKc / kBlock; ++m) {
        const int e = tid + kBlock * m, kk = e % kEnsKc, r = e / kEnsKc;
        const int j = j0 + kk;
        double xv = 0.0, yv = 0.0;
        if (j < rank) {
          if (b0 + r < nb) xv = xs_[static_cast<size_t>(xrow[m]) * rank + j];
          if (i0 + r < ni) yv = ys_[static_cast<size_t>(i0 + r) * rank + j];
        }
        xt[kk][r] = xv;
        yt[kk][r] = yv;
      }
      __syncthreads();
      for (int kk = 0; kk < kc; ++kk) {
        double xa[kEnsTm], yc[kEnsTm];
#pragma unroll
        for (int a = 0; a < kEnsTm; ++a) xa[a] = xt[kk][ty * kEnsTm + a];
#pragma unroll
        for (int c = 0; c < kEnsTm; ++c) yc[c] = yt[kk][tx + 16 * c];  // (neighbouring lanes: neighbouring items)
#pragma unroll
        for (int a = 0; a < kEnsTm; ++a)
#pragma unroll
          for (int c = 0; c < kEnsTm; ++c) acc[a][c] = fma(xa[a], yc[c], acc[a][c]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < kEnsTm; ++a)
#pragma unroll
      for (int c = 0; c < kEnsTm; ++c) run[a][c].close(s, acc[a][c]);
  }
  const double n_slots = static_cast<double>(slots);
#pragma unroll
  for (int a = 0; a < kEnsTm; ++a) {
    const int b = b0 + ty * kEnsTm + a;
    if (b >= nb) continue;
    double *row = out + static_cast<size_t>(b) * ld;
#pragma unroll
    for (int c = 0; c < kEnsTm; ++c) {
      const int i = i0 + tx + 16 * c;
      if (i >= ni) continue;
      double v = run[a][c].v;
      if (MODE == kEnsLcb) {
        double mean, sd;
        ens_mean_std(run[a][c].v, run[a][c].D, run[a][c].Q, n_slots, mean, sd);
        v = ens_lcb(mean, sd, risk);
      }
      row[i] = v;
    }
  }
}

// stats[e * 4 ...] = mean, std, worst, best of pair (users[e], items[e]), e < n_pairs; per_slot (or null)
// [s * n_pairs + e] = a_s.  One thread per pair.
__global__ __launch_bounds__(kBlock) void ens_pairs_kernel(const double *__restrict__ x, size_t xs,
                                                           const double *__restrict__ y, size_t ys, int rank, int slots,
                                                           const int32_t *__restrict__ users,
                                                           const int32_t *__restrict__ items, int64_t n_pairs,
                                                           double *__restrict__ stats, double *__restrict__ per_slot) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n_pairs) return;
  const double *xr = x + static_cast<size_t>(users[e]) * rank, *yr = y + static_cast<size_t>(items[e]) * rank;
  EnsRun<kEnsMin> lo;
  EnsRun<kEnsMax> hi;
  EnsRun<kEnsLcb> sp;
  lo.open();
  hi.open();
  sp.open();
  for (int s = 0; s < slots; ++s) {
    const double *xv = xr + static_cast<size_t>(s) * xs, *yv = yr + static_cast<size_t>(s) * ys;
    double a = 0.0;
    for (int j = 0; j < rank; ++j) a = fma(xv[j], yv[j], a);
    lo.close(s, a);
    hi.close(s, a);
    sp.close(s, a);
    if (per_slot) per_slot[static_cast<size_t>(s) * n_pairs + e] = a;
  }
  double mean, sd;
  ens_mean_std(sp.v, sp.D, sp.Q, static_cast<double>(slots), mean, sd);
  double *o = stats + static_cast<size_t>(e) * 4;
  o[0] = mean;
  o[1] = sd;
  o[2] = lo.v;
  o[3] = hi.v;
}

}  // namespace
