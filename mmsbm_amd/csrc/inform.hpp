// inform.hpp -- the items whose rating tells most about a user (mmsbm_hip_inform_*): the information gain of every
// (user, item) pair of a request and the N most informative items per user, on the device.
//
// A rating of item i by user u is generated as k ~ theta[u], l ~ eta[i], r ~ p[k, l, .].  With the item profile
//   q_s[i, k, r] = sum_l eta_s[i, l] p_s[k, l, r]                 (similar.hpp: sim_profile_kernel, side items)
// the information the rating carries about the group k the user acts from, under the belief theta_s[u], is
//   gain_s(u, i) = I(k ; r) = H( sum_k theta_s[u,k] q_s[i,k,.] ) - sum_k theta_s[u,k] H( q_s[i,k,.] )      (nats)
//   gain(u, i)   = (1/S) sum_s gain_s(u, i),       0 <= gain <= log min(K, R)
// -- zero for an item every group rates alike and for a one-hot theta, largest where the groups the user may belong to
// disagree.  Not bilinear in (theta, eta): it cannot go through rec_tile_acc or the folded factors of recommend.hpp.
// Invariant under a relabelling of the groups, so the mean over the restarts needs no alignment.
//
// Per restart slot added to the session (external sides throughout: a swapped context reads the same values in the
// same order):
//   rec_fold_kernel     (recommend.hpp, without a matrix) the users' theta rows [U][K];
//   sim_mass_kernel     (similar.hpp, R = 1) sum_u theta_s[u, k] in its fixed order; theta-bar_s[k] is that over U;
//   sim_profile_kernel  (similar.hpp) the profile table q [I][K R];
//   inf_entropy_kernel  h_s[i, k] = sum_r phi(q_s[i, k, r]), r ascending from +0.0, phi(x) = x > 0 ? -(x log x) : +0.0.
// Per batch of users:
//   inf_score_kernel    the gain tile (64 users x 64 items per workgroup, 4 x 4 outputs per thread; theta rows and the
//                       (k, r) slices of q staged through LDS 16 k at a time) writes gain, or -inf where the candidate
//                       mask (one byte per item, optional) is 0, into the batch buffer [users][items];
//   rec_exclude_kernel / cat_exclude_kernel, rec_select_kernel and the merge, as they are (top_n_run, serve_frame.hpp).
// Determinism: an output is built as
//   for s ascending:  for r ascending:  m_r = ONE fma chain over k ascending from +0.0 of theta[u,k] q[i,k,r];
//                                        H += phi(m_r)                                        (H from +0.0)
//                     lin = ONE fma chain over k ascending from +0.0 of theta[u,k] h[i,k]
//                     acc += max(H - lin, +0.0)                                               (acc from +0.0)
//   acc / S
// -- the same operations whatever the tile, the batch, the other users of the call or the slots the context holds
// beyond those added.  phi is ONE function, its product rounded before it is added (no contraction), used by the
// prologue and the score kernel: a one-hot theta row makes m_r the bits of q[i,k*,r] and lin the bits of h[i,k*], so
// H - lin is exactly +0.0 for every item.  No atomics anywhere.
#pragma once

namespace {

constexpr int kInfTile = 64;                // users x items of one gain workgroup
constexpr int kInfTm = 4;                   // outputs per thread along each side (16 x 16 threads)
constexpr int kInfKc = 16;                  // groups k staged in LDS per step
constexpr int kInfLdsRow = kInfTile + 2;    // (padded LDS row, 16-byte aligned rows)

// -(x log x), +0.0 at and below 0.  THE entropy term: inf_entropy_kernel and inf_score_kernel both add exactly this.
__device__ __forceinline__ double inf_phi(double x) {
#pragma clang fp contract(off)
  const double t = x * log(x);
  return x > 0.0 ? -t : 0.0;
}

// h[e] = sum_r phi(q[e * R + r]), r ascending from +0.0, for the n = rows x K (item, group) entries e
__global__ __launch_bounds__(kBlock) void inf_entropy_kernel(const double *__restrict__ q, double *__restrict__ h,
                                                             size_t n, int R) {
#pragma clang fp contract(off)
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n) return;
  const double *qe = q + e * R;
  double acc = 0.0;
  for (int r = 0; r < R; ++r) acc += inf_phi(qe[r]);
  h[e] = acc;
}

// out[b * ld + i] = gain(ids[b], i) for b < nb, i < rows; -inf where mask && !mask[i].
// th: `slots` tables [.][K] ts doubles apart, row ids[b]; q: [rows][K R], qs apart; h: [rows][K], hs apart.
// grid (item tiles, user tiles).  Pass j < R of a slot forms m_j of the 4 x 4 outputs (staged: theta[., k] and
// q[., k, j]), pass j == R the linear term (staged: theta and h); with K <= kInfKc the theta tile of a slot is staged
// by its first pass only.
// (three waves per SIMD: the bound keeps the 16 inlined logarithms of a pass within 168 registers, without scratch)
__global__ __launch_bounds__(kBlock, 3) void inf_score_kernel(const double *__restrict__ th, size_t ts,
                                                              const double *__restrict__ q, size_t qs,
                                                              const double *__restrict__ h, size_t hs,
                                                              const int32_t *__restrict__ ids, int nb, int rows, int K,
                                                              int R, int slots, const uint8_t *__restrict__ mask,
                                                              double *__restrict__ out, size_t ld) {
#pragma clang fp contract(off)
  __shared__ double xt[kInfKc][kInfLdsRow];
  __shared__ double yt[kInfKc][kInfLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * kInfTile, b0 = blockIdx.y * kInfTile;
  double acc[kInfTm][kInfTm];
#pragma unroll
  for (int a = 0; a < kInfTm; ++a)
#pragma unroll
    for (int c = 0; c < kInfTm; ++c) acc[a][c] = 0.0;
  // the rows this thread stages: (kk, r) = (e % 16, e / 16) for e = tid + 256 m; its users' ids are read once
  size_t xrow[kInfTile * kInfKc / kBlock];
#pragma unroll
  for (int m = 0; m < kInfTile * kInfKc / kBlock; ++m) {
    const int r = (tid + kBlock * m) / kInfKc;
    xrow[m] = b0 + r < nb ? static_cast<size_t>(ids[b0 + r]) : 0;
  }
  const int W = K * R;
  const bool one_step = K <= kInfKc;
  for (int s = 0; s < slots; ++s) {
    const double *ths = th + static_cast<size_t>(s) * ts;
    double H[kInfTm][kInfTm];
#pragma unroll
    for (int a = 0; a < kInfTm; ++a)
#pragma unroll
      for (int c = 0; c < kInfTm; ++c) H[a][c] = 0.0;
    for (int j = 0; j <= R; ++j) {
      // entry (i, k) of this pass at src[i * is + k * ks]
      const double *src = j < R ? q + static_cast<size_t>(s) * qs + j : h + static_cast<size_t>(s) * hs;
      const size_t is = j < R ? W : K, ks = j < R ? R : 1;
      const bool stage_x = !one_step || j == 0;
      double mm[kInfTm][kInfTm];
#pragma unroll
      for (int a = 0; a < kInfTm; ++a)
#pragma unroll
        for (int c = 0; c < kInfTm; ++c) mm[a][c] = 0.0;
      for (int k0 = 0; k0 < K; k0 += kInfKc) {
        const int kc = min(kInfKc, K - k0);
#pragma unroll
        for (int m = 0; m < kInfTile * kInfKc / kBlock; ++m) {
          const int e = tid + kBlock * m, kk = e % kInfKc, r = e / kInfKc;
          const int k = k0 + kk;
          double xv = 0.0, yv = 0.0;
          if (k < K) {
            if (stage_x && b0 + r < nb) xv = ths[xrow[m] * K + k];
            if (i0 + r < rows) yv = src[static_cast<size_t>(i0 + r) * is + static_cast<size_t>(k) * ks];
          }
          if (stage_x) xt[kk][r] = xv;
          yt[kk][r] = yv;
        }
        __syncthreads();
        for (int kk = 0; kk < kc; ++kk) {
          double xa[kInfTm], yc[kInfTm];
#pragma unroll
          for (int a = 0; a < kInfTm; ++a) xa[a] = xt[kk][ty * kInfTm + a];
#pragma unroll
          for (int c = 0; c < kInfTm; ++c) yc[c] = yt[kk][tx + 16 * c];  // (neighbouring lanes: neighbouring items)
#pragma unroll
          for (int a = 0; a < kInfTm; ++a)
#pragma unroll
            for (int c = 0; c < kInfTm; ++c) mm[a][c] = fma(xa[a], yc[c], mm[a][c]);
        }
        __syncthreads();
      }
#pragma unroll
      for (int a = 0; a < kInfTm; ++a)
#pragma unroll
        for (int c = 0; c < kInfTm; ++c) {
          if (j < R) {
            H[a][c] += inf_phi(mm[a][c]);
          } else {
            const double g = H[a][c] - mm[a][c];
            acc[a][c] += g > 0.0 ? g : 0.0;
          }
        }
    }
  }
  const double n_slots = static_cast<double>(slots);
#pragma unroll
  for (int a = 0; a < kInfTm; ++a) {
    const int b = b0 + ty * kInfTm + a;
    if (b >= nb) continue;
    double *row = out + static_cast<size_t>(b) * ld;
#pragma unroll
    for (int c = 0; c < kInfTm; ++c) {
      const int i = i0 + tx + 16 * c;
      if (i < rows) row[i] = mask && !mask[i] ? -INFINITY : acc[a][c] / n_slots;
    }
  }
}

}  // namespace
