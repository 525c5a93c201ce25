// similar.hpp -- nearest items and users (mmsbm_hip_similar_*): the distance of every (query row, row) pair of one side
// and the N nearest rows per query row, on the device.
//
// Items (side 0; users, side 1, are the same with the roles exchanged: theta <-> eta, k <-> l, U <-> I):
//   q_s[i, k, r] = sum_l eta_s[i, l] p_s[k, l, r]      the rating profile of item i over the user groups (l ascending)
//   m_s[k]       = sum_u theta_s[u, k]                  the mass of user group k (all U training users)
//   D(i, j)      = ( sum_s sum_k sum_r m_s[k] (q_s[i,k,r] - q_s[j,k,r])^2 ) / (S U)
// -- how differently a user drawn from the training population rates the two items, in [0, 2].  The DIRECT form:
// subtract, square, accumulate.  Every term is non-negative, D(i, i) is exactly 0 and items with identical eta rows
// are at distance exactly 0 from each other and exactly equally far from every third item (the expansion
// |a|^2 + |b|^2 - 2 a.b cancels and keeps none of this).
//
// Per restart slot added to the session:
//   sim_mass_kernel     m_s, each entry written R times (mf[g * R + r] = m_s[g]: the weight of profile entry f);
//   sim_profile_kernel  the profile table [rows][G R] of the slot, read through RowTab / the p strides as
//                       rec_fold_kernel / rec_w_kernel read them (external sides: a swapped context reads the same
//                       values in the same order).
// Per batch of query rows:
//   sim_dist_kernel     the pair tile (64 query rows x 64 rows per workgroup, 4 x 4 outputs per thread, the profile
//                       staged through LDS 16 entries at a time with the matching slice of mf beside it) writes -D into
//                       the batch buffer [queries][rows] and -inf at the query's own column;
//   rec_select_kernel   (recommend.hpp) as it is: "score descending, ties by ascending id, -inf is no candidate" on -D
//                       is "D ascending, ties by ascending id, never the query row itself".  The host negates on the
//                       way out, so a zero distance leaves as +0.0.
// Determinism: a pair's numerator is ONE chain over f = (s, g, r) in ascending order from +0.0,
// t = m_f * d (rounded), acc = fma(t, d, acc), then ONE division by S U (S I) -- the same operations whatever the tile,
// the batch, the split of the selection, the other ids of the request or the slots the context holds beyond those
// added.  m_s[g] is reduced in an order that depends on the number of rows only: thread t of 256 adds rows t, t + 256,
// ... in ascending order from +0.0, then the 256 partial sums are halved 8 times (stride 128, 64, ... 1).  The longest
// run of dependent additions is c_m = ceil(rows / 256) + 8.  No atomics anywhere.
#pragma once

namespace {

constexpr int kSimTile = 64;                // query rows x rows of one distance workgroup
constexpr int kSimTm = 4;                   // outputs per thread along each side (16 x 16 threads)
constexpr int kSimKc = 16;                  // profile entries staged in LDS per step
constexpr int kSimLdsRow = kSimTile + 2;    // (padded LDS row, 16-byte aligned rows)

// mf[g * R + r] = sum over rows of src(row, g), r < R.  One workgroup per column g; the order is stated above.
__global__ __launch_bounds__(kBlock) void sim_mass_kernel(RowTab src, int rows, int R, double *__restrict__ mf) {
  __shared__ double part[kBlock];
  const int g = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  for (int row = tid; row < rows; row += kBlock) acc += *rowtab_ptr(src, static_cast<size_t>(row), g);
  part[tid] = acc;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  for (int r = tid; r < R; r += kBlock) mf[static_cast<size_t>(g) * R + r] = part[0];
}

// out[row * (G * R) + g * R + r] = sum_t src(row, t) p[r * rs + g * gs + t * ts]   (t < T, ascending)
// p of one slot in the device layout (rec_w_kernel): external (k, l) at r * rs + k * ks + l * ls.  Items: g = k, t = l;
// users: g = l, t = k.
__global__ __launch_bounds__(kBlock) void sim_profile_kernel(RowTab src, int T, const double *__restrict__ p, size_t rs,
                                                             int gs, int ts, double *__restrict__ out, int rows, int G,
                                                             int R) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int width = G * R;
  if (e >= static_cast<size_t>(rows) * width) return;
  const size_t row = e / width;
  const int j = static_cast<int>(e % width), g = j / R, r = j - g * R;
  const double *pg = p + static_cast<size_t>(r) * rs + static_cast<size_t>(g) * gs;
  double acc = 0.0;
  for (int t = 0; t < T; ++t) acc = fma(*rowtab_ptr(src, row, t), pg[static_cast<size_t>(t) * ts], acc);
  out[e] = acc;
}

// out[b * ld + i] = -( sum_f mf[f] (q[ids[b], f] - q[i, f])^2 / denom ) for b < nb, i < rows, -inf where i == ids[b];
// q: `slots` tables [rows][width] qs doubles apart, mf: [slots][width], f = s * width + j.
// grid (row tiles, query tiles).  A tile loop of its own, not rec_tile_acc (recommend.hpp): 64 x 64 with 4 x 4 outputs,
// the step d = x - y, acc = fma(w * d, d, acc) with the masses staged beside the rows -- a template wide enough for
// both would be more machinery than the two loops.
__global__ __launch_bounds__(kBlock) void sim_dist_kernel(const double *__restrict__ q, size_t qs,
                                                          const double *__restrict__ mf,
                                                          const int32_t *__restrict__ ids, int nb, int rows, int width,
                                                          int slots, double denom, double *__restrict__ out, size_t ld) {
  __shared__ double xt[kSimKc][kSimLdsRow];
  __shared__ double yt[kSimKc][kSimLdsRow];
  __shared__ double mt[kSimKc];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * kSimTile, b0 = blockIdx.y * kSimTile;
  double acc[kSimTm][kSimTm];
#pragma unroll
  for (int a = 0; a < kSimTm; ++a)
#pragma unroll
    for (int c = 0; c < kSimTm; ++c) acc[a][c] = 0.0;
  // the rows this thread stages: (kk, r) = (e % 16, e / 16) for e = tid + 256 m; its query row ids are read once
  size_t xrow[kSimTile * kSimKc / kBlock];
#pragma unroll
  for (int m = 0; m < kSimTile * kSimKc / kBlock; ++m) {
    const int r = (tid + kBlock * m) / kSimKc;
    xrow[m] = b0 + r < nb ? static_cast<size_t>(ids[b0 + r]) : 0;
  }
  const int F = width * slots;
  for (int f0 = 0; f0 < F; f0 += kSimKc) {
    const int kc = min(kSimKc, F - f0);
#pragma unroll
    for (int m = 0; m < kSimTile * kSimKc / kBlock; ++m) {
      const int e = tid + kBlock * m, kk = e % kSimKc, r = e / kSimKc;
      const int f = f0 + kk, s = f / width, j = f - s * width;
      double xv = 0.0, yv = 0.0;
      if (f < F) {
        const double *tab = q + static_cast<size_t>(s) * qs + j;
        if (b0 + r < nb) xv = tab[xrow[m] * width];
        if (i0 + r < rows) yv = tab[static_cast<size_t>(i0 + r) * width];
      }
      xt[kk][r] = xv;
      yt[kk][r] = yv;
    }
    if (tid < kSimKc) mt[tid] = f0 + tid < F ? mf[f0 + tid] : 0.0;
    __syncthreads();
    for (int kk = 0; kk < kc; ++kk) {
      double xa[kSimTm], yc[kSimTm];
      const double w = mt[kk];
#pragma unroll
      for (int a = 0; a < kSimTm; ++a) xa[a] = xt[kk][ty * kSimTm + a];
#pragma unroll
      for (int c = 0; c < kSimTm; ++c) yc[c] = yt[kk][tx + 16 * c];  // (neighbouring lanes: neighbouring rows)
#pragma unroll
      for (int a = 0; a < kSimTm; ++a)
#pragma unroll
        for (int c = 0; c < kSimTm; ++c) {
          const double d = xa[a] - yc[c];
          acc[a][c] = fma(w * d, d, acc[a][c]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < kSimTm; ++a) {
    const int b = b0 + ty * kSimTm + a;
    if (b >= nb) continue;
    const int self = ids[b];
    double *row = out + static_cast<size_t>(b) * ld;
#pragma unroll
    for (int c = 0; c < kSimTm; ++c) {
      const int i = i0 + tx + 16 * c;
      if (i < rows) row[i] = i == self ? -INFINITY : -(acc[a][c] / denom);
    }
  }
}

}  // namespace
