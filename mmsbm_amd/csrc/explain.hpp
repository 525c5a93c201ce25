// explain.hpp -- which of a user's training rows carry a recommendation (mmsbm_hip_explain_*).
//
// With eta and p held fixed, the theta half of the M-step writes a user's membership as an average over the user's
// training rows j = (u, i_j, r_j):
//
//   v_j[k]      = sum_l p[k, l, r_j] eta[i_j, l]                    (fold_in.hpp's v: fold_v_step, the one copy)
//   c_j[k]      = theta_u[k] v_j[k] / max(theta_u . v_j, eps)       (the share of row j that group k takes)
//   theta'_u[k] = (1/d_u) sum_j c_j[k]
//
// and the score of a candidate item t is linear in theta: score(u, t) = sum_k theta_u[k] g_t[k], g_t = W eta_t
// (recommend.hpp's W).  So a(u, t, j) = (1/d_u) sum_k c_j[k] g_t[k] is the part of the recommendation that row j
// carries: the a of all rows of u add up to the score under one more theta update, which IS the score at a fixed point
// of EM.  Over S added slots the attribution is the mean of the slots', as the score is.
//
// Everything is in EXTERNAL terms (the session holds external copies of theta, G = eta W^T, p and eta per added slot,
// and a CSR of the training rows per external user in the order they were given), so a swapped context gives the same
// bits.  No atomics.  Per batch of requested users:
//   exp_row_kernel   one lane per (training row of the batch, slot).  v[k] is fold-in's chain over l, link by link
//                    (fold_v_step), with the row of eta read once into registers instead of once per k; the dot product
//                    theta . v is ONE fma chain over k ascending from +0.0; then ONE division inv = 1 / max(dot, eps) and
//                    c[k] = (theta[k] * v[k]) * inv -- the product as fold_kernel forms it, then the one multiply by
//                    inv.  One lane per row whatever K: the dot product is one chain, so lanes cannot share a row; the
//                    lanes of a wave hold neighbouring rows and the c rows go out rows innermost, c[(s K + k) ld + row],
//                    so each of a wave's stores and, in the pair kernel, each of its loads is one contiguous piece.
//   exp_pair_kernel  one wave per requested pair (u, t); lane x takes the user's rows x, x + 64, ... in ascending order.
//                    acc_j = ONE fma chain over f = s K + k ascending from +0.0 of c_{s,j}[k] G_s[t, k] (G_t is uniform
//                    over the wave), contribution_j = acc_j / (S d_u): one division by the product formed in double.
//                    The n largest go through the shared candidate list (RecList, rec_sort_cut of recommend.hpp) with
//                    the key (history item << 32 | rating): contribution descending, exactly equal contributions (fp64
//                    equality) by ascending history item id, then ascending rating.
//                    explained(u, t): every lane adds its rows' contributions in ascending row order from +0.0 (lane x:
//                    rows x, x + 64, ...), and the 64 lane sums are added by the butterfly xor 1, 2, 4, ... 32 -- a tree
//                    fixed by d_u alone (lanes without rows add +0.0), every lane ending with the same bits.
//                    score(u, t): ONE fma chain over f of theta_s[u, k] G_s[t, k], divided by S.  Where K <= L these are
//                    the operations of rec_tile_acc (x = theta, y = eta W^T), so the score is bitwise recommend_query's;
//                    where K > L recommend folds W into theta instead, and the two agree up to rounding only.
// There is one form of each chain.  How the loads are issued depends on d_u and L alone and changes no bit: a round of
// at most 64 rows loads one row per lane, a longer round four (exp_row_acc); beyond L = 16 a v chain's value so far
// waits in the c buffer between two pieces of the eta row.  A pair's answer depends on its user, its item and the
// added slots only, bit for bit: not on the other pairs of the call or on how the users are batched.
#pragma once

namespace {

constexpr int kExpWave = 64;       // exp_pair_kernel: one wave per workgroup
constexpr int kExpPerLane = 4;     // rows a lane examines per round
constexpr int kExpLc = 16;         // exp_row_kernel: entries of the eta row a lane holds in registers at a time

// The key of a history row in the candidate list: (item << 32 | rating), both non-negative, so the integer order is
// ascending item id, then ascending rating.
using ExpKey = uint64_t;
__device__ __forceinline__ ExpKey exp_key(int32_t item, int32_t rating) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(item)) << 32) | static_cast<uint32_t>(rating);
}

// out[(r * K + k) * L + l] = p(k, l, r) in external (k, l): a slot's p as the session keeps it.  p in the device
// layout, element (k, l, r) at p + r * rs + k * ks + l * ls.
__global__ __launch_bounds__(kBlock) void exp_p_kernel(const double *__restrict__ p, size_t rs, int ks, int ls, int K,
                                                       int L, int R, double *__restrict__ out) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= static_cast<size_t>(R) * K * L) return;
  const size_t kl = static_cast<size_t>(K) * L, r = e / kl, k = (e % kl) / L, l = e % L;
  out[e] = p[r * rs + k * ks + l * ls];
}

// The batch: occurrences b < nb of requested users, users[b] their external ids, off[b] - base the first of b's rows in
// the batch (off[nb] - base = rows).  Row jj of occurrence b is training row csr_off[users[b]] + (jj - (off[b] - base)).
// Session tables: th [S][U][K], p [S][R][K][L] external, eta [S][I][L].  c [(s K + k) ld + jj]; grid (row blocks, S).
__global__ __launch_bounds__(kBlock) void exp_row_kernel(const int32_t *__restrict__ users,
                                                         const int64_t *__restrict__ off, int64_t base, int nb,
                                                         int64_t rows, const int64_t *__restrict__ csr_off,
                                                         const int32_t *__restrict__ csr_item,
                                                         const int32_t *__restrict__ csr_rating,
                                                         const double *__restrict__ th, const double *__restrict__ p,
                                                         const double *__restrict__ eta, int U, int I, int K, int L,
                                                         int R, double *__restrict__ c, size_t ld) {
  const int64_t jj = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (jj >= rows) return;
  const size_t s = blockIdx.y;
  int lo = 0, hi = nb;  // the last occurrence whose first row is <= jj (empty ones in front of it share that row)
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (off[mid] - base <= jj) lo = mid;
    else hi = mid;
  }
  const int u = users[lo];
  const int64_t row = csr_off[u] + (jj - (off[lo] - base));
  const int32_t item = csr_item[row], rating = csr_rating[row];
  const double *tu = th + (s * U + u) * K;
  const double *pr = p + (s * R + rating) * K * L;
  const double *er = eta + (s * I + item) * L;
  double *cs = c + s * K * ld + jj;
  // v[k] into cs[k]: the eta row comes into registers kExpLc entries at a time and every k's chain runs on over them --
  // where L is beyond kExpLc the chain's value so far waits in cs[k] (the same bits: one chain over l per k)
  double dot = 0.0;
  for (int l0 = 0; l0 < L; l0 += kExpLc) {
    double e[kExpLc];
#pragma unroll
    for (int x = 0; x < kExpLc; ++x) e[x] = l0 + x < L ? er[l0 + x] : 0.0;
    const bool last = l0 + kExpLc >= L;
    for (int k = 0; k < K; ++k) {
      const double *pk = pr + static_cast<size_t>(k) * L;
      double v = l0 == 0 ? 0.0 : cs[k * ld];
#pragma unroll
      for (int x = 0; x < kExpLc; ++x)
        if (l0 + x < L) v = fold_v_step(pk, 1, l0 + x, e[x], v);
      cs[k * ld] = v;
      if (last) dot = fma(tu[k], v, dot);
    }
  }
  const double inv = 1.0 / fmax(dot, kEps);
  for (int k = 0; k < K; ++k) cs[k * ld] = (tu[k] * cs[k * ld]) * inv;
}

// acc[e] = sum_f c[(s K + k) ld + e * 64] g[s gs + k] for the NE first rows of a lane's round (c: the lane's first row;
// rows beyond NE: 0.0, unused): ONE fma chain per row over f = s K + k ascending from +0.0.  A lane without a row
// (!ok[e]) reads the round's first row instead: inside the buffer, unused.
template <int NE>
__device__ __forceinline__ void exp_row_acc(const double *__restrict__ c, const bool (&ok)[kExpPerLane], size_t ld,
                                            const double *__restrict__ g, size_t gs, int K, int S,
                                            double (&acc)[kExpPerLane]) {
  const double *cj[NE];
#pragma unroll
  for (int e = 0; e < kExpPerLane; ++e) acc[e] = 0.0;
#pragma unroll
  for (int e = 0; e < NE; ++e) cj[e] = ok[e] ? c + e * kExpWave : c - (threadIdx.x % kExpWave);
  for (int s = 0; s < S; ++s) {
    const double *gk = g + s * gs;
    const size_t at = static_cast<size_t>(s) * K * ld;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const double gv = gk[k];
#pragma unroll
      for (int e = 0; e < NE; ++e) acc[e] = fma(cj[e][at + k * ld], gv, acc[e]);
    }
  }
}

// One wave per pair q of the batch: occurrence occ[q] (of the batch), candidate item item[q].  g [S][I][K].  Outputs at
// pair q: hist_item / hist_rating / contribution [q * n ...] (counts[q] = min(n, d_u) entries, then -1 / -1 / -inf),
// explained, score, degree [q].  Dynamic LDS: cap x (double + ExpKey), cap a power of two >= n + 64 * kExpPerLane.
__global__ __launch_bounds__(kExpWave) void exp_pair_kernel(const int32_t *__restrict__ users,
                                                            const int64_t *__restrict__ off, int64_t base,
                                                            const int32_t *__restrict__ occ,
                                                            const int32_t *__restrict__ item,
                                                            const int64_t *__restrict__ csr_off,
                                                            const int32_t *__restrict__ csr_item,
                                                            const int32_t *__restrict__ csr_rating,
                                                            const double *__restrict__ c, size_t ld,
                                                            const double *__restrict__ th, const double *__restrict__ g,
                                                            int U, int I, int K, int S, int n, int cap,
                                                            int32_t *__restrict__ hist_item,
                                                            int32_t *__restrict__ hist_rating,
                                                            double *__restrict__ contribution,
                                                            int32_t *__restrict__ counts, double *__restrict__ explained,
                                                            double *__restrict__ score, int32_t *__restrict__ degree) {
  extern __shared__ double exp_lds[];
  RecList<ExpKey> list{exp_lds, reinterpret_cast<ExpKey *>(exp_lds + cap)};
  const int lane = threadIdx.x;
  const size_t q = blockIdx.x;
  const int b = occ[q], t = item[q], u = users[b];
  const int64_t j0 = off[b] - base;
  const int d = static_cast<int>(off[b + 1] - off[b]);
  const int64_t row0 = csr_off[u];
  const double denom = static_cast<double>(S) * static_cast<double>(d);
  const size_t gs = static_cast<size_t>(I) * K, ts = static_cast<size_t>(U) * K;
  const double *gt = g + static_cast<size_t>(t) * K, *tu = th + static_cast<size_t>(u) * K;
  double part = 0.0;
  for (int b0 = 0; b0 < d; b0 += kExpWave * kExpPerLane) {
    // no room for a whole round: keep the n best, raise the threshold
    if (list.cnt + kExpWave * kExpPerLane > cap) rec_sort_cut<kExpWave>(list, n);
    double acc[kExpPerLane];
    bool ok[kExpPerLane];
#pragma unroll
    for (int e = 0; e < kExpPerLane; ++e) ok[e] = b0 + e * kExpWave + lane < d;
    // (a round of at most 64 rows -- every round of most users -- loads one row per lane, not four: the same chains)
    if (d - b0 <= kExpWave) exp_row_acc<1>(c + j0 + b0 + lane, ok, ld, gt, gs, K, S, acc);
    else exp_row_acc<kExpPerLane>(c + j0 + b0 + lane, ok, ld, gt, gs, K, S, acc);
#pragma unroll
    for (int e = 0; e < kExpPerLane; ++e) {
      const int pos = b0 + e * kExpWave + lane;
      double a = -INFINITY;
      ExpKey key = std::numeric_limits<ExpKey>::max();
      if (ok[e]) {
        a = acc[e] / denom;
        part += a;
        key = exp_key(csr_item[row0 + pos], csr_rating[row0 + pos]);
      }
      const bool in = ok[e] && list.admits(a, key);
      const uint64_t mask = __ballot(in);
      const uint64_t below = lane == 0 ? 0 : (mask & ((~uint64_t(0)) >> (64 - lane)));
      if (in) {
        const int at = list.cnt + __popcll(below);
        list.ks[at] = a;
        list.kk[at] = key;
      }
      list.cnt += __popcll(mask);
    }
    __syncthreads();
  }
  rec_sort_cut<kExpWave>(list, n);
  for (int k = lane; k < n; k += kExpWave) {
    const bool have = k < list.cnt;
    hist_item[q * n + k] = have ? static_cast<int32_t>(list.kk[k] >> 32) : -1;
    hist_rating[q * n + k] = have ? static_cast<int32_t>(list.kk[k] & 0xffffffffu) : -1;
    contribution[q * n + k] = have ? list.ks[k] : -INFINITY;
  }
#pragma unroll
  for (int m = 1; m < kExpWave; m <<= 1) part += __shfl_xor(part, m, kExpWave);
  double sc = 0.0;
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < K; ++k) sc = fma(tu[s * ts + k], gt[s * gs + k], sc);
  if (lane == 0) {
    counts[q] = list.cnt;
    explained[q] = part;
    score[q] = sc / static_cast<double>(S);
    degree[q] = d;
  }
}

}  // namespace
