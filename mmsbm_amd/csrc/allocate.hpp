// allocate.hpp -- capacity-aware allocation (mmsbm_hip_recommend_allocate): every user of a request asks for n items,
// item i can be given out cap[i] times.  The one constraint that couples the users of a request.
//
// Semantics (the one definition): walk all candidate pairs (u, i) of the request in top_pairs' order -- score
// descending, equal scores by ascending user id, then ascending item id -- and take a pair iff u holds fewer than n
// items and i was given out fewer than cap[i] times.  What the session leaves out for u is no candidate.
//
// The walk yields a stable many-to-many matching (no user and item that both prefer each other to something they
// hold), and because every preference is read off ONE strict order of the pairs the stable matching is unique: take the
// best pair of the whole order that two stable matchings disagree on -- both of its ends are free for it in the one
// that lacks it, or hold something better, which they would hold in the other too.  So user-proposing deferred
// acceptance computes the walk's answer, and needs no sort of U x I pairs:
//   state  per capped item a threshold key tau_i = (score, user id), -inf at first; (u, i) with score s is ACCEPTABLE
//          to i iff s > tau_i.score, or s == tau_i.score and u <= tau_i.user;
//   round  user pass: P_u = u's n best candidates (recommend's order) among those acceptable to their item, sigma_u =
//          the (score, item) key of the n-th of them (-inf: fewer than n);
//          item pass: the proposers of i are the users with i in P_u -- exactly those with (u, i) a candidate,
//          acceptable under tau_i, and (s, i) not behind sigma_u in u's order -- in recommend_query_items' order (score
//          descending, user ascending); at least cap_i of them: tau_i = the cap_i-th key;
//   stop   when no tau changed.  tau only rises, so it ends; then no item holds more than cap_i proposers and P is the
//          answer.
// On the device both passes are the batches of a top-N query (serve_frame.hpp) with ONE change: the score tile's
// epilogue compares each score with its column's key and its row's key in registers and stores -inf in place of a score
// that fails either (alloc_score_kernel: rec_tile_acc, then the same single division rec_score_kernel stores).  The
// exclusions and the selection that follow are recommend's own kernels (on the host: exclude_seen and one SelectStage
// whose scratch serves both passes, serve_frame.hpp), so the scores are recommend_query's bits and the orders are its
// orders.  No atomics; nothing depends on the batch or grid shape.
//   alloc_score_kernel   user pass: rows = the request's users, column keys = tau (by item), no row keys;
//                        item pass: the tables exchanged as in recommend_query_items, rows = the capped items, row
//                        keys = tau (by item), column keys = sigma (by user; +inf for users outside the request)
//   alloc_sigma_kernel   P -> sigma, one thread per request row
//   alloc_tau_kernel     the items' lists, counts and caps -> tau, and a changed byte per item; one thread per item
//   alloc_changed_kernel the changed bytes summed to one int (one workgroup): what the host reads once per round
//   alloc_cut_kernel     drops from P_u what is no longer acceptable under the final tau and compacts; nothing to drop
//                        at the fixed point, and after a round limit it leaves a feasible answer
#pragma once

namespace {

// scores[b * ld + i] = the score of (rows[b], column i) as rec_score_kernel stores it, or -inf when it fails a key:
//   the column's key (cks, cki)[i]:        kept iff s > cks[i], or s == cks[i] and rows[b] <= cki[i]
//   the row's key (rks, rki)[rows[b]]:     kept iff s > rks[.], or s == rks[.] and i <= rki[.]     (rks null: no row keys)
// Only b < nb and i < ni are written (the tile's padding is masked by index: its zero accumulators meet no key).
// grid (column tiles, row tiles).
__global__ __launch_bounds__(kBlock) void alloc_score_kernel(const double *__restrict__ x, size_t xs,
                                                             const double *__restrict__ y, size_t ys,
                                                             const int32_t *__restrict__ rows, int nb, int ni, int rank,
                                                             int slots, const double *__restrict__ rks,
                                                             const int32_t *__restrict__ rki,
                                                             const double *__restrict__ cks,
                                                             const int32_t *__restrict__ cki,
                                                             double *__restrict__ scores, size_t ld) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * kRecTile, b0 = blockIdx.y * kRecTile;
  double acc[kRecTm][kRecTm];
  rec_tile_acc(x, xs, y, ys, rows, nb, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
  const double n_slots = static_cast<double>(slots);
  double ck[kRecTm];
  int ci[kRecTm];
#pragma unroll
  for (int c = 0; c < kRecTm; ++c) {
    const int i = i0 + tx + 16 * c;
    ck[c] = INFINITY;
    ci[c] = -1;
    if (i < ni) {
      ck[c] = cks[i];
      ci[c] = cki[i];
    }
  }
#pragma unroll
  for (int a = 0; a < kRecTm; ++a) {
    const int b = b0 + ty * kRecTm + a;
    if (b >= nb) continue;
    const int rid = rows[b];
    double rk = -INFINITY;
    int ri = INT_MAX;
    if (rks) {
      rk = rks[rid];
      ri = rki[rid];
    }
    double *row = scores + static_cast<size_t>(b) * ld;
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) {
      const int i = i0 + tx + 16 * c;
      if (i >= ni) continue;
      const double s = acc[a][c] / n_slots;
      const bool col_ok = s > ck[c] || (s == ck[c] && rid <= ci[c]);
      const bool row_ok = s > rk || (s == rk && i <= ri);
      row[i] = col_ok && row_ok ? s : -INFINITY;
    }
  }
}

// sigma of request row b (user users[b]) from its list of the user pass: the n-th entry's (score, item), or (-inf,
// INT_MAX) -- behind which nothing stands -- when the list holds fewer than n
__global__ __launch_bounds__(kBlock) void alloc_sigma_kernel(const int32_t *__restrict__ users, int n_users, int n,
                                                             const double *__restrict__ ps,
                                                             const int32_t *__restrict__ pi,
                                                             const int32_t *__restrict__ pn,
                                                             double *__restrict__ sig_s, int32_t *__restrict__ sig_i) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= n_users) return;
  const int u = users[b];
  const bool full = pn[b] == n;
  const size_t last = static_cast<size_t>(b) * n + (n - 1);
  sig_s[u] = full ? ps[last] : -INFINITY;
  sig_i[u] = full ? pi[last] : INT_MAX;
}

// tau of the batch's capped items: row r is item items[r] with cap caps[r] >= 1, its proposers ls / lu [r * nsel + k],
// k < ln[r], best first (nsel >= every cap of the batch).  At least cap proposers: tau = the cap-th key; changed[r] = 1
// when that is not the key it held.
__global__ __launch_bounds__(kBlock) void alloc_tau_kernel(const int32_t *__restrict__ items,
                                                           const int32_t *__restrict__ caps, int nb, int nsel,
                                                           const double *__restrict__ ls,
                                                           const int32_t *__restrict__ lu,
                                                           const int32_t *__restrict__ ln, double *__restrict__ tau_s,
                                                           int32_t *__restrict__ tau_u,
                                                           unsigned char *__restrict__ changed) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= nb) return;
  const int i = items[r], cap = caps[r];
  unsigned char ch = 0;
  if (ln[r] >= cap) {
    const size_t at = static_cast<size_t>(r) * nsel + (cap - 1);
    const double s = ls[at];
    const int u = lu[at];
    ch = s != tau_s[i] || u != tau_u[i];
    tau_s[i] = s;
    tau_u[i] = u;
  }
  changed[r] = ch;
}

// total[0] = the number of set bytes of changed[0 .. n): one workgroup, summed in a fixed order
__global__ __launch_bounds__(kBlock) void alloc_changed_kernel(const unsigned char *__restrict__ changed, int n,
                                                               int32_t *__restrict__ total) {
  __shared__ int red[kBlock / kRecWave];
  int v = 0;
  for (int e = threadIdx.x; e < n; e += kBlock) v += changed[e] != 0;
  for (int o = kRecWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kRecWave);
  if (threadIdx.x % kRecWave == 0) red[threadIdx.x / kRecWave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kBlock / kRecWave; ++w) t += red[w];
    total[0] = t;
  }
}

// Request row b keeps the entries of its list that are acceptable under tau, in their order, and its count follows
__global__ __launch_bounds__(kBlock) void alloc_cut_kernel(const int32_t *__restrict__ users, int n_users, int n,
                                                           const double *__restrict__ tau_s,
                                                           const int32_t *__restrict__ tau_u, double *__restrict__ ps,
                                                           int32_t *__restrict__ pi, int32_t *__restrict__ pn) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= n_users) return;
  const int u = users[b], cnt = pn[b];
  double *s = ps + static_cast<size_t>(b) * n;
  int32_t *it = pi + static_cast<size_t>(b) * n;
  int w = 0;
  for (int k = 0; k < cnt; ++k) {
    const double v = s[k];
    const int i = it[k];
    if (v > tau_s[i] || (v == tau_s[i] && u <= tau_u[i])) {
      s[w] = v;
      it[w] = i;
      ++w;
    }
  }
  pn[b] = w;
}

}  // namespace
