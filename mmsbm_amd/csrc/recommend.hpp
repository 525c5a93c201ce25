// recommend.hpp -- top-N item recommendation (mmsbm_hip_recommend_*): the expected score of every (user, item) pair
// of a request and the N best items per user, on the device.
//
//   score_w(u, i) = (1/S) sum_s sum_r w_r P_s(r | u, i) = (1/S) sum_s theta_s[u,:] W_s eta_s[i,:]^T,
//   W_s[k,l]      = sum_r w_r p_s[k,l,r]                                           (K x L, external sides)
//
// Per restart slot a small prologue folds W_s into the side with the larger group count, so that the product has
// rank min(K, L): x_s = theta_s (U x K) and y_s = eta_s W_s^T (I x K) when K <= L, else x_s = theta_s W_s (U x L) and
// y_s = eta_s.  The slots' factors are concatenated along the rank, f = s * rank + j, and a score is ONE fma chain
// over f in ascending order, divided by S at the end -- the same operations in the same order whatever the tile, the
// launch shape or the request's other users (bitwise request independence; identical eta rows tie exactly).
// Everything is stated in EXTERNAL terms (user side = the caller's users, whichever internal side holds them), so a
// swapped context gives bitwise the same scores as an unswapped one.
//
// Then, per batch of users:
//   rec_score_kernel    the score tile (128 users x 128 items per workgroup, 8 x 8 fp64 FMA per thread on the
//                       vector ALU: users 8 in a row, items 16 apart; rank staged through LDS 16 at a time) into a
//                       batch buffer [users][items];
//   rec_exclude_kernel  -inf over the items each user has in the training triples (exclude_seen);
//   rec_select_kernel   one wave per (user, item range): a running candidate list in LDS, filtered against the current
//                       N-th best, compacted by ballot (no atomics) and re-sorted (bitonic) when it fills; the same
//                       kernel then merges the ranges' lists when the items were split across waves.
//   rec_position_kernel / rec_position_sum_kernel  (mmsbm_hip_recommend_positions) the position of caller-given items
//                       in a user's full order: per (user, item range) the items of the range that beat each test
//                       item, counted as integers with up to kPosKeys test keys in registers per pass over the row;
//                       the ranges' counts are then summed in range order (no atomics).
// Shared with top_pairs.hpp, which holds no copy of either: the tile's accumulation (rec_tile_acc: staging + the 8 x 8
// fma loop; rec_score_kernel stores the tile, gtop_fused_kernel filters it in registers) and the candidate list
// (RecList, rec_better, rec_sort, rec_sort_cut: one order, one bitonic network, one "sort, cut to n, take the n-th as
// threshold", by key type and workgroup width).  How survivors are appended stays with each kernel: a one-wave ballot
// here, a workgroup prefix sum there.
// Order: score descending, equal scores (exact fp64 equality) by ascending item id -- a strict total order, so the
// top N is unique and the split into ranges cannot change it.  N is bounded by kRecMaxN (larger N: the C ABI answers
// MMSBM_E_UNSUPPORTED); the candidate list holds the next power of two >= N + 256 entries (<= 2,048).
#pragma once

namespace {

constexpr int kRecMaxN = MMSBM_HIP_RECOMMEND_MAX_N;  // largest N a query may ask for (include/mmsbm_hip.h)
// (kRecTile, kRecTm, kRecWave, kRecPerLane: serve_plan.hpp -- the host's plans are made from them too)
constexpr int kRecKc = 16;          // rank entries staged in LDS per step
constexpr int kRecLdsRow = kRecTile + 2;  // (padded LDS row: fewer bank conflicts, 16-byte aligned rows)

// W[k * L + l] = sum_r w[r] p[r][k, l] in external (k, l); p of one slot in the device layout [R][kp][lp], internal
// (k, l) = external (k, l) or (l, k) when swapped: element (k, l) at p + r * rs + k * ks + l * ls.
__global__ __launch_bounds__(kBlock) void rec_w_kernel(const double *__restrict__ p, const double *__restrict__ w,
                                                       double *__restrict__ wout, int K, int L, int R, size_t rs,
                                                       int ks, int ls) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= K * L) return;
  const int k = e / L, l = e % L;
  double acc = 0.0;
  for (int r = 0; r < R; ++r) acc = fma(w[r], p[static_cast<size_t>(r) * rs + static_cast<size_t>(k) * ks + static_cast<size_t>(l) * ls], acc);
  wout[e] = acc;
}

// out[row * rank + j] = src(row, j)                                (m == nullptr)
//                     = sum_t src(row, t) m[t * mt + j * mj]       (t < d, ascending)
__global__ __launch_bounds__(kBlock) void rec_fold_kernel(RowTab src, int d, const double *__restrict__ m, int mt,
                                                          int mj, double *__restrict__ out, int rows, int rank) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= static_cast<size_t>(rows) * rank) return;
  const size_t row = e / rank;
  const int j = static_cast<int>(e % rank);
  if (!m) {
    out[e] = *rowtab_ptr(src, row, j);
    return;
  }
  double acc = 0.0;
  for (int t = 0; t < d; ++t) acc = fma(*rowtab_ptr(src, row, t), m[static_cast<size_t>(t) * mt + static_cast<size_t>(j) * mj], acc);
  out[e] = acc;
}

// THE score tile (the one copy: rec_score_kernel and gtop_fused_kernel of top_pairs.hpp both call it, so a pair's score
// is the same bits in both).  acc[a][c] = sum_f x[users[b0 + ty * 8 + a], f] y[i0 + tx + 16 * c, f]: ONE fma chain per
// output over f = s * rank + j ascending from +0.0, rows beyond nb / ni as 0.0; the caller divides once by S.
// x / y: `slots` tables [rows][rank] one after the other (x: xs doubles apart, y: ys).  All 256 threads; (tx, ty) =
// (tid % 16, tid / 16) is the caller's, which reads acc by it (derived again in here, the compiler no longer proves the
// 16-byte alignment of a thread's eight x entries and narrows their LDS reads); xt / yt: the workgroup's two staging
// tiles, free again on return.
__device__ __forceinline__ void rec_tile_acc(const double *__restrict__ x, size_t xs, const double *__restrict__ y,
                                             size_t ys, const int32_t *__restrict__ users, int nb, int ni, int rank,
                                             int slots, int b0, int i0, int tx, int ty, double (&xt)[kRecKc][kRecLdsRow],
                                             double (&yt)[kRecKc][kRecLdsRow], double (&acc)[kRecTm][kRecTm]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int a = 0; a < kRecTm; ++a)
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) acc[a][c] = 0.0;
  // the rows this thread stages: (kk, r) = (e % 16, e / 16) for e = tid + 256 m
  const int F = rank * slots;
  for (int f0 = 0; f0 < F; f0 += kRecKc) {
    const int kc = min(kRecKc, F - f0);
#pragma unroll
    for (int m = 0; m < kRecTile * kRecKc / kBlock; ++m) {
      const int e = tid + kBlock * m, kk = e % kRecKc, r = e / kRecKc;
      const int f = f0 + kk, s = f / rank, j = f - s * rank;
      double xv = 0.0, yv = 0.0;
      if (f < F) {
        if (b0 + r < nb) xv = x[static_cast<size_t>(s) * xs + static_cast<size_t>(users[b0 + r]) * rank + j];
        if (i0 + r < ni) yv = y[static_cast<size_t>(s) * ys + static_cast<size_t>(i0 + r) * rank + j];
      }
      xt[kk][r] = xv;
      yt[kk][r] = yv;
    }
    __syncthreads();
    for (int kk = 0; kk < kc; ++kk) {
      double xa[kRecTm], yc[kRecTm];
#pragma unroll
      for (int a = 0; a < kRecTm; ++a) xa[a] = xt[kk][ty * kRecTm + a];
#pragma unroll
      for (int c = 0; c < kRecTm; ++c) yc[c] = yt[kk][tx + 16 * c];  // (neighbouring lanes: neighbouring items)
#pragma unroll
      for (int a = 0; a < kRecTm; ++a)
#pragma unroll
        for (int c = 0; c < kRecTm; ++c) acc[a][c] = fma(xa[a], yc[c], acc[a][c]);
    }
    __syncthreads();
  }
}

// scores[b * ld + i] = (1/S) sum_f x[users[b], f] y[i, f] for b < nb, i < ni (rec_tile_acc).  grid (item tiles, user
// tiles).
__global__ __launch_bounds__(kBlock) void rec_score_kernel(const double *__restrict__ x, size_t xs,
                                                           const double *__restrict__ y, size_t ys,
                                                           const int32_t *__restrict__ users, int nb, int ni,
                                                           int rank, int slots, double *__restrict__ scores, size_t ld) {
  __shared__ double xt[kRecKc][kRecLdsRow];
  __shared__ double yt[kRecKc][kRecLdsRow];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * kRecTile, b0 = blockIdx.y * kRecTile;
  double acc[kRecTm][kRecTm];
  rec_tile_acc(x, xs, y, ys, users, nb, ni, rank, slots, b0, i0, tx, ty, xt, yt, acc);
  const double n_slots = static_cast<double>(slots);
#pragma unroll
  for (int a = 0; a < kRecTm; ++a) {
    const int b = b0 + ty * kRecTm + a;
    if (b >= nb) continue;
    double *row = scores + static_cast<size_t>(b) * ld;
#pragma unroll
    for (int c = 0; c < kRecTm; ++c) {
      const int i = i0 + tx + 16 * c;
      if (i < ni) row[i] = acc[a][c] / n_slots;
    }
  }
}

// scores[b * ld + item] = -inf for every item user users[b] has in the training triples (one workgroup per user)
__global__ __launch_bounds__(kBlock) void rec_exclude_kernel(const int32_t *__restrict__ users,
                                                             const int32_t *__restrict__ seen_off,
                                                             const int32_t *__restrict__ seen_item,
                                                             double *__restrict__ scores, size_t ld) {
  const int b = blockIdx.x;
  const int u = users[b];
  double *row = scores + static_cast<size_t>(b) * ld;
  for (int e = seen_off[u] + threadIdx.x; e < seen_off[u + 1]; e += kBlock) row[seen_item[e]] = -INFINITY;
}

// THE order of every candidate list (the one definition): score descending, equal scores by ascending key.  Key: the
// item id (int) of a top-N query, (user << 32 | item) (uint64_t) of top_pairs.hpp.
template <class Key>
__device__ __forceinline__ bool rec_better(double sa, Key ka, double sb, Key kb) {
  return sa > sb || (sa == sb && ka < kb);
}

// A candidate list in LDS: entries [0, cnt) of (ks, kk), and the threshold -- the n-th best -- once n entries were
// accepted.  Everything but the arrays is uniform over the workgroup.
template <class Key>
struct RecList {
  double *ks;
  Key *kk;
  int cnt = 0;
  bool have_thr = false;
  double thr_s = 0.0;
  Key thr_k = 0;
  __device__ bool admits(double s, Key k) const { return !have_thr || rec_better(s, k, thr_s, thr_k); }
};

// Sorts the first `cnt` entries of (ks, kk) best first (THE bitonic network; entries up to the next power of two are
// padded with the sentinel (-inf, largest key), worse than any candidate: the arrays hold a power of two).  All THREADS
// threads of the workgroup; what they wrote to the list before is ordered by the first barrier in here.
template <int THREADS, class Key>
__device__ void rec_sort(double *ks, Key *kk, int cnt) {
  int sz = 2;
  while (sz < cnt) sz <<= 1;
  for (int t = cnt + threadIdx.x; t < sz; t += THREADS) { ks[t] = -INFINITY; kk[t] = std::numeric_limits<Key>::max(); }
  __syncthreads();
  for (int k = 2; k <= sz; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < sz / 2; t += THREADS) {
        const int i = (t / j) * 2 * j + (t % j), q = i + j;
        const double si = ks[i], sq = ks[q];
        const Key ki = kk[i], kq = kk[q];
        const bool up = (i & k) == 0;  // this half: best first
        if (up ? rec_better(sq, kq, si, ki) : rec_better(si, ki, sq, kq)) {
          ks[i] = sq; kk[i] = kq; ks[q] = si; kk[q] = ki;
        }
      }
      __syncthreads();
    }
  }
}

// Sorts the list best first, cuts it to n and takes the n-th as the threshold.  All THREADS threads.
template <int THREADS, class Key>
__device__ void rec_sort_cut(RecList<Key> &L, int n) {
  rec_sort<THREADS>(L.ks, L.kk, L.cnt);
  L.cnt = min(L.cnt, n);
  if (L.cnt == n) {
    L.thr_s = L.ks[n - 1];
    L.thr_k = L.kk[n - 1];
    L.have_thr = true;
  }
  __syncthreads();  // (the threshold is read before the list is written again)
}

// The N best of one (user, range).  One wave per workgroup; grid (parts, users).
// !MERGE: the candidates are scores[b * ld + i] for i in the part's slice [part * per, min(ni, part * per + per)),
//         excluded items (-inf) are never candidates.
// MERGE:  the candidates are the lists of `in_parts` earlier parts: in_s / in_i [(b * in_parts + p) * n + k] for
//         k < in_n[b * in_parts + p].
// Output: out_s / out_i [(b * gridDim.x + part) * n + k], k < out_n[b * gridDim.x + part].
template <bool MERGE>
__global__ __launch_bounds__(kRecWave) void rec_select_kernel(const double *__restrict__ scores, size_t ld, int ni,
                                                              int per, const double *__restrict__ in_s,
                                                              const int32_t *__restrict__ in_i,
                                                              const int32_t *__restrict__ in_n, int in_parts, int n,
                                                              int cap, double *__restrict__ out_s,
                                                              int32_t *__restrict__ out_i, int32_t *__restrict__ out_n) {
  extern __shared__ double rec_lds[];
  RecList<int> L{rec_lds, reinterpret_cast<int *>(rec_lds + cap)};
  const int lane = threadIdx.x, part = blockIdx.x, b = blockIdx.y;
  int lo, hi;
  if (MERGE) {
    lo = 0;
    hi = in_parts * n;
  } else {
    lo = part * per;
    hi = min(ni, lo + per);
  }
  const double *row = MERGE ? nullptr : scores + static_cast<size_t>(b) * ld;
  for (int base = lo; base < hi; base += kRecWave * kRecPerLane) {
    // no room for a whole round: keep the N best, raise the threshold
    if (L.cnt + kRecWave * kRecPerLane > cap) rec_sort_cut<kRecWave>(L, n);
    double sv[kRecPerLane];
    int iv[kRecPerLane];
    bool ok[kRecPerLane];
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const int pos = base + e * kRecWave + lane;
      ok[e] = false;
      sv[e] = -INFINITY;
      iv[e] = INT_MAX;
      if (pos < hi) {
        if (MERGE) {
          const int p = pos / n, k = pos - p * n;
          const size_t at = static_cast<size_t>(b) * in_parts + p;
          if (k < in_n[at]) {
            sv[e] = in_s[at * n + k];
            iv[e] = in_i[at * n + k];
            ok[e] = true;
          }
        } else {
          sv[e] = row[pos];
          iv[e] = pos;
          ok[e] = sv[e] != -INFINITY;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const bool q = ok[e] && L.admits(sv[e], iv[e]);
      const uint64_t mask = __ballot(q);
      const uint64_t below = lane == 0 ? 0 : (mask & ((~uint64_t(0)) >> (64 - lane)));
      if (q) {
        const int at = L.cnt + __popcll(below);
        L.ks[at] = sv[e];
        L.kk[at] = iv[e];
      }
      L.cnt += __popcll(mask);
    }
    __syncthreads();
  }
  rec_sort_cut<kRecWave>(L, n);
  const size_t o = (static_cast<size_t>(b) * gridDim.x + part);
  for (int k = lane; k < L.cnt; k += kRecWave) {
    out_s[o * n + k] = L.ks[k];
    out_i[o * n + k] = L.kk[k];
  }
  if (lane == 0) out_n[o] = L.cnt;
}

// ---- positions of test items (mmsbm_hip_recommend_positions) --------------------------------------------------------
constexpr int kPosKeys = 16;   // test keys held in registers per pass over a row (TQ)
constexpr int kPosSmall = 4;   // a chunk of at most this many keys takes the narrow pass (most users hold 1-2)

// Adds to cnt[q] the items j of [lo, hi) this thread visits that come before key q in the order:
// score(j) > ks[q], or score(j) == ks[q] and j < ki[q].  Padding keys (+inf, -1) are beaten by nothing; excluded
// items (-inf) beat no finite key.
template <int Q>
__device__ __forceinline__ void rec_count_pass(const double *__restrict__ row, int lo, int hi, const double *ks,
                                               const int *ki, int *cnt) {
  for (int j = lo + static_cast<int>(threadIdx.x); j < hi; j += kBlock) {
    const double s = row[j];
#pragma unroll
    for (int q = 0; q < Q; ++q) cnt[q] += (s > ks[q]) | ((s == ks[q]) & (j < ki[q]));
  }
}

// One chunk of keys: test entries c0 .. c0 + nq of the row; the workgroup's counts over [lo, hi) go to
// out[(c0 + q) * parts + part] (entries relative to the batch's first).
template <int Q>
__device__ __forceinline__ void rec_count_chunk(const double *__restrict__ row, int lo, int hi,
                                                const int32_t *__restrict__ titem, int c0, int nq, int parts,
                                                int part, int32_t *__restrict__ out, int (*red)[kPosKeys]) {
  double ks[Q];
  int ki[Q], cnt[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    ki[q] = -1;
    ks[q] = INFINITY;
    if (q < nq) {
      ki[q] = titem[c0 + q];
      ks[q] = row[ki[q]];
    }
    cnt[q] = 0;
  }
  rec_count_pass<Q>(row, lo, hi, ks, ki, cnt);
  const int lane = threadIdx.x % kRecWave, wave = threadIdx.x / kRecWave;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    int v = cnt[q];
    for (int o = kRecWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kRecWave);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < nq) {
    int v = 0;
    for (int w = 0; w < kBlock / kRecWave; ++w) v += red[w][threadIdx.x];
    out[static_cast<size_t>(c0 + threadIdx.x) * parts + part] = v;
  }
  __syncthreads();  // (red is reused by the next chunk)
}

// grid (parts, rows of the batch).  Row b scores[b * ld ...] holds the test entries toff[b] .. toff[b + 1) (item ids
// titem[e]; entries counted from toff[0], the batch's first); the workgroup counts over items [part * per, + per).
__global__ __launch_bounds__(kBlock) void rec_position_kernel(const double *__restrict__ scores, size_t ld, int ni,
                                                              int per, const int32_t *__restrict__ toff,
                                                              const int32_t *__restrict__ titem,
                                                              int32_t *__restrict__ part_cnt) {
  __shared__ int red[kBlock / kRecWave][kPosKeys];
  const int part = blockIdx.x, parts = gridDim.x, b = blockIdx.y;
  const int lo = part * per, hi = min(ni, lo + per);
  const double *row = scores + static_cast<size_t>(b) * ld;
  const int base = toff[0], e1 = toff[b + 1] - base;
  const int32_t *it = titem + base;
  for (int c0 = toff[b] - base; c0 < e1; c0 += kPosKeys) {
    const int nq = min(kPosKeys, e1 - c0);
    if (nq <= kPosSmall)
      rec_count_chunk<kPosSmall>(row, lo, hi, it, c0, nq, parts, part, part_cnt, red);
    else
      rec_count_chunk<kPosKeys>(row, lo, hi, it, c0, nq, parts, part, part_cnt, red);
  }
}

// positions[e] = 0 when the test item's score is -inf (excluded: not a candidate), else 1 + the ranges' counts summed
// in range order.  One workgroup per row of the batch; e is the global entry (toff as in rec_position_kernel).
__global__ __launch_bounds__(kBlock) void rec_position_sum_kernel(const double *__restrict__ scores, size_t ld,
                                                                  const int32_t *__restrict__ toff,
                                                                  const int32_t *__restrict__ titem,
                                                                  const int32_t *__restrict__ part_cnt, int parts,
                                                                  int32_t *__restrict__ positions) {
  const int b = blockIdx.x, base = toff[0];
  const double *row = scores + static_cast<size_t>(b) * ld;
  for (int e = toff[b] + threadIdx.x; e < toff[b + 1]; e += kBlock) {
    int pos = 0;
    if (row[titem[e]] != -INFINITY) {
      pos = 1;
      for (int p = 0; p < parts; ++p) pos += part_cnt[static_cast<size_t>(e - base) * parts + p];
    }
    positions[e] = pos;
  }
}

}  // namespace
