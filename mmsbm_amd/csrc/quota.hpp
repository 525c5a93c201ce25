// quota.hpp -- per-category caps on a top-N list (mmsbm_hip_recommend_query_quota / _query_theta_quota): at most q items
// of one category, as a MASK over the batch buffer between the exclusions and the unchanged selection.
//
// Semantics (the one definition): walk a row's candidates in recommend_query's order -- score descending, equal scores
// by ascending item id -- and take an item unless q items of its category were taken before it; stop after n.  An item
// is skipped exactly when q better items of its own category precede it, whatever the other categories do, so the walk
// IS the top-n of the items whose rank inside their own category is at most q: the mask writes -inf over the others
// and rec_select_kernel does the rest.  Exact, without a pool or an over-fetch, at any catalogue size.
//
// Contract of both kernels, for row b and a category with columns c_0 < ... < c_{m-1} and cap q: among the columns with
// sc[b][c] != -inf the first q in (score descending, column ascending) keep their bits, the others become -inf;
// nothing else in the row is touched.  Columns are those of the query's buffer (the items, or the places in the
// ascending candidate list: column order is item order, so the tie rule carries over).  The categories are disjoint, so
// no two waves of a launch touch the same entry.  No atomics, no arithmetic on a score: comparisons and stores.
//   quota_short_kernel  m <= 64: a category is a group of w = the next power of two >= m lanes, 64 / w categories to a
//                       wave (serve_plan.hpp packs a wave with categories of one width).  A lane holds one column's
//                       (score, column), reads the w - 1 others of its group by shuffles, counts those that come
//                       before it and writes -inf when the count reaches q (q = 0: always).  No LDS.
//   quota_long_kernel   m > 64: one wave per (row, category).  The category's scores of the row go through the
//                       candidate list of recommend.hpp (RecList, rec_better, rec_sort_cut with n = q <= 1,023); the
//                       q-th best is the threshold, and a second pass writes -inf over every finite column that is
//                       worse.  Fewer than q finite columns: nothing is written.  q = 0: one pass that writes them all.
#pragma once

namespace {

constexpr int kQuotaWaves = kBlock / kRecWave;  // waves per workgroup of the short form

// grid (waves / kQuotaWaves, rows of the batch).  wave_first / wave_info [n_waves]: the wave's first category and its
// width | categories << 8 (QuotaPlan); off / col / cap: the kept categories' columns and caps.
__global__ __launch_bounds__(kBlock) void quota_short_kernel(const int32_t *__restrict__ wave_first,
                                                             const int32_t *__restrict__ wave_info, int n_waves,
                                                             const int32_t *__restrict__ off,
                                                             const int32_t *__restrict__ col,
                                                             const int32_t *__restrict__ cap,
                                                             double *__restrict__ scores, size_t ld) {
  const int lane = threadIdx.x % kRecWave, wv = blockIdx.x * kQuotaWaves + threadIdx.x / kRecWave;
  if (wv >= n_waves) return;  // (whole waves leave: the shuffles below stay inside one wave)
  const int info = wave_info[wv], w = info & 0xff, cats = info >> 8;
  const int pos = lane & (w - 1), g = (lane - pos) / w;
  double *row = scores + static_cast<size_t>(blockIdx.y) * ld;
  double s = -INFINITY;  // (a lane without a column: never counted by the others, never written)
  int c = INT_MAX, q = 0;
  if (g < cats) {
    const int cat = wave_first[wv] + g, lo = off[cat];
    q = cap[cat];
    if (pos < off[cat + 1] - lo) {
      c = col[lo + pos];
      s = row[c];
    }
  }
  int before = 0;  // the finite columns of the category that come before this one in the order
  for (int j = 1; j < w; ++j) {
    const int src = lane - pos + ((pos + j) & (w - 1));
    const double so = __shfl(s, src, kRecWave);
    const int co = __shfl(c, src, kRecWave);
    before += (so != -INFINITY && rec_better(so, co, s, c)) ? 1 : 0;
  }
  if (s != -INFINITY && before >= q) row[c] = -INFINITY;
}

// grid (long categories, rows of the batch), one wave per workgroup.  Category first + blockIdx.x of off / col / cap;
// `places`: the list's places (select_list of the largest cap of the launch), a score and a column each in LDS.
__global__ __launch_bounds__(kRecWave) void quota_long_kernel(const int32_t *__restrict__ off,
                                                              const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ cap, int first, int places,
                                                              double *__restrict__ scores, size_t ld) {
  extern __shared__ double quota_lds[];
  RecList<int> L{quota_lds, reinterpret_cast<int *>(quota_lds + places)};
  const int lane = threadIdx.x, cat = first + blockIdx.x;
  const int lo = off[cat], hi = off[cat + 1], q = cap[cat];
  double *row = scores + static_cast<size_t>(blockIdx.y) * ld;
  if (q == 0) {  // a banned category
    for (int e = lo + lane; e < hi; e += kRecWave) row[col[e]] = -INFINITY;
    return;
  }
  for (int base = lo; base < hi; base += kRecWave * kRecPerLane) {
    // no room for a whole round: keep the q best, raise the threshold
    if (L.cnt + kRecWave * kRecPerLane > places) rec_sort_cut<kRecWave>(L, q);
    double sv[kRecPerLane];
    int iv[kRecPerLane];
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const int at = base + e * kRecWave + lane;
      sv[e] = -INFINITY;
      iv[e] = INT_MAX;
      if (at < hi) {
        iv[e] = col[at];
        sv[e] = row[iv[e]];
      }
    }
#pragma unroll
    for (int e = 0; e < kRecPerLane; ++e) {
      const bool ok = sv[e] != -INFINITY && L.admits(sv[e], iv[e]);
      const uint64_t mask = __ballot(ok);
      const uint64_t below = lane == 0 ? 0 : (mask & ((~uint64_t(0)) >> (64 - lane)));
      if (ok) {
        const int at = L.cnt + __popcll(below);
        L.ks[at] = sv[e];
        L.kk[at] = iv[e];
      }
      L.cnt += __popcll(mask);
    }
    __syncthreads();
  }
  rec_sort_cut<kRecWave>(L, q);
  if (!L.have_thr) return;  // fewer than q finite columns: the category is never full
  const double thr_s = L.thr_s;
  const int thr_k = L.thr_k;
  for (int e = lo + lane; e < hi; e += kRecWave) {
    const int c = col[e];
    const double s = row[c];
    if (s != -INFINITY && rec_better(thr_s, thr_k, s, c)) row[c] = -INFINITY;
  }
}

}  // namespace
