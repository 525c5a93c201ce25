// diverse.hpp -- diversified top-N (mmsbm_hip_recommend_diverse) and the distance of given pairs (mmsbm_hip_similar_pairs):
// the greedy re-ranking of a user's `pool` best candidates by score + trade_off x (distance to the nearest item picked
// so far), with the scores of the open recommend session (recommend.hpp) and the distance D of the open similarity
// session (similar.hpp), on the device from end to end.
//
// Request row b, user u = users[b]:
//   pool   P = the row recommend_query_within(n = pool) returns -- ids, score bits and order (score descending, equal
//          scores by ascending item id); M = |P|.  It is selected by rec_select_kernel as it is (top_n_run's batches,
//          serve_frame.hpp) and stays on the device;
//   pick 1 t_1 = P[0];
//   pick j for j = 2 .. min(n, M): over every i of P not picked yet, m_i = min over a < j of D(t_a, i),
//          v_i = fma(trade_off, m_i, score_i) -- ONE rounding -- and t_j = the i with the largest v_i, equal v_i (as
//          doubles) to the earlier place in P;
//   out    the id, the pool's score and m at the moment of the pick (+inf for pick 1); behind min(n, M): -1, -inf, +inf.
//
// Kernels:
//   div_ids_kernel     a candidate subset gives the pool as columns of the compact table (catalogue.hpp): columns ->
//                      item ids, on the device, before the greedy kernel (it finds the profile rows by id);
//   div_greedy_kernel  one wave per request row.  The pool -- id, score, running m, picked flag: 21 bytes an entry --
//                      lives in dynamic LDS sized from `pool`; lane l owns places l, l + 64, ... and nobody else reads or
//                      writes their m and flag.  Per step a lane forms D(pick, i) of each of its places that are still
//                      open, takes the minimum into m_i (the minimum over the picks so far: min is exact, so the running
//                      form is the definition's), forms v_i, keeps its best (v, place); then a butterfly over the 64
//                      lanes (__shfl_xor, 6 levels) on (v, place) with the rule above.  No atomics, and no sum across
//                      lanes: a pair's terms are added by ONE lane in ONE order.
//   div_pairs_kernel   D of caller-given (a, b) pairs of the similarity session's side, one thread per pair.
//                      (Not "sim_pairs_kernel": every compiled sim_* kernel has to be launched by the similarity tests'
//                      own file, which knows nothing of this one.)
// Bit for bit: div_distance below is sim_dist_kernel's number with `a` as the query row -- ONE chain over
// f = s * width + j ascending from +0.0, d = q[a, f] - q[b, f], t = mf[f] * d (rounded), acc = fma(t, d, acc), then ONE
// division by S x (rows of the other side).  Exchanging a and b changes the sign of d and of t, never t * d:
// D(a, b) and D(b, a) have equal bits; D(a, a) and D between identical rows is +0.0.  Nothing depends on the tile, the
// lane, the pool's other entries or the rest of the request.
//
// The gathered candidate rows: each lane reads ITS OWN row, 4 entries (32 bytes) at a time, straight into registers --
// no LDS tile.  A profile row is `width` contiguous doubles (840 / 1,152 bytes at K R = 105 / 144), so every 32-byte
// sector a lane fetches is used whole, by that lane, exactly once per step: staging 64 rows x 16 entries through LDS
// as sim_dist_kernel does would only transpose them -- there a staged row is used by 64 outputs, here by one -- and
// costs a write, a barrier and a read per entry on top of the same global traffic.  Whole rows gathered into registers
// read at the same rate as rows staged through LDS (MI355X_MICROARCH.md, "Indexed rows: gather into LDS"), and a
// row's pool (at most 1,024 rows of about 1 KB per slot) stays in the L2 across the n - 1 steps that read it again.
// The picked row's entries and the masses are the same address in every lane (one broadcast load each).  Rows are only
// 8-byte aligned when `width` is odd, so the pieces are issued as 8-byte loads.
#pragma once

namespace {

constexpr int kDivWave = 64;   // lanes of a greedy workgroup: one wave per request row
constexpr int kDivPiece = 4;   // profile entries a lane reads ahead of its chain (32 bytes)

// D(a, b) of the similarity session: rows a and b of q (`slots` tables [rows][width], qs doubles apart), masses mf
// [slots][width], denom = S x rows of the other side.  THE chain of sim_dist_kernel (similar.hpp).
__device__ __forceinline__ double div_distance(const double *__restrict__ q, size_t qs, const double *__restrict__ mf,
                                               int width, int slots, size_t a, size_t b, double denom) {
  double acc = 0.0;
  for (int s = 0; s < slots; ++s) {
    const double *qa = q + static_cast<size_t>(s) * qs + a * width;
    const double *qb = q + static_cast<size_t>(s) * qs + b * width;
    const double *w = mf + static_cast<size_t>(s) * width;
    int j = 0;
    for (; j + kDivPiece <= width; j += kDivPiece) {
      double x[kDivPiece], y[kDivPiece], m[kDivPiece];
#pragma unroll
      for (int e = 0; e < kDivPiece; ++e) {
        x[e] = qa[j + e];
        y[e] = qb[j + e];
        m[e] = w[j + e];
      }
#pragma unroll
      for (int e = 0; e < kDivPiece; ++e) {
        const double d = x[e] - y[e];
        acc = fma(m[e] * d, d, acc);
      }
    }
    for (; j < width; ++j) {
      const double d = qa[j] - qb[j];
      acc = fma(w[j] * d, d, acc);
    }
  }
  return acc / denom;
}

// ids[e] = cand[ids[e]] for the entries in front of each row's count: ids [rows][ld] columns of the compact table
__global__ __launch_bounds__(kBlock) void div_ids_kernel(const int32_t *__restrict__ cand, int n_cand,
                                                         const int32_t *__restrict__ counts, int rows, int ld,
                                                         int32_t *__restrict__ ids) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= static_cast<size_t>(rows) * ld) return;
  const int b = static_cast<int>(e / ld), k = static_cast<int>(e - static_cast<size_t>(b) * ld);
  if (k >= counts[b]) return;
  const int col = ids[e];
  if (col >= 0 && col < n_cand) ids[e] = cand[col];
}

// out_d[a] = D(a[e], b[e]) for e < n_pairs
__global__ __launch_bounds__(kBlock) void div_pairs_kernel(const double *__restrict__ q, size_t qs,
                                                           const double *__restrict__ mf, int width, int slots,
                                                           double denom, const int32_t *__restrict__ a,
                                                           const int32_t *__restrict__ b, int64_t n_pairs,
                                                           double *__restrict__ out_d) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n_pairs) return;
  out_d[e] = div_distance(q, qs, mf, width, slots, static_cast<size_t>(a[e]), static_cast<size_t>(b[e]), denom);
}

// The greedy picks of request row b = blockIdx.x.  pool_s / pool_i [b * pool + k], k < pool_n[b]: the row's pool (item
// ids of the similarity session's rows, < rows).  Output [b * n + j]: item, score, distance; out_n[b] = min(n, pool_n[b]);
// the entries behind it are written too (-1, -inf, +inf).  One wave per workgroup; dynamic LDS: pool x 21 bytes.
__global__ __launch_bounds__(kDivWave) void div_greedy_kernel(const double *__restrict__ q, size_t qs,
                                                              const double *__restrict__ mf, int width, int slots,
                                                              int rows, double denom,
                                                              const double *__restrict__ pool_s,
                                                              const int32_t *__restrict__ pool_i,
                                                              const int32_t *__restrict__ pool_n, int pool, int n,
                                                              double lambda, int32_t *__restrict__ out_i,
                                                              double *__restrict__ out_s, double *__restrict__ out_d,
                                                              int32_t *__restrict__ out_n) {
  extern __shared__ double div_lds[];
  double *sc = div_lds, *md = div_lds + pool;                   // score, running minimum distance
  int32_t *id = reinterpret_cast<int32_t *>(div_lds + 2 * static_cast<size_t>(pool));
  unsigned char *picked = reinterpret_cast<unsigned char *>(id + pool);
  const int lane = threadIdx.x, b = blockIdx.x;
  const int M = min(max(pool_n[b], 0), pool);
  const size_t po = static_cast<size_t>(b) * pool, o = static_cast<size_t>(b) * n;
  for (int k = lane; k < M; k += kDivWave) {
    const int item = pool_i[po + k];
    sc[k] = pool_s[po + k];
    md[k] = INFINITY;
    id[k] = item;
    picked[k] = item < 0 || item >= rows;                       // (never: the pool holds ids of the catalogue)
  }
  __syncthreads();
  const int picks = min(n, M);
  int done = 0;
  int at = 0;                                                   // the place picked last: P[0] first
  while (done < picks) {
    if (done > 0) {
      const size_t t = static_cast<size_t>(__builtin_amdgcn_readfirstlane(id[at]));
      double best = -INFINITY;
      int best_at = INT_MAX;
      for (int k = lane; k < M; k += kDivWave) {                // ascending places: the earlier one keeps a tie
        if (picked[k]) continue;
        const double d = div_distance(q, qs, mf, width, slots, t, static_cast<size_t>(id[k]), denom);
        const double m = fmin(md[k], d);
        md[k] = m;
        const double v = fma(lambda, m, sc[k]);
        if (v > best || best_at == INT_MAX) {
          best = v;
          best_at = k;
        }
      }
#pragma unroll
      for (int off = kDivWave / 2; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off, kDivWave);
        const int oa = __shfl_xor(best_at, off, kDivWave);
        // a lane without a place (INT_MAX) never wins; else the larger v, equal v to the earlier place
        const bool take = oa != INT_MAX && (best_at == INT_MAX || ov > best || (ov == best && oa < best_at));
        if (take) {
          best = ov;
          best_at = oa;
        }
      }
      at = __builtin_amdgcn_readfirstlane(best_at);
      if (at < 0 || at >= M) break;                             // (no open place: cannot happen while done < picks)
    }
    if (picked[at]) break;                                      // (never: P[0] with an id outside the rows)
    if (lane == at % kDivWave) {                                // the owner of the place
      picked[at] = 1;
      out_i[o + done] = id[at];
      out_s[o + done] = sc[at];
      out_d[o + done] = md[at];
    }
    ++done;
    __syncthreads();                                            // (id[at] and picked[] are read by other lanes / steps)
  }
  for (int k = done + lane; k < n; k += kDivWave) {
    out_i[o + k] = -1;
    out_s[o + k] = -INFINITY;
    out_d[o + k] = INFINITY;
  }
  if (lane == 0) out_n[b] = done;
}

}  // namespace
