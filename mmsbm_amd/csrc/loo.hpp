// loo.hpp -- leave-one-out reliability of the training rows (mmsbm_hip_loo_*): the probability of every observed rating
// under parameters that never saw it.
//
// The M-step writes theta_u as the average of its rows' shares (explain.hpp's identity) and eta_i likewise, so "one EM
// step without row j" is a downdate of two sums.  Per added slot, in EXTERNAL k, l, r, for training row j = (u, i, r):
//
//   v_j[k] = sum_l p[k,l,r] eta[i,l]          fold_v_step's chain, l ascending from +0.0
//   w_j[l] = sum_k p[k,l,r] theta[u,k]        one fma chain, k ascending from +0.0
//   fit_j  = sum_k theta[u,k] v_j[k]          one fma chain over k (hold_rows_kernel's P: the in-sample probability)
//   inv    = 1 / max(fit_j, eps)              ONE division
//   c_j[k] = (theta[u,k] v_j[k]) inv          as exp_row_kernel forms it;     e_j[l] = (eta[i,l] w_j[l]) inv
//   C_u = sum_{j in u} c_j,  E_i = sum_{j in i} e_j     (the n_theta / n_eta numerators of the EM step)
//   theta-[k] = max(C_u[k] - c_j[k], 0) / (d_u - 1)     d_u = 1: theta-bar[k], the mean theta row over the U users
//   eta-[l]   = max(E_i[l] - e_j[l], 0) / (d_i - 1)     d_i = 1: eta-bar[l], the mean eta row over the I items
//   rel_j = sum_k theta-[k] (sum_l p[k,l,r] eta-[l])    inner fma chain over l, outer fma chain over k, both from +0.0
//
// p stays the fitted p: a row is one of d_u rows of its user but one of very many soft counts of a block, and
// (n - omega) / (N - omega) is ill-conditioned for a block that only this row supports.
//
// Order of the sums over a segment (the rows of one user, or of one item, in ascending position in the training table):
// the segment is cut into chunks of kLooChunk rows; a chunk's rows are added one after the other from +0.0 in ascending
// position; the chunk sums are added one after the other from +0.0 in ascending chunk order.  The tree is fixed by the
// segment's length alone.  The same order serves the users' and items' sums of the rows' surprises.  No atomics.
//
//   loo_mean_kernel    theta-bar / eta-bar: one workgroup per column; thread t adds rows t, t + 256, ... ascending from
//                      +0.0, the 256 sums are halved 8 times (sim_mass_kernel's order), ONE division by the row count.
//   loo_fit_kernel     a group of W lanes per row (W a power of two, four entries of the wider of K and L per lane, at
//                      most 16 lanes; wider rows in pieces).  The group's lanes bring theta_u and eta_i into LDS, each
//                      lane one piece of the row: the indexed rows are gathered once, in whole contiguous pieces, and
//                      every chain then reads them on chip.  Lane x runs v's chains for k = x, x + W, x + 2 W, x + 3 W
//                      side by side (loo_chains: four independent fma chains per lane) and leaves v[k] in LDS; lane 0
//                      runs the one chain over k.  fit_j goes to the slot's fit column and is added to the row's
//                      running sum (one writer per row).  A workgroup takes kLooRounds rounds of 256 / W rows.
//   loo_sum_kernel     a group of lanes per chunk of one side (users: own = theta, other = eta, g = k; items: own = eta,
//                      other = theta, g = l): lane x takes g = x, x + W, ... and walks the chunk's rows in order, each
//                      row's (own[g] chain_g) inv read with inv = 1 / max(fit_j, eps) from the fit column, into one
//                      running sum.  Nothing of size N x K exists: a row's share is formed, added and forgotten.
//   PLDS               the three kernels above and below keep p of every rating in LDS where it fits beside the rows
//                      (R K (L | 1) doubles + the groups' rows <= 64 KB), staged once per workgroup, and read the
//                      slot's own table where it does not: the same values in the same order.  The template
//                      parameter, not a flag, so that the reads of the copy are LDS instructions (as a run-time choice
//                      between two address spaces they were flat loads and the row pass took 2.4 times as long).
//   loo_comb_kernel    a thread per (segment, g): the segment's chunk sums in chunk order; optionally one division by
//                      the segment's length (the mean surprises).
//   loo_row_kernel     a group of W lanes per row: c_j and e_j again from the four gathered rows (theta_u, eta_i, C_u,
//                      E_i) -- the same operations as in loo_sum_kernel, so the same bits --, theta- and eta- into LDS,
//                      t[k] = sum_l p[k,l,r] eta-[l] per lane, and lane 0 runs the outer chain.  rel_j is added to the
//                      row's running sum (one writer per row).
//   loo_finish_kernel  reliability = rel_sum / S, fitted = fit_sum / S (one division each), surprise = -log(max(., eps)).
//   loo_agg_kernel     a thread per chunk: the chunk's sums of both surprises (loo_comb_kernel finishes, with the mean).
//   loo_gather_kernel  the columns at a list of row positions.
//   loo_low_kernel     the m rows of smallest reliability: the candidate list of recommend.hpp (RecList, rec_sort_cut) on
//                      the score -reliability with the row position as key -- "score descending, equal scores by
//                      ascending key" is "reliability ascending, exactly equal doubles by ascending position".  One wave
//                      per range of rows, then (MERGE) one wave over the ranges' lists: the m best of a union are among
//                      the m best of each part, so the split changes nothing.
// Every number depends on its row, its user's rows, its item's rows and the added slots only, bit for bit.
#pragma once

namespace {

constexpr int kLooChunk = 64;    // rows of one chunk of a segment
constexpr int kLooWave = 64;     // loo_low_kernel: one wave per workgroup
constexpr int kLooPerLane = 4;   // rows a lane examines per round
constexpr size_t kLooLdsP = size_t(64) << 10;  // bytes of LDS up to which p of every rating is staged beside the rows

// What the row kernels read of the slot being added (external sides, ExtSlot) and of the session's training table
struct LooArgs {
  RowTab users, items;             // theta / eta rows by external id
  const double *p;                 // external (k, l, r) at p[r * rs + k * ks + l * ls]
  size_t rs;
  int ks, ls, K, L, R;
  const int32_t *user, *item, *rating;  // [N] the training table in the order it was given
  int64_t n;
};

// doubles of LDS that hold p of every rating as [r][k][L | 1] (the odd row stride keeps the lanes of a group, which read
// the same l of neighbouring k at the same time, on different banks)
__host__ __device__ inline size_t loo_p_doubles(int K, int L, int R) { return static_cast<size_t>(R) * K * (L | 1); }

// p into LDS (all kBlock threads; the caller synchronises), or not: afterwards element (k, l) of rating r is
// base[k * sk + l * sl] with base = loo_p_tile(...) -- the staged copy or the slot's own table, the same values
template <bool PLDS>
__device__ __forceinline__ void loo_stage_p(const LooArgs &a, double *pl) {
  if constexpr (!PLDS) return;
  const int kl = a.K * a.L, ldp = a.L | 1;
  for (int e = threadIdx.x; e < a.R * kl; e += kBlock) {
    const int r = e / kl, k = (e - r * kl) / a.L, l = e % a.L;
    pl[(r * a.K + k) * ldp + l] = a.p[static_cast<size_t>(r) * a.rs + static_cast<size_t>(k) * a.ks + static_cast<size_t>(l) * a.ls];
  }
}
template <bool PLDS>
__device__ __forceinline__ const double *loo_p_tile(const LooArgs &a, const double *pl, int r, int &sk, int &sl) {
  sk = PLDS ? (a.L | 1) : a.ks;
  sl = PLDS ? 1 : a.ls;
  if constexpr (PLDS) return pl + static_cast<size_t>(r) * a.K * (a.L | 1);
  else return a.p + static_cast<size_t>(r) * a.rs;
}

constexpr int kLooRounds = 8;    // rounds of kBlock / W rows a workgroup of the row kernels takes (one staging of p)
constexpr int kLooPerChain = 4;  // chains a lane runs side by side (independent fma chains: the latency of one hides
                                 // behind the others)
constexpr int kLooMaxLanes = 16; // lanes of a group at most (wider rows are walked in pieces of 4 x 16 entries)

// lanes of a group for rows of `width` entries, kLooPerChain entries per lane: a power of two, at most kLooMaxLanes
inline int loo_lanes(int width) {
  int w = 1;
  while (w * kLooPerChain < width && w < kLooMaxLanes) w <<= 1;
  return w;
}

// put(x, g, sum_t base[g * sg + t * st] vec(t)) for g = lane, lane + W, ... < G (x: which of the lane's chains of the
// piece, a constant where put is expanded): every sum ONE chain of fold_v_step over
// t ascending from +0.0.  A lane runs kLooPerChain chains side by side (g, g + W, g + 2 W, g + 3 W), G beyond that in
// pieces; a chain beyond G repeats the last one and is dropped.  How the chains are dealt to the lanes changes no bit.
template <class Vec, class Put>
__device__ __forceinline__ void loo_chains(const double *base, int sg, int st, int G, int T, int lane, int W, Vec &&vec,
                                           Put &&put) {
  for (int g0 = 0; g0 < G; g0 += kLooPerChain * W) {
    const double *pg[kLooPerChain];
    double acc[kLooPerChain];
#pragma unroll
    for (int x = 0; x < kLooPerChain; ++x) {
      pg[x] = base + static_cast<size_t>(min(g0 + x * W + lane, G - 1)) * sg;
      acc[x] = 0.0;
    }
    for (int t = 0; t < T; ++t) {
      const double e = vec(t);
#pragma unroll
      for (int x = 0; x < kLooPerChain; ++x) acc[x] = fold_v_step(pg[x], st, t, e, acc[x]);
    }
#pragma unroll
    for (int x = 0; x < kLooPerChain; ++x)
      if (g0 + x * W + lane < G) put(x, g0 + x * W + lane, acc[x]);
  }
}

// out[g] = (sum over rows of src(row, g)) / rows.  One workgroup per column g.
__global__ __launch_bounds__(kBlock) void loo_mean_kernel(RowTab src, int rows, double *__restrict__ out) {
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
  if (tid == 0) out[g] = part[0] / static_cast<double>(rows);
}

// fit[j] = sum_k theta[u,k] (sum_l p[k,l,r] eta[i,l]); fit_sum[j] += fit[j].  W lanes per row, kBlock / W rows per
// workgroup: the group's lanes bring theta_u and eta_i into LDS (one piece of the row per lane), lane x runs v's chain
// for k = x, x + W, ... and lane 0 the chain over k.  Dynamic LDS: p (when staged) + (kBlock / W) x (2 K + L) doubles.
template <bool PLDS>
__global__ __launch_bounds__(kBlock) void loo_fit_kernel(LooArgs a, int W, double *__restrict__ fit,
                                                         double *__restrict__ fit_sum) {
  extern __shared__ double loo_lds[];
  const int tid = threadIdx.x, grp = tid / W, lane = tid % W, K = a.K, L = a.L;
  double *mine = loo_lds + (PLDS ? loo_p_doubles(K, L, a.R) : 0) + static_cast<size_t>(grp) * (2 * K + L);
  double *th = mine, *vb = th + K, *et = vb + K;
  loo_stage_p<PLDS>(a, loo_lds);  // (once per workgroup: kLooRounds rounds of rows share it)
  for (int round = 0; round < kLooRounds; ++round) {  // (the same trip count for every thread: the barriers are met by all)
    const int64_t j = (static_cast<int64_t>(blockIdx.x) * kLooRounds + round) * (kBlock / W) + grp;
    const bool valid = j < a.n;
    const int64_t jj = valid ? j : 0;  // (a group without a row walks row 0 and keeps nothing)
    const size_t u = static_cast<size_t>(a.user[jj]), i = static_cast<size_t>(a.item[jj]);
    for (int k = lane; k < K; k += W) th[k] = *rowtab_ptr(a.users, u, k);
    for (int l = lane; l < L; l += W) et[l] = *rowtab_ptr(a.items, i, l);
    __syncthreads();
    int sk, sl;
    const double *pr = loo_p_tile<PLDS>(a, loo_lds, a.rating[jj], sk, sl);
    loo_chains(pr, sk, sl, K, L, lane, W, [&](int l) { return et[l]; }, [&](int, int k, double v) { vb[k] = v; });
    __syncthreads();
    if (valid && lane == 0) {
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(th[k], vb[k], acc);
      fit[j] = acc;
      fit_sum[j] += acc;
    }
    __syncthreads();  // (the rows in LDS have been read)
  }
}

// The chunks of one side's segments.  seg_off [segments + 1]: a segment's rows are rows[seg_off[s] .. seg_off[s + 1]),
// positions in the training table, ascending; chunk_seg [chunks]: the segment of a chunk; chunk_off [segments + 1]: the
// first chunk of a segment.
struct LooSide {
  const int64_t *seg_off;
  const int32_t *rows, *chunk_seg;
  const int64_t *chunk_off;
  int64_t chunks;
  int segments;
};

// part[chunk * G + g] = the chunk's rows' shares of g, added in row order from +0.0.  items_side 0: own = theta, g = k,
// the chain runs over l; 1: own = eta, g = l, the chain runs over k.  W lanes per chunk, kBlock / W chunks per workgroup.
// Dynamic LDS: p (when staged).
template <bool PLDS>
__global__ __launch_bounds__(kBlock) void loo_sum_kernel(LooArgs a, LooSide sd, int items_side, int W,
                                                         const double *__restrict__ fit, double *__restrict__ part) {
  extern __shared__ double loo_lds[];
  const int tid = threadIdx.x, grp = tid / W, lane = tid % W;
  loo_stage_p<PLDS>(a, loo_lds);
  __syncthreads();  // (the only barrier: from here on the groups go their own ways)
  const int64_t ch = static_cast<int64_t>(blockIdx.x) * (kBlock / W) + grp;
  if (ch >= sd.chunks) return;
  const int seg = sd.chunk_seg[ch];
  const int64_t first = sd.seg_off[seg] + (ch - sd.chunk_off[seg]) * kLooChunk;
  const int n = static_cast<int>(min(static_cast<int64_t>(kLooChunk), sd.seg_off[seg + 1] - first));
  const int G = items_side ? a.L : a.K, T = items_side ? a.K : a.L;
  const RowTab &own = items_side ? a.items : a.users, &other = items_side ? a.users : a.items;
  const int32_t *other_id = items_side ? a.user : a.item;
  for (int g0 = 0; g0 < G; g0 += kLooPerChain * W) {  // (a piece of the row: kLooPerChain entries per lane)
    const int ng = min(kLooPerChain * W, G - g0);
    double mine[kLooPerChain], acc[kLooPerChain];
#pragma unroll
    for (int x = 0; x < kLooPerChain; ++x) {
      mine[x] = *rowtab_ptr(own, static_cast<size_t>(seg), g0 + min(x * W + lane, ng - 1));
      acc[x] = 0.0;
    }
    for (int t = 0; t < n; ++t) {
      const int32_t j = sd.rows[first + t];
      const size_t o = static_cast<size_t>(other_id[j]);
      int sk, sl;
      const double *pr = loo_p_tile<PLDS>(a, loo_lds, a.rating[j], sk, sl);
      const int gs = items_side ? sl : sk, ts = items_side ? sk : sl;
      const double inv = 1.0 / fmax(fit[j], kEps);
      loo_chains(pr + static_cast<size_t>(g0) * gs, gs, ts, ng, T, lane, W,
                 [&](int x) { return *rowtab_ptr(other, o, x); },
                 [&](int x, int, double v) { acc[x] += (mine[x] * v) * inv; });
    }
#pragma unroll
    for (int x = 0; x < kLooPerChain; ++x)
      if (x * W + lane < ng) part[ch * G + g0 + x * W + lane] = acc[x];
  }
}

// out[seg * G + g] = the segment's chunk sums part[chunk * G + g] added in chunk order from +0.0; mean: divided once by
// the segment's length (a segment without rows: NaN).
__global__ __launch_bounds__(kBlock) void loo_comb_kernel(LooSide sd, int G, int mean, const double *__restrict__ part,
                                                          double *__restrict__ out) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= static_cast<size_t>(sd.segments) * G) return;
  const size_t seg = e / G, g = e % G;
  double acc = 0.0;
  for (int64_t ch = sd.chunk_off[seg]; ch < sd.chunk_off[seg + 1]; ++ch) acc += part[ch * G + g];
  if (mean) acc = acc / static_cast<double>(sd.seg_off[seg + 1] - sd.seg_off[seg]);
  out[e] = acc;
}

// rel_sum[j] += rel_j of the slot.  cu [U][K], ei [I][L]: the slot's C and E; tbar [K], ebar [L]; u_off / i_off: the
// segments' offsets (degrees).  W lanes per row; theta_u and eta_i come into LDS as in loo_fit_kernel.  Dynamic LDS:
// p (when staged) + (kBlock / W) x (3 K + 2 L) doubles.
template <bool PLDS>
__global__ __launch_bounds__(kBlock) void loo_row_kernel(LooArgs a, int W, const double *__restrict__ fit,
                                                         const double *__restrict__ cu, const double *__restrict__ ei,
                                                         const double *__restrict__ tbar,
                                                         const double *__restrict__ ebar,
                                                         const int64_t *__restrict__ u_off,
                                                         const int64_t *__restrict__ i_off,
                                                         double *__restrict__ rel_sum) {
  extern __shared__ double loo_lds[];
  const int tid = threadIdx.x, grp = tid / W, lane = tid % W, K = a.K, L = a.L;
  double *mine = loo_lds + (PLDS ? loo_p_doubles(K, L, a.R) : 0) + static_cast<size_t>(grp) * (3 * K + 2 * L);
  double *th = mine, *tm = th + K, *tt = tm + K, *et = tt + K, *em = et + L;
  loo_stage_p<PLDS>(a, loo_lds);  // (once per workgroup: kLooRounds rounds of rows share it)
  for (int round = 0; round < kLooRounds; ++round) {  // (the same trip count for every thread: the barriers are met by all)
    const int64_t j = (static_cast<int64_t>(blockIdx.x) * kLooRounds + round) * (kBlock / W) + grp;
    const bool valid = j < a.n;
    const int64_t jj = valid ? j : 0;  // (a group without a row walks row 0 and keeps nothing)
    const size_t u = static_cast<size_t>(a.user[jj]), i = static_cast<size_t>(a.item[jj]);
    const int64_t du = u_off[u + 1] - u_off[u], di = i_off[i + 1] - i_off[i];
    const double inv = 1.0 / fmax(fit[jj], kEps);
    for (int k = lane; k < K; k += W) th[k] = *rowtab_ptr(a.users, u, k);
    for (int l = lane; l < L; l += W) et[l] = *rowtab_ptr(a.items, i, l);
    __syncthreads();
    int sk, sl;
    const double *pr = loo_p_tile<PLDS>(a, loo_lds, a.rating[jj], sk, sl);
    loo_chains(pr, sl, sk, L, K, lane, W, [&](int k) { return th[k]; }, [&](int, int l, double w) {
      const double e = (et[l] * w) * inv;
      em[l] = di > 1 ? fmax(ei[i * L + l] - e, 0.0) / static_cast<double>(di - 1) : ebar[l];
    });
    loo_chains(pr, sk, sl, K, L, lane, W, [&](int l) { return et[l]; }, [&](int, int k, double v) {
      const double c = (th[k] * v) * inv;
      tm[k] = du > 1 ? fmax(cu[u * K + k] - c, 0.0) / static_cast<double>(du - 1) : tbar[k];
    });
    __syncthreads();
    loo_chains(pr, sk, sl, K, L, lane, W, [&](int l) { return em[l]; }, [&](int, int k, double t) { tt[k] = t; });
    __syncthreads();
    if (valid && lane == 0) {
      double rel = 0.0;
      for (int k = 0; k < K; ++k) rel = fma(tm[k], tt[k], rel);
      rel_sum[j] += rel;
    }
    __syncthreads();  // (the rows in LDS have been read)
  }
}

// The four columns of the S slots added: reliability, fitted (one division each) and their surprises
__global__ __launch_bounds__(kBlock) void loo_finish_kernel(const double *__restrict__ rel_sum,
                                                            const double *__restrict__ fit_sum, int64_t n, double slots,
                                                            double *__restrict__ rel, double *__restrict__ fitted,
                                                            double *__restrict__ sur, double *__restrict__ fsur) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n) return;
  const double r = rel_sum[j] / slots, f = fit_sum[j] / slots;
  rel[j] = r;
  fitted[j] = f;
  sur[j] = -log(fmax(r, kEps));
  fsur[j] = -log(fmax(f, kEps));
}

// part[chunk * 2 + {0, 1}] = the chunk's rows' surprise / fitted surprise, added in row order from +0.0
__global__ __launch_bounds__(kBlock) void loo_agg_kernel(LooSide sd, const double *__restrict__ sur,
                                                         const double *__restrict__ fsur, double *__restrict__ part) {
  const int64_t ch = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (ch >= sd.chunks) return;
  const int seg = sd.chunk_seg[ch];
  const int64_t first = sd.seg_off[seg] + (ch - sd.chunk_off[seg]) * kLooChunk;
  const int n = static_cast<int>(min(static_cast<int64_t>(kLooChunk), sd.seg_off[seg + 1] - first));
  double s = 0.0, f = 0.0;
  for (int t = 0; t < n; ++t) {
    const int32_t j = sd.rows[first + t];
    s += sur[j];
    f += fsur[j];
  }
  part[ch * 2] = s;
  part[ch * 2 + 1] = f;
}

// out_a[m] = a[rows[m]], out_b[m] = b[rows[m]]
__global__ __launch_bounds__(kBlock) void loo_gather_kernel(const int64_t *__restrict__ rows, int64_t n,
                                                            const double *__restrict__ a, const double *__restrict__ b,
                                                            double *__restrict__ out_a, double *__restrict__ out_b) {
  const int64_t m = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (m >= n) return;
  out_a[m] = a[rows[m]];
  out_b[m] = b[rows[m]];
}

// The m best of one part under the order (-reliability descending, position ascending).  One wave per workgroup.
// !MERGE: the candidates are the rows [part * per, min(n, part * per + per)) whose user and item are flagged (a null
//         flag array flags everyone); grid: parts.
// MERGE:  the candidates are the lists of `in_parts` earlier parts: in_s / in_k [p * m + k], k < in_n[p]; grid: 1.
// Output: out_s / out_k [part * m + k], k < out_n[part].  Dynamic LDS: cap x 16 bytes, cap a power of two >= m + 256.
template <bool MERGE>
__global__ __launch_bounds__(kLooWave) void loo_low_kernel(const double *__restrict__ rel,
                                                           const int32_t *__restrict__ user,
                                                           const int32_t *__restrict__ item,
                                                           const uint8_t *__restrict__ uflag,
                                                           const uint8_t *__restrict__ iflag, int64_t n, int64_t per,
                                                           const double *__restrict__ in_s,
                                                           const int64_t *__restrict__ in_k,
                                                           const int32_t *__restrict__ in_n, int in_parts, int m,
                                                           int cap, double *__restrict__ out_s,
                                                           int64_t *__restrict__ out_k, int32_t *__restrict__ out_n) {
  extern __shared__ double loo_list[];
  RecList<int64_t> L{loo_list, reinterpret_cast<int64_t *>(loo_list + cap)};
  const int lane = threadIdx.x;
  const int64_t part = blockIdx.x;
  const int64_t lo = MERGE ? 0 : part * per, hi = MERGE ? static_cast<int64_t>(in_parts) * m : min(n, lo + per);
  for (int64_t base = lo; base < hi; base += kLooWave * kLooPerLane) {
    // no room for a whole round: keep the m best, raise the threshold
    if (L.cnt + kLooWave * kLooPerLane > cap) rec_sort_cut<kLooWave>(L, m);
#pragma unroll
    for (int e = 0; e < kLooPerLane; ++e) {
      const int64_t pos = base + e * kLooWave + lane;
      bool ok = false;
      double s = -INFINITY;
      int64_t key = std::numeric_limits<int64_t>::max();
      if (pos < hi) {
        if (MERGE) {
          const int64_t q = pos / m, k = pos - q * m;
          if (k < in_n[q]) {
            s = in_s[q * m + k];
            key = in_k[q * m + k];
            ok = true;
          }
        } else if ((!uflag || uflag[user[pos]]) && (!iflag || iflag[item[pos]])) {
          s = -rel[pos];
          key = pos;
          ok = true;
        }
      }
      const bool in = ok && L.admits(s, key);
      const uint64_t mask = __ballot(in);
      const uint64_t below = lane == 0 ? 0 : (mask & ((~uint64_t(0)) >> (64 - lane)));
      if (in) {
        const int at = L.cnt + __popcll(below);
        L.ks[at] = s;
        L.kk[at] = key;
      }
      L.cnt += __popcll(mask);
    }
    __syncthreads();
  }
  rec_sort_cut<kLooWave>(L, m);
  for (int k = lane; k < L.cnt; k += kLooWave) {
    out_s[part * m + k] = L.ks[k];
    out_k[part * m + k] = L.kk[k];
  }
  if (lane == 0) out_n[part] = L.cnt;
}

}  // namespace
