// heldout.hpp -- held-out predictive log-likelihood (mmsbm_hip_heldout_*): log P(observed rating | user, item) summed
// over rows the fit has not seen, for every restart slot in one set of launches.
//
// For a row m = (u, i, r) and the parameters of one slot (EXTERNAL k, l, r: the model is read through ExtSlot):
//   t[k] = sum_l p[k, l, r] eta[i, l]        one fma chain over l ascending, from +0.0
//   P(m) = sum_k theta[u, k] t[k]            one fma chain over k ascending, from +0.0
//   ll   = sum_m log(max(P(m), eps))
// The session keeps its rows rating-major (a stable counting sort at begin) and cuts every rating's run into blocks of
// at most kHoldRows rows: a workgroup works under ONE p_r, staged in LDS where it fits (PLDS) and read from global
// memory where it does not.
//   hold_rows_kernel   grid (blocks, slots).  G lanes per row -- G follows the row width as the (G, VEC) forms of the
//                      triple passes do, so kBlock / G rows are in flight per workgroup.  Lane g of a group owns
//                      k = g, g + G, ... of the current piece of 4 G groups: it runs that k's chain over l with the row's
//                      eta staged in LDS (read by broadcast), leaves t[k] in LDS, and then EVERY lane of the group runs
//                      the one chain over k (broadcast reads again: no cross-lane traffic, all lanes hold the same
//                      bits).  K, L beyond 4 G are walked in pieces of 4 G; t[k] carries over the pieces of l and the
//                      chain over k over the pieces of k, so the operations and their order are those above whatever
//                      G, PLDS, the block, the slot count or the side layout.  Row j of the block leaves
//                      log(max(P, eps)) in LDS entry j; with `sum` set (heldout_add) it also adds P to the row's
//                      running sum, in request order -- one writer per row, no atomics.
//   block sum          the kHoldRows entries (zero beyond the block's rows) are halved 8 times (stride 128, 64, ... 1):
//                      an order that depends on the number of rows of the block only.
//   hold_sum_kernel    one workgroup per slot: thread t adds the block sums t, t + 256, ... in ascending order from
//                      +0.0, then the same halving.  The blocks depend on the session's rows only, so ll is bitwise the
//                      same from call to call, whatever the slot count and the CU count.  No rows: ll = +0.0.
//   hold_mean_kernel   (heldout_mean) P_mean(m) = sum(m) / S -- one division --, its log, and block sums over the rows
//                      in REQUEST order, kHoldRows at a time; hold_sum_kernel finishes.
#pragma once

namespace {

constexpr int kHoldRows = kBlock;  // rows of one block = entries of one block sum

struct HoldArgs {
  RowTab users, items;        // the external users' / items' rows of the launch's first slot; slot s: slot_tab(., s)
  const double *p;            // that slot's p: external (k, l, r) at p[r * rs + k * ks + l * ls]; slot s: + s * p_slot
  size_t p_slot, rs;
  int ks, ls;
  const int32_t *user, *item, *orig;  // the session's rows (rating-major) and their place in the request
  const int4 *blocks;         // (rating, first row, rows, 0)
  int K, L;
  double *part;               // [slot][blocks]: the block sums
  size_t part_slot;
  double *sum;                // null, or the running per-row sum of P (request order)
};

// lds[0 .. kBlock) -> lds[0]; the caller has synchronised its writes
__device__ __forceinline__ void hold_halve(double *lds, int tid) {
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o) lds[tid] += lds[tid + o];
    __syncthreads();
  }
}

// doubles of dynamic LDS: the block's logs, per group a piece of theta, of eta and of t (4 G + 1 doubles each: the odd
// stride puts the groups of a wave, which read the same entry of their own piece at the same time, on different banks;
// at most kBlock / 4 groups), and the rating's tile
constexpr int kHoldStage = 4 * kBlock + kBlock / 4;
inline size_t hold_lds_doubles(int K, int L, bool plds) {
  return static_cast<size_t>(kHoldRows) + 3 * kHoldStage + (plds ? static_cast<size_t>(K) * (L | 1) : 0);
}

template <int G, bool PLDS>
__global__ __launch_bounds__(kBlock) void hold_rows_kernel(HoldArgs a) {
  constexpr int NG = kBlock / G, KC = 4 * G, GS = KC + 1;  // rows in flight, groups per piece, a group's stride in LDS
  static_assert(NG * GS <= kHoldStage, "staging area");
  extern __shared__ double hold_lds[];
  double *lg = hold_lds;                      // [kHoldRows]
  double *ths = lg + kHoldRows;               // [NG][GS] each, kHoldStage apart
  double *es = ths + kHoldStage, *tts = es + kHoldStage;
  double *pl = tts + kHoldStage;              // [K][ldp] (PLDS)
  const int tid = threadIdx.x, grp = tid / G, lane = tid % G;
  const int4 blk = a.blocks[blockIdx.x];
  const int first = blk.y, rows = blk.z, K = a.K, L = a.L, ldp = L | 1;
  const size_t slot = blockIdx.y;
  const RowTab users = slot_tab(a.users, slot), items = slot_tab(a.items, slot);
  const double *pr = a.p + slot * a.p_slot + static_cast<size_t>(blk.x) * a.rs;
  lg[tid] = 0.0;
  if constexpr (PLDS)
    for (int e = tid; e < K * L; e += kBlock) {
      const int k = e / L, l = e - k * L;
      pl[k * ldp + l] = pr[static_cast<size_t>(k) * a.ks + static_cast<size_t>(l) * a.ls];
    }
  double *my_th = ths + grp * GS, *my_e = es + grp * GS, *my_t = tts + grp * GS;
  const int n_it = (rows + NG - 1) / NG;
  for (int it = 0; it < n_it; ++it) {  // (every trip count below is the same for all threads: the barriers are met by all)
    const int j = it * NG + grp;
    const bool valid = j < rows;
    const int m = first + (valid ? j : 0);  // (a group without a row walks the block's first one and keeps nothing)
    const size_t u = static_cast<size_t>(a.user[m]), i = static_cast<size_t>(a.item[m]);
    double acc = 0.0;
    for (int k0 = 0; k0 < K; k0 += KC) {
      const int nk = min(KC, K - k0);
      int kx[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int kk = x * G + lane;
        my_th[kk] = kk < nk ? *rowtab_ptr(users, u, k0 + kk) : 0.0;
        kx[x] = k0 + min(kk, nk - 1);  // (beyond the piece: an address inside the tile, a value nobody reads)
      }
      double t[4] = {0.0, 0.0, 0.0, 0.0};
      for (int l0 = 0; l0 < L; l0 += KC) {
        const int nl = min(KC, L - l0);
        __syncthreads();  // the last piece of eta has been read
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int ll = x * G + lane;
          my_e[ll] = ll < nl ? *rowtab_ptr(items, i, l0 + ll) : 0.0;
        }
        __syncthreads();
        for (int ll = 0; ll < nl; ++ll) {
          const double e = my_e[ll];
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            double pv;
            if constexpr (PLDS) pv = pl[kx[x] * ldp + l0 + ll];
            else pv = pr[static_cast<size_t>(kx[x]) * a.ks + static_cast<size_t>(l0 + ll) * a.ls];
            t[x] = fma(pv, e, t[x]);
          }
        }
      }
#pragma unroll
      for (int x = 0; x < 4; ++x) my_t[x * G + lane] = t[x];
      __syncthreads();
      for (int kk = 0; kk < nk; ++kk) acc = fma(my_th[kk], my_t[kk], acc);
      __syncthreads();  // theta and t of this piece have been read
    }
    if (valid && lane == 0) {
      lg[j] = log(fmax(acc, kEps));
      if (a.sum) a.sum[a.orig[m]] += acc;
    }
  }
  __syncthreads();
  hold_halve(lg, tid);
  if (tid == 0) a.part[slot * a.part_slot + blockIdx.x] = lg[0];
}

// out[slot] = the n block sums of the slot, added as stated above
__global__ __launch_bounds__(kBlock) void hold_sum_kernel(const double *__restrict__ part, size_t part_slot, int n,
                                                          double *__restrict__ out) {
  __shared__ double lds[kBlock];
  const int tid = threadIdx.x;
  const double *mine = part + blockIdx.x * part_slot;
  double acc = 0.0;
  for (int b = tid; b < n; b += kBlock) acc += mine[b];
  lds[tid] = acc;
  __syncthreads();
  hold_halve(lds, tid);
  if (tid == 0) out[blockIdx.x] = lds[0];
}

// mean[m] = sum[m] / denom, part[b] = the block sum of log(max(mean, eps)) over rows b * kHoldRows ... (request order)
__global__ __launch_bounds__(kBlock) void hold_mean_kernel(const double *__restrict__ sum, int64_t rows, double denom,
                                                           double *__restrict__ mean, double *__restrict__ part) {
  __shared__ double lds[kBlock];
  const int tid = threadIdx.x;
  const int64_t m = static_cast<int64_t>(blockIdx.x) * kHoldRows + tid;
  double v = 0.0;
  if (m < rows) {
    const double pm = sum[m] / denom;
    mean[m] = pm;
    v = log(fmax(pm, kEps));
  }
  lds[tid] = v;
  __syncthreads();
  hold_halve(lds, tid);
  if (tid == 0) part[blockIdx.x] = lds[0];
}

}  // namespace
