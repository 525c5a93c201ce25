// fold_in.hpp -- fold new users into a fitted model (mmsbm_hip_fold_in): the theta half of the M-step for users that
// were not in the training triples, with eta and p of the selected slot held fixed, iterated to a fixed point on chip.
//
//   v_j[k]      = sum_l p[k, l, r_j] eta[i_j, l]                                    (row j = (u, i_j, r_j), external)
//   theta'_u[k] = (1/d_u) sum_{j in u} theta_u[k] v_j[k] / max(theta_u . v_j, eps)
//
// With v fixed this is EM for the mixture weights of one user: sum_j log(theta_u . v_j) never decreases, and every user
// is a problem of its own (d_u x K numbers).  fold_v_kernel forms v once per request row (one fma chain over l in
// ascending order); fold_kernel then runs ALL iterations of a user in one launch, theta_u in registers:
//   - a group of G lanes per user holds K in NT registers per lane (k = lane + G t); a row's dot product is the lane's
//     own sum over t followed by a butterfly over the G lanes (every lane ends with the same bits: fp addition is
//     commutative), then ONE division 1 / max(dot, eps) and an fma per k;
//   - RS = 1: the group walks the rows one after the other; the rows (d_u x K doubles) sit in LDS, copied once;
//   - RS = 64 / G (one wave per user): the wave's G-lane groups take every RS-th row and the RS partial sums are added by
//     a butterfly at the end of the iteration; the rows are read from global memory every iteration (long users).
// Which form a user gets depends on d_u and K only (fold_onchip), so a user's theta is bitwise the same whatever the
// other users asked with it.  All of it is in EXTERNAL terms (a swapped context reads the same numbers).  No atomics.
#pragma once

namespace {

constexpr int kFoldWave = 64;            // one wave per workgroup
constexpr int kFoldUserLds = 1024;       // doubles of rows a user may keep in LDS (8 KB): more, the streamed form
constexpr int kFoldWaveLds = 1024;       // doubles of rows the users of one wave keep in LDS together
constexpr int kFoldMaxK = 1024;          // K the register forms cover (64 lanes x 16)

// the (G, NT) instantiation for K: code 0..8 (-1: beyond kFoldMaxK)
inline int fold_code(int K) {
  if (K <= 4) return 0;
  if (K <= 8) return 1;
  if (K <= 16) return 2;
  if (K <= 32) return 3;
  if (K <= 64) return 4;
  if (K <= 128) return 5;
  if (K <= 256) return 6;
  if (K <= 512) return 7;
  if (K <= kFoldMaxK) return 8;
  return -1;
}
inline int fold_lanes(int code) {
  static const int g[9] = {1, 2, 4, 8, 16, 32, 64, 64, 64};
  return g[code];
}
// a user's rows stay in LDS when they are few enough (depends on d_u and K only)
inline bool fold_onchip(int64_t d, int K) { return d * K <= kFoldUserLds; }

#define DISPATCH_FOLD(code, CALL) \
  switch (code) {                 \
    case 0: CALL(1, 4); break;    \
    case 1: CALL(2, 4); break;    \
    case 2: CALL(4, 4); break;    \
    case 3: CALL(8, 4); break;    \
    case 4: CALL(16, 4); break;   \
    case 5: CALL(32, 4); break;   \
    case 6: CALL(64, 4); break;   \
    case 7: CALL(64, 8); break;   \
    default: CALL(64, 16); break; \
  }

// THE link of v's chain (the one copy: fold_v_at here and exp_row_kernel of explain.hpp, which keeps the eta row in
// registers): acc + p(k, l, r) eta(item, l) as one fma, `pk` = p + r * rs + k * ks.
__device__ __forceinline__ double fold_v_step(const double *__restrict__ pk, int ls, int l, double eta_l, double acc) {
  return fma(pk[static_cast<size_t>(l) * ls], eta_l, acc);
}

// v[k] of a row (item, rating) = sum_l p(k, l, rating) eta(item, l): ONE chain of fold_v_step over l ascending from
// +0.0.  p of one slot, element (k, l, r) at p + r * rs + k * ks + l * ls in external (k, l); `et`: the external items'
// rows.
__device__ __forceinline__ double fold_v_at(const RowTab &et, const double *__restrict__ p, size_t rs, int ks, int ls,
                                            int32_t item, int32_t rating, int k, int L) {
  const double *pk = p + static_cast<size_t>(rating) * rs + static_cast<size_t>(k) * ks;
  const size_t i = static_cast<size_t>(item);
  double acc = 0.0;
  for (int l = 0; l < L; ++l) acc = fold_v_step(pk, ls, l, *rowtab_ptr(et, i, l), acc);
  return acc;
}

// v[j * K + k] = fold_v_at(item[j], rating[j], k) for every row j of the request and every k.
__global__ __launch_bounds__(kBlock) void fold_v_kernel(RowTab et, const double *__restrict__ p, size_t rs, int ks,
                                                        int ls, const int32_t *__restrict__ item,
                                                        const int32_t *__restrict__ rating, int64_t rows, int K, int L,
                                                        double *__restrict__ v) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= static_cast<size_t>(rows) * K) return;
  const size_t j = e / K;
  const int k = static_cast<int>(e % K);
  v[e] = fold_v_at(et, p, rs, ks, ls, item[j], rating[j], k, L);
}

// One job per group of G * RS lanes: int2 (user, LDS offset in doubles); user -1: no work.  Users are local to the batch:
// rows off[u] .. off[u + 1] of v, theta0 / theta rows u ([u][K]), iters[u].
template <int G, int NT, int RS, bool ONCHIP>
__global__ __launch_bounds__(kFoldWave) void fold_kernel(const int2 *__restrict__ jobs, const int64_t *__restrict__ off,
                                                         const double *__restrict__ v, const double *__restrict__ th0,
                                                         double *__restrict__ th, int32_t *__restrict__ iters, int K,
                                                         int n_iters, double tol) {
  constexpr int GS = G * RS, GPW = kFoldWave / GS;
  static_assert(GS <= kFoldWave && kFoldWave % GS == 0, "group size");
  extern __shared__ double fold_lds[];
  const int lane = threadIdx.x, grp = lane / GS, gl = lane % GS, kl = lane % G, rs = gl / G;
  const int2 job = jobs[static_cast<size_t>(blockIdx.x) * GPW + grp];
  const int u = job.x;
  const bool active = u >= 0;
  int64_t a = 0;
  int d = 0;
  if (active) {
    a = off[u];
    d = static_cast<int>(off[u + 1] - a);
  }
  const double *vu = v + static_cast<size_t>(a) * K;
  if constexpr (ONCHIP) {
    if (active)
      for (int e = gl; e < d * K; e += GS) fold_lds[job.y + e] = vu[e];
    __syncthreads();
  }
  if (!active) return;
  auto vat = [&](int j, int k) -> double {
    if constexpr (ONCHIP) return fold_lds[job.y + j * K + k];
    else return vu[static_cast<size_t>(j) * K + k];
  };
  double t[NT];
#pragma unroll
  for (int x = 0; x < NT; ++x) {
    const int k = kl + G * x;
    t[x] = k < K ? th0[static_cast<size_t>(u) * K + k] : 0.0;
  }
  const double dd = static_cast<double>(d);
  int used = n_iters;
  for (int it = 0; it < n_iters; ++it) {
    double acc[NT];
#pragma unroll
    for (int x = 0; x < NT; ++x) acc[x] = 0.0;
    for (int j = rs; j < d; j += RS) {
      double q[NT];
      double dot = 0.0;
#pragma unroll
      for (int x = 0; x < NT; ++x) {
        const int k = kl + G * x;
        q[x] = k < K ? t[x] * vat(j, k) : 0.0;
        dot += q[x];
      }
#pragma unroll
      for (int m = 1; m < G; m <<= 1) dot += __shfl_xor(dot, m);
      const double inv = 1.0 / fmax(dot, kEps);
#pragma unroll
      for (int x = 0; x < NT; ++x) acc[x] = fma(q[x], inv, acc[x]);
    }
#pragma unroll
    for (int m = G; m < GS; m <<= 1)
#pragma unroll
      for (int x = 0; x < NT; ++x) acc[x] += __shfl_xor(acc[x], m);
    double delta = 0.0;
#pragma unroll
    for (int x = 0; x < NT; ++x) {
      const double nv = acc[x] / dd;
      delta = fmax(delta, fabs(nv - t[x]));
      t[x] = nv;
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) delta = fmax(delta, __shfl_xor(delta, m));
    if (tol > 0.0 && delta <= tol) {
      used = it + 1;
      break;
    }
  }
  if (rs == 0) {
#pragma unroll
    for (int x = 0; x < NT; ++x) {
      const int k = kl + G * x;
      if (k < K) th[static_cast<size_t>(u) * K + k] = t[x];
    }
    if (kl == 0) iters[u] = used;
  }
}

}  // namespace
