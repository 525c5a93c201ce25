// pass_dense.hpp -- the two triple passes AND the T + S stage in one launch: the C rows never leave the chip
// Included by tu_fused.hip after seg_pass.hpp and pair_block.hpp (see prelude.hpp for the order); not a stand-alone header.
#pragma once

namespace {

// ======================================================================================
// Every C row is produced by one group of lanes of the pair pass and consumed by exactly one 64-pair unit of the
// T + S launch.  In the four-launch form it goes to memory (16 MB at C3), crosses a launch boundary and is loaded
// again behind T + S's chain of dependent loads.  Here one grid has two roles, chosen per workgroup from blockIdx.x:
//
//   pair unit      one 64-pair unit of one rating (pairs_fused_kernel's mechanism; the unit computes the fixed rows A(t)
//                  of its pairs itself -- it holds the eta rows and the rating's tile anyway -- and does not read the A table)
//                    eta rows of the unit -> es, and transposed -> cst (asked for first, landed before the gathers: no
//                             register holds them)
//                    A[q,:] = pT_r eta[i_q,:]   the A launch's mat-vec (pair_block_kernel's A mode: lane = pair, wave =
//                             chunk of four outputs, the same multiply-add order), its outputs held in registers until
//                             every wave has read the eta transpose, then stored over it: cst[d][pair] = A[pair][d];
//                             the first four theta rows of round 0 are asked for before it and travel under it
//                    C[q,:] = sum_{n in pair q} theta[u_n,:] / max(theta[u_n,:] . A[q,:], eps)   seg_body's arithmetic,
//                             two rounds of 32 eight-lane groups; a group reads column `pair` of cst (A) at the start of
//                             its round and writes its finished C row into the same column at the end: no region of its own
//                    barrier; S, T = p_r^T C and the slab exactly as pair_block_body<false, true, 1, false, 256, 2, false>
//   user segments  seg_body<G, VEC, 4, 1>, unchanged
//
// The pair units come first in the grid (seg_pass_kernel's order), the user workgroups after them: short-lived, they
// only gather, and fill the slots beside the pair units while those are in their LDS and ALU phases.  (User
// workgroups first, or one pair unit per 1, 2 or 3 user workgroups: all slower, EXPERIMENTS.md section C.)  The C table is
// not written.  Arithmetic and association
// order of every sum are those of the separate launches: results are bitwise identical (tests/test_gpu_pass_dense.py).
// ======================================================================================
struct PassDenseArgs {
  RowTab theta;            // gathered by pair_user
  const int32_t *pair_off, *pair_user, *pair_item;
  const mmsbm::Chunk *chunks;  // one 64-pair unit each (empty ones: padding)
  const double *p_tiles;   // p  [R][kp][lp]  (T mat-vec)
  const double *pt_tiles;  // pT [R][lp][kp]  (A mat-vec)
  const double *eta;       // [I][lp]
  double *t_out;           // T [Q][lp]
  double *partial;         // one K x L slab per unit
  int kp, lp, spb, nsub;
  int nt;                  // bit 0: T rows as non-temporal stores
  int n_units;             // blocks [0, n_units) are pair units, the rest user workgroups
};

template <int G, int VEC>
__device__ __forceinline__ void pass_dense_unit(const PassDenseArgs &pa, int unit) {
  constexpr int CS = kUnitPairs + 1, KT = 2, TV = KT * 4, B = 4;
  constexpr int NGRP = kBlock / G, ROUNDS = kUnitPairs / NGRP;
  constexpr int CH = (G < 16) ? 2 * G : G;  // seg_body's index chunk
  static_assert(B <= G, "the rows asked for ahead of the A mat-vec take their ids from a group's first G indices");
  constexpr int NE = 3;  // eta loads per thread (ev0 .. ev2): 64 pairs x <= 24 entries / 2 per load / 256 threads
  const int kp = pa.kp, lp = pa.lp;
  extern __shared__ double lds[];
  // (shapes.hpp: pass_dense_lds)
  double *cst = lds;                                // [max(kp, lp)][CS]  transposed: the unit's eta rows, then A, then C rows
  double *es = cst + static_cast<size_t>(max(kp, lp)) * CS;  // [64][lp]  gathered eta rows ...
  double *tout = es;                                // ... then the T rows
  const mmsbm::Chunk ch = pa.chunks[unit];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int q0 = ch.q_begin, np = ch.q_end - ch.q_begin;  // (np <= 64; 0: padding of the unit list)
  const int grp = tid / G, gl = tid % G;
  typedef const double __attribute__((address_space(4))) * const_tile_ptr;
  const const_tile_ptr gtile = (const_tile_ptr)(reinterpret_cast<uintptr_t>(
      pa.p_tiles + static_cast<size_t>(ch.rating) * kp * lp));
  const const_tile_ptr gpt = (const_tile_ptr)(reinterpret_cast<uintptr_t>(
      pa.pt_tiles + static_cast<size_t>(ch.rating) * lp * kp));

  // ---- level 1: the segments' ranges of both rounds and the item ids of this thread's eta elements ----
  int beg[ROUNDS], end[ROUNDS], ids[NE];
  const int tot = np * lp;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int p = grp + r * NGRP;
    beg[r] = p < np ? pa.pair_off[q0 + p] : 0;
    end[r] = p < np ? pa.pair_off[q0 + p + 1] : 0;
  }
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int t = min(tid * 2 + j * kBlock * 2, max(tot - 2, 0));
    ids[j] = tot > 0 ? pa.pair_item[q0 + t / lp] : 0;
  }
  // ---- level 2: the eta rows, and the first index chunk of round 0 ----
  // (three named values, not an array: the array went to scratch memory)
  const auto eta_row = [&](int j) {
    const int t = min(tid * 2 + j * kBlock * 2, max(tot - 2, 0));
    return *reinterpret_cast<const double2 *>(pa.eta + static_cast<size_t>(ids[j]) * lp + t % lp);
  };
  const double2 ev0 = eta_row(0), ev1 = eta_row(1), ev2 = eta_row(2);
  int m0, m1;
  {
    const int cnt = min(CH, end[0] - beg[0]);
    m0 = cnt > 0 ? pa.pair_user[beg[0] + min(gl, cnt - 1)] : 0;
    m1 = (CH > G && cnt > 0) ? pa.pair_user[beg[0] + min(G + gl, cnt - 1)] : 0;
  }
  __builtin_amdgcn_sched_barrier(0);
  const bool act = gl * VEC < kp;
  const int lane_off = act ? gl * VEC : 0;
  const bool g_main = lane_off < pa.theta.mw;
  const double *gbase = g_main ? pa.theta.main + lane_off : pa.theta.tail + (lane_off - pa.theta.mw);
  const size_t gstride = g_main ? pa.theta.rs_m : pa.theta.rs_t;
  // ---- level 3: the first B theta rows of round 0, asked for ahead of the A mat-vec: they travel under it (the
  // barriers below wait for LDS traffic only, not for vector loads).  The same rows, clamped the same way, as the first
  // step of the segment loop would ask for; they land in the loop's own row registers.  Without this the unit gathers
  // nothing while it multiplies: C3 +1.5 us per iteration, K = 32 with L = 24 slower than reading A from the table.
  double g[B][VEC];
  {
    const int cnt = min(CH, end[0] - beg[0]);
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int id = __shfl(m0, min(b, max(cnt - 1, 0)), G);
      if (cnt > 0) load_vec<VEC>(gbase + static_cast<size_t>(id) * gstride, g[b]);  // (whole groups)
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  const auto eta_put = [&](int j, const double2 &v) {  // row-major for S, transposed for the A mat-vec
    const int t = tid * 2 + j * kBlock * 2;
    if (t < tot) {
      const int pr = t / lp, d = t - pr * lp;
      *reinterpret_cast<double2 *>(es + t) = v;
      cst[d * CS + pr] = v.x;
      cst[(d + 1) * CS + pr] = v.y;
    }
  };
  eta_put(0, ev0); eta_put(1, ev1); eta_put(2, ev2);
  if (np < kUnitPairs) {  // ragged tail of a rating: the missing pairs are zero columns
    for (int t = tid; t < (kUnitPairs - np) * lp; t += kBlock)
      cst[(t / (kUnitPairs - np)) * CS + np + t % (kUnitPairs - np)] = 0.0;
  }
  __syncthreads();
  // ---- A[q,:] = pT_r eta_q: lane = pair, wave = chunk of 4 outputs, the tile through scalar loads (pair_block's A
  // mode, multiply-add for multiply-add).  kp <= 32: a wave has at most two chunks, eight outputs in named registers ----
  {
    const int nck = kp >> 2;
    const int c0 = __builtin_amdgcn_readfirstlane(wave), c1 = c0 + kBlock / 64;
    const auto a_chunk = [&](int c, double &a0, double &a1, double &a2, double &a3) {
      for (int d = 0; d < lp; d += 4) {
        double x[4];
        double2 t0[4], t1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x[i] = cst[(d + i) * CS + lane];
          const const_tile_ptr row = gpt + static_cast<size_t>(d + i) * kp + c * 4;  // uniform
          t0[i].x = row[0]; t0[i].y = row[1];
          t1[i].x = row[2]; t1[i].y = row[3];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a0 = fma(x[i], t0[i].x, a0);
          a1 = fma(x[i], t0[i].y, a1);
          a2 = fma(x[i], t1[i].x, a2);
          a3 = fma(x[i], t1[i].y, a3);
        }
      }
    };
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    if (c0 < nck) a_chunk(c0, a0, a1, a2, a3);
    if (c1 < nck) a_chunk(c1, b0, b1, b2, b3);
    __syncthreads();  // every wave has read the eta transpose: A, transposed, takes its place
    if (c0 < nck) {
      double *col = cst + c0 * 4 * CS + lane;
      col[0] = a0; col[CS] = a1; col[2 * CS] = a2; col[3 * CS] = a3;
    }
    if (c1 < nck) {
      double *col = cst + c1 * 4 * CS + lane;
      col[0] = b0; col[CS] = b1; col[2 * CS] = b2; col[3 * CS] = b3;
    }
    __syncthreads();
  }

  // ---- the pair segments (seg_body's arithmetic): a group of G lanes per pair, its C row into cst ----
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int p = grp + r * NGRP;
    double f[VEC], acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
    if (p < np) {  // (whole groups)
#pragma unroll
      for (int v = 0; v < VEC; ++v) f[v] = act ? cst[(lane_off + v) * CS + p] : 0.0;  // A(t)[q0 + p]: this group's column
      int mine0 = m0, mine1 = m1;
      if (r > 0) {  // (round 0's first indices were asked for beside the eta rows)
        const int cnt = min(CH, end[r] - beg[r]);
        mine0 = cnt > 0 ? pa.pair_user[beg[r] + min(gl, cnt - 1)] : 0;
        mine1 = (CH > G && cnt > 0) ? pa.pair_user[beg[r] + min(G + gl, cnt - 1)] : 0;
      }
      bool ahead = r == 0;  // (the first step of round 0: its rows were asked for before the A mat-vec and are in g)
      for (int c0 = beg[r]; c0 < end[r]; c0 += CH) {
        const int cnt = min(CH, end[r] - c0);
        for (int n = 0; n < cnt; n += B) {
          if (!ahead) {
#pragma unroll
            for (int b = 0; b < B; ++b) {
              const int jj = min(n + b, cnt - 1);
              const int id = __shfl((CH > G && jj >= G) ? mine1 : mine0, jj, G);
              load_vec<VEC>(gbase + static_cast<size_t>(id) * gstride, g[b]);
            }
          }
          ahead = false;
#pragma unroll
          for (int b = 0; b < B; ++b) {
            if (n + b < cnt) {
              double pt = 0.0;
#pragma unroll
              for (int v = 0; v < VEC; ++v) pt = fma(g[b][v], f[v], pt);
              const double s = group_sum<G>(pt);
              const double w = 1.0 / fmax(s, kEps);
#pragma unroll
              for (int v = 0; v < VEC; ++v) acc[v] = fma(g[b][v], w, acc[v]);
            }
          }
        }
        if (c0 + CH < end[r]) {  // (more than one index chunk: the next one, as seg_body fetches it)
          const int c1 = c0 + CH, cn = min(CH, end[r] - c1);
          mine0 = pa.pair_user[c1 + min(gl, cn - 1)];
          mine1 = (CH > G) ? pa.pair_user[c1 + min(G + gl, cn - 1)] : 0;
        }
      }
    }
    if (act) {  // (pairs >= np: zero columns)
#pragma unroll
      for (int v = 0; v < VEC; ++v) cst[(lane_off + v) * CS + p] = acc[v];
    }
  }
  __syncthreads();

  // ---- S: thread = (k, 4 l) slot of a KT x 4 register tile, copies split the unit's pairs (pair_block_body) ----
  const int nch = lp >> 2;
  const int nslot = (kp / KT) * nch, spb = pa.spb, nsub = pa.nsub;
  const int sub = tid / spb, slot0 = tid % spb;
  const bool s_active = sub < nsub;
  const int o = min(slot0, nslot - 1);
  const int coff = (o / nch) * KT * CS, eoff = (o % nch) * 4;
  double sacc[TV];
#pragma unroll
  for (int j = 0; j < TV; ++j) sacc[j] = 0.0;
  if (s_active) {
#pragma unroll 2
    for (int j = sub; j < np; j += nsub) {
      double cv[KT];
#pragma unroll
      for (int i = 0; i < KT; ++i) cv[i] = cst[coff + i * CS + j];
      const double2 e0 = *reinterpret_cast<const double2 *>(es + j * lp + eoff);
      const double2 e1 = *reinterpret_cast<const double2 *>(es + j * lp + eoff + 2);
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        sacc[4 * i + 0] = fma(cv[i], e0.x, sacc[4 * i + 0]);
        sacc[4 * i + 1] = fma(cv[i], e0.y, sacc[4 * i + 1]);
        sacc[4 * i + 2] = fma(cv[i], e1.x, sacc[4 * i + 2]);
        sacc[4 * i + 3] = fma(cv[i], e1.y, sacc[4 * i + 3]);
      }
    }
  }
  __syncthreads();  // es is dead: its space takes the T rows
  // ---- T[q,:] = p_r^T C_q: lane = pair, wave = chunk of 4 outputs; the tile through scalar loads ----
  for (int c = __builtin_amdgcn_readfirstlane(wave); c < nch; c += kBlock / 64) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int d = 0; d < kp; d += 4) {
      double x[4];
      double2 t0[4], t1[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[i] = cst[(d + i) * CS + lane];
        const const_tile_ptr row = gtile + static_cast<size_t>(d + i) * lp + c * 4;  // uniform
        t0[i].x = row[0]; t0[i].y = row[1];
        t1[i].x = row[2]; t1[i].y = row[3];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a0 = fma(x[i], t0[i].x, a0);
        a1 = fma(x[i], t0[i].y, a1);
        a2 = fma(x[i], t1[i].x, a2);
        a3 = fma(x[i], t1[i].y, a3);
      }
    }
    double2 w0, w1;
    w0.x = a0; w0.y = a1; w1.x = a2; w1.y = a3;
    *reinterpret_cast<double2 *>(tout + lane * lp + c * 4) = w0;
    *reinterpret_cast<double2 *>(tout + lane * lp + c * 4 + 2) = w1;
  }
  __syncthreads();
  {  // the unit's T rows are contiguous in memory
    double *dst = pa.t_out + static_cast<size_t>(q0) * lp;
    for (int t = tid * 2; t < tot; t += kBlock * 2)
      store_out2(dst + t, *reinterpret_cast<const double2 *>(tout + t), (pa.nt & 1) != 0);
  }
  // ---- the slab: the other copies hand their sums over through LDS, added in copy order ----
  if (nsub > 1) {
    __syncthreads();
    if (s_active && sub > 0 && slot0 < nslot) {
#pragma unroll
      for (int j = 0; j < TV; ++j) lds[(j * (nsub - 1) + sub - 1) * nslot + slot0] = sacc[j];
    }
    __syncthreads();
    if (sub == 0 && slot0 < nslot) {
      for (int oo = 1; oo < nsub; ++oo)
#pragma unroll
        for (int j = 0; j < TV; ++j) sacc[j] += lds[(j * (nsub - 1) + oo - 1) * nslot + slot0];
    }
  }
  if (sub == 0 && slot0 < nslot) {
    double *cell = pa.partial + static_cast<size_t>(unit) * kp * lp + (o / nch) * KT * lp + eoff;
#pragma unroll
    for (int h = 0; h < KT; ++h) {
      double2 x, y;
      x.x = sacc[4 * h]; x.y = sacc[4 * h + 1]; y.x = sacc[4 * h + 2]; y.y = sacc[4 * h + 3];
      *reinterpret_cast<double2 *>(cell + h * lp) = x;
      *reinterpret_cast<double2 *>(cell + h * lp + 2) = y;
    }
  }
}

// (second launch bound: seg_pass_kernel's six waves per SIMD, i.e. <= 80 VGPRs -- the gathers' rows in flight are what
// the launch lives on)
template <int G, int VEC>
__global__ __launch_bounds__(kBlock, 6) void pass_dense_kernel(PassDenseArgs pa, SegArgs su, int dp) {
  const int bx = static_cast<int>(blockIdx.x);
  if (bx < pa.n_units) pass_dense_unit<G, VEC>(pa, bx);
  else seg_body<G, VEC, 4, 1>(su, (bx - pa.n_units) * (kBlock / G) + threadIdx.x / G, dp, 1);
}

}  // namespace
