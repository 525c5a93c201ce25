// tu_pairs_bulk.hip -- translation unit of the device sorts behind mmsbm_hip_recommend_top_pairs_bulk (pairs_bulk.hpp):
// the collected bin of the radix select, and phase 3, the order of the m entries.  The sorts are rocPRIM's stable radix
// sorts -- library calls for a library job, as in tu_layout.hip; the two kernels around them are element-wise.  Also the
// sort of a round's bids of mmsbm_hip_recommend_assign (assign.hpp): rocPRIM's merge sort under a strict total order.
#include "prelude.hpp"

#include <rocprim/rocprim.hpp>

namespace mmsbm_hip_impl {

namespace {

// skey[j] = the order key of score[j], idx[j] = j
__global__ __launch_bounds__(kBlock) void pbulk_sortkey_kernel(const double *__restrict__ score, size_t n,
                                                               uint64_t *__restrict__ skey, uint32_t *__restrict__ idx) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n) return;
  skey[j] = pb_key_of_bits(static_cast<uint64_t>(__double_as_longlong(score[j])));
  idx[j] = static_cast<uint32_t>(j);
}

// out[j] = in[idx[j]] of both columns
__global__ __launch_bounds__(kBlock) void pbulk_gather_kernel(const uint32_t *__restrict__ idx,
                                                              const uint64_t *__restrict__ key,
                                                              const double *__restrict__ score, size_t n,
                                                              uint64_t *__restrict__ out_key,
                                                              double *__restrict__ out_score) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t e = idx[j];
  out_key[j] = key[e];
  out_score[j] = score[e];
}

unsigned blocks_for(size_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

// The order of the bids of a round of assign.hpp, over their places: item ascending, bid descending, place ascending
// -- a strict total order, so the sorted sequence is one whatever the sort's own order of work
struct AssignBidBefore {
  const int32_t *item;
  const double *bid;
  __device__ bool operator()(uint32_t a, uint32_t b) const {
    const int32_t ia = item[a], ib = item[b];
    if (ia != ib) return ia < ib;
    const double ba = bid[a], bb = bid[b];
    if (ba != bb) return ba > bb;
    return a < b;
  }
};

}  // namespace

size_t assign_sort_bytes(size_t n) {
  size_t bytes = 0;
  HIP_CHECK(rocprim::merge_sort(nullptr, bytes, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr),
                                std::max<size_t>(n, 1), AssignBidBefore{nullptr, nullptr}, hipStream_t(nullptr)));
  return bytes;
}

void assign_sort_bids(hipStream_t st, void *tmp, size_t bytes, const int32_t *item, const double *bid,
                      const uint32_t *place, uint32_t *sorted, size_t n) {
  if (n == 0) return;
  HIP_CHECK(rocprim::merge_sort(tmp, bytes, place, sorted, n, AssignBidBefore{item, bid}, st));
}

void pairs_bulk_sort_desc(mmsbm_hip_ctx *c, const uint64_t *keys, uint64_t *sorted, size_t n) {
  if (n == 0) return;
  hipStream_t st = c->stream;
  size_t bytes = 0;
  HIP_CHECK(rocprim::radix_sort_keys_desc(nullptr, bytes, keys, sorted, n, 0u, 64u, st));
  DevBuf<char> tmp;
  tmp.alloc(bytes);
  HIP_CHECK(rocprim::radix_sort_keys_desc(tmp.ptr, bytes, keys, sorted, n, 0u, 64u, st));
  HIP_CHECK(hipStreamSynchronize(st));  // (tmp goes with the scope)
}

void pairs_bulk_order(mmsbm_hip_ctx *c, const uint64_t *key, const double *score, size_t n, uint64_t *out_key,
                      double *out_score) {
  if (n == 0) return;
  hipStream_t st = c->stream;
  DevBuf<uint64_t> k1, skey, skey2;
  DevBuf<double> s1;
  DevBuf<uint32_t> idx, idx2;
  DevBuf<char> tmp;
  k1.alloc(n); s1.alloc(n); skey.alloc(n); skey2.alloc(n); idx.alloc(n); idx2.alloc(n);
  size_t b1 = 0, b2 = 0;
  HIP_CHECK(rocprim::radix_sort_pairs(nullptr, b1, key, k1.ptr, score, s1.ptr, n, 0u, 64u, st));
  HIP_CHECK(rocprim::radix_sort_pairs_desc(nullptr, b2, skey.ptr, skey2.ptr, idx.ptr, idx2.ptr, n, 0u, 64u, st));
  const size_t bytes = std::max(b1, b2);
  tmp.alloc(bytes);
  // by (user, item) ascending; then, stable, by the score's key descending: equal scores stay in (user, item) order
  size_t tb = bytes;
  HIP_CHECK(rocprim::radix_sort_pairs(tmp.ptr, tb, key, k1.ptr, score, s1.ptr, n, 0u, 64u, st));
  LAUNCH(pbulk_sortkey_kernel, blocks_for(n), kBlock, 0, st, static_cast<const double *>(s1.ptr), n, skey.ptr, idx.ptr);
  tb = bytes;
  HIP_CHECK(rocprim::radix_sort_pairs_desc(tmp.ptr, tb, skey.ptr, skey2.ptr, idx.ptr, idx2.ptr, n, 0u, 64u, st));
  LAUNCH(pbulk_gather_kernel, blocks_for(n), kBlock, 0, st, static_cast<const uint32_t *>(idx2.ptr),
         static_cast<const uint64_t *>(k1.ptr), static_cast<const double *>(s1.ptr), n, out_key, out_score);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(st));  // (the buffers go with the scope)
}

}  // namespace mmsbm_hip_impl
