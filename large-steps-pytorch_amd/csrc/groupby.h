// groupby.h -- what the backward passes of the renderer (raster.hip, texture.hip) share: items grouped by an int key with the sort of
// radix.h, and a sum over the items of every key in ONE fixed order. No float atomics anywhere: the order of additions below IS the
// definition that the bitwise reproducibility of those gradients, and the error bounds of their tests, rest on.
#pragma once
#include "common.h"
#include "radix.h"

namespace ls {

template <int UNIT = 0>
__global__ __launch_bounds__(256) void k_gb_sorted_keys(const int* __restrict__ keys, const int* __restrict__ order, int64_t n, int* __restrict__ sk) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) sk[i] = keys[order[i]];
}

// seg[k] = first sorted position whose key is >= k, k in [0, nk]
template <int UNIT = 0>
__global__ __launch_bounds__(256) void k_gb_segments(const int* __restrict__ sk, int64_t n, int64_t nk, int* __restrict__ seg) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > nk) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sk[mid] < k) lo = mid + 1; else hi = mid;
    }
    seg[k] = (int)lo;
}

// The sum of one key per thread, keys [0, nkeys) over a grid of 256-thread workgroups. A key of at most 64 items is added by its own
// thread, items in order; a longer one by its whole wave, lane l adding items l, l + 64, ... in order and wave_sum_xor adding the lanes.
// G provides count(key), the number of items of the key; walk(key, start, step, acc), which adds items start, start + step, ... of the
// key to acc[K] in order; store(key, acc), which writes the K sums. A is the type the sums are formed in (wave_sum_xor has the same
// butterfly for float and double). (Kernels here are templates only so that several units can include them.)
template <int K, class G, class A = float>
__device__ __forceinline__ void seg_sum(int64_t nkeys, const G& g) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool ok = k < nkeys;
    const bool lng = ok && g.count(k) > 64;
    if (ok && !lng) {
        A acc[K];
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = A(0);
        g.walk(k, 0, 1, acc);
        g.store(k, acc);
    }
    unsigned long long m = __ballot(lng);
    while (m) {                                       // (wave-uniform)
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t kk = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63) + src;
        A acc[K];
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = A(0);
        g.walk(kk, lane, 64, acc);
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = wave_sum_xor(acc[q]);
        if (lane == 0) g.store(kk, acc);
    }
}

}  // namespace ls

// n >= 1 int keys in [0, nk], nk meaning "no group" -> order (n): the items sorted stably by key; seg (nk + 2): the items of key k are
// order[seg[k] .. seg[k + 1]). s: a scratch of sort_scratch_bytes(n, CARRIED). CARRIED picks the sort variant -- the same permutation
// either way (radix.h), at different costs in time and scratch. The sorted keys go into s.ord_b: once the result is in `order` (it
// landed there, or the stream-ordered copy below put it there) the sort's second id buffer is dead, so no caller keeps a region for them.
template <bool CARRIED>
static inline int group_by_key(const int* keys, int64_t n, int64_t nk, int* order, int* seg, const SortScratch& s, hipStream_t st) {
    const int passes = radix_passes(nk);               // the largest key is nk itself
    const int* sorted = nullptr;
    int rc;
    if constexpr (CARRIED) rc = radix_argsort_words(ls::KeyInt{keys}, n, 1, order, s, st, &sorted, passes);
    else rc = radix_argsort(ls::KeyInt{keys}, n, passes, order, s, st, &sorted);
    if (rc) return rc;
    if (sorted != order) LS_HIP(hipMemcpyAsync(order, sorted, 4 * (size_t)n, hipMemcpyDeviceToDevice, st));
    int* sk = s.ord_b;                                 // the sort is done with it
    hipLaunchKernelGGL(ls::k_gb_sorted_keys<0>, dim3(ls::div_up(n, 256)), dim3(256), 0, st, keys, (const int*)order, n, sk);
    hipLaunchKernelGGL(ls::k_gb_segments<0>, dim3(ls::div_up(nk + 1, 256)), dim3(256), 0, st, (const int*)sk, n, nk, seg);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
