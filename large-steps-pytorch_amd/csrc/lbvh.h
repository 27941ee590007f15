// lbvh.h -- a linear BVH over the triangles of a mesh (fp32 positions (V, 3), int32 faces (T, 3) in [0, V)), shared by the remesher's
// projection (remesh.hip) and, through the handle of meshbvh.h (built in meshbvh.hip), by the point-to-mesh distance (distance.hip), the
// ray queries (raycast.hip) and the winding number (winding.hip); the last two walk it their own way.
//
// Build (lbvh_bounds, then lbvh_build): 30-bit Morton codes of the triangle centroids in the vertex box (the box of every row of P, a
// NaN coordinate passed over; an axis that is all NaN has a NaN box and the extent 1; a centroid's cell is its place in the box times
// 1024, clamped to [0, 1023] as a float and then truncated, so that a NaN centroid lands in cell 0), the stable radix sort of
// radix.h, Karras' hierarchy (internal node i of T - 1, leaves at T - 1 + i, leaf i = triangle tri[i]), a bottom-up refit of the
// leaves' corner boxes widened by `margin` (an atomic visit counter: the last child's thread goes on; min / max boxes are
// order-independent) and escape links (the node that follows a node's subtree in the pre-order, -1 past the end). lbvh_walk visits
// a query's candidates without a stack or scratch, templated on the query's bound and leaf test. lbvh_climb is the bottom-up pass
// of the refit, which the winding number's node moments (winding.hip) run again with another combine step; lbvh_point_tri is the
// closest-point rule of every user, with the barycentric weights of the point on request. Everything is deterministic.
// Kernels are templates only so that the header can be included by several translation units.
#pragma once
#include "common.h"
#include "radix.h"
#include <algorithm>
#include <cstring>

namespace ls {

// the device arrays of one hierarchy over T triangles (N = 2 T - 1 nodes); the caller owns them. Sizes in ints unless said:
//   code, ord_a: T; sort: sort_scratch_bytes(T, false) bytes, carved by sort_scratch_carve; tri, scode (unsigned), left, right: T;
//   parent, esc: N; rflag: T; box: 6 N floats (min xyz, max xyz of node i at box[6 i]); bb: 6 unsigned (the vertex box's keys)
struct Lbvh {
    int *code, *ord_a;
    SortScratch sort;
    int* tri;
    unsigned* scode;
    int *left, *right, *parent, *esc, *rflag;
    float* box;
    unsigned* bb;
};

__device__ __forceinline__ float3 lbvh_ld(const float* __restrict__ P, int v) { return make_float3(P[3 * (size_t)v], P[3 * (size_t)v + 1], P[3 * (size_t)v + 2]); }
__device__ __forceinline__ unsigned lbvh_key_inv(unsigned k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_lbvh_bbox(const float* __restrict__ P, int V, unsigned* __restrict__ box /* 6: min keys, max keys */) {
    __shared__ unsigned s[6];
    if (threadIdx.x < 6) s[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int v = blockIdx.x * BLOCK + threadIdx.x; v < V; v += gridDim.x * BLOCK)
        for (int q = 0; q < 3; ++q) {
            const float x = P[3 * (size_t)v + q];
            if (!(x == x)) continue;                  // a NaN is passed over, as fminf / fmaxf pass it over in the node boxes
            const unsigned k = key_of(x);
            mn[q] = min(mn[q], k); mx[q] = max(mx[q], k);
        }
    for (int q = 0; q < 3; ++q) { atomicMin(&s[q], mn[q]); atomicMax(&s[3 + q], mx[q]); }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&box[threadIdx.x], s[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&box[threadIdx.x], s[threadIdx.x]);
}
__device__ __forceinline__ unsigned lbvh_expand(unsigned x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_lbvh_morton(const float* __restrict__ P, const int* __restrict__ faces, int T, const unsigned* __restrict__ box,
                                                       int* __restrict__ code) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= T) return;
    const float3 a = lbvh_ld(P, faces[3 * f]), b = lbvh_ld(P, faces[3 * f + 1]), c = lbvh_ld(P, faces[3 * f + 2]);
    const float cen[3] = {((a.x + b.x) + c.x) / 3.0f, ((a.y + b.y) + c.y) / 3.0f, ((a.z + b.z) + c.z) / 3.0f};
    unsigned q[3];
    for (int k = 0; k < 3; ++k) {
        const float lo = __uint_as_float(lbvh_key_inv(box[k])), hi = __uint_as_float(lbvh_key_inv(box[3 + k]));
        const float ext = hi - lo > 0.0f ? hi - lo : 1.0f;
        q[k] = (unsigned)(int)fminf(fmaxf((cen[k] - lo) / ext * 1024.0f, 0.0f), 1023.0f);      // clamped in float: the cast is defined, a NaN gives 0
    }
    code[f] = (int)((lbvh_expand(q[0]) << 2) | (lbvh_expand(q[1]) << 1) | lbvh_expand(q[2]));
}
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_lbvh_sorted_codes(const int* __restrict__ order, const int* __restrict__ code, int T, int* __restrict__ tri,
                                                             unsigned* __restrict__ scode) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < T) { tri[i] = order[i]; scode[i] = (unsigned)code[order[i]]; }
}
__device__ __forceinline__ int lbvh_delta(const unsigned* __restrict__ k, int T, int i, int j) {
    if (j < 0 || j >= T) return -1;
    const unsigned a = k[i], b = k[j];
    return a == b ? 32 + __clz((unsigned)(i ^ j)) : __clz(a ^ b);
}
// Karras (2012): internal node i of T - 1, leaves at T - 1 + i
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_lbvh_karras(const unsigned* __restrict__ k, int T, int* __restrict__ left, int* __restrict__ right,
                                                       int* __restrict__ parent) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= T - 1) return;
    const int d = lbvh_delta(k, T, i, i + 1) - lbvh_delta(k, T, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = lbvh_delta(k, T, i, i - d);
    int lmax = 2;
    while (lbvh_delta(k, T, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(k, T, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d, dnode = lbvh_delta(k, T, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (lbvh_delta(k, T, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + min(d, 0);
    const int L = min(i, j) == gamma ? T - 1 + gamma : gamma, R = max(i, j) == gamma + 1 ? T - 1 + gamma + 1 : gamma + 1;
    left[i] = L; right[i] = R;
    parent[L] = i; parent[R] = i;
}
// The bottom-up pass from a finished leaf: at every internal node on the way to the root the thread that arrives FIRST stops (the
// sibling's subtree is not done yet), the one that arrives second runs combine(node, left[node], right[node]) and goes on. The fence
// before the atomic publishes what this thread wrote below the node, the fence after it orders the reads of what the sibling's thread
// published; combine reads the children through volatile pointers. Which thread does a node's combine does not change its operands.
template <class Combine>
__device__ __forceinline__ void lbvh_climb(int leaf, const int* __restrict__ left, const int* __restrict__ right, const int* __restrict__ parent,
                                           int* __restrict__ flag, Combine combine) {
    int node = parent[leaf];
    while (node >= 0) {
        __threadfence();
        if (atomicAdd(&flag[node], 1) == 0) return;       // the sibling's subtree is not done yet: its last thread goes on
        __threadfence();
        combine(node, left[node], right[node]);
        node = parent[node];
    }
}
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_lbvh_refit(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ tri, int T,
                                                      float margin, const int* __restrict__ left, const int* __restrict__ right,
                                                      const int* __restrict__ parent, int* __restrict__ flag, float* __restrict__ box) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= T) return;
    const int f = tri[i];
    const float3 a = lbvh_ld(P, faces[3 * f]), b = lbvh_ld(P, faces[3 * f + 1]), c = lbvh_ld(P, faces[3 * f + 2]);
    const int node = T - 1 + i;
    float* bx = box + 6 * (size_t)node;
    bx[0] = fminf(fminf(a.x, b.x), c.x) - margin; bx[1] = fminf(fminf(a.y, b.y), c.y) - margin; bx[2] = fminf(fminf(a.z, b.z), c.z) - margin;
    bx[3] = fmaxf(fmaxf(a.x, b.x), c.x) + margin; bx[4] = fmaxf(fmaxf(a.y, b.y), c.y) + margin; bx[5] = fmaxf(fmaxf(a.z, b.z), c.z) + margin;
    if (T == 1) return;
    lbvh_climb(node, left, right, parent, flag, [&](int nd, int lc, int rc) {
        const volatile float* l = box + 6 * (size_t)lc;
        const volatile float* r = box + 6 * (size_t)rc;
        float* o = box + 6 * (size_t)nd;
        for (int q = 0; q < 3; ++q) { o[q] = fminf(l[q], r[q]); o[3 + q] = fmaxf(l[3 + q], r[3 + q]); }
    });
}
// escape link: the node that follows a node's subtree in the pre-order (left first), -1 past the end
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_lbvh_escape(const int* __restrict__ left, const int* __restrict__ right, const int* __restrict__ parent, int N,
                                                       int* __restrict__ esc) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    int x = i, e = -1;
    while (x != 0) {
        const int p = parent[x];
        if (left[p] == x) { e = right[p]; break; }
        x = p;
    }
    esc[i] = e;
}

// the box of the V vertices (min and max per axis, fp32, NaNs passed over; NaN on an axis without a number) into lo / hi on the host;
// also left in a.bb for lbvh_build. SYNC.
static inline int lbvh_bounds(const float* P, int V, const Lbvh& a, hipStream_t st, float lo[3], float hi[3]) {
    const unsigned init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    LS_HIP(hipMemcpyAsync(a.bb, init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lbvh_bbox<0>, dim3(std::min(div_up(V, BLOCK), 1024)), dim3(BLOCK), 0, st, P, V, a.bb);
    unsigned hb[6];
    LS_HIP(hipMemcpyAsync(hb, a.bb, sizeof(hb), hipMemcpyDeviceToHost, st));
    LS_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < 3; ++q) {
        unsigned k = hb[q];
        k = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
        memcpy(&lo[q], &k, 4);
        k = hb[3 + q];
        k = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
        memcpy(&hi[q], &k, 4);
    }
    return LS_OK;
}

// the hierarchy over faces (T, 3) of P, after lbvh_bounds on the same P; leaf boxes widened by `margin`. ASYNC.
static inline int lbvh_build(const float* P, const int* faces, int T, float margin, const Lbvh& a, hipStream_t st) {
    const int N = 2 * T - 1;
    const dim3 grid_t(div_up(std::max(T, 1), BLOCK)), grid_n(div_up(std::max(N, 1), BLOCK)), block(BLOCK);
    hipLaunchKernelGGL(k_lbvh_morton<0>, grid_t, block, 0, st, P, faces, T, (const unsigned*)a.bb, a.code);
    const int* order = nullptr;
    int rc = radix_argsort(KeyInt{(const int*)a.code}, T, 4, a.ord_a, a.sort, st, &order);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lbvh_sorted_codes<0>, grid_t, block, 0, st, order, (const int*)a.code, T, a.tri, a.scode);
    LS_HIP(hipMemsetAsync(a.parent, 0xff, sizeof(int) * N, st));
    LS_HIP(hipMemsetAsync(a.rflag, 0, sizeof(int) * T, st));
    if (T > 1) hipLaunchKernelGGL(k_lbvh_karras<0>, dim3(div_up(T - 1, BLOCK)), block, 0, st, (const unsigned*)a.scode, T, a.left, a.right, a.parent);
    hipLaunchKernelGGL(k_lbvh_refit<0>, grid_t, block, 0, st, P, faces, (const int*)a.tri, T, margin, (const int*)a.left, (const int*)a.right,
                       (const int*)a.parent, a.rflag, a.box);
    hipLaunchKernelGGL(k_lbvh_escape<0>, grid_n, block, 0, st, (const int*)a.left, (const int*)a.right, (const int*)a.parent, N, a.esc);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// The walk of one query. Q provides
//   bound(node)  a lower bound of the query's measure over the triangles under node (any type comparable with best())
//   best()       the best measure so far
//   leaf(i)      tests leaf i (triangle tri[i]) and updates the best
// A first bound comes from the greedy descent to one leaf (the child with the smaller bound, the left one on a tie); then every node is
// visited in pre-order through the escape links, and a subtree is skipped when bound(node) > best(): strictly greater, so a subtree that
// may hold an equal measure is visited.
template <typename Q>
__device__ __forceinline__ void lbvh_walk(const int* __restrict__ left, const int* __restrict__ right, const int* __restrict__ esc, int T, Q& q) {
    const int leaf0 = T - 1;
    int node = 0;
    while (node < leaf0) {
        const int l = left[node], r = right[node];
        node = q.bound(r) < q.bound(l) ? r : l;
    }
    q.leaf(node - leaf0);
    node = 0;
    while (node >= 0) {
        if (q.bound(node) > q.best()) { node = esc[node]; continue; }
        if (node >= leaf0) { q.leaf(node - leaf0); node = esc[node]; }
        else node = left[node];
    }
}

__device__ __forceinline__ double lbvh_dd(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }
// closest point of p on triangle (a, b, c) in fp64: the region tests of tests/remesh_statement.py:point_triangle (no guard for a
// degenerate triangle: the remesher's input has none, the distance path guards it in meshbvh.h). WW: also w[3], the weights of the
// point on (a, b, c), from the quotient of the same branch (r is never rebuilt from them); the distance's gradient asks for them.
template <bool WW = false>
__device__ inline void lbvh_point_tri(const double p[3], const double a[3], const double b[3], const double c[3], double r[3], double* w = nullptr) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double d1 = lbvh_dd(ab[0], ab[1], ab[2], ap[0], ap[1], ap[2]), d2 = lbvh_dd(ac[0], ac[1], ac[2], ap[0], ap[1], ap[2]);
    if (d1 <= 0.0 && d2 <= 0.0) {
        r[0] = a[0]; r[1] = a[1]; r[2] = a[2];
        if constexpr (WW) { w[0] = 1.0; w[1] = 0.0; w[2] = 0.0; }
        return;
    }
    const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const double d3 = lbvh_dd(ab[0], ab[1], ab[2], bp[0], bp[1], bp[2]), d4 = lbvh_dd(ac[0], ac[1], ac[2], bp[0], bp[1], bp[2]);
    if (d3 >= 0.0 && d4 <= d3) {
        r[0] = b[0]; r[1] = b[1]; r[2] = b[2];
        if constexpr (WW) { w[0] = 0.0; w[1] = 1.0; w[2] = 0.0; }
        return;
    }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        for (int q = 0; q < 3; ++q) r[q] = a[q] + ab[q] * v;
        if constexpr (WW) { w[0] = 1.0 - v; w[1] = v; w[2] = 0.0; }
        return;
    }
    const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const double d5 = lbvh_dd(ab[0], ab[1], ab[2], cp[0], cp[1], cp[2]), d6 = lbvh_dd(ac[0], ac[1], ac[2], cp[0], cp[1], cp[2]);
    if (d6 >= 0.0 && d5 <= d6) {
        r[0] = c[0]; r[1] = c[1]; r[2] = c[2];
        if constexpr (WW) { w[0] = 0.0; w[1] = 0.0; w[2] = 1.0; }
        return;
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double u = d2 / (d2 - d6);
        for (int q = 0; q < 3; ++q) r[q] = a[q] + ac[q] * u;
        if constexpr (WW) { w[0] = 1.0 - u; w[1] = 0.0; w[2] = u; }
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double u = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int q = 0; q < 3; ++q) r[q] = b[q] + (c[q] - b[q]) * u;
        if constexpr (WW) { w[0] = 0.0; w[1] = 1.0 - u; w[2] = u; }
        return;
    }
    const double den = 1.0 / ((va + vb) + vc), v = vb * den, u = vc * den;
    for (int q = 0; q < 3; ++q) r[q] = (a[q] + ab[q] * v) + ac[q] * u;
    if constexpr (WW) { w[0] = (1.0 - v) - u; w[1] = v; w[2] = u; }
}

}  // namespace ls
