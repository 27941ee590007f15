// meshbvh.h -- what the queries against one mesh share (distance.hip: point-to-mesh distance; raycast.hip: ray casting; winding.hip:
// winding number; selfx.hip: self-intersections; sample.hip: the gradient tail only). Three things:
//   * the handle that owns a device copy of the mesh and the LBVH of lbvh.h over its faces (created, updated and destroyed in
//     meshbvh.hip), and MeshView, what a query kernel reads of it, passed by value;
//   * the guarded closest point of a query point on a face, with its barycentric weights on request;
//   * the sum of per-item terms into a gradient to the vertices without float atomics (md_vertex_grad) -- the items grouped by their
//     face (groupby.h: stable, so ascending item id within a face), seg_sum adding the 9 terms of a face's items in that order, a thread
//     per vertex adding its corners' face rows in the rank order of meshface.h. It needs no handle: the sampler has none.
// (Kernels here are templates only so that every unit can include them.)
#pragma once
#include "common.h"
#include "groupby.h"
#include "lbvh.h"
#include <algorithm>

namespace ls {

constexpr double MD_SLACK = 0x1p-40, MD_SHRINK = 1.0 - 0x1p-40;

// ---- the view --------------------------------------------------------------------------------------------------------------------
// the mesh and the arrays of its hierarchy that the walks read (lbvh.h has their sizes); slack: MD_SLACK x the largest |coordinate|
// that is not a NaN
struct MeshView {
    const float* __restrict__ P;
    const int* __restrict__ faces;
    int T;
    const int* __restrict__ tri;
    const float* __restrict__ box;
    const int* __restrict__ left;
    const int* __restrict__ right;
    const int* __restrict__ esc;
    double slack;
};
// the fp32 corners of face f widened to fp64: y[3 v + k] = coordinate k of corner v (IDX: the caller's index type, int or size_t;
// 3 T fits an int)
template <class IDX>
__device__ __forceinline__ void mesh_corners(const MeshView& m, IDX f, double* y) {
    const size_t a = 3 * (size_t)m.faces[3 * f], b = 3 * (size_t)m.faces[3 * f + 1], c = 3 * (size_t)m.faces[3 * f + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) { y[k] = (double)m.P[a + k]; y[3 + k] = (double)m.P[b + k]; y[6 + k] = (double)m.P[c + k]; }
}

// ---- the closest point of a face ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double md_d2(const double p[3], const double r[3]) {
    const double dx = p[0] - r[0], dy = p[1] - r[1], dz = p[2] - r[2];
    return (dx * dx + dy * dy) + dz * dz;
}
// closest point of p on the segment a b: a when ap . ab <= 0, b when ap . ab >= ab . ab, else a + ab (ap . ab / ab . ab). WW: also
// w[2], the weights of the point on the two ends
template <bool WW = false>
__device__ __forceinline__ void md_point_seg(const double p[3], const double a[3], const double b[3], double r[3], double* w = nullptr) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double t = lbvh_dd(p[0] - a[0], p[1] - a[1], p[2] - a[2], ab[0], ab[1], ab[2]), l = lbvh_dd(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2]);
    if (t <= 0.0) {
        r[0] = a[0]; r[1] = a[1]; r[2] = a[2];
        if constexpr (WW) { w[0] = 1.0; w[1] = 0.0; }
    } else if (t >= l) {
        r[0] = b[0]; r[1] = b[1]; r[2] = b[2];
        if constexpr (WW) { w[0] = 0.0; w[1] = 1.0; }
    } else {
        const double s = t / l;
        for (int q = 0; q < 3; ++q) r[q] = a[q] + ab[q] * s;
        if constexpr (WW) { w[0] = 1.0 - s; w[1] = s; }
    }
}
// the guarded point-triangle test of distance.hip's header comment: lbvh_point_tri, but a triangle whose area term |ab x ac|^2 is not
// positive, or whose region test gives a non-finite point, is measured as the closest of its segments ab, bc, ca (a later one only when
// strictly closer). WW: also w[3], the weights of the point on (a, b, c); on a degenerate face the corner off the chosen segment gets 0
template <bool WW = false>
__device__ inline void md_point_tri(const double p[3], const double a[3], const double b[3], const double c[3], double r[3], double* w = nullptr) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double cx = ab[1] * ac[2] - ab[2] * ac[1], cy = ab[2] * ac[0] - ab[0] * ac[2], cz = ab[0] * ac[1] - ab[1] * ac[0];
    if ((cx * cx + cy * cy) + cz * cz > 0.0) {
        lbvh_point_tri<WW>(p, a, b, c, r, w);
        if (isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2])) return;
    }
    double s[3], u[2];
    md_point_seg<WW>(p, a, b, r, u);
    double d = md_d2(p, r);
    if constexpr (WW) { w[0] = u[0]; w[1] = u[1]; w[2] = 0.0; }
    md_point_seg<WW>(p, b, c, s, u);
    double e = md_d2(p, s);
    if (e < d) {
        r[0] = s[0]; r[1] = s[1]; r[2] = s[2]; d = e;
        if constexpr (WW) { w[0] = 0.0; w[1] = u[0]; w[2] = u[1]; }
    }
    md_point_seg<WW>(p, c, a, s, u);
    e = md_d2(p, s);
    if (e < d) {
        r[0] = s[0]; r[1] = s[1]; r[2] = s[2];
        if constexpr (WW) { w[0] = u[1]; w[1] = 0.0; w[2] = u[0]; }
    }
}

// ---- the vertex gradient -----------------------------------------------------------------------------------------------------------
// the group-by key of an item: its face, or T ("no group") for an I outside [0, T)
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_md_keys(const int64_t* __restrict__ I, int n, int T, int* __restrict__ keys) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t f = I[i];
    keys[i] = (f < 0 || f >= T) ? T : (int)f;
}
// the rows of T faces from the G of seg_sum (the distance's, the rays' or the sampler's terms), accumulated in A
template <class A, class G>
__global__ __launch_bounds__(256) void k_md_face_rows(G r, int64_t T) { seg_sum<9, G, A>(T, r); }
// gV[v] = the (x, y, z) of the vertex's corners in its faces' rows, added in rank order in the rows' type A and rounded to fp32 once (no
// rounding for fp32 rows; 0 for a vertex without faces)
template <class A>
__global__ __launch_bounds__(256) void k_md_gather_verts(const A* __restrict__ rows, const int* __restrict__ vptr, const int* __restrict__ order, int64_t V,
                                                         float* __restrict__ gV) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    A s0 = A(0), s1 = A(0), s2 = A(0);
    for (int r = vptr[v]; r < vptr[v + 1]; ++r) {
        const int c = order[r];
        const A* row = rows + (size_t)(c / 3) * 9 + 3 * (c % 3);
        s0 += row[0]; s1 += row[1]; s2 += row[2];
    }
    gV[3 * v] = (float)s0; gV[3 * v + 1] = (float)s1; gV[3 * v + 2] = (float)s2;
}

// a backward's workspace (sized from n and F alone), carved: what md_vertex_grad runs in, and what the G of a caller points into (order,
// seg, rows; W for the distance)
template <class A>
struct MdCarved {
    int *keys, *order, *seg;
    SortScratch sort;
    double* W;
    A* rows;
    size_t total;
};
// with_w: a region for the (n, 3) fp64 weights (the distance computes them in its backward; the rays and the sampler are given them);
// A: the accumulator's type, 9 sums per face
template <class A>
static inline MdCarved<A> md_carve(void* ws, int64_t n, int64_t F, bool with_w) {
    const int64_t m = std::max<int64_t>(n, 1);
    WsWalk w(ws);
    int *keys = w.take<int>((size_t)m), *order = w.take<int>((size_t)m), *seg = w.take<int>((size_t)(F + 2));
    const SortScratch sort = sort_scratch_take(w, m, true);
    double* W = w.take<double>(with_w ? 3 * (size_t)m : 0);
    A* rows = w.take<A>(9 * (size_t)std::max<int64_t>(F, 1));
    return {keys, order, seg, sort, W, rows, w.bytes()};
}
// gV (V, 3) from the terms G of n >= 1 items with faces I in a mesh of F faces and V vertices: face keys, the stable group-by, the
// face rows in A, the gather in the corner ranking (vptr, corner_order). g reads c.order and c.seg and stores into c.rows. ASYNC.
template <class A, class G>
static inline int md_vertex_grad(const int64_t* I, int64_t n, int64_t F, int64_t V, const G& g, const int* vptr, const int* corner_order, float* gV,
                                 const MdCarved<A>& c, hipStream_t st) {
    hipLaunchKernelGGL(k_md_keys<0>, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, I, (int)n, (int)F, c.keys);
    if (int rc = group_by_key<true>(c.keys, n, F, c.order, c.seg, c.sort, st)) return rc;
    hipLaunchKernelGGL((k_md_face_rows<A, G>), dim3(div_up(F, 256)), dim3(256), 0, st, g, F);
    hipLaunchKernelGGL(k_md_gather_verts<A>, dim3(div_up(V, 256)), dim3(256), 0, st, (const A*)c.rows, vptr, corner_order, V, gV);
    return LS_OK;
}

// ---- the handle ----------------------------------------------------------------------------------------------------------------
struct MeshDistanceHandle {
    int device = 0, V = 0, T = 0;
    double slack = 0.0;
    void* mem = nullptr;            // one device buffer holding every array below
    size_t cap = 0;
    float* pos = nullptr;
    int* faces = nullptr;
    int* small = nullptr;           // [0]: the index check's flag, [8..13]: the vertex box of lbvh_bounds
    Lbvh bvh{};
    MeshView view() const { return {pos, faces, T, bvh.tri, bvh.box, bvh.left, bvh.right, bvh.esc, slack}; }
};

}  // namespace ls
