// meshbvh.h -- what the queries against one mesh share (distance.hip: point-to-mesh distance; raycast.hip: ray casting): the handle that
// owns a device copy of the mesh and the LBVH of lbvh.h over its faces, and the sum of per-query terms into a gradient to the vertices
// without float atomics -- the queries grouped by their face (groupby.h: stable, so ascending query id within a face), seg_sum adding the
// 9 terms of a face's queries in that order, a thread per vertex adding its corners' face rows in the rank order of meshface.h.
// (Kernels here are templates only so that both units can include them.)
#pragma once
#include "common.h"
#include "groupby.h"
#include "lbvh.h"
#include <algorithm>

namespace ls {

constexpr double MD_SLACK = 0x1p-40, MD_SHRINK = 1.0 - 0x1p-40;

// the group-by key of a point: its face, or T ("no group") for an I outside [0, T)
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_md_keys(const int64_t* __restrict__ I, int n, int T, int* __restrict__ keys) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t f = I[i];
    keys[i] = (f < 0 || f >= T) ? T : (int)f;
}
// rows[f][3 k + q] = sum over the points of face f, in sorted order, of fl32(-(2 g w_k) d_q): the G of seg_sum
struct MdRows {
    const float* __restrict__ Q; const double* __restrict__ C; const double* __restrict__ g; const double* __restrict__ W;
    const int* __restrict__ order; const int* __restrict__ seg; float* __restrict__ rows;
    __device__ __forceinline__ int count(int64_t key) const { return seg[key + 1] - seg[key]; }
    __device__ __forceinline__ void walk(int64_t key, int start, int step, float (&acc)[9]) const {
        const int e = seg[key + 1];
        for (int j = seg[key] + start; j < e; j += step) {
            const size_t i = (size_t)order[j];
            const double s = 2.0 * g[i];
            const double d[3] = {(double)Q[3 * i] - C[3 * i], (double)Q[3 * i + 1] - C[3 * i + 1], (double)Q[3 * i + 2] - C[3 * i + 2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double sw = s * W[3 * i + k];
#pragma unroll
                for (int q = 0; q < 3; ++q) acc[3 * k + q] += (float)(-(sw * d[q]));
            }
        }
    }
    __device__ __forceinline__ void store(int64_t key, const float (&acc)[9]) const {
#pragma unroll
        for (int q = 0; q < 9; ++q) rows[key * 9 + q] = acc[q];
    }
};
// the rows of T faces from the G of seg_sum (MdRows, or the ray terms of raycast.hip)
template <class G>
__global__ __launch_bounds__(256) void k_md_face_rows(G r, int64_t T) { seg_sum<9>(T, r); }
// gV[v] = the (x, y, z) of the vertex's corners in its faces' rows, added in rank order (0 for a vertex without faces)
template <int UNIT = 0>
__global__ __launch_bounds__(256) void k_md_gather_verts(const float* __restrict__ rows, const int* __restrict__ vptr, const int* __restrict__ order, int64_t V,
                                                         float* __restrict__ gV) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int r = vptr[v]; r < vptr[v + 1]; ++r) {
        const int c = order[r];
        const float* row = rows + (size_t)(c / 3) * 9 + 3 * (c % 3);
        s0 += row[0]; s1 += row[1]; s2 += row[2];
    }
    gV[3 * v] = s0; gV[3 * v + 1] = s1; gV[3 * v + 2] = s2;
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
};

struct MdWs {          // the regions of a backward's workspace (sized from n and F alone)
    size_t keys, order, seg, sort, W, rows, total;
};
// with_w: a region for the (n, 3) fp64 weights (the distance computes them in its backward; a ray query returns them)
static inline MdWs md_layout(int64_t n, int64_t F, bool with_w = true) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const int64_t m = std::max<int64_t>(n, 1);
    MdWs w;
    size_t o = 0;
    w.keys = o; o += al(4 * (size_t)m);
    w.order = o; o += al(4 * (size_t)m);
    w.seg = o; o += al(4 * (size_t)(F + 2));
    w.sort = o; o += al(sort_scratch_bytes(m, true));
    w.W = o; o += with_w ? al(24 * (size_t)m) : 0;
    w.rows = o; o += al(36 * (size_t)F);
    w.total = o;
    return w;
}

}  // namespace ls
