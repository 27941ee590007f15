// distance.hip -- point-to-mesh squared distance and its directed maximum on the device (gfx950, wave64): libigl's
// point_mesh_squared_distance / hausdorff, which the reference's figures call on every recorded step.
//
// The mesh (fp32 positions, int32 faces) is held by a handle (meshbvh.h, built in meshbvh.hip; raycast.hip and winding.hip query the
// same one) with the LBVH of lbvh.h over its faces (leaf boxes exact: margin 0). A
// query point p (fp32) walks it stacklessly. Everything after the load is fp64:
//   * the leaf test is md_point_tri of meshbvh.h: lbvh_point_tri (the remesher's region tests), guarded: a triangle whose area term
//     |ab x ac|^2 is not positive, or whose region test gives a non-finite point, is measured as the closest of its segments ab, bc, ca
//     (the first on a tie);
//   * a tie of the squared distance goes to the lower triangle id, so the answer is what a brute-force scan in the same arithmetic
//     gives (tests/distance_statement.py);
//   * a subtree is skipped only when a lower bound of its distance is strictly greater than the best so far. The bound is the box
//     distance in fp64 with every per-axis gap shrunk by MD_SLACK x the mesh's largest coordinate and the sum shrunk by MD_SHRINK:
//     it stays below the true distance of every triangle in the box at any distance from the origin (the fp32 box distance of the
//     remesher's walk does not, beyond about 170 diagonals).
// The directed maximum reduces max_p d2(p) per wave and adds it with an integer atomicMax on the bits: for non-negative doubles the
// bit order is the value order, so the result does not depend on the schedule.
//
// The gradient of sqrD ("Gradient"). With C the closest point on face I = (a, b, c), C = w_a a + w_b b + w_c c: the
// weights w come from the same fp64 region / segment tests that produce C (md_point_tri<true>: the branch that sets the point sets the
// weights), one face per point, after the walk. C minimises over the face, so no derivative of w enters (envelope theorem): with
// d = p - C and g the incoming gradient, d sqrD / dp = 2 g d and d sqrD / d V[F[I, k]] = -2 g w_k d, each term formed in fp64 and rounded
// to fp32 once.
// The vertex gradient has no float atomics: the points are grouped by their face (groupby.h: stable, so ascending point id within a face),
// seg_sum adds the 9 terms of a face's points in that order (a thread up to 64 points, else the wave lane-strided and the xor butterfly),
// and a thread per vertex adds its corners' face rows in the rank order of meshface.h (md_vertex_grad of meshbvh.h). Bitwise
// reproducible, no host synchronisation.
#include "common.h"
#include "groupby.h"
#include "lbvh.h"
#include "meshbvh.h"
#include <algorithm>
#include <cmath>

namespace ls {

typedef unsigned long long u64;

// the query of lbvh_walk
struct MdQuery {
    const MeshView& m;
    double p[3];
    double d2, r[3];
    int id;
    __device__ __forceinline__ double bound(int node) const {
        const float* bx = m.box + 6 * (size_t)node;
        const double x = fmax(fmax((double)bx[0] - p[0], p[0] - (double)bx[3]) - m.slack, 0.0);
        const double y = fmax(fmax((double)bx[1] - p[1], p[1] - (double)bx[4]) - m.slack, 0.0);
        const double z = fmax(fmax((double)bx[2] - p[2], p[2] - (double)bx[5]) - m.slack, 0.0);
        return ((x * x + y * y) + z * z) * MD_SHRINK;
    }
    __device__ __forceinline__ double best() const { return d2; }
    __device__ __forceinline__ void leaf(int i) {
        const int f = m.tri[i];
        double y[9], q[3];
        mesh_corners(m, f, y);
        md_point_tri(p, y, y + 3, y + 6, q);
        const double e = md_d2(p, q);
        if (e < d2 || (e == d2 && f < id)) { d2 = e; id = f; r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; }
    }
};

// one thread per query point; any of sqrD / I / C may be null; dmax: the bits of max d2 over the points (or null). The mesh arrives as
// loose pointers and the view is built here: passed by value it changed the walk's scalar loads and exec-mask code and measured about
// 1 % slower (docs/measurements.md, the mesh-query refactor)
__global__ __launch_bounds__(BLOCK) void k_md_query(const float* __restrict__ Q, int n, const float* __restrict__ P, const int* __restrict__ faces, int T,
                                                    const int* __restrict__ tri, const float* __restrict__ box, const int* __restrict__ left,
                                                    const int* __restrict__ right, const int* __restrict__ esc, double slack, double* __restrict__ sqrD,
                                                    int64_t* __restrict__ I, double* __restrict__ C, u64* __restrict__ dmax) {
    const MeshView m{P, faces, T, tri, box, left, right, esc, slack};
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double d2 = 0.0;
    if (i < n) {
        MdQuery q{m, {Q[3 * (size_t)i], Q[3 * (size_t)i + 1], Q[3 * (size_t)i + 2]}, 0.0, {0.0, 0.0, 0.0}, 0x7fffffff};
        q.d2 = __longlong_as_double(0x7ff0000000000000ll);
        lbvh_walk(m.left, m.right, m.esc, m.T, q);
        d2 = q.d2;
        if (sqrD) sqrD[i] = d2;
        if (I) I[i] = q.id;
        if (C) { C[3 * (size_t)i] = q.r[0]; C[3 * (size_t)i + 1] = q.r[1]; C[3 * (size_t)i + 2] = q.r[2]; }
    }
    if (!dmax) return;
    for (int s = WAVE / 2; s >= 1; s /= 2) d2 = fmax(d2, __shfl_xor(d2, s));
    if ((threadIdx.x & (WAVE - 1)) == 0) atomicMax(dmax, (u64)__double_as_longlong(d2));
}

// one thread per point: W[i] = the barycentric weights of point i's closest point on face I[i], from the one call that also finds the
// point; an I outside [0, T) gives NaN weights (and reads nothing)
__global__ __launch_bounds__(BLOCK) void k_md_weights(const float* __restrict__ Q, int n, const MeshView m, const int64_t* __restrict__ I,
                                                      double* __restrict__ W) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t f = I[i];
    double w[3];
    if (f < 0 || f >= m.T) w[0] = w[1] = w[2] = __longlong_as_double(0x7ff8000000000000ll);
    else {
        const double p[3] = {Q[3 * (size_t)i], Q[3 * (size_t)i + 1], Q[3 * (size_t)i + 2]};
        double y[9], r[3];
        mesh_corners(m, (size_t)f, y);
        md_point_tri<true>(p, y, y + 3, y + 6, r, w);
    }
    W[3 * (size_t)i] = w[0]; W[3 * (size_t)i + 1] = w[1]; W[3 * (size_t)i + 2] = w[2];
}

// ---- the gradient ----------------------------------------------------------------------------------------------------------------
// gP[i] = fl32(2 g_i (p_i - C_i)), fp64 until the one rounding
__global__ __launch_bounds__(BLOCK) void k_md_grad_points(const float* __restrict__ Q, const double* __restrict__ C, const double* __restrict__ g, int n,
                                                          float* __restrict__ gP) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double s = 2.0 * g[i];
    for (int q = 0; q < 3; ++q) gP[3 * (size_t)i + q] = (float)(s * ((double)Q[3 * (size_t)i + q] - C[3 * (size_t)i + q]));
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
}  // namespace ls

using namespace ls;

static int md_launch(MeshDistanceHandle* H, const float* P, int64_t n, double* sqrD, int64_t* I, double* C, u64* dmax, hipStream_t st) {
    const MeshView v = H->view();
    hipLaunchKernelGGL(k_md_query, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, P, (int)n, v.P, v.faces, v.T, v.tri, v.box, v.left, v.right, v.esc, v.slack,
                       sqrD, I, C, dmax);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_distance_query(void* handle, const float* P, int64_t n, double* sqrD, int64_t* I, double* C, void* stream) {
    LS_REQUIRE(handle && n >= 0 && (n == 0 || P), LS_E_INVALID, "ls_mesh_distance_query: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_distance_query: more than 2^31 query points");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    if (n == 0 || (!sqrD && !I && !C)) return LS_OK;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    return md_launch(H, P, n, sqrD, I, C, nullptr, (hipStream_t)stream);
}

extern "C" int ls_mesh_distance_max(void* handle, const float* P, int64_t n, double* out_sqd, void* stream) {
    LS_REQUIRE(handle && out_sqd && n >= 0 && (n == 0 || P), LS_E_INVALID, "ls_mesh_distance_max: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_distance_max: more than 2^31 query points");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    LS_HIP(hipMemsetAsync(out_sqd, 0, sizeof(double), (hipStream_t)stream));
    if (n == 0) return LS_OK;
    return md_launch(H, P, n, nullptr, nullptr, nullptr, (u64*)out_sqd, (hipStream_t)stream);
}

extern "C" int ls_mesh_distance_weights(void* handle, const float* P, int64_t n, const int64_t* I, double* W, void* stream) {
    LS_REQUIRE(handle && n >= 0 && (n == 0 || (P && I && W)), LS_E_INVALID, "ls_mesh_distance_weights: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_distance_weights: more than 2^31 query points");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    if (n == 0) return LS_OK;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    hipLaunchKernelGGL(k_md_weights, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, P, (int)n, H->view(), I, W);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_distance_backward_workspace_bytes(int64_t n, int64_t F, size_t* bytes) {
    LS_REQUIRE(bytes && n >= 0 && F > 0, LS_E_INVALID, "ls_mesh_distance_backward_workspace_bytes: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK && 3 * F < INT32_MAX, LS_E_OVERFLOW, "ls_mesh_distance_backward_workspace_bytes: more than 2^31 points or corners");
    *bytes = md_carve<float>(nullptr, n, F, true).total;
    return LS_OK;
}

extern "C" int ls_mesh_distance_backward(void* handle, const float* P, int64_t n, const int64_t* I, const double* C, const double* g,
                                         const int32_t* vptr, const int32_t* corner_order, float* gP, float* gV, void* ws, size_t ws_bytes,
                                         void* stream) {
    LS_REQUIRE(handle && n >= 0 && (n == 0 || (P && C && g)), LS_E_INVALID, "ls_mesh_distance_backward: bad argument");
    LS_REQUIRE(!gV || (vptr && corner_order && ws && (n == 0 || I)), LS_E_INVALID,
               "ls_mesh_distance_backward: the vertex gradient needs I, the corner ranking and a workspace");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_distance_backward: more than 2^31 query points");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    const MdCarved<float> c = md_carve<float>(ws, n, H->T, true);
    LS_REQUIRE(!gV || ws_bytes >= c.total, LS_E_WORKSPACE, "ls_mesh_distance_backward: workspace too small (%zu < %zu bytes)", ws_bytes, c.total);
    DeviceGuard guard(H->device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    if (gP && n > 0) hipLaunchKernelGGL(k_md_grad_points, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, P, C, g, (int)n, gP);
    if (gV && n == 0) LS_HIP(hipMemsetAsync(gV, 0, sizeof(float) * 3 * (size_t)H->V, st));
    if (gV && n > 0) {
        hipLaunchKernelGGL(k_md_weights, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, P, (int)n, H->view(), I, c.W);
        if (int rc = md_vertex_grad<float>(I, n, H->T, H->V, MdRows{P, C, g, c.W, c.order, c.seg, c.rows}, vptr, corner_order, gV, c, st)) return rc;
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}
