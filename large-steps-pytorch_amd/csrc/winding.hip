// winding.hip -- the generalized winding number of query points against the mesh of a mesh-distance handle (meshbvh.h) on the device
// (gfx950, wave64): libigl's winding_number (the exact sum) and fast_winding_number (Barill et al. 2018, the tree-accelerated sum over
// the LBVH of lbvh.h), and with them the sign of largesteps.distance.signed_distance. tests/winding_statement.py
// restates the rule below in numpy fp64.
//
// The rule. All arithmetic is fp64 from the fp32 inputs, no FMA contraction (-ffp-contract=off).
// Solid angle of face (a, b, c) seen from q (van Oosterom and Strackee), A = a - q, B = b - q, C = c - q:
//   num = A . (B x C),   den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|,   Omega = 2 atan2(num, den);  the face contributes Omega / 4 pi.
// A face contributes 0 when num == 0 (either sign of zero): a query in the plane of the face (inside its outline the principal value, the
// mean of +1/2 and -1/2), on a vertex or an edge, and a zero-area or repeated-index face; nothing depends on the sign of a computed zero.
// A query with a non-finite component gives NaN without walking anything.
// Exact winding number: w(q) = sum over the faces, in ascending id, of Omega_f / 4 pi.
//
// Node moments, for every node of the hierarchy (internal nodes 0 .. T - 2, leaf i at T - 1 + i holding face tri[i]); a_t = (b - a) x
// (c - a) / 2 the area vector of face t, |a_t| its area, c_t its centroid, sums over the faces under the node:
//   N = sum a_t,   Ar = sum |a_t|,   p = sum |a_t| c_t / Ar (the centre of the node's box when Ar == 0),
//   C_ij = sum (a_t)_i (c_t - p)_j,
//   T_ijk = sum (a_t)_i / 12 (sum over the corners y of y_j y_k + 9 c_j c_k), corners y and centroid c relative to p: this is
//           (n_t)_i times the integral of (x - p)_j (x - p)_k over the face; symmetric in jk, 18 values,
//   r = the distance from p to the farthest corner of the node's box as lbvh.h stores it (fp32 bounds, margin included): a query inside
//       the box always has |q - p| <= r.
// They are computed without per-node loops and deterministically: the leaves write raw moments about the centre o of the vertex box
// (plainly additive), the bottom-up pass of the refit (lbvh_climb of lbvh.h) adds left + right in that operand order (the thread that arrives
// second does the addition; which thread that is does not change the sum), and a pass per node re-centres from o to p:
//   C = C' - N (x) s,   T_ijk = T'_ijk - s_j C'_ik - s_k C'_ij + s_j s_k N_i,   s = p - o.
// The re-centring cancels terms of size Ar R^k (R the diagonal of the mesh's box) down to Ar r^k: a relative error of (R / r)^2 2^-53 in
// the second-order moment of a node of radius r, an absolute one of Ar R^2 2^-53 -- what the tests bound by Ar R^k 2^-40.
//
// Far-field value of a node, rho = p - q, d = |rho|, three terms:
//   4 pi w_far = rho . N / d^3 + [tr C / d^3 - 3 rho^T C rho / d^5]
//              + 1/2 sum_ijk T_ijk [-3 (delta_ij rho_k + delta_ik rho_j + delta_jk rho_i) / d^5 + 15 rho_i rho_j rho_k / d^7].
// The walk: one thread per query, pre-order through the escape links (no stack, no LDS, no scratch). At a node: if d > beta r, add w_far
// and go to esc; else if it is a leaf, add the leaf's exact term and go to esc; else go left. Terms are added in visiting order, so a
// result is a function of (mesh, query, beta) alone: bitwise reproducible, capturable, no atomics. beta >= 1; beta = +inf selects the
// exact kernel: the dense sum, a workgroup staging tiles of 256 faces' corners in LDS (fp64, 18 KiB; every lane reads the same face, a
// broadcast without bank conflicts) while each thread keeps one query in registers and adds the tile's faces in ascending id.
//
// The moment buffer (ls_mesh_winding_bytes) belongs to the caller: WN_STRIDE doubles per node -- p (3), r, N (3), Ar, C (9, row i column
// j at 3 i + j), T (18: row i at 6 i, columns jk = 00 01 02 11 12 22), one pad -- and after them the visit counters of the bottom-up pass.
#include "common.h"
#include "lbvh.h"
#include "meshbvh.h"
#include <algorithm>
#include <cmath>

namespace ls {

constexpr int WN_STRIDE = 36, WN_TILE = 256;
constexpr int WN_P = 0, WN_R = 3, WN_N = 4, WN_AR = 7, WN_C = 8, WN_T = 17;
constexpr double WN_4PI = 12.566370614359172;           // fl64(4 pi) = 4 fl64(pi)

__device__ __forceinline__ double wn_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ int wn_sym(int j, int k) { return j == 0 ? k : (j == 1 ? 2 + k : 5); }        // j <= k: 00 01 02 11 12 22

// Omega / 4 pi of the face with corners a, b, c seen from q
__device__ __forceinline__ double wn_face(const double q[3], const double a[3], const double b[3], const double c[3]) {
    const double A[3] = {a[0] - q[0], a[1] - q[1], a[2] - q[2]}, B[3] = {b[0] - q[0], b[1] - q[1], b[2] - q[2]};
    const double C[3] = {c[0] - q[0], c[1] - q[1], c[2] - q[2]};
    const double x0 = B[1] * C[2] - B[2] * C[1], x1 = B[2] * C[0] - B[0] * C[2], x2 = B[0] * C[1] - B[1] * C[0];
    const double num = (A[0] * x0 + A[1] * x1) + A[2] * x2;
    if (num == 0.0) return 0.0;
    const double la = sqrt(lbvh_dd(A[0], A[1], A[2], A[0], A[1], A[2])), lb = sqrt(lbvh_dd(B[0], B[1], B[2], B[0], B[1], B[2]));
    const double lc = sqrt(lbvh_dd(C[0], C[1], C[2], C[0], C[1], C[2]));
    const double ab = lbvh_dd(A[0], A[1], A[2], B[0], B[1], B[2]), bc = lbvh_dd(B[0], B[1], B[2], C[0], C[1], C[2]);
    const double ca = lbvh_dd(C[0], C[1], C[2], A[0], A[1], A[2]);
    const double den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
    return (2.0 * atan2(num, den)) / WN_4PI;
}

// the centre o of the vertex box that lbvh_bounds left as keys
__device__ __forceinline__ void wn_origin(const unsigned* __restrict__ bb, double o[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = 0.5 * ((double)__uint_as_float(lbvh_key_inv(bb[k])) + (double)__uint_as_float(lbvh_key_inv(bb[3 + k])));
}

// the raw moments about o: a thread per leaf writes its face's, then climbs; at an internal node the thread that finds its sibling done
// adds left + right (lbvh_climb). Slots: S = sum |a| c at WN_P, 0 at WN_R and the pad, N, Ar, C', T' in their places
__global__ __launch_bounds__(BLOCK) void k_wn_raw(const MeshView mesh, const unsigned* __restrict__ bb, const int* __restrict__ parent,
                                                  int* __restrict__ flag, double* __restrict__ mom) {
    const int i = blockIdx.x * BLOCK + threadIdx.x, T = mesh.T;
    if (i >= T) return;
    double o[3];
    wn_origin(bb, o);
    double y[3][3];
    mesh_corners(mesh, (size_t)mesh.tri[i], &y[0][0]);
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int k = 0; k < 3; ++k) y[v][k] -= o[k];
    const double e1[3] = {y[1][0] - y[0][0], y[1][1] - y[0][1], y[1][2] - y[0][2]}, e2[3] = {y[2][0] - y[0][0], y[2][1] - y[0][1], y[2][2] - y[0][2]};
    const double a[3] = {0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]), 0.5 * (e1[0] * e2[1] - e1[1] * e2[0])};
    const double ar = sqrt(lbvh_dd(a[0], a[1], a[2], a[0], a[1], a[2]));
    const double c[3] = {((y[0][0] + y[1][0]) + y[2][0]) / 3.0, ((y[0][1] + y[1][1]) + y[2][1]) / 3.0, ((y[0][2] + y[1][2]) + y[2][2]) / 3.0};
    const int node = T - 1 + i;
    double* m = mom + (size_t)WN_STRIDE * node;
#pragma unroll
    for (int k = 0; k < 3; ++k) { m[WN_P + k] = ar * c[k]; m[WN_N + k] = a[k]; }
    m[WN_R] = 0.0; m[WN_AR] = ar; m[WN_STRIDE - 1] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            m[WN_C + 3 * j + k] = a[j] * c[k];
            if (k >= j) {
                const double s = (((y[0][j] * y[0][k] + y[1][j] * y[1][k]) + y[2][j] * y[2][k]) + 9.0 * (c[j] * c[k])) / 12.0;
#pragma unroll
                for (int q = 0; q < 3; ++q) m[WN_T + 6 * q + wn_sym(j, k)] = a[q] * s;
            }
        }
    if (T == 1) return;
    lbvh_climb(node, mesh.left, mesh.right, parent, flag, [&](int nd, int lc, int rc) {
        const volatile double* l = mom + (size_t)WN_STRIDE * lc;
        const volatile double* r = mom + (size_t)WN_STRIDE * rc;
        double* out = mom + (size_t)WN_STRIDE * nd;
        for (int q = 0; q < WN_STRIDE; ++q) out[q] = l[q] + r[q];
    });
}

// a thread per node: p, r and the moments about p from the raw ones about o
__global__ __launch_bounds__(BLOCK) void k_wn_centre(int N, const unsigned* __restrict__ bb, const float* __restrict__ box, double* __restrict__ mom) {
    const int node = blockIdx.x * BLOCK + threadIdx.x;
    if (node >= N) return;
    double o[3];
    wn_origin(bb, o);
    double* m = mom + (size_t)WN_STRIDE * node;
    const float* bx = box + 6 * (size_t)node;
    const double ar = m[WN_AR];
    double p[3], s[3], n[3], c[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (ar > 0.0) { s[k] = m[WN_P + k] / ar; p[k] = o[k] + s[k]; }
        else { p[k] = 0.5 * ((double)bx[k] + (double)bx[3 + k]); s[k] = p[k] - o[k]; }
        n[k] = m[WN_N + k];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) c[q] = m[WN_C + q];
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double e = fmax(fabs(p[k] - (double)bx[k]), fabs((double)bx[3 + k] - p[k]));
        r2 += e * e;
        m[WN_P + k] = p[k];
    }
    m[WN_R] = sqrt(r2);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            m[WN_C + 3 * i + j] = c[3 * i + j] - n[i] * s[j];
#pragma unroll
            for (int k = j; k < 3; ++k) {
                double* t = m + WN_T + 6 * i + wn_sym(j, k);
                *t = ((*t - s[j] * c[3 * i + k]) - s[k] * c[3 * i + j]) + (s[j] * s[k]) * n[i];
            }
        }
}

// 4 pi w_far of the node with moments m (p and r already consumed) from rho = p - q and d2 = |rho|^2, d = sqrt(d2); the moments are
// used as they are read
__device__ __forceinline__ double wn_far(const double* __restrict__ m, const double rho[3], double d2, double d) {
    const double i2 = 1.0 / d2, i3 = i2 / d, i5 = i3 * i2, i7 = i5 * i2;
    const double t1 = lbvh_dd(rho[0], rho[1], rho[2], m[WN_N], m[WN_N + 1], m[WN_N + 2]) * i3;
    double tr = 0.0, quad = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double* c = m + WN_C + 3 * i;
        tr += c[i];
        quad += rho[i] * lbvh_dd(c[0], c[1], c[2], rho[0], rho[1], rho[2]);
    }
    const double t2 = tr * i3 - 3.0 * (quad * i5);
    double lin = 0.0, cub = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double* t = m + WN_T + 6 * i;                    // 00 01 02 11 12 22
        const double t00 = t[0], t01 = t[1], t02 = t[2], t11 = t[3], t12 = t[4], t22 = t[5];
        const double row = i == 0 ? lbvh_dd(t00, t01, t02, rho[0], rho[1], rho[2])
                         : i == 1 ? lbvh_dd(t01, t11, t12, rho[0], rho[1], rho[2]) : lbvh_dd(t02, t12, t22, rho[0], rho[1], rho[2]);
        lin += 2.0 * row + rho[i] * ((t00 + t11) + t22);
        const double qd = ((t00 * (rho[0] * rho[0]) + t11 * (rho[1] * rho[1])) + t22 * (rho[2] * rho[2])) +
                          2.0 * ((t01 * (rho[0] * rho[1]) + t02 * (rho[0] * rho[2])) + t12 * (rho[1] * rho[2]));
        cub += rho[i] * qd;
    }
    const double t3 = 0.5 * (15.0 * (cub * i7) - 3.0 * (lin * i5));
    return (t1 + t2) + t3;
}

// one thread per query: the walk
__global__ __launch_bounds__(BLOCK) void k_wn_walk(const float* __restrict__ Q, int n, const MeshView mesh, const double* __restrict__ mom, double beta,
                                                   double* __restrict__ w) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double q[3] = {(double)Q[3 * (size_t)i], (double)Q[3 * (size_t)i + 1], (double)Q[3 * (size_t)i + 2]};
    if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]))) { w[i] = wn_nan(); return; }
    const int leaf0 = mesh.T - 1;
    double acc = 0.0;
    int node = 0;
    while (node >= 0) {
        const double* m = mom + (size_t)WN_STRIDE * node;
        const double rho[3] = {m[WN_P] - q[0], m[WN_P + 1] - q[1], m[WN_P + 2] - q[2]};
        const double d2 = lbvh_dd(rho[0], rho[1], rho[2], rho[0], rho[1], rho[2]), d = sqrt(d2);
        if (d > beta * m[WN_R]) { acc += wn_far(m, rho, d2, d) / WN_4PI; node = mesh.esc[node]; continue; }
        if (node >= leaf0) {
            double c[9];
            mesh_corners(mesh, (size_t)mesh.tri[node - leaf0], c);
            acc += wn_face(q, c, c + 3, c + 6);
            node = mesh.esc[node];
        } else node = mesh.left[node];
    }
    w[i] = acc;
}

// the exact sum: a query per thread, tiles of WN_TILE faces' corners in LDS, added in ascending face id
__global__ __launch_bounds__(WN_TILE) void k_wn_exact(const float* __restrict__ Q, int n, const MeshView mesh, double* __restrict__ w) {
    __shared__ double tile[WN_TILE][9];
    const int i = blockIdx.x * WN_TILE + threadIdx.x;
    const size_t qi = (size_t)(i < n ? i : n - 1);
    const double q[3] = {(double)Q[3 * qi], (double)Q[3 * qi + 1], (double)Q[3 * qi + 2]};
    const int T = mesh.T;
    double acc = 0.0;
    for (int base = 0; base < T; base += WN_TILE) {
        const int f = base + (int)threadIdx.x;
        __syncthreads();
        if (f < T) mesh_corners(mesh, (size_t)f, tile[threadIdx.x]);
        __syncthreads();
        const int m = min(WN_TILE, T - base);
        for (int t = 0; t < m; ++t) acc += wn_face(q, &tile[t][0], &tile[t][3], &tile[t][6]);
    }
    if (i < n) w[i] = (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) ? acc : wn_nan();
}

// the moment buffer of F faces: the moments of the 2 F - 1 nodes, then the build's one flag per face. The queries hold it const: they
// carve it the same way and read only mom
struct WnBuf { double* mom; int* flag; size_t total; };
static inline WnBuf wn_carve(const void* moments, int64_t F) {
    WsWalk w(moments);
    double* mom = w.take<double>(WN_STRIDE * (size_t)(2 * F - 1));
    int* flag = w.take<int>((size_t)F);
    return {mom, flag, w.bytes()};
}

}  // namespace ls

using namespace ls;

extern "C" int ls_mesh_winding_bytes(int64_t F, size_t* bytes) {
    LS_REQUIRE(bytes && F > 0, LS_E_INVALID, "ls_mesh_winding_bytes: bad argument");
    LS_REQUIRE(3 * F < INT32_MAX, LS_E_OVERFLOW, "ls_mesh_winding_bytes: more than 2^31 corners");
    *bytes = wn_carve(nullptr, F).total;
    return LS_OK;
}

extern "C" int ls_mesh_winding_prepare(void* handle, void* moments, void* stream) {
    LS_REQUIRE(handle && moments, LS_E_INVALID, "ls_mesh_winding_prepare: null argument");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    const hipStream_t st = (hipStream_t)stream;
    const int T = H->T, N = 2 * T - 1;
    const WnBuf b = wn_carve(moments, T);
    LS_HIP(hipMemsetAsync(b.flag, 0, sizeof(int) * (size_t)T, st));
    hipLaunchKernelGGL(k_wn_raw, dim3(div_up(T, BLOCK)), dim3(BLOCK), 0, st, H->view(), (const unsigned*)H->bvh.bb, (const int*)H->bvh.parent, b.flag, b.mom);
    hipLaunchKernelGGL(k_wn_centre, dim3(div_up(N, BLOCK)), dim3(BLOCK), 0, st, N, (const unsigned*)H->bvh.bb, (const float*)H->bvh.box, b.mom);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_winding_exact(void* handle, const float* P, int64_t n, double* w, void* stream) {
    LS_REQUIRE(handle && n >= 0 && (n == 0 || (P && w)), LS_E_INVALID, "ls_mesh_winding_exact: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_winding_exact: more than 2^31 query points");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    if (n == 0) return LS_OK;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    hipLaunchKernelGGL(k_wn_exact, dim3(div_up(n, WN_TILE)), dim3(WN_TILE), 0, (hipStream_t)stream, P, (int)n, H->view(), w);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_winding_query(void* handle, const void* moments, const float* P, int64_t n, double beta, double* w, void* stream) {
    LS_REQUIRE(beta >= 1.0, LS_E_INVALID, "winding number: beta must be at least 1, got %g", beta);
    if (std::isinf(beta)) return ls_mesh_winding_exact(handle, P, n, w, stream);
    LS_REQUIRE(handle && moments && n >= 0 && (n == 0 || (P && w)), LS_E_INVALID, "ls_mesh_winding_query: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_winding_query: more than 2^31 query points");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    if (n == 0) return LS_OK;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    hipLaunchKernelGGL(k_wn_walk, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, P, (int)n, H->view(),
                       (const double*)wn_carve(moments, H->T).mom, beta, w);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_winding_arrays(void* handle, const void* moments, int32_t* left, int32_t* right, int32_t* esc, int32_t* tri, float* box,
                                      double* mom, void* stream) {
    LS_REQUIRE(handle && (moments || !mom), LS_E_INVALID, "ls_mesh_winding_arrays: bad argument");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    const hipStream_t st = (hipStream_t)stream;
    const size_t T = (size_t)H->T, N = 2 * T - 1;
    if (left && T > 1) LS_HIP(hipMemcpyAsync(left, H->bvh.left, 4 * (T - 1), hipMemcpyDeviceToDevice, st));
    if (right && T > 1) LS_HIP(hipMemcpyAsync(right, H->bvh.right, 4 * (T - 1), hipMemcpyDeviceToDevice, st));
    if (esc) LS_HIP(hipMemcpyAsync(esc, H->bvh.esc, 4 * N, hipMemcpyDeviceToDevice, st));
    if (tri) LS_HIP(hipMemcpyAsync(tri, H->bvh.tri, 4 * T, hipMemcpyDeviceToDevice, st));
    if (box) LS_HIP(hipMemcpyAsync(box, H->bvh.box, 24 * N, hipMemcpyDeviceToDevice, st));
    if (mom) LS_HIP(hipMemcpyAsync(mom, wn_carve(moments, H->T).mom, sizeof(double) * WN_STRIDE * N, hipMemcpyDeviceToDevice, st));
    return LS_OK;
}
