// distance.hip -- point-to-mesh squared distance and its directed maximum on the device (gfx950, wave64): libigl's
// point_mesh_squared_distance / hausdorff, which the reference's figures call on every recorded step.
//
// The mesh (fp32 positions, int32 faces) is held by a handle (meshbvh.h; raycast.hip queries the same one) with the LBVH of lbvh.h over
// its faces (leaf boxes exact: margin 0). A
// query point p (fp32) walks it stacklessly. Everything after the load is fp64:
//   * the leaf test is lbvh_point_tri (the remesher's region tests), guarded: a triangle whose area term |ab x ac|^2 is not positive,
//     or whose region test gives a non-finite point, is measured as the closest of its segments ab, bc, ca (the first on a tie);
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
// weights w come from the same fp64 region / segment tests that produce C (md_weights below mirrors md_point_tri branch by branch), one
// face per point, after the walk. C minimises over the face, so no derivative of w enters (envelope theorem): with d = p - C and g the
// incoming gradient, d sqrD / dp = 2 g d and d sqrD / d V[F[I, k]] = -2 g w_k d, each term formed in fp64 and rounded to fp32 once.
// The vertex gradient has no float atomics: the points are grouped by their face (groupby.h: stable, so ascending point id within a face),
// seg_sum adds the 9 terms of a face's points in that order (a thread up to 64 points, else the wave lane-strided and the xor butterfly),
// and a thread per vertex adds its corners' face rows in the rank order of meshface.h. Bitwise reproducible, no host synchronisation.
#include "common.h"
#include "groupby.h"
#include "lbvh.h"
#include "meshbvh.h"
#include "meshface.h"
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>

namespace ls {

typedef unsigned long long u64;

__device__ __forceinline__ double md_d2(const double p[3], const double r[3]) {
    const double dx = p[0] - r[0], dy = p[1] - r[1], dz = p[2] - r[2];
    return (dx * dx + dy * dy) + dz * dz;
}
// closest point of p on the segment a b: a when ap . ab <= 0, b when ap . ab >= ab . ab, else a + ab (ap . ab / ab . ab)
__device__ __forceinline__ void md_point_seg(const double p[3], const double a[3], const double b[3], double r[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double t = lbvh_dd(p[0] - a[0], p[1] - a[1], p[2] - a[2], ab[0], ab[1], ab[2]), l = lbvh_dd(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2]);
    if (t <= 0.0) { r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; }
    else if (t >= l) { r[0] = b[0]; r[1] = b[1]; r[2] = b[2]; }
    else { const double s = t / l; for (int q = 0; q < 3; ++q) r[q] = a[q] + ab[q] * s; }
}
// the guarded point-triangle test of the header comment
__device__ inline void md_point_tri(const double p[3], const double a[3], const double b[3], const double c[3], double r[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double cx = ab[1] * ac[2] - ab[2] * ac[1], cy = ab[2] * ac[0] - ab[0] * ac[2], cz = ab[0] * ac[1] - ab[1] * ac[0];
    if ((cx * cx + cy * cy) + cz * cz > 0.0) {
        lbvh_point_tri(p, a, b, c, r);
        if (isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2])) return;
    }
    double s[3];
    md_point_seg(p, a, b, r);
    double d = md_d2(p, r);
    md_point_seg(p, b, c, s);
    double e = md_d2(p, s);
    if (e < d) { r[0] = s[0]; r[1] = s[1]; r[2] = s[2]; d = e; }
    md_point_seg(p, c, a, s);
    e = md_d2(p, s);
    if (e < d) { r[0] = s[0]; r[1] = s[1]; r[2] = s[2]; }
}

// the query of lbvh_walk
struct MdQuery {
    const float* __restrict__ P;
    const int* __restrict__ faces;
    const int* __restrict__ tri;
    const float* __restrict__ box;
    double slack;
    double p[3];
    double d2, r[3];
    int id;
    __device__ __forceinline__ double bound(int node) const {
        const float* bx = box + 6 * (size_t)node;
        const double x = fmax(fmax((double)bx[0] - p[0], p[0] - (double)bx[3]) - slack, 0.0);
        const double y = fmax(fmax((double)bx[1] - p[1], p[1] - (double)bx[4]) - slack, 0.0);
        const double z = fmax(fmax((double)bx[2] - p[2], p[2] - (double)bx[5]) - slack, 0.0);
        return ((x * x + y * y) + z * z) * MD_SHRINK;
    }
    __device__ __forceinline__ double best() const { return d2; }
    __device__ __forceinline__ void leaf(int i) {
        const int f = tri[i];
        double a[3], b[3], c[3], q[3];
        for (int k = 0; k < 3; ++k) { a[k] = P[3 * (size_t)faces[3 * f] + k]; b[k] = P[3 * (size_t)faces[3 * f + 1] + k]; c[k] = P[3 * (size_t)faces[3 * f + 2] + k]; }
        md_point_tri(p, a, b, c, q);
        const double e = md_d2(p, q);
        if (e < d2 || (e == d2 && f < id)) { d2 = e; id = f; r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; }
    }
};

// one thread per query point; any of sqrD / I / C may be null; dmax: the bits of max d2 over the points (or null)
__global__ __launch_bounds__(BLOCK) void k_md_query(const float* __restrict__ Q, int n, const float* __restrict__ P, const int* __restrict__ faces, int T,
                                                    const int* __restrict__ tri, const float* __restrict__ box, const int* __restrict__ left,
                                                    const int* __restrict__ right, const int* __restrict__ esc, double slack, double* __restrict__ sqrD,
                                                    int64_t* __restrict__ I, double* __restrict__ C, u64* __restrict__ dmax) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double d2 = 0.0;
    if (i < n) {
        MdQuery q{P, faces, tri, box, slack, {Q[3 * (size_t)i], Q[3 * (size_t)i + 1], Q[3 * (size_t)i + 2]}, 0.0, {0.0, 0.0, 0.0}, 0x7fffffff};
        q.d2 = __longlong_as_double(0x7ff0000000000000ll);
        lbvh_walk(left, right, esc, T, q);
        d2 = q.d2;
        if (sqrD) sqrD[i] = d2;
        if (I) I[i] = q.id;
        if (C) { C[3 * (size_t)i] = q.r[0]; C[3 * (size_t)i + 1] = q.r[1]; C[3 * (size_t)i + 2] = q.r[2]; }
    }
    if (!dmax) return;
    for (int m = WAVE / 2; m >= 1; m /= 2) d2 = fmax(d2, __shfl_xor(d2, m));
    if ((threadIdx.x & (WAVE - 1)) == 0) atomicMax(dmax, (u64)__double_as_longlong(d2));
}

// ---- the barycentric weights of the closest point ------------------------------------------------------------------------------
// the weights of lbvh_point_tri's point on (a, b, c): its tests, in its order, with its quotients
__device__ inline void md_tri_weights(const double p[3], const double a[3], const double b[3], const double c[3], double w[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double d1 = lbvh_dd(ab[0], ab[1], ab[2], ap[0], ap[1], ap[2]), d2 = lbvh_dd(ac[0], ac[1], ac[2], ap[0], ap[1], ap[2]);
    if (d1 <= 0.0 && d2 <= 0.0) { w[0] = 1.0; w[1] = 0.0; w[2] = 0.0; return; }
    const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const double d3 = lbvh_dd(ab[0], ab[1], ab[2], bp[0], bp[1], bp[2]), d4 = lbvh_dd(ac[0], ac[1], ac[2], bp[0], bp[1], bp[2]);
    if (d3 >= 0.0 && d4 <= d3) { w[0] = 0.0; w[1] = 1.0; w[2] = 0.0; return; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        w[0] = 1.0 - v; w[1] = v; w[2] = 0.0;
        return;
    }
    const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const double d5 = lbvh_dd(ab[0], ab[1], ab[2], cp[0], cp[1], cp[2]), d6 = lbvh_dd(ac[0], ac[1], ac[2], cp[0], cp[1], cp[2]);
    if (d6 >= 0.0 && d5 <= d6) { w[0] = 0.0; w[1] = 0.0; w[2] = 1.0; return; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double u = d2 / (d2 - d6);
        w[0] = 1.0 - u; w[1] = 0.0; w[2] = u;
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double u = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        w[0] = 0.0; w[1] = 1.0 - u; w[2] = u;
        return;
    }
    const double den = 1.0 / ((va + vb) + vc), v = vb * den, u = vc * den;
    w[0] = (1.0 - v) - u; w[1] = v; w[2] = u;
}
// the weights of md_point_seg's point on the two ends of the segment a b
__device__ __forceinline__ void md_seg_weights(const double p[3], const double a[3], const double b[3], double& wa, double& wb) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double t = lbvh_dd(p[0] - a[0], p[1] - a[1], p[2] - a[2], ab[0], ab[1], ab[2]), l = lbvh_dd(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2]);
    if (t <= 0.0) { wa = 1.0; wb = 0.0; }
    else if (t >= l) { wa = 0.0; wb = 1.0; }
    else { const double s = t / l; wa = 1.0 - s; wb = s; }
}
// the weights of md_point_tri's point: the guard, and on a degenerate face the segment md_point_tri picks (ab, bc, ca; a later one only
// when strictly closer), the corner off that segment getting 0
__device__ inline void md_weights(const double p[3], const double a[3], const double b[3], const double c[3], double w[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double cx = ab[1] * ac[2] - ab[2] * ac[1], cy = ab[2] * ac[0] - ab[0] * ac[2], cz = ab[0] * ac[1] - ab[1] * ac[0];
    double r[3], s[3], u0, u1;
    if ((cx * cx + cy * cy) + cz * cz > 0.0) {
        lbvh_point_tri(p, a, b, c, r);
        if (isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2])) { md_tri_weights(p, a, b, c, w); return; }
    }
    md_point_seg(p, a, b, r);
    double d = md_d2(p, r);
    md_seg_weights(p, a, b, u0, u1);
    w[0] = u0; w[1] = u1; w[2] = 0.0;
    md_point_seg(p, b, c, s);
    double e = md_d2(p, s);
    if (e < d) { d = e; md_seg_weights(p, b, c, u0, u1); w[0] = 0.0; w[1] = u0; w[2] = u1; }
    md_point_seg(p, c, a, s);
    e = md_d2(p, s);
    if (e < d) { md_seg_weights(p, c, a, u0, u1); w[0] = u1; w[1] = 0.0; w[2] = u0; }
}

// one thread per point: W[i] = the weights of point i on face I[i]; an I outside [0, T) gives NaN weights (and reads nothing)
__global__ __launch_bounds__(BLOCK) void k_md_weights(const float* __restrict__ Q, int n, const float* __restrict__ P, const int* __restrict__ faces, int T,
                                                      const int64_t* __restrict__ I, double* __restrict__ W) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t f = I[i];
    double w[3];
    if (f < 0 || f >= T) w[0] = w[1] = w[2] = __longlong_as_double(0x7ff8000000000000ll);
    else {
        const double p[3] = {Q[3 * (size_t)i], Q[3 * (size_t)i + 1], Q[3 * (size_t)i + 2]};
        double a[3], b[3], c[3];
        for (int k = 0; k < 3; ++k) { a[k] = P[3 * (size_t)faces[3 * f] + k]; b[k] = P[3 * (size_t)faces[3 * f + 1] + k]; c[k] = P[3 * (size_t)faces[3 * f + 2] + k]; }
        md_weights(p, a, b, c, w);
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
}  // namespace ls

using namespace ls;

// carves the handle's arrays out of one buffer (256-byte aligned) of the scratch pool
static int md_alloc(MeshDistanceHandle* H) {
    const int64_t T = H->T, N = 2 * T - 1;
    void* sort = nullptr;
    void** slot[] = {(void**)&H->pos, (void**)&H->faces, (void**)&H->small, (void**)&H->bvh.code, (void**)&H->bvh.ord_a, &sort,
                     (void**)&H->bvh.tri, (void**)&H->bvh.scode, (void**)&H->bvh.left, (void**)&H->bvh.right, (void**)&H->bvh.parent,
                     (void**)&H->bvh.esc, (void**)&H->bvh.rflag, (void**)&H->bvh.box};
    const int64_t bytes[] = {12 * (int64_t)H->V, 12 * T, 4 * 16, 4 * T, 4 * T, (int64_t)sort_scratch_bytes(T, false),
                             4 * T, 4 * T, 4 * T, 4 * T, 4 * N, 4 * N, 4 * T, 24 * N};
    size_t total = 0;
    for (int64_t b : bytes) total += ((size_t)b + 255) & ~(size_t)255;
    void* p = pool_take(H->device, total, &H->cap);
    if (!p) { LS_HIP(pool_alloc(H->device, &p, total)); H->cap = total; }
    H->mem = p;
    size_t off = 0;
    for (int k = 0; k < (int)(sizeof(bytes) / sizeof(bytes[0])); ++k) {
        *slot[k] = (char*)p + off;
        off += ((size_t)bytes[k] + 255) & ~(size_t)255;
    }
    H->bvh.sort = sort_scratch_carve(sort, T, false);
    H->bvh.bb = (unsigned*)(H->small + 8);
    return LS_OK;
}
// the bounds, the slack and the LBVH of the positions in H->pos, in the handle's buffer; the stream is synchronised
static int md_build(MeshDistanceHandle* H, hipStream_t st) {
    float lo[3], hi[3];
    int rc = lbvh_bounds(H->pos, H->V, H->bvh, st, lo, hi);
    if (rc) return rc;
    double M = 0.0;
    for (int q = 0; q < 3; ++q) M = std::max(M, std::max(std::fabs((double)lo[q]), std::fabs((double)hi[q])));
    H->slack = MD_SLACK * M;
    if ((rc = lbvh_build(H->pos, H->faces, H->T, 0.0f, H->bvh, st))) return rc;
    LS_HIP(hipStreamSynchronize(st));
    return LS_OK;
}
extern "C" int ls_mesh_distance_create(const float* verts, int64_t V, const void* faces, int idx_bytes, int64_t F, int device, void* stream,
                                       void** handle) {
    LS_REQUIRE(handle, LS_E_INVALID, "ls_mesh_distance_create: null handle pointer");
    *handle = nullptr;
    LS_REQUIRE(verts && faces && (idx_bytes == 4 || idx_bytes == 8), LS_E_INVALID, "ls_mesh_distance_create: bad argument");
    LS_REQUIRE(F > 0, LS_E_INVALID, "mesh distance: the mesh has no faces");
    LS_REQUIRE(V > 0, LS_E_INVALID, "mesh distance: the mesh has no vertices");
    LS_REQUIRE(V < INT32_MAX / 3 && 3 * F < INT32_MAX, LS_E_OVERFLOW, "ls_mesh_distance_create: the mesh does not fit int32 indices");
    DeviceGuard g(device);
    LS_HIP(g.err);
    MeshDistanceHandle* H = new (std::nothrow) MeshDistanceHandle();
    LS_REQUIRE(H, LS_E_INVALID, "ls_mesh_distance_create: out of host memory");
    H->device = device;
    H->V = (int)V;
    H->T = (int)F;
    const hipStream_t st = (hipStream_t)stream;
    auto fail = [&](int rc) { ls_mesh_distance_destroy(H); return rc; };
    const int n = 3 * H->T;
    int rc = md_alloc(H);
    if (rc) return fail(rc);
    if (hipMemsetAsync(H->small, 0, sizeof(int) * 16, st) != hipSuccess ||
        hipMemcpyAsync(H->pos, verts, sizeof(float) * 3 * V, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return fail(hip_fail(hipGetLastError(), "ls_mesh_distance_create copies", __FILE__, __LINE__));
    int bad = 0;
    if (!faces_in(faces, idx_bytes, n, V, H->faces, H->small, st, &bad))
        return fail(hip_fail(hipGetLastError(), "ls_mesh_distance_create", __FILE__, __LINE__));
    if (bad) { set_error("mesh distance: a face index is outside [0, %lld)", (long long)V); return fail(LS_E_INDEX); }
    if ((rc = md_build(H, st))) return fail(rc);
    *handle = H;
    return LS_OK;
}

extern "C" int ls_mesh_distance_update(void* handle, const float* verts, void* stream) {
    LS_REQUIRE(handle && verts, LS_E_INVALID, "ls_mesh_distance_update: null argument");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    const hipStream_t st = (hipStream_t)stream;
    LS_HIP(hipMemcpyAsync(H->pos, verts, sizeof(float) * 3 * (size_t)H->V, hipMemcpyDeviceToDevice, st));
    return md_build(H, st);
}

static int md_launch(MeshDistanceHandle* H, const float* P, int64_t n, double* sqrD, int64_t* I, double* C, u64* dmax, hipStream_t st) {
    hipLaunchKernelGGL(k_md_query, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, P, (int)n, (const float*)H->pos, (const int*)H->faces, H->T,
                       (const int*)H->bvh.tri, (const float*)H->bvh.box, (const int*)H->bvh.left, (const int*)H->bvh.right, (const int*)H->bvh.esc,
                       H->slack, sqrD, I, C, dmax);
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
    hipLaunchKernelGGL(k_md_weights, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, P, (int)n, (const float*)H->pos, (const int*)H->faces, H->T,
                       I, W);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_distance_backward_workspace_bytes(int64_t n, int64_t F, size_t* bytes) {
    LS_REQUIRE(bytes && n >= 0 && F > 0, LS_E_INVALID, "ls_mesh_distance_backward_workspace_bytes: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK && 3 * F < INT32_MAX, LS_E_OVERFLOW, "ls_mesh_distance_backward_workspace_bytes: more than 2^31 points or corners");
    *bytes = md_layout(n, F).total;
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
    const MdWs L = md_layout(n, H->T);
    LS_REQUIRE(!gV || ws_bytes >= L.total, LS_E_WORKSPACE, "ls_mesh_distance_backward: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard guard(H->device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    if (gP && n > 0) hipLaunchKernelGGL(k_md_grad_points, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, P, C, g, (int)n, gP);
    if (gV && n == 0) LS_HIP(hipMemsetAsync(gV, 0, sizeof(float) * 3 * (size_t)H->V, st));
    if (gV && n > 0) {
        char* w = (char*)ws;
        int* keys = (int*)(w + L.keys);
        int* order = (int*)(w + L.order);
        int* seg = (int*)(w + L.seg);
        double* W = (double*)(w + L.W);
        float* rows = (float*)(w + L.rows);
        hipLaunchKernelGGL(k_md_weights, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, P, (int)n, (const float*)H->pos, (const int*)H->faces, H->T, I, W);
        hipLaunchKernelGGL(k_md_keys<0>, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, I, (int)n, H->T, keys);
        int rc = group_by_key<true>(keys, n, H->T, order, seg, sort_scratch_carve(w + L.sort, n, true), st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_md_face_rows<MdRows>, dim3(div_up(H->T, 256)), dim3(256), 0, st, MdRows{P, C, g, W, order, seg, rows}, (int64_t)H->T);
        hipLaunchKernelGGL(k_md_gather_verts<0>, dim3(div_up(H->V, 256)), dim3(256), 0, st, (const float*)rows, vptr, corner_order, (int64_t)H->V, gV);
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_distance_destroy(void* handle) {
    if (!handle) return LS_OK;
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    {
        DeviceGuard g(H->device);
        (void)hipDeviceSynchronize();          // queries may have run on any stream of the device
        if (H->mem && !pool_give(H->device, H->mem, H->cap)) (void)hipFree(H->mem);
    }
    delete H;
    return LS_OK;
}
