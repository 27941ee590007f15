// distance.hip -- point-to-mesh squared distance and its directed maximum on the device (gfx950, wave64): libigl's
// point_mesh_squared_distance / hausdorff, which the reference's figures call on every recorded step.
//
// The mesh (fp32 positions, int32 faces) is held by a handle with the LBVH of lbvh.h over its faces (leaf boxes exact: margin 0). A
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
#include "common.h"
#include "lbvh.h"
#include "meshface.h"
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>

namespace ls {

typedef unsigned long long u64;
constexpr double MD_SLACK = 0x1p-40, MD_SHRINK = 1.0 - 0x1p-40;

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
    float lo[3], hi[3];
    if ((rc = lbvh_bounds(H->pos, H->V, H->bvh, st, lo, hi))) return fail(rc);
    double M = 0.0;
    for (int q = 0; q < 3; ++q) M = std::max(M, std::max(std::fabs((double)lo[q]), std::fabs((double)hi[q])));
    H->slack = MD_SLACK * M;
    if ((rc = lbvh_build(H->pos, H->faces, H->T, 0.0f, H->bvh, st))) return fail(rc);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(hip_fail(hipGetLastError(), "ls_mesh_distance_create", __FILE__, __LINE__));
    *handle = H;
    return LS_OK;
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
