// meshbvh.hip -- the handle of meshbvh.h: a device copy of one mesh (fp32 positions, int32 faces, the face indices checked) and the LBVH
// of lbvh.h over its faces (leaf boxes exact: margin 0), in one buffer of the scratch pool. distance.hip, raycast.hip, winding.hip and
// selfx.hip query it; `update` replaces the positions and rebuilds the hierarchy in the same buffer. The entry points keep the names of the
// first query that had a handle, the distance.
#include "common.h"
#include "lbvh.h"
#include "meshbvh.h"
#include "meshface.h"
#include <algorithm>
#include <cmath>
#include <new>

using namespace ls;

// the handle's arrays as the regions (256-byte aligned) of one buffer at `base`; returns the buffer's size
static size_t md_carve_handle(MeshDistanceHandle* H, void* base) {
    const size_t T = (size_t)H->T, N = 2 * T - 1;
    Lbvh& b = H->bvh;
    WsWalk w(base);
    H->pos = w.take<float>(3 * (size_t)H->V);
    H->faces = w.take<int>(3 * T);
    H->small = w.take<int>(16);
    b.code = w.take<int>(T);
    b.ord_a = w.take<int>(T);
    b.sort = sort_scratch_take(w, H->T, false);
    b.tri = w.take<int>(T);
    b.scode = w.take<unsigned>(T);
    b.left = w.take<int>(T);
    b.right = w.take<int>(T);
    b.parent = w.take<int>(N);
    b.esc = w.take<int>(N);
    b.rflag = w.take<int>(T);
    b.box = w.take<float>(6 * N);
    b.bb = base ? (unsigned*)(H->small + 8) : nullptr;
    return w.bytes();
}
// the handle's buffer from the scratch pool: measure, allocate, carve
static int md_alloc(MeshDistanceHandle* H) {
    const size_t total = md_carve_handle(H, nullptr);
    void* p = pool_take(H->device, total, &H->cap);
    if (!p) { LS_HIP(pool_alloc(H->device, &p, total)); H->cap = total; }
    H->mem = p;
    md_carve_handle(H, p);
    return LS_OK;
}
// the bounds, the slack and the LBVH of the positions in H->pos, in the handle's buffer; the stream is synchronised
static int md_build(MeshDistanceHandle* H, hipStream_t st) {
    float lo[3], hi[3];
    int rc = lbvh_bounds(H->pos, H->V, H->bvh, st, lo, hi);
    if (rc) return rc;
    double M = 0.0;         // the largest |coordinate| that is not a NaN (lbvh_bounds passes NaNs over), 0 when there is none
    for (int q = 0; q < 3; ++q)
        for (const float x : {lo[q], hi[q]})
            if (x == x) M = std::max(M, std::fabs((double)x));
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
