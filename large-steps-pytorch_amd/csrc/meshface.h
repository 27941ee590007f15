// meshface.h -- what the translation units that run a thread per face (or per vertex, over its corners) share: normals.hip,
// meshgeom.hip, and the index narrowing of remesh.hip and distance.hip. fp32 positions (V, 3), faces (F, 3) of int32 or int64.
//
// The corner-rank contract (ls_corner_ranks builds the arrays once per face tensor). The 3 F corners are ranked
// vertex-major, a vertex's corners in ascending corner id 3 f + i: cpos[3 f + i] is the rank of a corner, vptr[v] .. vptr[v + 1] the
// ranks vertex v owns, order[] the inverse of cpos. A per-face kernel writes the 3-vector of a corner at slot cpos[3 f + i] of a
// corner buffer (3 F, 3); k_gather_corners sums the slots of each vertex in RANK ORDER. No atomics: rank order is summation order,
// so every per-vertex sum -- every gradient -- is bitwise reproducible. A pass that walks order[] instead (a thread per vertex
// recomputing its corners' faces) adds in the same order and gives the same bits.
// Kernels and the host functions that launch them are templates only so that the header can be included by several translation units
// (a unit gets the kernels it uses, no others).
#pragma once
#include "common.h"
#include <algorithm>

namespace ls {

constexpr int MESH_MAXG = 1024;     // partial sums per reduction (the grid of a looping reduction is capped to this)
static inline int reduce_grid(int64_t F) { return (int)std::min<int64_t>(MESH_MAXG, std::max<int64_t>(1, div_up(F, BLOCK))); }

template <typename IDX>
__device__ __forceinline__ void load_face(const IDX* __restrict__ faces, int64_t f, const float* __restrict__ verts,
                                          int (&id)[3], float (&p)[3][3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        id[c] = (int)faces[f * 3 + c];
#pragma unroll
        for (int q = 0; q < 3; ++q) p[c][q] = verts[(size_t)id[c] * 3 + q];
    }
}

// a 3-vector at a 4-byte aligned address as ONE 12-byte access (global_load_dwordx3)
typedef float f3_mesh __attribute__((ext_vector_type(3), aligned(4)));
typedef int i3_mesh __attribute__((ext_vector_type(3), aligned(4)));
__device__ __forceinline__ void ld3(const float* __restrict__ base, size_t row, float (&v)[3]) {
    const f3_mesh t = *reinterpret_cast<const f3_mesh*>(base + row * 3);
    v[0] = t.x; v[1] = t.y; v[2] = t.z;
}
__device__ __forceinline__ void ld_ids(const int32_t* __restrict__ faces, int64_t f, int (&id)[3]) {
    const i3_mesh t = *reinterpret_cast<const i3_mesh*>(faces + f * 3);
    id[0] = t.x; id[1] = t.y; id[2] = t.z;
}
__device__ __forceinline__ void ld_ids(const int64_t* __restrict__ faces, int64_t f, int (&id)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) id[c] = (int)faces[f * 3 + c];
}

__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// torch's CPU norm(dim=1) of a 3-vector a - b
__device__ __forceinline__ float edge_norm(const float (&a)[3], const float (&b)[3]) {
    const float x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
}

// dst[v] = sum of the corner vectors of vertex v, the slots [vptr[v], vptr[v + 1]) of `corner`, in rank order -- consecutive threads
// read consecutive memory. out != nullptr: also writes the unit vector there.
template <int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_gather_corners(const int* __restrict__ vptr, const float* __restrict__ corner, int64_t V,
                                                          float* __restrict__ dst, float* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int e0 = vptr[v], e1 = vptr[v + 1];
    // the first GC corners (a vertex of a triangle mesh has ~6) are requested together, from clamped addresses (no branch between
    // the loads); the sum runs over them in rank order as before
    constexpr int GC = 8;
    float c[GC][3];
    // e1 == e0 (unreferenced vertex): slot 0, which every corner buffer has (max(F, 1) x 3 slots); the value is not used. Not e0: the
    // unreferenced vertices after the last referenced one have e0 == 3 F, one slot past the buffer
    const int last = max(e1 - 1, 0);
#pragma unroll
    for (int t = 0; t < GC; ++t) {
        const size_t e = (size_t)min(e0 + t, last);
#pragma unroll
        for (int q = 0; q < 3; ++q) c[t][q] = corner[e * 3 + q];
    }
    float x = 0.0f, y = 0.0f, z = 0.0f;
#pragma unroll
    for (int t = 0; t < GC; ++t) {
        if (e0 + t < e1) { x += c[t][0]; y += c[t][1]; z += c[t][2]; }
    }
    for (int e = e0 + GC; e < e1; ++e) {
        x += corner[(size_t)e * 3]; y += corner[(size_t)e * 3 + 1]; z += corner[(size_t)e * 3 + 2];
    }
    dst[v * 3] = x; dst[v * 3 + 1] = y; dst[v * 3 + 2] = z;
    if (out) {
        const float len = sqrtf(x * x + y * y + z * z);
        out[v * 3] = x / len; out[v * 3 + 1] = y / len; out[v * 3 + 2] = z / len;
    }
}

// (a template although it is static inline: a plain function would instantiate the kernel in every unit that includes the header)
template <int UNIT = 0>
static inline void gather_corners(const int* vptr, const float* corner, int64_t V, float* dst, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_corners<UNIT>, dim3(div_up(V, BLOCK)), dim3(BLOCK), 0, st, vptr, corner, V, dst, out);
}

// out[i] = (int)in[i]; an index outside [0, V) raises bad[0] and is stored as 0
template <typename IDX, int UNIT = 0>
__global__ __launch_bounds__(BLOCK) void k_faces_in(const IDX* __restrict__ in, int64_t n, int64_t V, int* __restrict__ out, int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const IDX x = in[i];
    if (x < 0 || (int64_t)x >= V) { atomicOr(bad, 1); out[i] = 0; }
    else out[i] = (int)x;
}

}  // namespace ls

// runs the statements once with IDX = the index type of `bytes` bytes
#define LS_IDX(bytes, ...)                                                                     \
    do {                                                                                       \
        if ((bytes) == 8) { typedef int64_t IDX; __VA_ARGS__; } else { typedef int32_t IDX; __VA_ARGS__; } \
    } while (0)

namespace ls {

// the n indices of `faces` narrowed into `out` on `st`, then the flag d_bad[0] (zero before the call) read back into *bad: the stream is
// synchronised. false: a HIP call failed (the caller reports hipGetLastError under its own name). A template for the reason given at
// gather_corners.
template <int UNIT = 0>
static inline bool faces_in(const void* faces, int idx_bytes, int64_t n, int64_t V, int* out, int* d_bad, hipStream_t st, int* bad) {
    LS_IDX(idx_bytes, hipLaunchKernelGGL((k_faces_in<IDX, UNIT>), dim3(div_up(std::max<int64_t>(n, 1), BLOCK)), dim3(BLOCK), 0, st, (const IDX*)faces, n, V,
                                         out, d_bad));
    return hipMemcpyAsync(bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}

static inline int check_mesh_args(const void* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const char* who) {
    LS_REQUIRE(verts && (faces || F == 0) && (idx_bytes == 4 || idx_bytes == 8) && F >= 0 && V > 0 && V < INT32_MAX && 3 * F < INT32_MAX,
               LS_E_INVALID, "%s: bad argument (faces must be int32 or int64, V and 3 F < 2^31)", who);
    return LS_OK;
}

// the workspace requirement of an entry point: size_fn is its ls_*_workspace_bytes
typedef int (*mesh_ws_fn)(int64_t, int64_t, size_t*);
static inline int require_workspace(const char* who, mesh_ws_fn size_fn, int64_t F, int64_t V, size_t ws_bytes) {
    size_t need = 0;
    size_fn(F, V, &need);
    LS_REQUIRE(ws_bytes >= need, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, need);
    return LS_OK;
}

}  // namespace ls
