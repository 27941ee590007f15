// meshgeom.hip -- average edge length and Voronoi vertex areas with their gradients (gfx950, wave64).
//
// Reference semantics (rgl-epfl/large-steps-pytorch scripts/geometry.py):
//   average_edge_length :13-33   (sum over faces of |v1 - v2| + |v0 - v2| + |v0 - v1|) / F / 3 -- a 0-dim fp32 tensor; F == 0
//                                gives NaN (0 / 0). scripts/main.py:146 takes the remesher's target length from it.
//   massmatrix_voronoi :35-89    per face: edge lengths l_k (opposite corner k), law-of-cosines cosines, barycentric weights
//                                of the circumcentre, Heron's area A, corner quads 0.5 (t_k1 + t_k2) with t = A * bary, then
//                                three torch.where overrides (obtuse corner 0, 1, 2 in turn: A/2 at the obtuse corner, A/4 at
//                                the others, a later one wins, a NaN cosine selects nothing); scatter_add_ into column j =
//                                corner slot j, then .sum(dim=1). An unreferenced vertex gets 0, a face with a zero-length
//                                edge NaN cells.
// The forward cells follow the reference's fp32 operation order (the library is built with -ffp-contract=off; the edge length
// is torch's CPU norm, edge_norm of meshface.h), and the per-vertex sum follows its
// reduction: s_j = the vertex's slot-j corners in ascending face id, mass = (s0 + s1) + s2.
//
// Launch structure (bytes at the 1M-vertex sphere, F = 2V, 4-byte indices):
//   massmatrix forward   ONE vertex-major launch: a thread per vertex walks its corners in rank order (order[] = the inverse of
//                        cpos; the ranking sorts a vertex's corners by corner id, i.e. by face id within a slot) and recomputes
//                        the face of each -- 3x the face arithmetic, no corner buffer. Algorithmic bytes: vptr 4 V + order 12 F
//                        + faces 12 F + verts 12 V + mass 4 V = 20 V + 24 F (~68 MB); the 3 corner loads of a face re-read
//                        faces and verts that neighbouring threads share (L2).
//   massmatrix backward  per face: the 9 coordinates' gradient (reverse pass of the reference's torch graph, op by op) written
//                        at the corners' ranks, then gather_corners of meshface.h (2 launches).
//   average forward      per face l0 + l1 + l2 in fp32, fp64 partial sums per workgroup (grid fixed by F), one workgroup sums
//                        the partials in a fixed order and applies / F / 3 in fp32: bitwise reproducible, no host sync.
//   average backward     g read from device memory: each edge adds (g / 3 / F) (p_a - p_b) / |p_a - p_b| to its ends (0 for a
//                        zero-length edge), written per corner and gathered as above.
#include "meshface.h"
#include "workspace.h"

namespace ls {

// every intermediate of one face in the reference's fp32 order; l[k] = |p[k1] - p[k2]| (k1 = k + 1, k2 = k + 2 mod 3)
struct VoronoiFace {
    float l[3], cs[3], den[3], bary[3], S, s[4], r, A, cell[3];
    bool obtuse[3];
};
__device__ __forceinline__ VoronoiFace voronoi_face(const float (&p)[3][3]) {
    VoronoiFace t;
    t.l[0] = edge_norm(p[1], p[2]);
    t.l[1] = edge_norm(p[2], p[0]);
    t.l[2] = edge_norm(p[0], p[1]);
    const float sq[3] = {t.l[0] * t.l[0], t.l[1] * t.l[1], t.l[2] * t.l[2]};
    float braw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        t.den[k] = (2.0f * t.l[k1]) * t.l[k2];
        t.cs[k] = ((sq[k1] + sq[k2]) - sq[k]) / t.den[k];
        braw[k] = t.cs[k] * t.l[k];
        t.obtuse[k] = t.cs[k] < 0.0f;             // false for NaN
    }
    t.S = (braw[0] + braw[1]) + braw[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) t.bary[k] = braw[k] / t.S;
    t.s[0] = (t.l[0] + t.l[1]) + t.l[2];
    t.s[1] = (t.l[0] + t.l[1]) - t.l[2];
    t.s[2] = (t.l[0] - t.l[1]) + t.l[2];
    t.s[3] = (-t.l[0] + t.l[1]) + t.l[2];
    t.r = sqrtf(((t.s[0] * t.s[1]) * t.s[2]) * t.s[3]);
    t.A = 0.25f * t.r;
    const float ta[3] = {t.A * t.bary[0], t.A * t.bary[1], t.A * t.bary[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) t.cell[k] = 0.5f * (ta[(k + 1) % 3] + ta[(k + 2) % 3]);
    const float half = 0.5f * t.A, quarter = 0.25f * t.A;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (t.obtuse[k]) {
#pragma unroll
            for (int j = 0; j < 3; ++j) t.cell[j] = j == k ? half : quarter;
        }
    }
    return t;
}

// mass[v] = (s0 + s1) + s2, s_j = the cells of v's slot-j corners in rank order (= ascending face id); VG corners are requested
// together (clamped addresses), then summed in rank order
template <typename IDX, int VG>
__global__ __launch_bounds__(BLOCK) void k_voronoi_mass_gather(const float* __restrict__ verts, const IDX* __restrict__ faces, int64_t V,
                                                               const int* __restrict__ vptr, const int* __restrict__ order,
                                                               float* __restrict__ mass) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int e0 = vptr[v], e1 = vptr[v + 1];
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int eb = e0; eb < e1; eb += VG) {
        int cid[VG], id[VG][3];
        float p[VG][3][3];
#pragma unroll
        for (int t = 0; t < VG; ++t) cid[t] = order[min(eb + t, e1 - 1)];
#pragma unroll
        for (int t = 0; t < VG; ++t) {
#pragma unroll
            for (int c = 0; c < 3; ++c) id[t][c] = (int)faces[(int64_t)(cid[t] / 3) * 3 + c];
        }
#pragma unroll
        for (int t = 0; t < VG; ++t) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ld3(verts, (size_t)id[t][c], p[t][c]);
        }
#pragma unroll
        for (int t = 0; t < VG; ++t) {
            if (eb + t < e1) {
                const VoronoiFace fc = voronoi_face(p[t]);
                const int slot = cid[t] - 3 * (cid[t] / 3);
                if (slot == 0) s0 += fc.cell[0];
                else if (slot == 1) s1 += fc.cell[1];
                else s2 += fc.cell[2];
            }
        }
    }
    mass[v] = (s0 + s1) + s2;
}

// d sum(g * mass) / d verts of one face: the reverse pass of the reference's graph, op by op, with torch's backward rules
// (div: d/db = -g (a / b) / b; sqrt: g / (2 sqrt); norm: x (g / |x|), 0 where |x| == 0; where: the gradient goes to the
// selected branch, 0 to the other) -- so a collinear face (area 0, sum of the barycentric weights 0) gives what torch gives.
__device__ __forceinline__ void voronoi_face_bwd(const float (&p)[3][3], const float (&gc)[3], float (&gv)[3][3]) {
    const VoronoiFace t = voronoi_face(p);
    float G[3] = {gc[0], gc[1], gc[2]};
    float gA = 0.0f;
#pragma unroll
    for (int k = 2; k >= 0; --k) {                 // the overrides, last applied first
        if (t.obtuse[k]) {
#pragma unroll
            for (int j = 2; j >= 0; --j) {
                gA += (j == k ? 0.5f : 0.25f) * G[j];
                G[j] = 0.0f;
            }
        }
    }
    float gl[3] = {0.0f, 0.0f, 0.0f}, gbraw[3], gS = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float gt = 0.5f * G[(k + 1) % 3] + 0.5f * G[(k + 2) % 3];     // t_k enters the cells of corners k1 and k2
        gA += gt * t.bary[k];
        const float gb = gt * t.A;
        gbraw[k] = gb / t.S;
        gS -= gb * (t.bary[k] / t.S);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const float gbr = gbraw[k] + gS;
        const float gcos = gbr * t.l[k];
        gl[k] += gbr * t.cs[k];
        const float gnum = gcos / t.den[k];
        const float gden = -gcos * (t.cs[k] / t.den[k]);
        gl[k1] += 2.0f * (gden * t.l[k2]) + 2.0f * gnum * t.l[k1];
        gl[k2] += gden * (2.0f * t.l[k1]) + 2.0f * gnum * t.l[k2];
        gl[k] -= 2.0f * gnum * t.l[k];
    }
    const float gP = (0.25f * gA) / (2.0f * t.r);
    const float gs3 = gP * ((t.s[0] * t.s[1]) * t.s[2]);
    const float g012 = gP * t.s[3];
    const float gs2 = g012 * (t.s[0] * t.s[1]);
    const float g01 = g012 * t.s[2];
    const float gs0 = g01 * t.s[1], gs1 = g01 * t.s[0];
    gl[0] += gs0 + gs1 + gs2 - gs3;
    gl[1] += gs0 + gs1 - gs2 + gs3;
    gl[2] += gs0 - gs1 + gs2 + gs3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int q = 0; q < 3; ++q) gv[i][q] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const float w = t.l[k] == 0.0f ? 0.0f : gl[k] / t.l[k];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float gd = (p[k1][q] - p[k2][q]) * w;
            gv[k1][q] += gd;
            gv[k2][q] -= gd;
        }
    }
}

template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_voronoi_mass_bwd(const float* __restrict__ verts, const IDX* __restrict__ faces, int64_t F,
                                                            const float* __restrict__ g_mass, const int* __restrict__ cpos,
                                                            float* __restrict__ corner) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int id[3];
    float p[3][3], gv[3][3];
    load_face(faces, f, verts, id, p);
    const float gc[3] = {g_mass[id[0]], g_mass[id[1]], g_mass[id[2]]};
    voronoi_face_bwd(p, gc, gv);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const size_t c = (size_t)cpos[f * 3 + i] * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) corner[c + q] = gv[i][q];
    }
}

// fp64 partial sums of l0 + l1 + l2 (fp32 per face, as the reference adds A + B + C) over this workgroup's stride of faces
template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_edge_length_partials(const float* __restrict__ verts, const IDX* __restrict__ faces, int64_t F,
                                                                double* __restrict__ part) {
    __shared__ double smem[BLOCK / WAVE];
    double acc[1] = {0.0};
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * BLOCK) {
        int id[3];
        float p[3][3];
        load_face(faces, f, verts, id, p);
        acc[0] += (double)((edge_norm(p[1], p[2]) + edge_norm(p[0], p[2])) + edge_norm(p[0], p[1]));
    }
    block_sum<1>(acc, smem);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// out = (float)(sum of the G partials, fixed order) / F / 3 in fp32, as the reference divides; F == 0: 0 / 0 = NaN
constexpr int MG_FIN = 1024;
__global__ __launch_bounds__(MG_FIN) void k_edge_length_finish(const double* __restrict__ part, int G, int64_t F, float* __restrict__ out) {
    __shared__ double smem[MG_FIN / WAVE];
    double acc = 0.0;
    for (int g = threadIdx.x; g < G; g += MG_FIN) acc += part[g];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    acc = wave_sum(acc);
    if (lane == 0) smem[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int j = 0; j < MG_FIN / WAVE; ++j) t += smem[j];
        out[0] = ((float)t / (float)F) / 3.0f;
    }
}

// each edge adds (g / 3 / F) (p_a - p_b) / |p_a - p_b| to a and its negative to b (0 for a zero-length edge)
template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_edge_length_bwd(const float* __restrict__ verts, const IDX* __restrict__ faces, int64_t F,
                                                           const float* __restrict__ g_out, const int* __restrict__ cpos,
                                                           float* __restrict__ corner) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    const float c = (g_out[0] / 3.0f) / (float)F;
    int id[3];
    float p[3][3], gv[3][3];
    load_face(faces, f, verts, id, p);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int q = 0; q < 3; ++q) gv[i][q] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        const float l = edge_norm(p[k1], p[k2]);
        const float w = l == 0.0f ? 0.0f : c / l;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float gd = (p[k1][q] - p[k2][q]) * w;
            gv[k1][q] += gd;
            gv[k2][q] -= gd;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const size_t cp = (size_t)cpos[f * 3 + i] * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) corner[cp + q] = gv[i][q];
    }
}

}  // namespace ls

using namespace ls;

// the partial sums of the average edge length | one 3-vector per corner (backward passes): packed at natural alignment
struct GeomWs { double* part; float* corner; size_t total; };
static GeomWs carve(void* workspace, int64_t F) {
    WsWalk w(workspace);
    double* part = w.take<double>(MESH_MAXG, 8);
    float* corner = w.take<float>(9 * (size_t)std::max<int64_t>(F, 1), 4);
    return {part, corner, w.bytes()};
}

extern "C" int ls_meshgeom_workspace_bytes(int64_t F, int64_t V, size_t* h_bytes) {
    LS_REQUIRE(h_bytes && F >= 0 && V >= 0, LS_E_INVALID, "ls_meshgeom_workspace_bytes: bad argument");
    *h_bytes = carve(nullptr, F).total;
    return LS_OK;
}

extern "C" int ls_massmatrix_voronoi(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                                     const int32_t* order, float* mass, int device, void* stream) {
    int rc = check_mesh_args(verts, faces, idx_bytes, F, V, "ls_massmatrix_voronoi");
    if (rc) return rc;
    LS_REQUIRE(mass && vptr && (order || F == 0), LS_E_INVALID, "ls_massmatrix_voronoi: null argument");
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    LS_IDX(idx_bytes, hipLaunchKernelGGL((k_voronoi_mass_gather<IDX, 4>), dim3(div_up(V, BLOCK)), dim3(BLOCK), 0, st, verts, (const IDX*)faces, V,
                                         vptr, order, mass));
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_massmatrix_voronoi_backward(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                                              const int32_t* cpos, const float* g_mass, float* grad_verts, void* workspace, size_t ws_bytes,
                                              int device, void* stream) {
    int rc = check_mesh_args(verts, faces, idx_bytes, F, V, "ls_massmatrix_voronoi_backward");
    if (rc) return rc;
    LS_REQUIRE(g_mass && grad_verts && vptr && workspace && (cpos || F == 0), LS_E_INVALID, "ls_massmatrix_voronoi_backward: null argument");
    if ((rc = require_workspace("ls_massmatrix_voronoi_backward", ls_meshgeom_workspace_bytes, F, V, ws_bytes))) return rc;
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    float* corner = carve(workspace, F).corner;
    if (F > 0)
        LS_IDX(idx_bytes, hipLaunchKernelGGL(k_voronoi_mass_bwd<IDX>, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, verts, (const IDX*)faces, F,
                                             g_mass, cpos, corner));
    gather_corners(vptr, corner, V, grad_verts, nullptr, st);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_average_edge_length(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, float* out, void* workspace,
                                      size_t ws_bytes, int device, void* stream) {
    int rc = check_mesh_args(verts, faces, idx_bytes, F, V, "ls_average_edge_length");
    if (rc) return rc;
    LS_REQUIRE(out && workspace, LS_E_INVALID, "ls_average_edge_length: null argument");
    if ((rc = require_workspace("ls_average_edge_length", ls_meshgeom_workspace_bytes, F, V, ws_bytes))) return rc;
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    double* part = carve(workspace, F).part;
    const int G = F > 0 ? reduce_grid(F) : 0;
    if (G > 0)
        LS_IDX(idx_bytes, hipLaunchKernelGGL(k_edge_length_partials<IDX>, dim3(G), dim3(BLOCK), 0, st, verts, (const IDX*)faces, F, part));
    hipLaunchKernelGGL(k_edge_length_finish, dim3(1), dim3(MG_FIN), 0, st, (const double*)part, G, F, out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_average_edge_length_backward(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, const int32_t* vptr,
                                               const int32_t* cpos, const float* g_out, float* grad_verts, void* workspace, size_t ws_bytes,
                                               int device, void* stream) {
    int rc = check_mesh_args(verts, faces, idx_bytes, F, V, "ls_average_edge_length_backward");
    if (rc) return rc;
    LS_REQUIRE(g_out && grad_verts && vptr && workspace && (cpos || F == 0), LS_E_INVALID, "ls_average_edge_length_backward: null argument");
    if ((rc = require_workspace("ls_average_edge_length_backward", ls_meshgeom_workspace_bytes, F, V, ws_bytes))) return rc;
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    float* corner = carve(workspace, F).corner;
    if (F > 0)
        LS_IDX(idx_bytes, hipLaunchKernelGGL(k_edge_length_bwd<IDX>, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, verts, (const IDX*)faces, F,
                                             g_out, cpos, corner));
    gather_corners(vptr, corner, V, grad_verts, nullptr, st);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
