// selfx.hip -- the self-intersections of the mesh of a mesh-distance handle (meshbvh.h) on the device (gfx950, wave64): which pairs of
// faces cut through each other -- libigl's fast_find_self_intersections (largesteps/distance.py).
// tests/selfx_statement.py restates the rule below as a brute force over all pairs; the device answers with the same pairs.
//
// The rule. All arithmetic is fp64 from the fp32 coordinates, no FMA contraction (-ffp-contract=off).
// Segment against face. The segment (p, q) crosses the face (a, b, c) iff the ray rule of raycast.hip, with the origin o = p and the
// direction d = q - p formed in fp64 (not rounded to fp32), accepts the face with 0 <= t <= 1: the same axis choice kz (largest |d|, the
// lowest on a tie), kx, ky (swapped when d[kz] < 0), shear Sx, Sy, Sz, edge functions U, V, W, det = (U + V) + W and
// t = ((U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz])) / det, in the same operation order. Edges and vertices count; det == 0 never hits (a
// zero-area face, a segment in the face's plane); a d that is all zero or has a non-finite component hits nothing.
// Face pairs. For faces f < g let s be the number of equal (corner of f, corner of g) index pairs among the nine -- for faces without a
// repeated index, the number of vertex indices they share. Edge e of a face is (corner e, corner (e + 1) % 3), in that direction.
//   s >= 2 (edge neighbours, duplicates): never reported.
//   s == 1, corner i of f being corner j of g: reported iff the edge of f opposite corner i (edge (i + 1) % 3) crosses g, or the edge of
//           g opposite corner j crosses f.
//   s == 0: reported iff one of the three edges of f crosses g, or one of the three edges of g crosses f.
// The box clause. A pair is reported only if the corner boxes of f and g are within 2 e of each other on all three axes: the box of a
// face is the fminf / fmaxf of its three fp32 corners (the leaf boxes of the handle's LBVH, margin 0), e = the handle's slack, 2^-40 x
// the largest |coordinate| of the vertices (a NaN passed over). On an axis the boxes are apart iff lo_g - e > hi_f + e or hi_g + e < lo_f - e, each side
// rounded once in fp64; a comparison with a NaN is false, so such a pair is not apart. The clause is symmetric in f and g. It is part of
// the rule, not a shortcut of the walk: where the pair rule accepts with numbers that mean something, the segment passes within a few
// fp64 roundings of the face, far inside e; but on an exactly flat sheet whose shear rounds it accepts on rounding alone (U = W = 0,
// det = V = a rounding error, t in [0, 1]) for faces any distance apart in the sheet's plane, and the clause is what leaves those out.
// Coplanar overlaps are therefore not reported; two faces without a common index that touch at a point or along a segment are.
//
// The walk. One thread per LEAF of the LBVH: thread i takes face f = tri[i], so that the faces of a wave are neighbours in space and
// walk the same nodes. It holds the fp32 box of its three corners and goes through the pre-order by the escape links (no stack, no
// LDS, no scratch). A node is skipped exactly when its box and the face's are apart by the comparisons of the box clause. At a leaf that
// is the clause itself, the leaf's box being the corner box of its face; above the leaves it skips no pair the clause keeps: a node's
// box is the fminf / fmaxf of its leaves' boxes, and x -> x - e, x -> x + e are monotone under rounding, so a node apart from the face
// has every leaf apart from it. The pairs that are tested are therefore those of the clause, whatever the hierarchy. At a leaf g the
// pair is tested only when g > f: each pair once, by the thread of its lower face.
// sx_cross below repeats rc_ray and rc_face of raycast.hip for a fp64 direction (those take the fp32 ray of the ABI and keep what a
// closest-hit walk needs besides); tests/selfx_statement.py and tests/ray_statement.py hold the two to the same operations.
//
// Two passes. Count: counts[f] = the number of reported pairs (f, g), g > f; total = their sum (integer atomics, one per wave: exact in
// any order); flags[f] = flags[g] = 1 on request. Fill: the exclusive scan of the counts gives face f its segment, the walk is repeated
// and writes (f, g) there (a write past the segment's end or past k is dropped), and the stable radix sort of radix.h orders the pairs
// by the two-word key (f, g): the output is sorted lexicographically and depends on the mesh alone, not on the hierarchy.
#include "common.h"
#include "lbvh.h"
#include "meshbvh.h"
#include "radix.h"
#include <algorithm>
#include <cmath>

namespace ls {

// a face in registers: the corners widened to fp64 and their vertex indices
struct SxFace {
    double ax, ay, az, bx, by, bz, cx, cy, cz;
    int i0, i1, i2;
};
__device__ __forceinline__ SxFace sx_load(const MeshView& m, int f) {
    SxFace t;
    t.i0 = m.faces[3 * (size_t)f]; t.i1 = m.faces[3 * (size_t)f + 1]; t.i2 = m.faces[3 * (size_t)f + 2];
    const float* __restrict__ a = m.P + 3 * (size_t)t.i0;
    const float* __restrict__ b = m.P + 3 * (size_t)t.i1;
    const float* __restrict__ c = m.P + 3 * (size_t)t.i2;
    t.ax = a[0]; t.ay = a[1]; t.az = a[2];
    t.bx = b[0]; t.by = b[1]; t.bz = b[2];
    t.cx = c[0]; t.cy = c[1]; t.cz = c[2];
    return t;
}
__device__ __forceinline__ double sx_sel(int k, double x, double y, double z) { return k == 0 ? x : k == 1 ? y : z; }

// the segment (p, q) against the face t: rc_ray and rc_face of raycast.hip with o = p, d = q - p, accepted iff 0 <= t <= 1
__device__ __forceinline__ bool sx_cross(double px, double py, double pz, double qx, double qy, double qz, const SxFace& t) {
    const double d0 = qx - px, d1 = qy - py, d2 = qz - pz;
    const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
    if (!(isfinite(d0) && isfinite(d1) && isfinite(d2) && (a0 > 0.0 || a1 > 0.0 || a2 > 0.0))) return false;
    const int kz = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
    const double dz = sx_sel(kz, d0, d1, d2);
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    if (dz < 0.0) { const int s = kx; kx = ky; ky = s; }
    const double Sx = sx_sel(kx, d0, d1, d2) / dz, Sy = sx_sel(ky, d0, d1, d2) / dz, Sz = 1.0 / dz;
    const double ox = sx_sel(kx, px, py, pz), oy = sx_sel(ky, px, py, pz), oz = sx_sel(kz, px, py, pz);
    const double Akx = sx_sel(kx, t.ax, t.ay, t.az) - ox, Aky = sx_sel(ky, t.ax, t.ay, t.az) - oy, Akz = sx_sel(kz, t.ax, t.ay, t.az) - oz;
    const double Bkx = sx_sel(kx, t.bx, t.by, t.bz) - ox, Bky = sx_sel(ky, t.bx, t.by, t.bz) - oy, Bkz = sx_sel(kz, t.bx, t.by, t.bz) - oz;
    const double Ckx = sx_sel(kx, t.cx, t.cy, t.cz) - ox, Cky = sx_sel(ky, t.cx, t.cy, t.cz) - oy, Ckz = sx_sel(kz, t.cx, t.cy, t.cz) - oz;
    const double Ax = Akx - Sx * Akz, Ay = Aky - Sy * Akz;
    const double Bx = Bkx - Sx * Bkz, By = Bky - Sy * Bkz;
    const double Cx = Ckx - Sx * Ckz, Cy = Cky - Sy * Ckz;
    const double U = Cx * By - Cy * Bx;
    const double V = Ax * Cy - Ay * Cx;
    const double W = Bx * Ay - By * Ax;
    const double det = (U + V) + W;
    if (!(((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0)) && det != 0.0)) return false;
    const double tt = ((U * (Sz * Akz) + V * (Sz * Bkz)) + W * (Sz * Ckz)) / det;
    return tt >= 0.0 && tt <= 1.0;
}
// edge e of face s (corner e to corner (e + 1) % 3) against face t; e is a constant at every call
__device__ __forceinline__ bool sx_edge(const SxFace& s, int e, const SxFace& t) {
    return e == 0 ? sx_cross(s.ax, s.ay, s.az, s.bx, s.by, s.bz, t)
         : e == 1 ? sx_cross(s.bx, s.by, s.bz, s.cx, s.cy, s.cz, t)
                  : sx_cross(s.cx, s.cy, s.cz, s.ax, s.ay, s.az, t);
}
// the pair rule: which of the six edge tests the shared indices leave (bits 0..2: the edges of f against g, 3..5: those of g against
// f), then the tests until one accepts
__device__ __forceinline__ bool sx_pair(const SxFace& f, const SxFace& g) {
    const bool m00 = f.i0 == g.i0, m01 = f.i0 == g.i1, m02 = f.i0 == g.i2;
    const bool m10 = f.i1 == g.i0, m11 = f.i1 == g.i1, m12 = f.i1 == g.i2;
    const bool m20 = f.i2 == g.i0, m21 = f.i2 == g.i1, m22 = f.i2 == g.i2;
    const int s = ((m00 + m01 + m02) + (m10 + m11 + m12)) + (m20 + m21 + m22);
    if (s >= 2) return false;
    unsigned mask = 0x3fu;
    if (s == 1) {
        const int i = (m00 || m01 || m02) ? 0 : (m10 || m11 || m12) ? 1 : 2;      // the shared corner of f and of g
        const int j = (m00 || m10 || m20) ? 0 : (m01 || m11 || m21) ? 1 : 2;
        mask = (1u << (i == 2 ? 0 : i + 1)) | (8u << (j == 2 ? 0 : j + 1));       // the edges opposite them
    }
    if ((mask & 1u) && sx_edge(f, 0, g)) return true;
    if ((mask & 2u) && sx_edge(f, 1, g)) return true;
    if ((mask & 4u) && sx_edge(f, 2, g)) return true;
    if ((mask & 8u) && sx_edge(g, 0, f)) return true;
    if ((mask & 16u) && sx_edge(g, 1, f)) return true;
    if ((mask & 32u) && sx_edge(g, 2, f)) return true;
    return false;
}

// The walk of leaf i = blockIdx.x * BLOCK + threadIdx.x. FILL = false: counts[f], total, flags (or null). FILL = true: the pairs of f
// into pf / pg at off[f] .. min(off[f + 1], k), anything past that dropped.
template <bool FILL>
__device__ __forceinline__ void sx_walk(const MeshView& m, int* __restrict__ counts, unsigned long long* __restrict__ total,
                                        unsigned char* __restrict__ flags, const int* __restrict__ off, int k, int* __restrict__ pf,
                                        int* __restrict__ pg) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    int cnt = 0;
    if (i < m.T) {
        const int* __restrict__ left = m.left;
        const int* __restrict__ esc = m.esc;
        const float* __restrict__ box = m.box;
        const int leaf0 = m.T - 1;
        const int f = m.tri[i];
        const SxFace ff = sx_load(m, f);
        const double e = m.slack;
        // the face's box widened by e on every side
        const double lx = fmin(fmin(ff.ax, ff.bx), ff.cx) - e, ly = fmin(fmin(ff.ay, ff.by), ff.cy) - e, lz = fmin(fmin(ff.az, ff.bz), ff.cz) - e;
        const double hx = fmax(fmax(ff.ax, ff.bx), ff.cx) + e, hy = fmax(fmax(ff.ay, ff.by), ff.cy) + e, hz = fmax(fmax(ff.az, ff.bz), ff.cz) + e;
        int pos = 0, end = 0;
        if (FILL) { pos = off[f]; end = min(off[f + 1], k); }
        int node = 0;
        while (node >= 0) {
            const float* bx = box + 6 * (size_t)node;
            if ((double)bx[0] - e > hx || (double)bx[1] - e > hy || (double)bx[2] - e > hz || (double)bx[3] + e < lx || (double)bx[4] + e < ly ||
                (double)bx[5] + e < lz) {
                node = esc[node];
                continue;
            }
            if (node < leaf0) { node = left[node]; continue; }
            const int g = m.tri[node - leaf0];
            if (g > f && sx_pair(ff, sx_load(m, g))) {
                if (FILL) {
                    if (pos >= 0 && pos < end) { pf[pos] = f; pg[pos] = g; }
                    ++pos;
                } else {
                    ++cnt;
                    if (flags) { flags[f] = 1; flags[g] = 1; }
                }
            }
            node = esc[node];
        }
        if (!FILL) counts[f] = cnt;
    }
    if (!FILL) {
#pragma unroll
        for (int s = WAVE / 2; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s, WAVE);
        if ((threadIdx.x & (WAVE - 1)) == 0 && cnt) atomicAdd(total, (unsigned long long)cnt);
    }
}
__global__ __launch_bounds__(BLOCK) void k_selfx_count(const MeshView m, int* __restrict__ counts, unsigned long long* __restrict__ total,
                                                       unsigned char* __restrict__ flags) {
    sx_walk<false>(m, counts, total, flags, nullptr, 0, nullptr, nullptr);
}
__global__ __launch_bounds__(BLOCK) void k_selfx_fill(const MeshView m, const int* __restrict__ off, int k, int* __restrict__ pf, int* __restrict__ pg) {
    sx_walk<true>(m, nullptr, nullptr, nullptr, off, k, pf, pg);
}

// the sort key of pair `row`: two words, g the less significant
struct KeyPair {
    const int* pf;
    const int* pg;
    __device__ __forceinline__ unsigned word(int row, int w) const { return (unsigned)(w == 0 ? pg[row] : pf[row]); }
};
// pairs[j] = (f, g) of the j-th pair in sorted order
__global__ __launch_bounds__(BLOCK) void k_selfx_emit(const int* __restrict__ order, const int* __restrict__ pf, const int* __restrict__ pg, int k,
                                                      int64_t* __restrict__ pairs) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= k) return;
    const int r = order[j];
    pairs[2 * (size_t)j] = pf[r];
    pairs[2 * (size_t)j + 1] = pg[r];
}

struct SxWs {          // the regions of the fill pass's workspace
    int *off, *pf, *pg, *order;
    SortScratch sort;
    size_t total;
};
static inline SxWs sx_carve(void* ws, int64_t F, int64_t k) {
    const int64_t m = std::max<int64_t>(k, 1);
    WsWalk w(ws);
    int* off = w.take<int>((size_t)(F + 1));
    int *pf = w.take<int>((size_t)m), *pg = w.take<int>((size_t)m), *order = w.take<int>((size_t)m);
    const SortScratch sort = sort_scratch_take(w, m, true, F);       // its bsum also serves the scan of the F counts
    return {off, pf, pg, order, sort, w.bytes()};
}

}  // namespace ls

using namespace ls;

extern "C" int ls_mesh_selfx_count(void* handle, int32_t* counts, int64_t* total, unsigned char* flags, void* stream) {
    LS_REQUIRE(handle && counts && total, LS_E_INVALID, "ls_mesh_selfx_count: null argument");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    const hipStream_t st = (hipStream_t)stream;
    LS_HIP(hipMemsetAsync(total, 0, sizeof(int64_t), st));
    if (flags) LS_HIP(hipMemsetAsync(flags, 0, (size_t)H->T, st));
    hipLaunchKernelGGL(k_selfx_count, dim3(div_up(H->T, BLOCK)), dim3(BLOCK), 0, st, H->view(), counts, (unsigned long long*)total, flags);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_selfx_workspace_bytes(int64_t F, int64_t k, size_t* bytes) {
    LS_REQUIRE(bytes && F > 0 && k >= 0, LS_E_INVALID, "ls_mesh_selfx_workspace_bytes: bad argument");
    LS_REQUIRE(3 * F < INT32_MAX && 2 * k < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_selfx_workspace_bytes: more than 2^31 corners or pair entries");
    *bytes = sx_carve(nullptr, F, k).total;
    return LS_OK;
}

extern "C" int ls_mesh_selfx_pairs(void* handle, const int32_t* counts, int64_t k, int64_t* pairs, void* ws, size_t ws_bytes, void* stream) {
    LS_REQUIRE(handle && k >= 0 && (k == 0 || (counts && pairs && ws)), LS_E_INVALID, "ls_mesh_selfx_pairs: bad argument");
    LS_REQUIRE(2 * k < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_selfx_pairs: more than 2^31 pair entries");
    if (k == 0) return LS_OK;
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    const int64_t F = H->T;
    const SxWs w = sx_carve(ws, F, k);
    LS_REQUIRE(ws_bytes >= w.total, LS_E_WORKSPACE, "ls_mesh_selfx_pairs: workspace too small (%zu < %zu bytes)", ws_bytes, w.total);
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = exclusive_scan(counts, F, w.off, w.sort.bsum, st)) return rc;
    // pf and pg are adjacent: one memset up to order. Counts that are not this mesh's leave zeros, never stale memory
    LS_HIP(hipMemsetAsync(w.pf, 0, (size_t)((char*)w.order - (char*)w.pf), st));
    hipLaunchKernelGGL(k_selfx_fill, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, H->view(), (const int*)w.off, (int)k, w.pf, w.pg);
    LS_HIP(hipGetLastError());
    const int* sorted = nullptr;
    // f takes radix_passes(F - 1) bytes, g all four: radix_argsort_words shortens its last word only
    if (int rc = radix_argsort_words(KeyPair{w.pf, w.pg}, k, 2, w.order, w.sort, st, &sorted, radix_passes(F - 1))) return rc;
    hipLaunchKernelGGL(k_selfx_emit, dim3(div_up(k, BLOCK)), dim3(BLOCK), 0, st, sorted, (const int*)w.pf, (const int*)w.pg, (int)k, pairs);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
