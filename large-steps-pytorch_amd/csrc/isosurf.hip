// isosurf.hip -- the level set of a scalar field on a regular grid as a triangle mesh, on the device (gfx950, wave64), and the gradient
// of its vertices in the field: largesteps/levelset.py, DESIGN.md section 2.13. tests/isosurf_statement.py restates the rule below in
// numpy; the device returns the statement's arrays bit for bit.
//
// The rule: marching tetrahedra on the Kuhn split. No 256-entry table, no ambiguous faces; the level set of the piecewise-linear
// interpolant on a conforming tet mesh is a closed, oriented 2-manifold wherever it does not leave the grid, in pairwise disjoint tets.
// Grid. S is (nx, ny, nz) fp32; node (i, j, k) lies at origin + spacing * (i, j, k) and has id (i ny + j) nz + k. A cube is the 8 nodes
// c + {0, 1}^3, c < (nx - 1, ny - 1, nz - 1), with id (i (ny - 1) + j) (nz - 1) + k; its corner (di, dj, dk) has number 4 di + 2 dj + dk.
// A grid with a side of 1 has no cubes and, by definition, no vertices either.
// Tets. Every cube splits into the 6 Kuhn tets v0 = c, v1 = c + e_a, v2 = c + e_a + e_b, v3 = c + (1, 1, 1), one per permutation
// (a, b, .) of the axes in lexicographic order; the split is the same in every cube, so the face diagonals of neighbours agree. A tet
// is positively oriented iff its permutation is even. Its edges (v0 v1, v0 v2, v0 v3, v1 v2, v1 v3, v2 v3) = 0..5 run from the lower
// corner to the higher along one of 7 directions, 100 010 001 110 011 101 111 = slots 0..6; the node an edge starts at OWNS it.
// Low, high, live. A node is low iff S < iso, else high (a NaN is high). An edge is live iff both ends are finite and exactly one is low.
// A cube with a non-finite corner emits nothing: all cubes around such a node go together, so no face names a vertex that is not there.
// Vertices. One per live edge, ordered by (owning node, slot): index = offs[node] + popcount(mask[node] & ((1 << slot) - 1)), mask the
// node's 7-bit live mask, offs the exclusive scan of the popcounts. No sort, no atomics. With a the owner and b = a + d, in fp32 without
// contraction: t = (iso - S[a]) / (S[b] - S[a]); t = t > 0 ? t : 0; t = t < 1 ? t : 1; x = origin_x + spacing_x * ((float)i_a + t * d_x).
// S[a] == iso gives t = 0: legal, with coincident vertices and zero-area faces at that node. E = 8 node + slot.
// Faces. Ordered by (cube, tet, triangle). The 4-bit case of a tet has bit i set iff v_i is low. For a positive tet, a lone low v_i gives
// the triangle (edge to o0, edge to o1, edge to o2) with (o0, o1, o2) = 123, 032, 013, 021 for i = 0..3, a lone high v_i the same with the
// last two swapped; low {a, b} with (a, b, c, d) an even permutation -- (c, d) = 23, 31, 12, 03, 20, 01 for {a, b} = 01, 02, 03, 12, 13, 23
// -- gives the quad (ac, ad, bd, bc), cut along ac - bd into (ac, ad, bd) and (ac, bd, bc). A negative tet swaps the last two corners of
// every triangle. Every normal then points from the low side to the high side. ISO_CASE below is this paragraph, packed.
// Gradient. gS = sum over vertices of <gV, dV / dS>, in fp64 from the fp32 inputs: per live edge D = S[b] - S[a], t = (iso - S[a]) / D (the
// term is zero unless 0 <= t <= 1), e = spacing * d, ge = (g_x e_x + g_y e_y) + g_z e_z, term_a = (-(1 - t) / D) * ge, term_b = (-t / D) * ge.
// One thread per node adds the term_a of its 7 owned slots in order, then the term_b of the 7 edges owned by node - d in slot order, in
// fp64, and rounds the sum to fp32 once: a gather, no float atomics, bitwise reproducible.
//
// One thread per node; the thread of a cube's corner 0 is the thread of the cube. The fastest axis of the grid is k and consecutive
// threads are consecutive k: the 8 corner loads of a wave are 8 contiguous rows, each re-read from the caches by the 7 neighbours that
// share it. Only threads next to the level set go on to the tables and to the offsets of their neighbours.
#include "common.h"
#include "workspace.h"
#include <cmath>

namespace ls {

// case -> bits 3 j .. 3 j + 2: the tet edge of triangle corner j (j = 0..5), bits 18..19: the number of triangles (positive tet)
__constant__ unsigned ISO_CASE[16] = {0u, 262280u, 262368u, 639761u, 262489u, 701634u, 577888u, 262498u,
                                      262442u, 676168u, 697987u, 262377u, 607001u, 262424u, 262224u, 0u};
// tet -> 6 bits per edge: the cube corner that owns it, its slot << 3
constexpr unsigned long long ISO_EDGE[6] = {24229643776ull, 14568065536ull, 24327685640ull, 3930785800ull, 14378535440ull, 3643213840ull};
// tet -> 3 bits per tet corner: its cube corner
constexpr unsigned ISO_CORNER[6] = {4000u, 3936u, 3984u, 3792u, 3912u, 3784u};
constexpr unsigned ISO_NEG = 38u;                              // the negative tets
constexpr int ISO_SLOT_CORNER[7] = {4, 2, 1, 6, 3, 5, 7};      // slot -> the cube corner its edge from corner 0 ends at

struct IsoGrid {
    int nx, ny, nz;
    int N, Nc;
    float iso;
};
struct Iso3 { float x, y, z; };

// the node of a thread: its coordinates and the field at the 8 corners of the cube that starts at it, NaN where the grid ends
struct IsoNode {
    int i, j, k;
    float s[8];
};
__device__ __forceinline__ IsoNode iso_load(const float* __restrict__ S, const IsoGrid& g, int node) {
    IsoNode c;
    const int row = node / g.nz;
    c.k = node - row * g.nz;
    c.i = row / g.ny;
    c.j = row - c.i * g.ny;
    const bool ii = c.i + 1 < g.nx, jj = c.j + 1 < g.ny, kk = c.k + 1 < g.nz;
    const float* __restrict__ p = S + node;
    const size_t sj = (size_t)g.nz, si = (size_t)g.ny * g.nz;
    const float nan = __builtin_nanf("");
    c.s[0] = p[0];
    c.s[1] = kk ? p[1] : nan;
    c.s[2] = jj ? p[sj] : nan;
    c.s[3] = jj && kk ? p[sj + 1] : nan;
    c.s[4] = ii ? p[si] : nan;
    c.s[5] = ii && kk ? p[si + 1] : nan;
    c.s[6] = ii && jj ? p[si + sj] : nan;
    c.s[7] = ii && jj && kk ? p[si + sj + 1] : nan;
    return c;
}
// bits 0..7: corner c is low; bits 8..15: corner c is finite
__device__ __forceinline__ unsigned iso_bits(const IsoNode& c, float iso) {
    unsigned b = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) b |= (c.s[q] < iso ? 1u << q : 0u) | (isfinite(c.s[q]) ? 256u << q : 0u);
    return b;
}
__device__ __forceinline__ unsigned iso_mask(unsigned bits, const IsoGrid& g) {
    unsigned m = 0;
    if (g.Nc == 0 || !(bits & 256u)) return 0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int q = ISO_SLOT_CORNER[s];
        if ((bits >> (8 + q) & 1u) && ((bits ^ bits >> q) & 1u)) m |= 1u << s;
    }
    return m;
}
__device__ __forceinline__ unsigned iso_case(unsigned bits, int t) {
    unsigned c = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) c |= (bits >> (ISO_CORNER[t] >> (3 * v) & 7u) & 1u) << v;
    return c;
}
__device__ __forceinline__ bool iso_has_cube(const IsoNode& c, const IsoGrid& g) { return c.i + 1 < g.nx && c.j + 1 < g.ny && c.k + 1 < g.nz; }
__device__ __forceinline__ int iso_cube_id(const IsoNode& c, const IsoGrid& g) { return (c.i * (g.ny - 1) + c.j) * (g.nz - 1) + c.k; }

// mask[node], ncnt[node] = its popcount, ccnt[cube] = the number of faces of the cube, 0..12
__global__ __launch_bounds__(BLOCK) void k_iso_classify(const float* __restrict__ S, const IsoGrid g, unsigned char* __restrict__ mask,
                                                        int* __restrict__ ncnt, int* __restrict__ ccnt) {
    const int node = blockIdx.x * BLOCK + threadIdx.x;
    if (node >= g.N) return;
    const IsoNode c = iso_load(S, g, node);
    const unsigned bits = iso_bits(c, g.iso);
    const unsigned m = iso_mask(bits, g);
    mask[node] = (unsigned char)m;
    ncnt[node] = __popc(m);
    if (!iso_has_cube(c, g)) return;
    int faces = 0;
    if ((bits >> 8) == 255u && (bits & 255u) != 0u && (bits & 255u) != 255u) {
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const int low = __popc(iso_case(bits, t));
            faces += low == 2 ? 2 : (low == 1 || low == 3) ? 1 : 0;
        }
    }
    ccnt[iso_cube_id(c, g)] = faces;
}

__global__ void k_iso_totals(const int* __restrict__ offs, const int* __restrict__ coffs, int N, int Nc, int64_t* __restrict__ totals) {
    totals[0] = offs[N];
    totals[1] = coffs[Nc];
}

// the vertices of the node's owned live edges and the faces of its cube, through the offsets; rows past n / m are dropped
__global__ __launch_bounds__(BLOCK) void k_iso_fill(const float* __restrict__ S, const IsoGrid g, const Iso3 origin, const Iso3 spacing,
                                                    const unsigned char* __restrict__ mask, const int* __restrict__ offs,
                                                    const int* __restrict__ coffs, int n, int m, float* __restrict__ V,
                                                    int64_t* __restrict__ E, int64_t* __restrict__ F) {
    const int node = blockIdx.x * BLOCK + threadIdx.x;
    if (node >= g.N) return;
    const IsoNode c = iso_load(S, g, node);
    const unsigned bits = iso_bits(c, g.iso);
    const unsigned live = iso_mask(bits, g);
    if (live && n > 0) {
        int idx = offs[node];
        const float fi = (float)c.i, fj = (float)c.j, fk = (float)c.k;
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            if (!(live >> s & 1u)) continue;
            if (idx < n) {
                const int q = ISO_SLOT_CORNER[s];
                float t = (g.iso - c.s[0]) / (c.s[q] - c.s[0]);
                t = t > 0.f ? t : 0.f;
                t = t < 1.f ? t : 1.f;
                V[3 * (size_t)idx] = origin.x + spacing.x * ((q & 4) ? fi + t : fi);
                V[3 * (size_t)idx + 1] = origin.y + spacing.y * ((q & 2) ? fj + t : fj);
                V[3 * (size_t)idx + 2] = origin.z + spacing.z * ((q & 1) ? fk + t : fk);
                if (E) E[idx] = 8 * (int64_t)node + s;
            }
            ++idx;
        }
    }
    if (m <= 0 || !iso_has_cube(c, g) || (bits >> 8) != 255u || (bits & 255u) == 0u || (bits & 255u) == 255u) return;
    int row = coffs[iso_cube_id(c, g)];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned cs = iso_case(bits, t);
        const unsigned tab = ISO_CASE[cs];
        const int nt = (int)(tab >> 18);
        for (int j = 0; j < nt; ++j, ++row) {
            if (row >= m) continue;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const int vv = (ISO_NEG >> t & 1u) && v ? 3 - v : v;
                const unsigned e = tab >> (3 * (3 * j + vv)) & 7u;
                const unsigned oc = (unsigned)(ISO_EDGE[t] >> (6 * e)) & 63u;
                const int nd = node + (int)((oc >> 2 & 1u) * g.ny + (oc >> 1 & 1u)) * g.nz + (int)(oc & 1u);
                F[3 * (size_t)row + v] = offs[nd] + __popc(mask[nd] & ((1u << (oc >> 3)) - 1u));
            }
        }
    }
}

// one term of the gradient: the edge a -> b in slot s whose vertex has the incoming gradient g; `to_b` picks term_b
__device__ __forceinline__ double iso_term(float sa, float sb, float iso, const Iso3& spacing, int s, const float* __restrict__ g, bool to_b) {
    const int q = ISO_SLOT_CORNER[s];
    const double ex = (q & 4) ? (double)spacing.x : 0.0, ey = (q & 2) ? (double)spacing.y : 0.0, ez = (q & 1) ? (double)spacing.z : 0.0;
    const double ge = ((double)g[0] * ex + (double)g[1] * ey) + (double)g[2] * ez;
    const double D = (double)sb - (double)sa;
    const double t = ((double)iso - (double)sa) / D;
    if (!(t >= 0.0 && t <= 1.0)) return 0.0;
    return to_b ? (-t / D) * ge : (-(1.0 - t) / D) * ge;
}
__global__ __launch_bounds__(BLOCK) void k_iso_backward(const float* __restrict__ S, const IsoGrid g, const Iso3 spacing,
                                                        const unsigned char* __restrict__ mask, const int* __restrict__ offs, int n,
                                                        const float* __restrict__ gV, float* __restrict__ gS) {
    const int node = blockIdx.x * BLOCK + threadIdx.x;
    if (node >= g.N) return;
    const int row = node / g.nz, k = node - row * g.nz, i = row / g.ny, j = row - i * g.ny;
    const float s0 = S[node];
    double acc = 0.0;
    const unsigned own = mask[node];
    if (own) {
        int idx = offs[node];
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            if (!(own >> s & 1u)) continue;
            if (idx < n) {
                const int q = ISO_SLOT_CORNER[s];
                const int b = node + ((q >> 2 & 1) * g.ny + (q >> 1 & 1)) * g.nz + (q & 1);
                acc += iso_term(s0, S[b], g.iso, spacing, s, gV + 3 * (size_t)idx, false);
            }
            ++idx;
        }
    }
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int q = ISO_SLOT_CORNER[s];
        if (i < (q >> 2 & 1) || j < (q >> 1 & 1) || k < (q & 1)) continue;
        const int a = node - (((q >> 2 & 1) * g.ny + (q >> 1 & 1)) * g.nz + (q & 1));
        const unsigned ma = mask[a];
        if (!(ma >> s & 1u)) continue;
        const int idx = offs[a] + __popc(ma & ((1u << s) - 1u));
        if (idx < n) acc += iso_term(S[a], s0, g.iso, spacing, s, gV + 3 * (size_t)idx, true);
    }
    gS[node] = (float)acc;
}

struct IsoWs {          // the regions of the workspace
    unsigned char* mask;
    int *ncnt, *offs, *ccnt, *coffs, *bsum;
    size_t total;
};
// ls_iso_fill and ls_iso_backward hold the workspace const: they carve it the same way and hand every region to their kernels as const
static inline IsoWs iso_carve(const void* ws, int64_t N, int64_t Nc) {
    WsWalk w(ws);
    unsigned char* mask = w.take<unsigned char>((size_t)N);
    int* ncnt = w.take<int>((size_t)N);
    int* offs = w.take<int>((size_t)(N + 1));
    int* ccnt = w.take<int>((size_t)(Nc > 0 ? Nc : 1));
    int* coffs = w.take<int>((size_t)(Nc + 1));
    int* bsum = w.take<int>((size_t)scan_scratch_ints(N));
    return {mask, ncnt, offs, ccnt, coffs, bsum, w.bytes()};
}
// LS_OK and the sizes, or the code of a grid that cannot be
static int iso_sizes(const char* who, int64_t nx, int64_t ny, int64_t nz, int64_t* N, int64_t* Nc) {
    LS_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, LS_E_INVALID, "%s: a side of the grid is below 1", who);
    const int64_t lim = (int64_t)1 << 28;            // 8 N < 2^31
    LS_REQUIRE(nx < lim && ny < lim && nz < lim && nx * ny < lim && nx * ny * nz < lim, LS_E_OVERFLOW,
               "%s: 8 x the number of nodes reaches 2^31", who);
    *N = nx * ny * nz;
    *Nc = (nx - 1) * (ny - 1) * (nz - 1);
    LS_REQUIRE(12 * *Nc < ((int64_t)1 << 31), LS_E_OVERFLOW, "%s: 12 x the number of cubes reaches 2^31", who);
    return LS_OK;
}
static bool iso_spacing_ok(const float* sp) {
    for (int a = 0; a < 3; ++a)
        if (!(std::isfinite(sp[a]) && sp[a] > 0.f)) return false;
    return true;
}

}  // namespace ls

using namespace ls;

extern "C" int ls_iso_workspace_bytes(int64_t nx, int64_t ny, int64_t nz, size_t* bytes) {
    LS_REQUIRE(bytes, LS_E_INVALID, "ls_iso_workspace_bytes: null argument");
    int64_t N, Nc;
    if (int rc = iso_sizes("ls_iso_workspace_bytes", nx, ny, nz, &N, &Nc)) return rc;
    *bytes = iso_carve(nullptr, N, Nc).total;
    return LS_OK;
}

extern "C" int ls_iso_count(const float* S, int64_t nx, int64_t ny, int64_t nz, float iso, void* ws, size_t ws_bytes, int64_t* totals,
                            int device, void* stream) {
    LS_REQUIRE(S && ws && totals, LS_E_INVALID, "ls_iso_count: null argument");
    int64_t N, Nc;
    if (int rc = iso_sizes("ls_iso_count", nx, ny, nz, &N, &Nc)) return rc;
    const IsoWs L = iso_carve(ws, N, Nc);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_iso_count: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    const IsoGrid g{(int)nx, (int)ny, (int)nz, (int)N, (int)Nc, iso};
    hipLaunchKernelGGL(k_iso_classify, dim3(div_up(N, BLOCK)), dim3(BLOCK), 0, st, S, g, L.mask, L.ncnt, L.ccnt);
    LS_HIP(hipGetLastError());
    if (int rc = exclusive_scan(L.ncnt, N, L.offs, L.bsum, st)) return rc;
    if (int rc = exclusive_scan(L.ccnt, Nc, L.coffs, L.bsum, st)) return rc;
    hipLaunchKernelGGL(k_iso_totals, dim3(1), dim3(1), 0, st, (const int*)L.offs, (const int*)L.coffs, (int)N, (int)Nc, totals);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_iso_fill(const float* S, int64_t nx, int64_t ny, int64_t nz, float iso, const float* origin, const float* spacing,
                           const void* ws, size_t ws_bytes, int64_t n, int64_t m, float* V, int64_t* E, int64_t* F, int device,
                           void* stream) {
    LS_REQUIRE(S && ws && origin && spacing && n >= 0 && m >= 0 && (n == 0 || V) && (m == 0 || F), LS_E_INVALID, "ls_iso_fill: bad argument");
    LS_REQUIRE(iso_spacing_ok(spacing), LS_E_INVALID, "ls_iso_fill: the spacing must be positive and finite");
    int64_t N, Nc;
    if (int rc = iso_sizes("ls_iso_fill", nx, ny, nz, &N, &Nc)) return rc;
    LS_REQUIRE(n < ((int64_t)1 << 31) && m < ((int64_t)1 << 31), LS_E_OVERFLOW, "ls_iso_fill: 2^31 rows or more");
    const IsoWs L = iso_carve(ws, N, Nc);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_iso_fill: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    if (n == 0 && m == 0) return LS_OK;
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const IsoGrid g{(int)nx, (int)ny, (int)nz, (int)N, (int)Nc, iso};
    hipLaunchKernelGGL(k_iso_fill, dim3(div_up(N, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, S, g, Iso3{origin[0], origin[1], origin[2]},
                       Iso3{spacing[0], spacing[1], spacing[2]}, (const unsigned char*)L.mask, (const int*)L.offs,
                       (const int*)L.coffs, (int)n, (int)m, V, E, F);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_iso_backward(const float* S, int64_t nx, int64_t ny, int64_t nz, float iso, const float* origin, const float* spacing,
                               const void* ws, size_t ws_bytes, int64_t n, const float* gV, float* gS, int device, void* stream) {
    LS_REQUIRE(S && ws && origin && spacing && gS && n >= 0 && (n == 0 || gV), LS_E_INVALID, "ls_iso_backward: bad argument");
    LS_REQUIRE(iso_spacing_ok(spacing), LS_E_INVALID, "ls_iso_backward: the spacing must be positive and finite");
    int64_t N, Nc;
    if (int rc = iso_sizes("ls_iso_backward", nx, ny, nz, &N, &Nc)) return rc;
    LS_REQUIRE(n < ((int64_t)1 << 31), LS_E_OVERFLOW, "ls_iso_backward: 2^31 rows or more");
    const IsoWs L = iso_carve(ws, N, Nc);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_iso_backward: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        LS_HIP(hipMemsetAsync(gS, 0, sizeof(float) * (size_t)N, st));
        return LS_OK;
    }
    const IsoGrid g{(int)nx, (int)ny, (int)nz, (int)N, (int)Nc, iso};
    hipLaunchKernelGGL(k_iso_backward, dim3(div_up(N, BLOCK)), dim3(BLOCK), 0, st, S, g, Iso3{spacing[0], spacing[1], spacing[2]},
                       (const unsigned char*)L.mask, (const int*)L.offs, (int)n, gV, gS);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
