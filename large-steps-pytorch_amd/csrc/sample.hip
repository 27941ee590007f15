// sample.hip -- area-weighted points on a mesh surface and their gradient to the vertices (gfx950, wave64): what turns the point-to-mesh
// distance of distance.hip into a mesh-to-mesh measure (largesteps/sampling.py). The rule is stated here and in
// the module's docstring and restated in numpy by tests/sample_statement.py; the device answers with the same bits.
//
// Weights, recomputed on every call (they depend on V). With the fp32 corners a, b, c of a face widened to fp64, u = b - a, v = c - a,
// x = u x v (each component one product minus the other), area = 0.5 sqrt((x0 x0 + x1 x1) + x2 x2), contraction off. A face whose area
// is not finite or not positive, or which names a vertex outside [0, V), has weight 0. amax = the largest area (a max: any reduction
// tree gives it; here an integer atomicMax on the bits, whose order is the value order of non-negative doubles),
// q_f = (uint64) floor((area_f / amax) * 2^32), cumq = the inclusive uint64 prefix sum of q (integers: any association gives it),
// Q = cumq[F - 1]. A face smaller than amax 2^-32 is never drawn.
// Sample i (its index counts from the call's `offset`): Philox4x32-10 of the counter (i_lo, i_hi, stream, 0) under the key
// (seed_lo, seed_hi) gives x0 .. x3. r = x0 2^32 + x1, T = (r Q) >> 64, I_i = the first f with cumq[f] > T. u1 = (x2 + 0.5) 2^-32,
// u2 = (x3 + 0.5) 2^-32, s = sqrt(u1) (correctly rounded), w = (1 - s, s (1 - u2), s u2) in fp64, W_i = fp32(w),
// P_i = fp32((W0 a + W1 b) + W2 c) per coordinate in fp64 from the ROUNDED weights. Q == 0 (no face can be drawn, or F == 0): P = NaN,
// I = -1, W = 0, without a host check.
//
// Launches of the forward: memset of two scalars, k_sp_area, k_sp_quant, k_sp_scan_tiles, k_sp_scan, k_sp_sample -- no allocation, no
// host synchronisation (DESIGN.md section 2.9 has the byte model). The scan is the 64-bit one of this file: tiles of SP_TILE = LS_SAMPLE_SCAN_TILE faces (256 threads x 8), one
// sum per tile, the tile sums scanned by one workgroup (a contiguous span per thread), then every tile scanned with its offset.
//
// Gradient: gV[v] = sum_i W_ik gP_i over the samples whose face has v at corner k; I and W are held fixed. No float atomics: the samples
// are grouped by face (groupby.h: stable, so ascending i within a face), nine fp64 sums per face are formed in that order (a thread up
// to 64 samples, else the wave lane-strided and an xor butterfly: groupby.h's seg_sum with an fp64 accumulator), and a thread per vertex
// adds the rows of its corners in the rank order of meshface.h in fp64 and rounds ONCE to fp32 -- md_vertex_grad of meshbvh.h, the tail
// of the distance's and the rays' gradients, with fp64 rows. Every product W_ik gP_i is exact in fp64. Bitwise reproducible.
#include "common.h"
#include "groupby.h"
#include "meshbvh.h"
#include "meshface.h"
#include <algorithm>
#include <cmath>

namespace ls {

typedef unsigned long long u64;
constexpr int SP_ITEMS = 8, SP_TILE = BLOCK * SP_ITEMS;
static_assert(SP_TILE == LS_SAMPLE_SCAN_TILE, "the header states the scan's tile");

__device__ __forceinline__ u64 sp_wave_max(u64 x) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) { const u64 y = __shfl_down(x, off, WAVE); x = y > x ? y : x; }
    return x;       // valid in lane 0
}

// area[f] (the bits of a double; 0 for a face of weight 0) and the largest of them in amax[0] (zero before the launch). The grid loops
// (reduce_grid) and every workgroup ends with ONE atomic: one per wave of a thread-per-face grid, 31 000 on a 2M-face mesh, all to one
// address, took 0.37 ms there.
template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_sp_area(const float* __restrict__ verts, const IDX* __restrict__ faces, int64_t F, int64_t V,
                                                   u64* __restrict__ area, u64* __restrict__ amax) {
    __shared__ u64 sm[BLOCK / WAVE];
    u64 best = 0;
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < F; f += (int64_t)gridDim.x * BLOCK) {
        double ar = 0.0;
        int64_t id[3];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) { id[c] = (int64_t)faces[f * 3 + c]; ok = ok && id[c] >= 0 && id[c] < V; }
        if (ok) {
            double p[3][3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int q = 0; q < 3; ++q) p[c][q] = (double)verts[(size_t)id[c] * 3 + q];
            const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const double v[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const double x0 = u[1] * v[2] - u[2] * v[1], x1 = u[2] * v[0] - u[0] * v[2], x2 = u[0] * v[1] - u[1] * v[0];
            ar = 0.5 * sqrt((x0 * x0 + x1 * x1) + x2 * x2);
            if (!(ar > 0.0) || !isfinite(ar)) ar = 0.0;
        }
        const u64 b = (u64)__double_as_longlong(ar);
        area[f] = b;
        best = b > best ? b : best;
    }
    best = sp_wave_max(best);
    if ((threadIdx.x & (WAVE - 1)) == 0) sm[threadIdx.x / WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 1; j < BLOCK / WAVE; ++j) best = sm[j] > best ? sm[j] : best;
        if (best) atomicMax(amax, best);
    }
}

// Inclusive scan of one value per thread over the workgroup; total: the sum of all. sm: BLOCK / WAVE words.
__device__ __forceinline__ u64 sp_block_scan(u64 x, u64* sm, u64& total) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const u64 y = __shfl_up(x, off, WAVE);
        if (lane >= off) x += y;
    }
    if (lane == WAVE - 1) sm[w] = x;
    __syncthreads();
    u64 before = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < BLOCK / WAVE; ++j) {
        const u64 s = sm[j];
        if (j < w) before += s;
        total += s;
    }
    __syncthreads();
    return x + before;
}

// q[f] in place of area[f], and the sum of the tile's q in tsum[tile]
__global__ __launch_bounds__(BLOCK) void k_sp_quant(u64* __restrict__ aq, int64_t F, const u64* __restrict__ amax, u64* __restrict__ tsum) {
    __shared__ u64 sm[BLOCK / WAVE];
    const double am = __longlong_as_double((long long)amax[0]);
    const int64_t base = (int64_t)blockIdx.x * SP_TILE + (int64_t)threadIdx.x * SP_ITEMS;
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < SP_ITEMS; ++j) {
        const int64_t f = base + j;
        if (f < F) {
            const double a = __longlong_as_double((long long)aq[f]);
            const u64 q = (a > 0.0) ? (u64)floor((a / am) * 4294967296.0) : 0ull;       // a > 0 implies am >= a > 0
            aq[f] = q;
            s += q;
        }
    }
    u64 total;
    sp_block_scan(s, sm, total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// tsum[0 .. nt) -> its exclusive scan, in place; tsum[nt] = Q[0] = the total. One workgroup; thread t owns the contiguous span t.
__global__ __launch_bounds__(BLOCK) void k_sp_scan_tiles(u64* __restrict__ tsum, int64_t nt, u64* __restrict__ Q) {
    __shared__ u64 sm[BLOCK / WAVE];
    const int64_t span = (nt + BLOCK - 1) / BLOCK;
    const int64_t lo = threadIdx.x * span < nt ? threadIdx.x * span : nt, hi = lo + span < nt ? lo + span : nt;
    u64 s = 0;
    for (int64_t j = lo; j < hi; ++j) s += tsum[j];
    u64 total;
    u64 run = sp_block_scan(s, sm, total) - s;
    for (int64_t j = lo; j < hi; ++j) { const u64 t = tsum[j]; tsum[j] = run; run += t; }
    if (threadIdx.x == 0) { Q[0] = total; tsum[nt] = total; }
}

// q -> cumq in place, a tile per workgroup; and the two coarser levels of the search: lev1[j] = cumq[min(16 j + 15, F - 1)],
// lev2[j] = cumq[min(256 j + 255, F - 1)] (the level above them, one entry per tile, is tsum[t + 1])
constexpr int SP_FAN1 = 16, SP_FAN2 = 256;
static_assert(SP_FAN1 % SP_ITEMS == 0 && SP_FAN2 % SP_FAN1 == 0 && SP_TILE % SP_FAN2 == 0, "a coarse entry is some thread's last item");
__global__ __launch_bounds__(BLOCK) void k_sp_scan(u64* __restrict__ aq, int64_t F, const u64* __restrict__ tsum, u64* __restrict__ lev1,
                                                   u64* __restrict__ lev2) {
    __shared__ u64 sm[BLOCK / WAVE];
    const int64_t base = (int64_t)blockIdx.x * SP_TILE + (int64_t)threadIdx.x * SP_ITEMS;
    u64 v[SP_ITEMS];
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < SP_ITEMS; ++j) {
        v[j] = (base + j < F) ? aq[base + j] : 0ull;
        s += v[j];
        v[j] = s;
    }
    u64 total;
    const u64 before = sp_block_scan(s, sm, total) - s + tsum[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SP_ITEMS; ++j) {
        const int64_t f = base + j;
        if (f < F) {
            const u64 c = v[j] + before;
            aq[f] = c;
            if (f % SP_FAN1 == SP_FAN1 - 1 || f == F - 1) lev1[f / SP_FAN1] = c;
            if (f % SP_FAN2 == SP_FAN2 - 1 || f == F - 1) lev2[f / SP_FAN2] = c;
        }
    }
}

// the first j in [lo, hi] with a[j] > T; the caller knows that a[hi] > T
__device__ __forceinline__ int64_t sp_first_above(const u64* __restrict__ a, int64_t lo, int64_t hi, u64 T) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] > T) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// A thread per sample: the rule of the header comment. The first f with cumq[f] > T is found level by level -- the tile (tsum: one
// entry per SP_TILE faces, a dense array that stays in cache), then the 256 faces, the 16 faces and the face, each step a search in at
// most 16 neighbouring words (one or two cache lines): three lines fetched per sample where a plain binary search over cumq touches
// about log2 F - 4 (17 on a 2M-face mesh). Every level holds cumq at the END of its group, so "first entry above T" at one level
// names the group of the next, and the last group of a level is clamped to the level's size.
template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_sp_sample(const float* __restrict__ verts, const IDX* __restrict__ faces, int64_t F,
                                                     const u64* __restrict__ cumq, const u64* __restrict__ lev1, const u64* __restrict__ lev2,
                                                     const u64* __restrict__ tsum, const u64* __restrict__ Qp, int64_t n, u64 first, u64 seed,
                                                     unsigned stream_id, float* __restrict__ P, int64_t* __restrict__ I, float* __restrict__ W) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64 Q = Qp[0];
    if (Q == 0) {
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int q = 0; q < 3; ++q) { P[3 * i + q] = nan; W[3 * i + q] = 0.0f; }
        I[i] = -1;
        return;
    }
    const u64 idx = first + (u64)i;
    unsigned x[4] = {(unsigned)idx, (unsigned)(idx >> 32), stream_id, 0u};
    philox4x32_10(x, (unsigned)seed, (unsigned)(seed >> 32));
    const u64 T = __umul64hi(((u64)x[0] << 32) | x[1], Q);          // T < Q = cumq[F - 1]: the search below ends on a face with q > 0
    const int64_t n1 = (F + SP_FAN1 - 1) / SP_FAN1, n2 = (F + SP_FAN2 - 1) / SP_FAN2, nt = (F + SP_TILE - 1) / SP_TILE;
    const int64_t t = sp_first_above(tsum + 1, 0, nt - 1, T);
    int64_t g = t * (SP_TILE / SP_FAN2);
    g = sp_first_above(lev2, g, min(g + SP_TILE / SP_FAN2, n2) - 1, T) * (SP_FAN2 / SP_FAN1);
    g = sp_first_above(lev1, g, min(g + SP_FAN2 / SP_FAN1, n1) - 1, T) * SP_FAN1;
    const int64_t lo = sp_first_above(cumq, g, min(g + SP_FAN1, F) - 1, T);
    const double u1 = ((double)x[2] + 0.5) * 0x1p-32, u2 = ((double)x[3] + 0.5) * 0x1p-32;
    const double s = sqrt(u1);
    const float w[3] = {(float)(1.0 - s), (float)(s * (1.0 - u2)), (float)(s * u2)};
    double p[3][3];                 // a face with q > 0 passed the index check of k_sp_area
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t v = (size_t)faces[lo * 3 + c];
#pragma unroll
        for (int q = 0; q < 3; ++q) p[c][q] = (double)verts[v * 3 + q];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        P[3 * i + q] = (float)(((double)w[0] * p[0][q] + (double)w[1] * p[1][q]) + (double)w[2] * p[2][q]);
        W[3 * i + q] = w[q];
    }
    I[i] = lo;
}

// ---- gradient ----------------------------------------------------------------------------------------------------------------------
// rows[f][3 k + q] = sum over the samples of face f, in sorted order, of W_ik gP_iq: the G of seg_sum, in fp64
struct SpRows {
    const float* __restrict__ W; const float* __restrict__ gP; const int* __restrict__ order; const int* __restrict__ seg; double* __restrict__ rows;
    __device__ __forceinline__ int count(int64_t key) const { return seg[key + 1] - seg[key]; }
    // adds the samples start, start + step, ... of face `key` to acc, in order
    __device__ __forceinline__ void walk(int64_t key, int start, int step, double (&acc)[9]) const {
        const int e = seg[key + 1];
        for (int j = seg[key] + start; j < e; j += step) {
            const size_t i = (size_t)order[j];
            const double g[3] = {(double)gP[3 * i], (double)gP[3 * i + 1], (double)gP[3 * i + 2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double w = (double)W[3 * i + k];
#pragma unroll
                for (int q = 0; q < 3; ++q) acc[3 * k + q] += w * g[q];
            }
        }
    }
    __device__ __forceinline__ void store(int64_t key, const double (&acc)[9]) const {
#pragma unroll
        for (int q = 0; q < 9; ++q) rows[key * 9 + q] = acc[q];
    }
};

}  // namespace ls

using namespace ls;

namespace {
struct SpWs {          // the workspace: the forward's and the backward's regions both start at the base (a call is one or the other)
    u64 *scal, *cumq, *lev1, *lev2, *tsum;              // forward: [0] amax bits, [1] Q; F, F / 16, F / 256 and tiles + 1 words
    MdCarved<double> bwd;                               // backward: md_vertex_grad's, with fp64 rows
    size_t total;                                       // the larger of the two walks
};
SpWs sp_carve(void* ws, int64_t F, int64_t n) {
    SpWs r;
    WsWalk w(ws);
    r.scal = w.take<u64>(2);
    r.cumq = w.take<u64>((size_t)std::max<int64_t>(F, 1));
    r.lev1 = w.take<u64>((size_t)((F + SP_FAN1 - 1) / SP_FAN1 + 1));
    r.lev2 = w.take<u64>((size_t)((F + SP_FAN2 - 1) / SP_FAN2 + 1));
    r.tsum = w.take<u64>((size_t)((F + SP_TILE - 1) / SP_TILE + 1));
    r.bwd = md_carve<double>(ws, n, F, false);
    r.total = std::max(w.bytes(), r.bwd.total);
    return r;
}
// n is bounded below 2^31 - BLOCK: the sort's grids round it up to a workgroup
int sp_check_sizes(int64_t F, int64_t n, const char* who) {
    LS_REQUIRE(F >= 0 && n >= 0, LS_E_INVALID, "%s: bad argument (F and n must not be negative)", who);
    LS_REQUIRE(n < INT32_MAX - BLOCK && 3 * F < INT32_MAX, LS_E_OVERFLOW, "%s: more than 2^31 samples or corners", who);
    return LS_OK;
}
}  // namespace

extern "C" int ls_sample_workspace_bytes(int64_t F, int64_t n, size_t* bytes) {
    LS_REQUIRE(bytes, LS_E_INVALID, "ls_sample_workspace_bytes: bad argument");
    if (int rc = sp_check_sizes(F, n, "ls_sample_workspace_bytes")) return rc;
    *bytes = sp_carve(nullptr, F, n).total;
    return LS_OK;
}

extern "C" int ls_sample_surface(const float* verts, const void* faces, int idx_bytes, int64_t F, int64_t V, int64_t n, uint64_t seed,
                                 uint32_t stream_id, uint64_t offset, float* P, int64_t* I, float* W, void* ws, size_t ws_bytes, int device,
                                 void* stream) {
    LS_REQUIRE((verts || F == 0) && (faces || F == 0) && (idx_bytes == 4 || idx_bytes == 8) && V >= 0 && V < INT32_MAX && ws
                   && (n <= 0 || (P && I && W)),
               LS_E_INVALID, "ls_sample_surface: bad argument (faces must be int32 or int64, V < 2^31, no null pointer)");
    if (int rc = sp_check_sizes(F, n, "ls_sample_surface")) return rc;
    LS_REQUIRE(offset < ((uint64_t)1 << 31) && offset + (uint64_t)n < ((uint64_t)1 << 31), LS_E_OVERFLOW,
               "ls_sample_surface: offset + n must be below 2^31");
    const auto [scal, cumq, lev1, lev2, tsum, bwd, total] = sp_carve(ws, F, n);
    LS_REQUIRE(ws_bytes >= total, LS_E_WORKSPACE, "ls_sample_surface: workspace too small (%zu < %zu bytes)", ws_bytes, total);
    if (n == 0) return LS_OK;
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    LS_HIP(hipMemsetAsync(scal, 0, 16, st));
    const int tiles = div_up(F, SP_TILE);
    if (F > 0) {
        LS_IDX(idx_bytes, hipLaunchKernelGGL((k_sp_area<IDX>), dim3(reduce_grid(F)), dim3(BLOCK), 0, st, verts, (const IDX*)faces, F, V, cumq, scal));
        hipLaunchKernelGGL(k_sp_quant, dim3(tiles), dim3(BLOCK), 0, st, cumq, F, (const u64*)scal, tsum);
        hipLaunchKernelGGL(k_sp_scan_tiles, dim3(1), dim3(BLOCK), 0, st, tsum, (int64_t)tiles, scal + 1);
        hipLaunchKernelGGL(k_sp_scan, dim3(tiles), dim3(BLOCK), 0, st, cumq, F, (const u64*)tsum, lev1, lev2);
    }
    LS_IDX(idx_bytes, hipLaunchKernelGGL((k_sp_sample<IDX>), dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, verts, (const IDX*)faces, F, (const u64*)cumq,
                                         (const u64*)lev1, (const u64*)lev2, (const u64*)tsum, (const u64*)(scal + 1), n, (u64)offset, (u64)seed, (unsigned)stream_id, P, I, W));
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_sample_surface_backward(const void* faces, int idx_bytes, int64_t F, int64_t V, int64_t n, const int64_t* I, const float* W,
                                          const float* gP, const int32_t* vptr, const int32_t* corner_order, float* gV, void* ws,
                                          size_t ws_bytes, int device, void* stream) {
    (void)faces;                    // the ranking of ls_corner_ranks carries the connectivity
    LS_REQUIRE((idx_bytes == 4 || idx_bytes == 8) && V > 0 && V < INT32_MAX && gV && ws && vptr && (corner_order || F == 0)
                   && (n <= 0 || (I && W && gP)),
               LS_E_INVALID, "ls_sample_surface_backward: bad argument (V in [1, 2^31), no null pointer)");
    if (int rc = sp_check_sizes(F, n, "ls_sample_surface_backward")) return rc;
    const SpWs L = sp_carve(ws, F, n);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_sample_surface_backward: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    if (n == 0 || F == 0) {
        LS_HIP(hipMemsetAsync(gV, 0, sizeof(float) * 3 * (size_t)V, st));
        return LS_OK;
    }
    const MdCarved<double>& c = L.bwd;
    if (int rc = md_vertex_grad<double>(I, n, F, V, SpRows{W, gP, c.order, c.seg, c.rows}, vptr, corner_order, gV, c, st)) return rc;
    LS_HIP(hipGetLastError());
    return LS_OK;
}
