// subdiv.hip -- one level of midpoint or Loop subdivision of a triangle mesh as a topology built once and a linear map applied every
// step, on the device (gfx950, wave64): largesteps/subdivide.py, DESIGN.md section 2.14. X_fine = S X_coarse and gX = S^T g, the second
// as a gather over the same walk. tests/subdiv_statement.py restates the rule below in numpy; the device returns the statement's bits.
//
// Half-edges and edges. Half-edge h = 3 f + e runs from F[f, e] to F[f, (e + 1) % 3]; half-edges with the same unordered pair of ends
// form an edge. The OWNER of an edge is its half-edge of lowest id; edges are numbered by ascending owner, the exclusive scan of the
// owner flags in half-edge order. An edge of one half-edge is a boundary edge, of two an interior edge, of more an error. Orientation
// need not be consistent: nothing below reads it. edges[e] = (the smaller end, the larger end); opp[e] = (the corner opposite the owner in
// its face, the corner opposite the other half-edge in its face or -1).
// Faces. With m_e = V + eid(3 f + e), face f becomes 4 f .. 4 f + 3 = (F[f,0], m_0, m_2), (F[f,1], m_1, m_0), (F[f,2], m_2, m_1),
// (m_0, m_1, m_2).
// The walk. The corners of vertex v in the rank order of ls_corner_ranks (ascending corner id 3 f + i); at a corner first the outgoing
// half-edge 3 f + i, then the incoming one 3 f + (i + 2) % 3; an edge counts only at its owner, so every edge at v counts once. n_v is
// the number of edges counted, b_v the number of boundary edges among them: b_v = 0 is an interior vertex, b_v = 2 a boundary vertex
// whose boundary neighbours (p, q) are the far ends of its two boundary edges in walk order, anything else an error.
// Midpoint. An old vertex keeps its bits; an edge vertex is (a + b) * 0.5.
// Loop (Warren's weights). Edge vertex: 0.375 (a + b) + 0.125 (c + d) with (a, b) = edges[e], (c, d) = opp[e], or (a + b) * 0.5 on a
// boundary edge. Old vertex: interior (1 - n beta) x + beta W with W the sum of the neighbours over the walk and beta = 3 / 16 for
// n = 3, 3 / (8 n) otherwise; boundary 0.75 x + 0.125 (x_p + x_q); n = 0 keeps its bits. Every value is formed in fp64 from the fp32
// inputs, in exactly the order written here, and rounded to fp32 once.
// Backward. gX[v] = w_v g[v] + W, w_v the vertex's own weight (1, 0.75 or 1 - n beta) and W the sum over the walk, from 0, of: at an
// owner half-edge with far end u and edge e, first u's vertex-rule weight on v times g[u] (beta_u for an interior u; 0.125 for a
// boundary u when e is a boundary edge; no term otherwise; none for midpoint), then 0.375 g[V + e] (0.5 on a boundary edge and for
// midpoint); after the two half-edges of a corner, Loop only, 0.125 g[V + e'] for the edge e' opposite the corner when it is interior.
// The long walk. A vertex of more than 64 corners is summed by its whole wave, lane l taking corners l, l + 64, ... in order and the
// xor butterfly 32, 16, ... 1 adding the lanes (seg_sum of groupby.h): forward and backward, the same W in a different, fixed order.
//
// One thread per output row, channels in register groups of K | C. The gathers are index chases (order -> half-edge words and ends ->
// rows) like ls_vertex_normals_gathered: latency-bound, hidden by occupancy; the index arrays are int32 and read through the caches.
#include "common.h"
#include "groupby.h"
#include "meshface.h"
#include "radix.h"
#include "workspace.h"

namespace ls {

struct SdTopo {
    const int *tri, *he, *edges, *opp, *valence, *bnbr, *vptr, *order;
    const unsigned char* bflag;
    int V, E;
};
// he[h] = eid << 2 | boundary << 1 | owner
constexpr int SD_OWNER = 1, SD_BOUNDARY = 2;

__device__ __forceinline__ double sd_beta(int n) { return n == 3 ? 3.0 / 16.0 : 3.0 / (8.0 * (double)n); }

// ---- topology -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_sd_corners(const int* __restrict__ tri, int64_t F, int* __restrict__ cnt, int* __restrict__ status) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int id[3];
    ld_ids(tri, f, id);
    if (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) atomicOr(status, LS_SUBDIV_REPEATED_VERTEX);
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd(&cnt[id[c]], 1);
}

// the sorted half-edges: the first of a run of equal keys owns the edge (the sort is stable: it has the lowest id)
__global__ __launch_bounds__(BLOCK) void k_sd_pair(KeyEdge key, const int* __restrict__ sorted, int64_t n, int* __restrict__ own,
                                                   int* __restrict__ mate, int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int h = sorted[i];
    const unsigned a0 = key.word(h, 0), a1 = key.word(h, 1);
    auto same = [&](int64_t j) {
        if (j < 0 || j >= n) return false;
        const int g = sorted[j];
        return key.word(g, 0) == a0 && key.word(g, 1) == a1;
    };
    const bool next = same(i + 1);
    if (!same(i - 1)) {
        own[h] = 1;
        mate[h] = next ? sorted[i + 1] : -1;
        if (next && same(i + 2)) atomicOr(status, LS_SUBDIV_NONMANIFOLD_EDGE);
    } else {
        own[h] = 0;
        mate[h] = sorted[i - 1];
    }
}

__global__ __launch_bounds__(BLOCK) void k_sd_edges(const int* __restrict__ tri, const int* __restrict__ own, const int* __restrict__ mate,
                                                    const int* __restrict__ eoff, int64_t n, int* __restrict__ he, int* __restrict__ edges,
                                                    int* __restrict__ opp) {
    const int64_t h = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int o = own[h], m = mate[h];
    const int eid = eoff[o ? (int)h : m];                 // (a non-owner always has a mate)
    const int bnd = o && m < 0;
    he[h] = eid << 2 | (bnd ? SD_BOUNDARY : 0) | (o ? SD_OWNER : 0);
    if (!o) return;
    const int f = (int)(h / 3), e = (int)h - 3 * f;
    const int a = tri[h], b = tri[3 * f + (e + 1) % 3];
    edges[2 * (size_t)eid] = min(a, b);
    edges[2 * (size_t)eid + 1] = max(a, b);
    opp[2 * (size_t)eid] = tri[3 * f + (e + 2) % 3];
    int d = -1;
    if (m >= 0) {
        const int fm = m / 3, em = m - 3 * fm;
        d = tri[3 * fm + (em + 2) % 3];
    }
    opp[2 * (size_t)eid + 1] = d;
}

__global__ __launch_bounds__(BLOCK) void k_sd_vertices(const int* __restrict__ tri, const int* __restrict__ he, const int* __restrict__ vptr,
                                                       const int* __restrict__ order, int64_t V, int* __restrict__ valence,
                                                       unsigned char* __restrict__ bflag, int* __restrict__ bnbr, int* __restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    int n = 0, b = 0, pq[2] = {-1, -1};
    const int e1 = vptr[v + 1];
    for (int e = vptr[v]; e < e1; ++e) {
        const int c = order[e], f = c / 3, i = c - 3 * f;
        const int h1 = 3 * f + (i + 1) % 3, h2 = 3 * f + (i + 2) % 3;
        const int ho = he[c], hi = he[h2];
        if (ho & SD_OWNER) {
            ++n;
            if (ho & SD_BOUNDARY) { if (b < 2) pq[b] = tri[h1]; ++b; }
        }
        if (hi & SD_OWNER) {
            ++n;
            if (hi & SD_BOUNDARY) { if (b < 2) pq[b] = tri[h2]; ++b; }
        }
    }
    valence[v] = n;
    bflag[v] = b == 2;
    bnbr[2 * v] = b == 2 ? pq[0] : -1;
    bnbr[2 * v + 1] = b == 2 ? pq[1] : -1;
    if (b != 0 && b != 2) atomicOr(status, LS_SUBDIV_NONMANIFOLD_VERTEX);
}

template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_sd_fine_faces(const int* __restrict__ tri, const int* __restrict__ he, int64_t F, int64_t V,
                                                         IDX* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int id[3], w[3];
    ld_ids(tri, f, id);
    ld_ids(he, f, w);
    const IDX m0 = (IDX)(V + (w[0] >> 2)), m1 = (IDX)(V + (w[1] >> 2)), m2 = (IDX)(V + (w[2] >> 2));
    IDX* __restrict__ o = out + 12 * f;
    o[0] = (IDX)id[0]; o[1] = m0; o[2] = m2;
    o[3] = (IDX)id[1]; o[4] = m1; o[5] = m0;
    o[6] = (IDX)id[2]; o[7] = m2; o[8] = m1;
    o[9] = m0; o[10] = m1; o[11] = m2;
}

// ---- apply --------------------------------------------------------------------------------------------------------------------------
// row k of X_fine for the channels c0 .. c0 + K - 1: the policy seg_sum asks for
template <int K>
struct SdForward {
    SdTopo t;
    const float* __restrict__ X;
    float* __restrict__ out;
    int C, c0;
    bool loop;
    __device__ __forceinline__ bool walks(int64_t k) const { return loop && k < t.V && !t.bflag[k]; }
    __device__ __forceinline__ int count(int64_t k) const { return walks(k) ? t.vptr[k + 1] - t.vptr[k] : 0; }
    __device__ __forceinline__ void add(double (&acc)[K], int row) const {
        const float* __restrict__ r = X + (size_t)row * C + c0;
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] += (double)r[q];
    }
    __device__ __forceinline__ void walk(int64_t k, int start, int step, double (&acc)[K]) const {
        if (!walks(k)) return;
        const int e1 = t.vptr[k + 1];
        for (int e = t.vptr[k] + start; e < e1; e += step) {
            const int c = t.order[e], f = c / 3, i = c - 3 * f;
            const int h1 = 3 * f + (i + 1) % 3, h2 = 3 * f + (i + 2) % 3;
            const int ho = t.he[c], hi = t.he[h2];
            const int u1 = t.tri[h1], u2 = t.tri[h2];
            if (ho & SD_OWNER) add(acc, u1);
            if (hi & SD_OWNER) add(acc, u2);
        }
    }
    __device__ __forceinline__ void store(int64_t k, const double (&acc)[K]) const {
        float* __restrict__ o = out + (size_t)k * C + c0;
        if (k < t.V) {
            const float* __restrict__ x = X + (size_t)k * C + c0;
            const int n = t.valence[k];
            if (!loop || n == 0) {
#pragma unroll
                for (int q = 0; q < K; ++q) o[q] = x[q];
            } else if (t.bflag[k]) {
                const float* __restrict__ xp = X + (size_t)t.bnbr[2 * k] * C + c0;
                const float* __restrict__ xq = X + (size_t)t.bnbr[2 * k + 1] * C + c0;
#pragma unroll
                for (int q = 0; q < K; ++q) o[q] = (float)(0.75 * (double)x[q] + 0.125 * ((double)xp[q] + (double)xq[q]));
            } else {
                const double beta = sd_beta(n), w = 1.0 - (double)n * beta;
#pragma unroll
                for (int q = 0; q < K; ++q) o[q] = (float)(w * (double)x[q] + beta * acc[q]);
            }
            return;
        }
        const size_t e = (size_t)(k - t.V);
        const int a = t.edges[2 * e], b = t.edges[2 * e + 1], c = t.opp[2 * e], d = t.opp[2 * e + 1];
        const float* __restrict__ xa = X + (size_t)a * C + c0;
        const float* __restrict__ xb = X + (size_t)b * C + c0;
        if (!loop || d < 0) {
#pragma unroll
            for (int q = 0; q < K; ++q) o[q] = (float)(((double)xa[q] + (double)xb[q]) * 0.5);
        } else {
            const float* __restrict__ xc = X + (size_t)c * C + c0;
            const float* __restrict__ xd = X + (size_t)d * C + c0;
#pragma unroll
            for (int q = 0; q < K; ++q)
                o[q] = (float)(0.375 * ((double)xa[q] + (double)xb[q]) + 0.125 * ((double)xc[q] + (double)xd[q]));
        }
    }
};

// row v of S^T g for the channels c0 .. c0 + K - 1
template <int K>
struct SdBackward {
    SdTopo t;
    const float* __restrict__ g;
    float* __restrict__ gX;
    int C, c0;
    bool loop;
    __device__ __forceinline__ int count(int64_t k) const { return t.vptr[k + 1] - t.vptr[k]; }
    __device__ __forceinline__ void add(double (&acc)[K], double w, int64_t row) const {
        const float* __restrict__ r = g + (size_t)row * C + c0;
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] += w * (double)r[q];
    }
    // the owner half-edge word hw, its far end u
    __device__ __forceinline__ void edge(double (&acc)[K], int hw, int u) const {
        if (!(hw & SD_OWNER)) return;
        const bool bnd = hw & SD_BOUNDARY;
        if (loop) {
            if (!t.bflag[u]) add(acc, sd_beta(t.valence[u]), u);
            else if (bnd) add(acc, 0.125, u);
        }
        add(acc, loop && !bnd ? 0.375 : 0.5, (int64_t)t.V + (hw >> 2));
    }
    __device__ __forceinline__ void walk(int64_t k, int start, int step, double (&acc)[K]) const {
        const int e1 = t.vptr[k + 1];
        for (int e = t.vptr[k] + start; e < e1; e += step) {
            const int c = t.order[e], f = c / 3, i = c - 3 * f;
            const int h1 = 3 * f + (i + 1) % 3, h2 = 3 * f + (i + 2) % 3;
            const int ho = t.he[c], hi = t.he[h2], hf = t.he[h1];
            const int u1 = t.tri[h1], u2 = t.tri[h2];
            edge(acc, ho, u1);
            edge(acc, hi, u2);
            if (loop && !(hf & SD_BOUNDARY)) add(acc, 0.125, (int64_t)t.V + (hf >> 2));
        }
    }
    __device__ __forceinline__ void store(int64_t k, const double (&acc)[K]) const {
        const int n = t.valence[k];
        const double w = !loop || n == 0 ? 1.0 : t.bflag[k] ? 0.75 : 1.0 - (double)n * sd_beta(n);
        const float* __restrict__ r = g + (size_t)k * C + c0;
        float* __restrict__ o = gX + (size_t)k * C + c0;
#pragma unroll
        for (int q = 0; q < K; ++q) o[q] = (float)(w * (double)r[q] + acc[q]);
    }
};

template <int K>
__global__ __launch_bounds__(256) void k_sd_apply(const SdTopo t, const float* __restrict__ X, float* __restrict__ out, int C, bool loop) {
    for (int c0 = 0; c0 < C; c0 += K) seg_sum<K, SdForward<K>, double>((int64_t)t.V + t.E, SdForward<K>{t, X, out, C, c0, loop});
}
template <int K>
__global__ __launch_bounds__(256) void k_sd_apply_backward(const SdTopo t, const float* __restrict__ g, float* __restrict__ gX, int C, bool loop) {
    for (int c0 = 0; c0 < C; c0 += K) seg_sum<K, SdBackward<K>, double>((int64_t)t.V, SdBackward<K>{t, g, gX, C, c0, loop});
}

// runs the statement once with K = the widest register group that divides C
#define SD_GROUPS(C, ...)                                                                              \
    do {                                                                                               \
        if ((C) % 4 == 0) { constexpr int K = 4; __VA_ARGS__; }                                        \
        else if ((C) % 3 == 0) { constexpr int K = 3; __VA_ARGS__; }                                   \
        else if ((C) % 2 == 0) { constexpr int K = 2; __VA_ARGS__; }                                   \
        else { constexpr int K = 1; __VA_ARGS__; }                                                     \
    } while (0)

struct SdWs {          // the regions of the topology's workspace
    int *cnt, *ord_a, *own, *eoff, *mate, *status;
    SortScratch sort;
    size_t total;
};
static inline SdWs sd_carve(void* ws, int64_t F, int64_t V) {
    const int64_t n = 3 * F;
    WsWalk w(ws);
    int* cnt = w.take<int>((size_t)(V + 1));
    int* ord_a = w.take<int>((size_t)(n > 0 ? n : 1));
    int* own = w.take<int>((size_t)(n > 0 ? n : 1));
    int* eoff = w.take<int>((size_t)(n + 1));
    int* mate = w.take<int>((size_t)(n > 0 ? n : 1));
    int* status = w.take<int>(4);
    const SortScratch sort = sort_scratch_take(w, n > 0 ? n : 1, true, std::max(n, V));
    return {cnt, ord_a, own, eoff, mate, status, sort, w.bytes()};
}
static int sd_sizes(const char* who, int64_t F, int64_t V) {
    LS_REQUIRE(F >= 0 && V >= 0, LS_E_INVALID, "%s: a negative size", who);
    const int64_t lim = (int64_t)1 << 31;
    LS_REQUIRE(F < lim && 12 * F < lim, LS_E_OVERFLOW, "%s: 12 x the number of faces reaches 2^31", who);
    LS_REQUIRE(V < lim, LS_E_OVERFLOW, "%s: the number of vertices reaches 2^31", who);
    return LS_OK;
}
static int sd_apply_args(const char* who, const void* in, const void* out, int64_t F, int64_t V, int64_t E, int C, int scheme,
                         const int32_t* tri, const int32_t* he, const int32_t* edges, const int32_t* opp, const int32_t* valence,
                         const unsigned char* bflag, const int32_t* bnbr, const int32_t* vptr, const int32_t* order) {
    LS_REQUIRE(F >= 0 && V >= 0 && E >= 0 && E <= 3 * F, LS_E_INVALID, "%s: a negative size, or more edges than half-edges", who);
    LS_REQUIRE(C >= 1 && C <= 32, LS_E_INVALID, "%s: C must be in [1, 32], got %d", who, C);
    LS_REQUIRE(scheme == LS_SUBDIV_MIDPOINT || scheme == LS_SUBDIV_LOOP, LS_E_INVALID, "%s: unknown scheme %d", who, scheme);
    if (int rc = sd_sizes(who, F, V)) return rc;
    LS_REQUIRE(V + E < ((int64_t)1 << 31), LS_E_OVERFLOW, "%s: V + E reaches 2^31", who);
    LS_REQUIRE((V + E == 0 || (in && out)) && (V == 0 || (valence && bflag && bnbr && vptr)) && (F == 0 || (tri && he && order)) &&
                   (E == 0 || (edges && opp)), LS_E_INVALID, "%s: null argument", who);
    return LS_OK;
}

}  // namespace ls

using namespace ls;

extern "C" int ls_subdiv_workspace_bytes(int64_t F, int64_t V, size_t* bytes) {
    LS_REQUIRE(bytes, LS_E_INVALID, "ls_subdiv_workspace_bytes: null argument");
    if (int rc = sd_sizes("ls_subdiv_workspace_bytes", F, V)) return rc;
    *bytes = sd_carve(nullptr, F, V).total;
    return LS_OK;
}

extern "C" int ls_subdiv_topology(const void* faces, int idx_bytes, int64_t F, int64_t V, int32_t* tri, int32_t* he, int32_t* edges,
                                  int32_t* opp, int32_t* valence, unsigned char* bflag, int32_t* bnbr, int32_t* vptr, int32_t* order,
                                  void* fine_faces, int64_t* h_E, int* h_status, void* ws, size_t ws_bytes, int device, void* stream) {
    const char* who = "ls_subdiv_topology";
    LS_REQUIRE(h_E && h_status && vptr && ws && (idx_bytes == 4 || idx_bytes == 8), LS_E_INVALID,
               "%s: null argument, or faces that are neither int32 nor int64", who);
    if (int rc = sd_sizes(who, F, V)) return rc;
    LS_REQUIRE((V == 0 || (valence && bflag && bnbr)) && (F == 0 || (faces && tri && he && edges && opp && order && fine_faces)),
               LS_E_INVALID, "%s: null argument", who);
    const SdWs L = sd_carve(ws, F, V);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = 3 * F;
    *h_E = 0;
    *h_status = 0;
    LS_HIP(hipMemsetAsync(L.cnt, 0, sizeof(int) * (size_t)(V + 1), st));
    LS_HIP(hipMemsetAsync(L.status, 0, sizeof(int) * 4, st));
    if (n) {
        // the indices as int32 (an index outside [0, V) is stored as 0 and flagged: nothing below follows a bad index), the corners counted
        LS_IDX(idx_bytes, hipLaunchKernelGGL((k_faces_in<IDX, 0>), dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, (const IDX*)faces, n, V,
                                             (int*)tri, L.status + 1));
        hipLaunchKernelGGL(k_sd_corners, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, (const int*)tri, F, L.cnt, L.status);
        LS_HIP(hipGetLastError());
    }
    if (int rc = exclusive_scan(L.cnt, V, (int*)vptr, L.sort.bsum, st)) return rc;
    int E = 0;
    if (n) {
        // the corner ranking: the corners sorted stably by vertex
        const int* src = nullptr;
        if (int rc = radix_argsort(KeyInt{(const int*)tri}, n, radix_passes(std::max<int64_t>(V, 1) - 1), (int*)order, L.sort, st, &src)) return rc;
        if (src != order) LS_HIP(hipMemcpyAsync(order, src, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
        // the half-edges sorted stably by (smaller end, larger end), paired, and the owners numbered
        const KeyEdge key{(const int*)tri};
        const int* sorted = nullptr;
        if (int rc = radix_argsort_words(key, n, 2, L.ord_a, L.sort, st, &sorted, 4)) return rc;
        hipLaunchKernelGGL(k_sd_pair, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, key, sorted, n, L.own, L.mate, L.status);
        LS_HIP(hipGetLastError());
        if (int rc = exclusive_scan(L.own, n, L.eoff, L.sort.bsum, st)) return rc;
        hipLaunchKernelGGL(k_sd_edges, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, (const int*)tri, (const int*)L.own, (const int*)L.mate,
                           (const int*)L.eoff, n, (int*)he, (int*)edges, (int*)opp);
        LS_HIP(hipGetLastError());
        LS_HIP(hipMemcpyAsync(&E, L.eoff + n, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (V) {
        hipLaunchKernelGGL(k_sd_vertices, dim3(div_up(V, BLOCK)), dim3(BLOCK), 0, st, (const int*)tri, (const int*)he, (const int*)vptr,
                           (const int*)order, V, (int*)valence, bflag, (int*)bnbr, L.status);
        LS_HIP(hipGetLastError());
    }
    if (n) {
        LS_IDX(idx_bytes, hipLaunchKernelGGL(k_sd_fine_faces<IDX>, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, (const int*)tri, (const int*)he, F, V,
                                             (IDX*)fine_faces));
        LS_HIP(hipGetLastError());
    }
    int status[2] = {0, 0};
    LS_HIP(hipMemcpyAsync(status, L.status, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    LS_HIP(hipStreamSynchronize(st));
    *h_E = E;
    *h_status = status[0] | (status[1] ? LS_SUBDIV_BAD_INDEX : 0);
    LS_REQUIRE(*h_status || V + (int64_t)E < ((int64_t)1 << 31), LS_E_OVERFLOW, "%s: V + E reaches 2^31", who);
    return LS_OK;
}

extern "C" int ls_subdiv_apply(const float* X, int64_t F, int64_t V, int64_t E, int C, int scheme, const int32_t* tri, const int32_t* he,
                               const int32_t* edges, const int32_t* opp, const int32_t* valence, const unsigned char* bflag,
                               const int32_t* bnbr, const int32_t* vptr, const int32_t* order, float* out, int device, void* stream) {
    if (int rc = sd_apply_args("ls_subdiv_apply", X, out, F, V, E, C, scheme, tri, he, edges, opp, valence, bflag, bnbr, vptr, order)) return rc;
    if (V + E == 0) return LS_OK;
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const SdTopo t{tri, he, edges, opp, valence, bnbr, vptr, order, bflag, (int)V, (int)E};
    SD_GROUPS(C, hipLaunchKernelGGL(k_sd_apply<K>, dim3(div_up(V + E, 256)), dim3(256), 0, (hipStream_t)stream, t, X, out, C,
                                    scheme == LS_SUBDIV_LOOP));
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_subdiv_apply_backward(const float* g, int64_t F, int64_t V, int64_t E, int C, int scheme, const int32_t* tri,
                                        const int32_t* he, const int32_t* edges, const int32_t* opp, const int32_t* valence,
                                        const unsigned char* bflag, const int32_t* bnbr, const int32_t* vptr, const int32_t* order, float* gX,
                                        int device, void* stream) {
    if (int rc = sd_apply_args("ls_subdiv_apply_backward", g, gX, F, V, E, C, scheme, tri, he, edges, opp, valence, bflag, bnbr, vptr, order))
        return rc;
    if (V == 0) return LS_OK;
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const SdTopo t{tri, he, edges, opp, valence, bnbr, vptr, order, bflag, (int)V, (int)E};
    SD_GROUPS(C, hipLaunchKernelGGL(k_sd_apply_backward<K>, dim3(div_up(V, 256)), dim3(256), 0, (hipStream_t)stream, t, g, gX, C,
                                    scheme == LS_SUBDIV_LOOP));
    LS_HIP(hipGetLastError());
    return LS_OK;
}
