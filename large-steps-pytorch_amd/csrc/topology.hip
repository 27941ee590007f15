// topology.hip -- what a triangle mesh is made of, on the device (gfx950, wave64): its vertex and facet components, its edges with their
// faces and flags, its boundary loops, the area and signed volume of every facet component and the compaction that keeps some of them:
// largesteps/topology.py, DESIGN.md section 2.15. tests/topology_statement.py restates the rule below in numpy; every array the device
// returns is the statement's, the fp64 measures bit for bit.
//
// Edges. Half-edge h = 3 f + e runs from F[f, e] to F[f, (e + 1) % 3]; the half-edges of one unordered vertex pair form an edge, owned by
// the lowest h; edges are numbered by ascending owner (the rule of subdiv.hip). One half-edge: a boundary edge; more than two: a
// non-manifold edge; exactly two that run the same way: a misoriented edge. edge_faces[e] = the faces of the edge's two lowest half-edges.
// Components. Vertices joined by an edge are one vertex component, numbered by ascending lowest vertex id; faces that share an edge are
// one facet component (a shared vertex alone does not join them), numbered by ascending lowest face id.
// Hooking. parent[i] = i; one thread per joining pair finds both roots and hooks the LARGER root under the smaller with atomicMin on
// parent[larger]; when the value read back is not the root it expected it carries on with (value read, smaller). Every parent[x] <= x
// and every write lowers a value, so each loop is bounded; a write only ever names a member of the same component, so the root a
// component ends with is its lowest id whatever the interleaving: integer atomics, one result. No host loop, no flag read back.
// Boundary loops. Defined when every vertex on a boundary edge has one boundary half-edge leaving and one entering (status flag
// otherwise). The boundary vertices are compacted in ascending id; ceil(log2) rounds of pointer doubling give every vertex the lowest
// member of its cycle, the cycle is cut there, a second doubling (Wyllie) ranks it, and a scan of the cycle lengths at their heads places
// vertex i at start[head] + rank: loops in ascending lowest vertex, each from its lowest vertex along the half-edges.
// Measures. Per face in fp64 from the fp32 coordinates, n = (b - a) x (c - a), area 0.5 sqrt(nx nx + ny ny + nz nz), volume
// (ax (b x c)x + ay (b x c)y + az (b x c)z) / 6, added left to right (-ffp-contract=off); per component the terms of its faces in
// ascending face id in the one order of seg_sum (groupby.h) with A = double. No float atomics.
#include "common.h"
#include "groupby.h"
#include "meshface.h"
#include "radix.h"
#include "workspace.h"

namespace ls {

constexpr int TP_BOUNDARY = LS_TOPO_EDGE_BOUNDARY, TP_NONMANIFOLD = LS_TOPO_EDGE_NONMANIFOLD, TP_MISORIENTED = LS_TOPO_EDGE_MISORIENTED;      // eflag[e]

// ---- hooking and compression ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tp_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; on the way every visited entry is lowered to its grandparent (a member of the same component, never a raise)
__device__ __forceinline__ int tp_root(int* __restrict__ parent, int x) {
    for (;;) {
        const int p = tp_load(parent + x);
        if (p == x) return x;
        const int g = tp_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
    }
}

__device__ __forceinline__ void tp_hook(int* __restrict__ parent, int a, int b) {
    for (;;) {
        a = tp_root(parent, a);
        b = tp_root(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);      // a > b
        if (old == a) return;                          // a was a root and now hangs under b
        a = old;                                       // a had been hooked meanwhile: old < a, and (old, b) are still to be joined
    }
}

__global__ __launch_bounds__(BLOCK) void k_tp_iota(int* __restrict__ a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) a[i] = (int)i;
}

// one thread per half-edge: its two ends joined; the face checked for a repeated vertex
__global__ __launch_bounds__(BLOCK) void k_tp_hook_vertices(const int* __restrict__ tri, int64_t n, int* __restrict__ parent, int* __restrict__ status) {
    const int64_t h = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int f = (int)(h / 3), e = (int)h - 3 * f;
    const int a = tri[h], b = tri[3 * f + (e + 1) % 3];
    if (a == b) { atomicOr(status, LS_TOPO_REPEATED_VERTEX); return; }
    tp_hook(parent, a, b);
}

// label[i] = root(i) and flag[i] = (i is a root)
__global__ __launch_bounds__(BLOCK) void k_tp_compress(const int* __restrict__ parent, int64_t n, int* __restrict__ label, int* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    int x = (int)i;
    for (;;) {
        const int p = parent[x];
        if (p == x) break;
        x = p;
    }
    label[i] = x;
    flag[i] = x == (int)i;
}

__global__ __launch_bounds__(BLOCK) void k_tp_number(const int* __restrict__ label, const int* __restrict__ off, int64_t n, int* __restrict__ comp) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) comp[i] = off[label[i]];
}

// ---- the edge census ------------------------------------------------------------------------------------------------------------------
// one thread per sorted half-edge (the sort is stable: the first of a run of equal keys has the lowest id and owns the edge). The owner
// notes its second member and the edge's flags; every later member joins its face with the face of the member before it.
__global__ __launch_bounds__(BLOCK) void k_tp_census(KeyEdge key, const int* __restrict__ sorted, int64_t n, int* __restrict__ own,
                                                     int* __restrict__ mate, int* __restrict__ hflag, int* __restrict__ fparent) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int h = sorted[i];
    const unsigned a0 = key.word(h, 0), a1 = key.word(h, 1);
    auto same = [&](int64_t j) {
        if (j < 0 || j >= n) return false;
        const int g = sorted[j];
        return key.word(g, 0) == a0 && key.word(g, 1) == a1;
    };
    if (same(i - 1)) {
        own[h] = 0;
        mate[h] = -1;
        hflag[h] = 0;
        tp_hook(fparent, sorted[i - 1] / 3, h / 3);
        return;
    }
    own[h] = 1;
    if (!same(i + 1)) { mate[h] = -1; hflag[h] = TP_BOUNDARY; return; }
    const int g = sorted[i + 1];
    mate[h] = g;
    hflag[h] = same(i + 2) ? TP_NONMANIFOLD : key.tri[h] == key.tri[g] ? TP_MISORIENTED : 0;
}

// one thread per half-edge; an owner writes its edge: ends, faces, flag, the totals, and the boundary half-edge at its two ends
__global__ __launch_bounds__(BLOCK) void k_tp_edges(const int* __restrict__ tri, const int* __restrict__ own, const int* __restrict__ mate,
                                                    const int* __restrict__ hflag, const int* __restrict__ eoff, int64_t n, int* __restrict__ edges,
                                                    int* __restrict__ edge_faces, unsigned char* __restrict__ eflag, int* __restrict__ bout,
                                                    int* __restrict__ bin, int* __restrict__ nextv, int* __restrict__ totals) {
    const int64_t h = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n || !own[h]) return;
    const size_t e = (size_t)eoff[h];
    const int f = (int)(h / 3), c = (int)h - 3 * f;
    const int a = tri[h], b = tri[3 * f + (c + 1) % 3], m = mate[h], fl = hflag[h];
    edges[2 * e] = min(a, b);
    edges[2 * e + 1] = max(a, b);
    edge_faces[2 * e] = f;
    edge_faces[2 * e + 1] = m >= 0 ? m / 3 : -1;
    eflag[e] = (unsigned char)fl;
    if (fl & TP_BOUNDARY) {
        atomicAdd(totals + 0, 1);
        atomicAdd(bout + a, 1);
        atomicAdd(bin + b, 1);
        nextv[a] = b;                  // (one writer where the loops are defined)
    }
    if (fl & TP_NONMANIFOLD) atomicAdd(totals + 1, 1);
    if (fl & TP_MISORIENTED) atomicAdd(totals + 2, 1);
}

// ---- boundary loops -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_tp_bflags(const int* __restrict__ bout, const int* __restrict__ bin, int64_t V, int* __restrict__ bfl,
                                                     int* __restrict__ status) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int o = bout[v], i = bin[v];
    bfl[v] = o > 0;
    if ((o || i) && !(o == 1 && i == 1)) atomicOr(status, LS_TOPO_BAD_BOUNDARY);
}

// boundary vertex v = compact index cidx[v]: its vertex id, its successor (itself when the successor has no boundary half-edge leaving:
// only where the loops are not defined) and itself as the lowest member seen so far
__global__ __launch_bounds__(BLOCK) void k_tp_bcompact(const int* __restrict__ bfl, const int* __restrict__ cidx, const int* __restrict__ nextv,
                                                       int64_t V, int* __restrict__ vid, int* __restrict__ nx, int* __restrict__ mn) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V || !bfl[v]) return;
    const int i = cidx[v], u = nextv[v];
    vid[i] = (int)v;
    nx[i] = bfl[u] ? cidx[u] : i;
    mn[i] = i;
}

// B = *pB boundary vertices (a device scalar: the host launches for the most there can be)
__global__ __launch_bounds__(BLOCK) void k_tp_double_min(const int* __restrict__ pB, const int* __restrict__ nx, const int* __restrict__ mn,
                                                         int* __restrict__ nx2, int* __restrict__ mn2) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= *pB) return;
    const int j = nx[i];
    mn2[i] = min(mn[i], mn[j]);
    nx2[i] = nx[j];
}

// the cycles cut in front of their lowest member: the vertex before it becomes the tail (its own successor, 0 hops)
__global__ __launch_bounds__(BLOCK) void k_tp_cut(const int* __restrict__ pB, const int* __restrict__ nx0, const int* __restrict__ mn,
                                                  int* __restrict__ nx, int* __restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= *pB) return;
    const int j = nx0[i];
    const bool tail = mn[j] == j || j == (int)i;
    nx[i] = tail ? (int)i : j;
    d[i] = tail ? 0 : 1;
}

__global__ __launch_bounds__(BLOCK) void k_tp_double_rank(const int* __restrict__ pB, const int* __restrict__ nx, const int* __restrict__ d,
                                                          int* __restrict__ nx2, int* __restrict__ d2) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= *pB) return;
    const int j = nx[i];
    d2[i] = d[i] + d[j];
    nx2[i] = nx[j];
}

// len[i] = the length of the loop whose lowest member is i, 0 elsewhere; head[i] = 1 at such a member. Sized V + 1 and written for every
// i < V: the scans that follow run over V entries whatever B is.
__global__ __launch_bounds__(BLOCK) void k_tp_heads(const int* __restrict__ pB, const int* __restrict__ mn, const int* __restrict__ d, int64_t V,
                                                    int* __restrict__ len, int* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= V) return;
    const bool h = i < *pB && mn[i] == (int)i;
    len[i] = h ? d[i] + 1 : 0;
    head[i] = h;
}

__global__ __launch_bounds__(BLOCK) void k_tp_loops(const int* __restrict__ pB, const int* __restrict__ mn, const int* __restrict__ d,
                                                    const int* __restrict__ vid, const int* __restrict__ start, const int* __restrict__ hoff,
                                                    int* __restrict__ loops, int* __restrict__ ptr) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int B = *pB;
    if (i == 0) ptr[hoff[B]] = B;                       // ptr[L] (hoff is scanned over V >= B entries, zero flags past B)
    if (i >= B) return;
    const int m = mn[i];
    const int64_t pos = (int64_t)start[m] + (d[m] - d[i]);
    if (pos >= 0 && pos < B) loops[pos] = vid[i];       // (always, where the loops are defined)
    if (m == (int)i) ptr[hoff[i]] = start[i];
}

// ---- per-component counts -------------------------------------------------------------------------------------------------------------
// table[comp][col] += 1 for every lane with `on`; one add of the lane count where the wave's lanes share the component. Every lane of the
// wave calls it.
__device__ __forceinline__ void tp_count(unsigned long long* __restrict__ table, int comp, int col, bool on) {
    const unsigned long long m = __ballot(on);
    if (!m) return;
    const int lead = __ffsll((long long)m) - 1;
    const int first = __shfl(comp, lead, WAVE);
    if (__ballot(on && comp != first) == 0ull) {
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(table + 6 * (size_t)first + col, (unsigned long long)__popcll(m));
    } else if (on) {
        atomicAdd(table + 6 * (size_t)comp + col, 1ull);
    }
}

__global__ __launch_bounds__(BLOCK) void k_tp_count_faces(const int* __restrict__ fcomp, int64_t F, unsigned long long* __restrict__ table) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool on = f < F;
    tp_count(table, on ? fcomp[f] : 0, 0, on);
}

__global__ __launch_bounds__(BLOCK) void k_tp_count_edges(const int* __restrict__ fcomp, const int* __restrict__ edge_faces,
                                                          const unsigned char* __restrict__ eflag, int64_t E, unsigned long long* __restrict__ table) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool on = e < E;
    const int comp = on ? fcomp[edge_faces[2 * e]] : 0, fl = on ? eflag[e] : 0;
    tp_count(table, comp, 2, on);
    tp_count(table, comp, 3, on && (fl & TP_BOUNDARY));
    tp_count(table, comp, 4, on && (fl & TP_NONMANIFOLD));
    tp_count(table, comp, 5, on && (fl & TP_MISORIENTED));
}

// the corners sorted by vertex: corner e counts its vertex for its component unless an earlier corner of the vertex is of the same one
__global__ __launch_bounds__(BLOCK) void k_tp_count_vertices(const int* __restrict__ tri, const int* __restrict__ fcomp, const int* __restrict__ corder,
                                                             int64_t n, unsigned long long* __restrict__ table) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool on = e < n;
    int comp = 0;
    if (on) {
        const int c = corder[e], v = tri[c];
        comp = fcomp[c / 3];
        for (int64_t j = e - 1; j >= 0; --j) {
            const int cj = corder[j];
            if (tri[cj] != v) break;
            if (fcomp[cj / 3] == comp) { on = false; break; }
        }
    }
    tp_count(table, comp, 1, on);
}

// ---- measures -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_tp_terms(const float* __restrict__ verts, const int* __restrict__ tri, int64_t F, double* __restrict__ terms) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int id[3];
    ld_ids(tri, f, id);
    float p[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ld3(verts, (size_t)id[c], p[c]);
    const double ax = p[0][0], ay = p[0][1], az = p[0][2], bx = p[1][0], by = p[1][1], bz = p[1][2], cx = p[2][0], cy = p[2][1], cz = p[2][2];
    const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double kx = by * cz - bz * cy, ky = bz * cx - bx * cz, kz = bx * cy - by * cx;
    terms[2 * f] = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
    terms[2 * f + 1] = (ax * kx + ay * ky + az * kz) / 6.0;
}

struct TpMeasure {       // the policy seg_sum asks for: component k, its faces order[seg[k] .. seg[k + 1]) in ascending face id
    const double* __restrict__ terms;
    const int* __restrict__ order;
    const int* __restrict__ seg;
    double* __restrict__ out;
    __device__ __forceinline__ int count(int64_t k) const { return seg[k + 1] - seg[k]; }
    __device__ __forceinline__ void walk(int64_t k, int start, int step, double (&acc)[2]) const {
        const int e1 = seg[k + 1];
        for (int e = seg[k] + start; e < e1; e += step) {
            const size_t f = (size_t)order[e];
            acc[0] += terms[2 * f];
            acc[1] += terms[2 * f + 1];
        }
    }
    __device__ __forceinline__ void store(int64_t k, const double (&acc)[2]) const { out[2 * k] = acc[0]; out[2 * k + 1] = acc[1]; }
};

__global__ __launch_bounds__(256) void k_tp_measure(int64_t K, const TpMeasure g) { seg_sum<2, TpMeasure, double>(K, g); }

// ---- keep -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_tp_keep_flags(const int* __restrict__ tri, const int* __restrict__ fcomp, const unsigned char* __restrict__ mask,
                                                         int64_t F, int* __restrict__ fflag, int* __restrict__ vflag) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    const int k = mask[fcomp[f]] != 0;
    fflag[f] = k;
    if (!k) return;
    int id[3];
    ld_ids(tri, f, id);
#pragma unroll
    for (int c = 0; c < 3; ++c) vflag[id[c]] = 1;      // (every writer writes 1)
}

template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_tp_keep_faces(const int* __restrict__ tri, const int* __restrict__ fflag, const int* __restrict__ foff,
                                                         const int* __restrict__ voff, int64_t F, int64_t capF, IDX* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F || !fflag[f]) return;
    const int64_t row = foff[f];
    if (row >= capF) return;
    int id[3];
    ld_ids(tri, f, id);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * row + c] = (IDX)voff[id[c]];
}

template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_tp_keep_vertices(const int* __restrict__ vflag, const int* __restrict__ voff, const int* __restrict__ foff,
                                                            int64_t F, int64_t V, int64_t capV, IDX* __restrict__ I, IDX* __restrict__ J,
                                                            int64_t* __restrict__ sizes) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v == 0) { sizes[0] = foff[F]; sizes[1] = voff[V]; }
    if (v >= V) return;
    const bool k = vflag[v] != 0;
    const int64_t row = voff[v];
    I[v] = k ? (IDX)row : (IDX)-1;
    if (k && row < capV) J[row] = (IDX)v;
}

// ---- the workspaces -------------------------------------------------------------------------------------------------------------------
struct TpWs {           // the regions of ls_topo_build's workspace
    int *vpar, *fpar, *label, *flag, *off;                          // hooking, compression and numbering (vertices, then faces)
    int *ord_a, *own, *eoff, *mate, *hflag;                         // the edge census
    int *bout, *bin, *nextv, *bfl, *cidx, *vid, *nx[3], *mn[2], *d[2], *len, *start, *head, *hoff;      // boundary loops
    int *status, *totals;
    SortScratch sort, fsort;
    size_t total;
};
static inline TpWs tp_carve(void* ws, int64_t F, int64_t V) {
    const int64_t n = 3 * F, n1 = n > 0 ? n : 1, v1 = V + 1, m1 = std::max(F, V) + 1;
    WsWalk w(ws);
    TpWs L;
    L.vpar = w.take<int>((size_t)v1);
    L.fpar = w.take<int>((size_t)(F + 1));
    L.label = w.take<int>((size_t)m1);
    L.flag = w.take<int>((size_t)m1);
    L.off = w.take<int>((size_t)m1);
    L.ord_a = w.take<int>((size_t)n1);
    L.own = w.take<int>((size_t)n1);
    L.eoff = w.take<int>((size_t)(n + 1));
    L.mate = w.take<int>((size_t)n1);
    L.hflag = w.take<int>((size_t)n1);
    L.bout = w.take<int>((size_t)v1);
    L.bin = w.take<int>((size_t)v1);
    L.nextv = w.take<int>((size_t)v1);
    L.bfl = w.take<int>((size_t)v1);
    L.cidx = w.take<int>((size_t)v1);
    L.vid = w.take<int>((size_t)v1);
    for (int i = 0; i < 3; ++i) L.nx[i] = w.take<int>((size_t)v1);
    for (int i = 0; i < 2; ++i) L.mn[i] = w.take<int>((size_t)v1);
    for (int i = 0; i < 2; ++i) L.d[i] = w.take<int>((size_t)v1);
    L.len = w.take<int>((size_t)v1);
    L.start = w.take<int>((size_t)v1);
    L.head = w.take<int>((size_t)v1);
    L.hoff = w.take<int>((size_t)v1);
    L.status = w.take<int>(4);
    L.totals = w.take<int>(4);
    L.sort = sort_scratch_take(w, n1, true, std::max(n, V) + 1);
    L.fsort = sort_scratch_take(w, F > 0 ? F : 1, true);
    L.total = w.bytes();
    return L;
}

struct TpKeepWs {
    int *fflag, *foff, *vflag, *voff, *bsum;
    size_t total;
};
static inline TpKeepWs tp_keep_carve(void* ws, int64_t F, int64_t V) {
    WsWalk w(ws);
    TpKeepWs L;
    L.fflag = w.take<int>((size_t)(F + 1));
    L.foff = w.take<int>((size_t)(F + 1));
    L.vflag = w.take<int>((size_t)(V + 1));
    L.voff = w.take<int>((size_t)(V + 1));
    L.bsum = w.take<int>((size_t)scan_scratch_ints(std::max(F, V) + 1));
    L.total = w.bytes();
    return L;
}

static int tp_sizes(const char* who, int64_t F, int64_t V) {
    LS_REQUIRE(F >= 0 && V >= 0, LS_E_INVALID, "%s: a negative size", who);
    const int64_t lim = (int64_t)1 << 31;
    LS_REQUIRE(F < lim && 3 * F < lim, LS_E_OVERFLOW, "%s: 3 x the number of faces reaches 2^31", who);
    LS_REQUIRE(V < lim, LS_E_OVERFLOW, "%s: the number of vertices reaches 2^31", who);
    return LS_OK;
}

static inline int tp_rounds(int64_t n) {        // ceil(log2 n)
    int r = 0;
    while (((int64_t)1 << r) < n) ++r;
    return r;
}

// comp[i] = the number of item i's component; parent: the hooked forest over n items. *total (device) = off[n]
static int tp_label(const int* parent, int64_t n, const TpWs& L, int* comp, hipStream_t st) {
    hipLaunchKernelGGL(k_tp_compress, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, parent, n, L.label, L.flag);
    if (int rc = exclusive_scan(L.flag, n, L.off, L.sort.bsum, st)) return rc;
    hipLaunchKernelGGL(k_tp_number, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, (const int*)L.label, (const int*)L.off, n, comp);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace ls

using namespace ls;

extern "C" int ls_topo_workspace_bytes(int64_t F, int64_t V, size_t* bytes) {
    LS_REQUIRE(bytes, LS_E_INVALID, "ls_topo_workspace_bytes: null argument");
    if (int rc = tp_sizes("ls_topo_workspace_bytes", F, V)) return rc;
    *bytes = tp_carve(nullptr, F, V).total;
    return LS_OK;
}

extern "C" int ls_topo_keep_workspace_bytes(int64_t F, int64_t V, size_t* bytes) {
    LS_REQUIRE(bytes, LS_E_INVALID, "ls_topo_keep_workspace_bytes: null argument");
    if (int rc = tp_sizes("ls_topo_keep_workspace_bytes", F, V)) return rc;
    *bytes = tp_keep_carve(nullptr, F, V).total;
    return LS_OK;
}

extern "C" int ls_topo_build(const void* faces, int idx_bytes, int64_t F, int64_t V, int32_t* tri, int32_t* vcomp, int32_t* fcomp, int32_t* edges,
                             int32_t* edge_faces, unsigned char* eflag, int32_t* corder, int32_t* forder, int32_t* fseg, int32_t* loops,
                             int32_t* loop_ptr, int64_t* h_sizes, int* h_status, void* ws, size_t ws_bytes, int device, void* stream) {
    const char* who = "ls_topo_build";
    LS_REQUIRE(h_sizes && h_status && loop_ptr && ws && (idx_bytes == 4 || idx_bytes == 8), LS_E_INVALID,
               "%s: null argument, or faces that are neither int32 nor int64", who);
    if (int rc = tp_sizes(who, F, V)) return rc;
    LS_REQUIRE((V == 0 || (vcomp && loops)) && (F == 0 || (faces && tri && fcomp && edges && edge_faces && eflag && corder && forder && fseg)),
               LS_E_INVALID, "%s: null argument", who);
    const TpWs L = tp_carve(ws, F, V);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = 3 * F;
    for (int i = 0; i < LS_TOPO_SIZES; ++i) h_sizes[i] = 0;
    *h_status = 0;
    // status[0]: the flags, status[1]: a bad index; totals: boundary, non-manifold and misoriented edges
    LS_HIP(hipMemsetAsync(L.status, 0, sizeof(int) * 4, st));
    LS_HIP(hipMemsetAsync(L.totals, 0, sizeof(int) * 4, st));
    LS_HIP(hipMemsetAsync(loop_ptr, 0, sizeof(int), st));
    int E = 0, KV = 0, KF = 0, B = 0, NL = 0;
    int totals[4] = {0, 0, 0, 0};
    if (V) {
        hipLaunchKernelGGL(k_tp_iota, dim3(div_up(V, BLOCK)), dim3(BLOCK), 0, st, L.vpar, V);
        LS_HIP(hipMemsetAsync(L.bout, 0, sizeof(int) * (size_t)V, st));
        LS_HIP(hipMemsetAsync(L.bin, 0, sizeof(int) * (size_t)V, st));
        LS_HIP(hipMemsetAsync(L.nextv, 0, sizeof(int) * (size_t)V, st));
    }
    if (n) {
        // the indices as int32 (an index outside [0, V) is stored as 0 and flagged: nothing below follows a bad index; V = 0 flags all)
        LS_IDX(idx_bytes, hipLaunchKernelGGL((k_faces_in<IDX, 0>), dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, (const IDX*)faces, n, V,
                                             (int*)tri, L.status + 1));
        LS_HIP(hipGetLastError());
    }
    if (n && V) {
        hipLaunchKernelGGL(k_tp_hook_vertices, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, (const int*)tri, n, L.vpar, L.status);
        hipLaunchKernelGGL(k_tp_iota, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, L.fpar, F);
        LS_HIP(hipGetLastError());
        // the half-edges sorted stably by (smaller end, larger end); the census of the runs hooks the faces
        const KeyEdge key{(const int*)tri};
        const int* sorted = nullptr;
        if (int rc = radix_argsort_words(key, n, 2, L.ord_a, L.sort, st, &sorted, 4)) return rc;
        hipLaunchKernelGGL(k_tp_census, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, key, sorted, n, L.own, L.mate, L.hflag, L.fpar);
        LS_HIP(hipGetLastError());
        if (int rc = exclusive_scan(L.own, n, L.eoff, L.sort.bsum, st)) return rc;
        hipLaunchKernelGGL(k_tp_edges, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, (const int*)tri, (const int*)L.own, (const int*)L.mate,
                           (const int*)L.hflag, (const int*)L.eoff, n, (int*)edges, (int*)edge_faces, eflag, L.bout, L.bin, L.nextv, L.totals);
        LS_HIP(hipGetLastError());
        LS_HIP(hipMemcpyAsync(&E, L.eoff + n, sizeof(int), hipMemcpyDeviceToHost, st));
        // the facet components, and the faces grouped by them (keys < F: no face is without a group)
        if (int rc = tp_label(L.fpar, F, L, (int*)fcomp, st)) return rc;
        LS_HIP(hipMemcpyAsync(&KF, L.off + F, sizeof(int), hipMemcpyDeviceToHost, st));
        if (int rc = group_by_key<true>((const int*)fcomp, F, F, (int*)forder, (int*)fseg, L.fsort, st)) return rc;
        // the corners sorted stably by vertex
        const int* src = nullptr;
        if (int rc = radix_argsort(KeyInt{(const int*)tri}, n, radix_passes(V - 1), (int*)corder, L.sort, st, &src)) return rc;
        if (src != corder) LS_HIP(hipMemcpyAsync(corder, src, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
    }
    if (V) {
        if (int rc = tp_label(L.vpar, V, L, (int*)vcomp, st)) return rc;
        LS_HIP(hipMemcpyAsync(&KV, L.off + V, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (n && V) {
        // the boundary vertices compacted, doubled to their cycle's lowest member, cut there, ranked, and placed
        const int grid = div_up(V, BLOCK), rounds = tp_rounds(std::min(V, n));
        hipLaunchKernelGGL(k_tp_bflags, dim3(grid), dim3(BLOCK), 0, st, (const int*)L.bout, (const int*)L.bin, V, L.bfl, L.status);
        LS_HIP(hipGetLastError());
        if (int rc = exclusive_scan(L.bfl, V, L.cidx, L.sort.bsum, st)) return rc;
        const int* pB = L.cidx + V;
        hipLaunchKernelGGL(k_tp_bcompact, dim3(grid), dim3(BLOCK), 0, st, (const int*)L.bfl, (const int*)L.cidx, (const int*)L.nextv, V, L.vid,
                           L.nx[0], L.mn[0]);
        int a = 0;                                   // nx[0] stays the successor; nx[1 + a], mn[a] are the doubled ones
        hipLaunchKernelGGL(k_tp_double_min, dim3(grid), dim3(BLOCK), 0, st, pB, (const int*)L.nx[0], (const int*)L.mn[0], L.nx[1], L.mn[1]);
        a = 1;                                       // (one round even for B = 1: mn[1] is written)
        for (int r = 1; r < rounds; ++r) {
            // nx[0] must survive: the doubled successors alternate between nx[1] and nx[2]
            hipLaunchKernelGGL(k_tp_double_min, dim3(grid), dim3(BLOCK), 0, st, pB, (const int*)L.nx[1 + (r - 1) % 2], (const int*)L.mn[a],
                               L.nx[1 + r % 2], L.mn[1 - a]);
            a = 1 - a;
        }
        const int* mn = L.mn[a];
        hipLaunchKernelGGL(k_tp_cut, dim3(grid), dim3(BLOCK), 0, st, pB, (const int*)L.nx[0], mn, L.nx[1], L.d[0]);
        int b = 0;
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(k_tp_double_rank, dim3(grid), dim3(BLOCK), 0, st, pB, (const int*)L.nx[1 + r % 2], (const int*)L.d[b],
                               L.nx[1 + (r + 1) % 2], L.d[1 - b]);
            b = 1 - b;
        }
        const int* d = L.d[b];
        hipLaunchKernelGGL(k_tp_heads, dim3(grid), dim3(BLOCK), 0, st, pB, mn, d, V, L.len, L.head);
        LS_HIP(hipGetLastError());
        if (int rc = exclusive_scan(L.len, V, L.start, L.sort.bsum, st)) return rc;
        if (int rc = exclusive_scan(L.head, V, L.hoff, L.sort.bsum, st)) return rc;
        hipLaunchKernelGGL(k_tp_loops, dim3(grid), dim3(BLOCK), 0, st, pB, mn, d, (const int*)L.vid, (const int*)L.start, (const int*)L.hoff,
                           (int*)loops, (int*)loop_ptr);
        LS_HIP(hipGetLastError());
        LS_HIP(hipMemcpyAsync(&B, pB, sizeof(int), hipMemcpyDeviceToHost, st));
        LS_HIP(hipMemcpyAsync(&NL, L.hoff + V, sizeof(int), hipMemcpyDeviceToHost, st));
        LS_HIP(hipMemcpyAsync(totals, L.totals, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    }
    int status[2] = {0, 0};
    LS_HIP(hipMemcpyAsync(status, L.status, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    LS_HIP(hipStreamSynchronize(st));
    h_sizes[0] = E; h_sizes[1] = KV; h_sizes[2] = KF; h_sizes[3] = B; h_sizes[4] = NL;
    h_sizes[5] = totals[0]; h_sizes[6] = totals[1]; h_sizes[7] = totals[2];
    *h_status = status[0] | (status[1] ? LS_TOPO_BAD_INDEX : 0);
    return LS_OK;
}

extern "C" int ls_topo_counts(const int32_t* tri, const int32_t* fcomp, const int32_t* edge_faces, const unsigned char* eflag, const int32_t* corder,
                              int64_t F, int64_t E, int64_t K, int64_t* counts, int device, void* stream) {
    const char* who = "ls_topo_counts";
    if (int rc = tp_sizes(who, F, 0)) return rc;
    LS_REQUIRE(E >= 0 && E <= 3 * F && K >= 0 && K <= F, LS_E_INVALID, "%s: more edges than half-edges, or more components than faces", who);
    if (K == 0) return LS_OK;
    LS_REQUIRE(tri && fcomp && corder && counts && (E == 0 || (edge_faces && eflag)), LS_E_INVALID, "%s: null argument", who);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    unsigned long long* table = (unsigned long long*)counts;
    LS_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * 6 * (size_t)K, st));
    hipLaunchKernelGGL(k_tp_count_faces, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, fcomp, F, table);
    if (E) hipLaunchKernelGGL(k_tp_count_edges, dim3(div_up(E, BLOCK)), dim3(BLOCK), 0, st, fcomp, edge_faces, eflag, E, table);
    hipLaunchKernelGGL(k_tp_count_vertices, dim3(div_up(3 * F, BLOCK)), dim3(BLOCK), 0, st, tri, fcomp, corder, 3 * F, table);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_topo_measures(const float* verts, const int32_t* tri, const int32_t* forder, const int32_t* fseg, int64_t F, int64_t V, int64_t K,
                                double* terms, double* out, int device, void* stream) {
    const char* who = "ls_topo_measures";
    if (int rc = tp_sizes(who, F, V)) return rc;
    LS_REQUIRE(K >= 0 && K <= F, LS_E_INVALID, "%s: more components than faces", who);
    if (K == 0) return LS_OK;
    LS_REQUIRE(verts && tri && forder && fseg && terms && out && V > 0, LS_E_INVALID, "%s: null argument", who);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tp_terms, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, verts, tri, F, terms);
    hipLaunchKernelGGL(k_tp_measure, dim3(div_up(K, 256)), dim3(256), 0, st, K, TpMeasure{terms, forder, fseg, out});
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_topo_keep(const int32_t* tri, const int32_t* fcomp, const unsigned char* mask, int64_t F, int64_t V, int64_t K, int idx_bytes,
                            int64_t cap_faces, int64_t cap_vertices, void* faces_out, void* I, void* J, int64_t* sizes, void* ws, size_t ws_bytes,
                            int device, void* stream) {
    const char* who = "ls_topo_keep";
    if (int rc = tp_sizes(who, F, V)) return rc;
    LS_REQUIRE((idx_bytes == 4 || idx_bytes == 8) && K >= 0 && K <= F && cap_faces >= 0 && cap_vertices >= 0 && sizes && ws, LS_E_INVALID,
               "%s: null argument, a negative size, more components than faces, or an index type that is neither int32 nor int64", who);
    LS_REQUIRE((F == 0 || (tri && fcomp && mask && V > 0)) && (V == 0 || I) && (cap_faces == 0 || faces_out) && (cap_vertices == 0 || J),
               LS_E_INVALID, "%s: null argument", who);
    const TpKeepWs L = tp_keep_carve(ws, F, V);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    DeviceGuard guard(device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    LS_HIP(hipMemsetAsync(L.vflag, 0, sizeof(int) * (size_t)(V + 1), st));
    if (F) hipLaunchKernelGGL(k_tp_keep_flags, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, tri, fcomp, mask, F, L.fflag, L.vflag);
    if (int rc = exclusive_scan(L.fflag, F, L.foff, L.bsum, st)) return rc;
    if (int rc = exclusive_scan(L.vflag, V, L.voff, L.bsum, st)) return rc;
    if (F) LS_IDX(idx_bytes, hipLaunchKernelGGL(k_tp_keep_faces<IDX>, dim3(div_up(F, BLOCK)), dim3(BLOCK), 0, st, tri, (const int*)L.fflag,
                                                (const int*)L.foff, (const int*)L.voff, F, cap_faces, (IDX*)faces_out));
    LS_IDX(idx_bytes, hipLaunchKernelGGL(k_tp_keep_vertices<IDX>, dim3(div_up(std::max<int64_t>(V, 1), BLOCK)), dim3(BLOCK), 0, st, (const int*)L.vflag,
                                         (const int*)L.voff, (const int*)L.foff, F, V, cap_vertices, (IDX*)I, (IDX*)J, sizes));
    LS_HIP(hipGetLastError());
    return LS_OK;
}
