// remesh.hip -- Botsch-Kobbelt isotropic remeshing on the device (gfx950, wave64): split -> collapse -> flip -> relax -> project.
//
// The reference's loop calls remesh_botsch(v, f, 5, h, True) of an external CPU build (scripts/main.py:149). This is the same
// algorithm in fp32, run in ROUNDS: each round rebuilds the tables from the face list, chooses a conflict-free set of operations,
// applies it and compacts. DESIGN.md ("Isotropic remeshing") states the rules; tests/remesh_statement.py is their numpy statement,
// operation for operation (fp32 lengths as (dx dx + dy dy) + dz dz, the library builds with -ffp-contract=off).
//
// Tables of one round (int32; F faces, V vertices; half-edge h = 3 f + k runs faces[h] -> faces[3 f + (k + 1) % 3]):
//   cnt / vptr / vcorner   the corners of each vertex (= its outgoing half-edges), ascending corner id (atomic fill, then an
//                          insertion sort per vertex: the order never depends on the schedule)
//   twin                   the opposite half-edge or -1 (boundary); edge id = min(h, twin)
//   bnd                    1 for a vertex with a boundary half-edge; valence = cnt + bnd
// Winners of collapse / flip: a 64-bit key (value bits << 32 | edge id) min-propagated with integer atomicMin (order independent).
// Projection: the LBVH of lbvh.h over the call's input triangles (boxes inflated by 1e-5 of the box diagonal) walked stacklessly
// through escape links; the point-triangle test is fp64 and ties of the squared distance go to the lower triangle id, so the BVH
// answers what a brute-force scan answers.
#include "common.h"
#include "lbvh.h"
#include "meshface.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace ls {

typedef unsigned long long u64;
constexpr u64 RM_INF = ~0ull;
constexpr int RM_SPLIT_ROUNDS = 8, RM_COLLAPSE_ROUNDS = 64, RM_FLIP_ROUNDS = 64;

__device__ __forceinline__ float3 rm_ld(const float* __restrict__ P, int v) { return make_float3(P[3 * (size_t)v], P[3 * (size_t)v + 1], P[3 * (size_t)v + 2]); }
__device__ __forceinline__ void rm_st(float* __restrict__ P, int v, float3 p) { P[3 * (size_t)v] = p.x; P[3 * (size_t)v + 1] = p.y; P[3 * (size_t)v + 2] = p.z; }
__device__ __forceinline__ float rm_len2(float3 a, float3 b) {          // b - a, as the statement's len2
    const float x = b.x - a.x, y = b.y - a.y, z = b.z - a.z;
    return (x * x + y * y) + z * z;
}
__device__ __forceinline__ float3 rm_mid(float3 a, float3 b) { return make_float3((a.x + b.x) * 0.5f, (a.y + b.y) * 0.5f, (a.z + b.z) * 0.5f); }
__device__ __forceinline__ float3 rm_normal(float3 p0, float3 p1, float3 p2) {
    const float3 e1 = make_float3(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z), e2 = make_float3(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z);
    return make_float3(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
}
__device__ __forceinline__ float rm_dot(float3 a, float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ int rm_next(int h) { return 3 * (h / 3) + (h % 3 + 1) % 3; }
__device__ __forceinline__ int rm_prev(int h) { return 3 * (h / 3) + (h % 3 + 2) % 3; }

// ---- input ---------------------------------------------------------------------------------------------------------------------
template <typename IDX>
__global__ __launch_bounds__(BLOCK) void k_rm_faces_out(const int* __restrict__ in, int64_t n, IDX* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = (IDX)in[i];
}

// ---- tables of one round -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_rm_count(const int* __restrict__ faces, int n, int* __restrict__ cnt) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c < n) atomicAdd(&cnt[faces[c]], 1);
}
__global__ __launch_bounds__(BLOCK) void k_rm_fill(const int* __restrict__ faces, int n, const int* __restrict__ vptr, int* __restrict__ cursor,
                                                   int* __restrict__ vcorner) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c < n) { const int v = faces[c]; vcorner[vptr[v] + atomicAdd(&cursor[v], 1)] = c; }
}
__global__ __launch_bounds__(BLOCK) void k_rm_sort(const int* __restrict__ vptr, int V, int* __restrict__ vcorner) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int e0 = vptr[v], e1 = vptr[v + 1];
    for (int i = e0 + 1; i < e1; ++i) {
        const int x = vcorner[i];
        int j = i - 1;
        while (j >= e0 && vcorner[j] > x) { vcorner[j + 1] = vcorner[j]; --j; }
        vcorner[j + 1] = x;
    }
}
// twin of every half-edge; bad[1]: a half-edge a -> b that is not the only one of its direction, or that has two opposites;
// bad[2]: a face that repeats a vertex
__global__ __launch_bounds__(BLOCK) void k_rm_twin(const int* __restrict__ faces, int n, const int* __restrict__ vptr, const int* __restrict__ vcorner,
                                                   int* __restrict__ twin, int* __restrict__ bad) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int a = faces[h], b = faces[rm_next(h)];
    if (a == b) atomicOr(&bad[2], 1);
    int t = -1, nt = 0, same = 0;
    for (int e = vptr[b]; e < vptr[b + 1]; ++e) {
        const int c = vcorner[e];
        if (faces[rm_next(c)] == a) { t = c; ++nt; }
    }
    for (int e = vptr[a]; e < vptr[a + 1]; ++e) same += faces[rm_next(vcorner[e])] == b;
    if (nt > 1 || same != 1) atomicOr(&bad[1], 1);
    twin[h] = nt == 1 ? t : -1;
}
// boundary flags; VALIDATE: bad[3] = a vertex whose faces form more than one fan (walk next = twin(prev(c)) from its boundary
// corner, or its first corner, and count the corners met)
template <bool VALIDATE>
__global__ __launch_bounds__(BLOCK) void k_rm_vflags(const int* __restrict__ vptr, const int* __restrict__ vcorner, const int* __restrict__ twin, int V,
                                                     int* __restrict__ bnd, int* __restrict__ bad) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int e0 = vptr[v], e1 = vptr[v + 1];
    int nb = 0, start = e1 > e0 ? vcorner[e0] : -1;
    for (int e = e0; e < e1; ++e)
        if (twin[vcorner[e]] < 0) { ++nb; start = vcorner[e]; }
    bnd[v] = nb > 0;
    if (!VALIDATE || e1 == e0) return;
    if (nb > 1) { atomicOr(&bad[3], 1); return; }
    int cur = start, steps = 0;
    for (int s = 0; s <= e1 - e0; ++s) {
        ++steps;
        const int nx = twin[rm_prev(cur)];
        if (nx < 0 || nx == start) break;
        cur = nx;
    }
    if (steps != e1 - e0) atomicOr(&bad[3], 1);
}

// ---- split ---------------------------------------------------------------------------------------------------------------------
// a face with a locked (boundary) edge longer than hi keeps its interior edges: splitting them would only cut slivers off it
__device__ __forceinline__ bool rm_held(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ twin, int f, float hi2) {
    for (int k = 0; k < 3; ++k) {
        const int h = 3 * f + k;
        if (twin[h] < 0 && rm_len2(rm_ld(P, faces[h]), rm_ld(P, faces[rm_next(h)])) > hi2) return true;
    }
    return false;
}
__global__ __launch_bounds__(BLOCK) void k_rm_split_mark(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ twin, int n,
                                                         float hi2, int* __restrict__ flag) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int t = twin[h];
    flag[h] = t > h && rm_len2(rm_ld(P, faces[h]), rm_ld(P, faces[rm_next(h)])) > hi2 && !rm_held(P, faces, twin, h / 3, hi2) &&
              !rm_held(P, faces, twin, t / 3, hi2);
}
__device__ __forceinline__ int rm_mid_id(const int* __restrict__ twin, const int* __restrict__ flag, const int* __restrict__ scan, int V, int h) {
    const int t = twin[h];
    if (t < 0) return -1;
    const int e = min(h, t);
    return flag[e] ? V + scan[e] : -1;
}
__global__ __launch_bounds__(BLOCK) void k_rm_split_count(const int* __restrict__ twin, const int* __restrict__ flag, int F, int* __restrict__ fcnt) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int m = 0;
    for (int k = 0; k < 3; ++k) {
        const int h = 3 * f + k, t = twin[h];
        m += t >= 0 && flag[min(h, t)];
    }
    fcnt[f] = 1 + m;
}
__global__ __launch_bounds__(BLOCK) void k_rm_split_verts(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ flag,
                                                          const int* __restrict__ scan, int n, int V, float* __restrict__ Pn) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n || !flag[h]) return;
    rm_st(Pn, V + scan[h], rm_mid(rm_ld(P, faces[h]), rm_ld(P, faces[rm_next(h)])));
}
__device__ __forceinline__ void rm_put(int* __restrict__ out, int& o, int x, int y, int z) { out[3 * o] = x; out[3 * o + 1] = y; out[3 * o + 2] = z; ++o; }
// the face patterns of tests/remesh_statement.py:split_face
__global__ __launch_bounds__(BLOCK) void k_rm_split_faces(const float* __restrict__ Pn, const int* __restrict__ faces, const int* __restrict__ twin,
                                                          const int* __restrict__ flag, const int* __restrict__ scan, const int* __restrict__ foff, int F,
                                                          int V, int* __restrict__ out) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3], m[3], nm = 0;
    for (int k = 0; k < 3; ++k) { v[k] = faces[3 * f + k]; m[k] = rm_mid_id(twin, flag, scan, V, 3 * f + k); nm += m[k] >= 0; }
    int o = foff[f];
    if (nm == 0) rm_put(out, o, v[0], v[1], v[2]);
    else if (nm == 3) {
        rm_put(out, o, v[0], m[0], m[2]); rm_put(out, o, m[0], v[1], m[1]); rm_put(out, o, m[2], m[1], v[2]); rm_put(out, o, m[0], m[1], m[2]);
    } else if (nm == 1) {
        const int k = m[0] >= 0 ? 0 : m[1] >= 0 ? 1 : 2;
        const int a = v[k], b = v[(k + 1) % 3], c = v[(k + 2) % 3];
        rm_put(out, o, a, m[k], c); rm_put(out, o, m[k], b, c);
    } else {
        const int k = m[0] < 0 ? 0 : m[1] < 0 ? 1 : 2;     // the unmarked edge a -> b
        const int a = v[k], b = v[(k + 1) % 3], c = v[(k + 2) % 3], mb = m[(k + 1) % 3], mc = m[(k + 2) % 3];
        const float da = rm_len2(rm_ld(Pn, a), rm_ld(Pn, mb)), db = rm_len2(rm_ld(Pn, b), rm_ld(Pn, mc));
        rm_put(out, o, mc, mb, c);
        if (da <= db) { rm_put(out, o, a, b, mb); rm_put(out, o, a, mb, mc); }
        else { rm_put(out, o, a, b, mc); rm_put(out, o, b, mb, mc); }
    }
}

// ---- collapse ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_rm_collapse_cand(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ twin,
                                                            const int* __restrict__ vptr, const int* __restrict__ vcorner, const int* __restrict__ bnd,
                                                            int n, float lo2, float hi2, u64* __restrict__ key) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    key[h] = RM_INF;
    const int t = twin[h];
    if (t <= h) return;
    const int a = faces[h], b = faces[rm_next(h)];
    if (bnd[a] || bnd[b]) return;
    const float3 pa = rm_ld(P, a), pb = rm_ld(P, b);
    const float L = rm_len2(pa, pb);
    if (!(L < lo2)) return;
    const int a0 = vptr[a], a1 = vptr[a + 1], b0 = vptr[b], b1 = vptr[b + 1];
    if (a1 - a0 < 4 || b1 - b0 < 4) return;                      // interior: valence = corner count
    int common = 0;
    for (int i = a0; i < a1; ++i) {
        const int x = faces[rm_next(vcorner[i])];
        for (int j = b0; j < b1; ++j) {
            if (faces[rm_next(vcorner[j])] == x) {
                ++common;
                if (vptr[x + 1] - vptr[x] + bnd[x] - 1 < 3) return;
            }
        }
    }
    if (common != 2) return;
    const float3 p = rm_mid(pa, pb);
    for (int s = 0; s < 2; ++s) {
        const int e0 = s ? b0 : a0, e1 = s ? b1 : a1;
        for (int i = e0; i < e1; ++i) {
            const int w = faces[rm_next(vcorner[i])];
            if (w != a && w != b && rm_len2(p, rm_ld(P, w)) > hi2) return;
        }
    }
    for (int s = 0; s < 2; ++s) {
        const int e0 = s ? b0 : a0, e1 = s ? b1 : a1;
        for (int i = e0; i < e1; ++i) {
            const int c = vcorner[i], f = c / 3, slot = c % 3;
            const int f0 = faces[3 * f], f1 = faces[3 * f + 1], f2 = faces[3 * f + 2];
            const bool ha = f0 == a || f1 == a || f2 == a, hb = f0 == b || f1 == b || f2 == b;
            if (ha && hb) continue;
            float3 q[3] = {rm_ld(P, f0), rm_ld(P, f1), rm_ld(P, f2)};
            const float3 n0 = rm_normal(q[0], q[1], q[2]);
            q[slot] = p;
            if (rm_dot(n0, rm_normal(q[0], q[1], q[2])) <= 0.0f) return;
        }
    }
    key[h] = ((u64)__float_as_uint(L) << 32) | (u64)(unsigned)h;
}
// m[x] = min(m[x], key) for the endpoints of every live key (collapse: 2, flip: 4 vertices)
__global__ __launch_bounds__(BLOCK) void k_rm_key_scatter(const int* __restrict__ faces, const int* __restrict__ twin, const u64* __restrict__ key, int n,
                                                          int four, u64* __restrict__ m) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n || key[h] == RM_INF) return;
    const u64 k = key[h];
    atomicMin(&m[faces[h]], k);
    atomicMin(&m[faces[rm_next(h)]], k);
    if (four) { atomicMin(&m[faces[rm_prev(h)]], k); atomicMin(&m[faces[rm_prev(twin[h])]], k); }
}
// dst[v] = min over v and its edge neighbours of src (dst holds a copy of src on entry)
__global__ __launch_bounds__(BLOCK) void k_rm_ring_min(const int* __restrict__ faces, int n, const u64* __restrict__ src, u64* __restrict__ dst) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int a = faces[h], b = faces[rm_next(h)];
    const u64 ka = src[a], kb = src[b];
    if (ka != RM_INF) atomicMin(&dst[b], ka);
    if (kb != RM_INF) atomicMin(&dst[a], kb);
}
__global__ __launch_bounds__(BLOCK) void k_rm_winners(const int* __restrict__ faces, const int* __restrict__ twin, const u64* __restrict__ key, int n,
                                                      int four, const u64* __restrict__ m, int* __restrict__ win, int* __restrict__ count) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const u64 k = key[h];
    bool w = k != RM_INF && m[faces[h]] == k && m[faces[rm_next(h)]] == k;
    if (w && four) w = m[faces[rm_prev(h)]] == k && m[faces[rm_prev(twin[h])]] == k;
    win[h] = w;
    if (w) atomicAdd(count, 1);
}
// a winner (a, b) keeps min(a, b) at the midpoint, drops max(a, b) and its two faces
__global__ __launch_bounds__(BLOCK) void k_rm_collapse_apply(float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ twin,
                                                             const int* __restrict__ win, int n, int* __restrict__ remap, int* __restrict__ vkeep,
                                                             int* __restrict__ fkeep) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n || !win[h]) return;
    const int a = faces[h], b = faces[rm_next(h)], keep = min(a, b), gone = max(a, b);
    rm_st(P, keep, rm_mid(rm_ld(P, a), rm_ld(P, b)));
    remap[gone] = keep;
    vkeep[gone] = 0;
    fkeep[h / 3] = 0;
    fkeep[twin[h] / 3] = 0;
}
__global__ __launch_bounds__(BLOCK) void k_rm_iota(int* __restrict__ x, int n) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) x[i] = i;
}
__global__ __launch_bounds__(BLOCK) void k_rm_fill_int(int* __restrict__ x, int n, int val) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) x[i] = val;
}
__global__ __launch_bounds__(BLOCK) void k_rm_compact_verts(const float* __restrict__ P, const int* __restrict__ vkeep, const int* __restrict__ vscan, int V,
                                                            float* __restrict__ Pn) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v < V && vkeep[v]) rm_st(Pn, vscan[v], rm_ld(P, v));
}
__global__ __launch_bounds__(BLOCK) void k_rm_compact_faces(const int* __restrict__ faces, const int* __restrict__ fkeep, const int* __restrict__ fscan,
                                                            const int* __restrict__ remap, const int* __restrict__ vscan, int F, int* __restrict__ out) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F || !fkeep[f]) return;
    const int o = fscan[f];
    for (int k = 0; k < 3; ++k) out[3 * o + k] = vscan[remap[faces[3 * f + k]]];
}
__global__ __launch_bounds__(BLOCK) void k_rm_used(const int* __restrict__ vptr, int V, int* __restrict__ used) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v < V) used[v] = vptr[v + 1] > vptr[v];
}

// ---- flip ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool rm_has_edge(const int* __restrict__ faces, const int* __restrict__ vptr, const int* __restrict__ vcorner, int c, int d) {
    for (int e = vptr[c]; e < vptr[c + 1]; ++e) if (faces[rm_next(vcorner[e])] == d) return true;
    for (int e = vptr[d]; e < vptr[d + 1]; ++e) if (faces[rm_next(vcorner[e])] == c) return true;
    return false;
}
__global__ __launch_bounds__(BLOCK) void k_rm_flip_cand(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ twin,
                                                        const int* __restrict__ vptr, const int* __restrict__ vcorner, const int* __restrict__ bnd, int n,
                                                        u64* __restrict__ key) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    key[h] = RM_INF;
    const int t = twin[h];
    if (t <= h) return;
    const int a = faces[h], b = faces[rm_next(h)], c = faces[rm_prev(h)], d = faces[rm_prev(t)];
    const int va = vptr[a + 1] - vptr[a] + bnd[a], vb = vptr[b + 1] - vptr[b] + bnd[b];
    const int vc = vptr[c + 1] - vptr[c] + bnd[c], vd = vptr[d + 1] - vptr[d] + bnd[d];
    const int ta = bnd[a] ? 4 : 6, tb = bnd[b] ? 4 : 6, tc = bnd[c] ? 4 : 6, td = bnd[d] ? 4 : 6;
    const int before = (abs(va - ta) + abs(vb - tb)) + (abs(vc - tc) + abs(vd - td));
    const int after = (abs(va - 1 - ta) + abs(vb - 1 - tb)) + (abs(vc + 1 - tc) + abs(vd + 1 - td));
    const int gain = before - after;
    if (gain <= 0 || va - 1 < 3 || vb - 1 < 3 || c == d) return;
    if (rm_has_edge(faces, vptr, vcorner, c, d)) return;
    const int f = h / 3, g = t / 3;
    const float3 nf = rm_normal(rm_ld(P, faces[3 * f]), rm_ld(P, faces[3 * f + 1]), rm_ld(P, faces[3 * f + 2]));
    const float3 ng = rm_normal(rm_ld(P, faces[3 * g]), rm_ld(P, faces[3 * g + 1]), rm_ld(P, faces[3 * g + 2]));
    const float3 pa = rm_ld(P, a), pb = rm_ld(P, b), pc = rm_ld(P, c), pd = rm_ld(P, d);
    const float3 n1 = rm_normal(pc, pa, pd), n2 = rm_normal(pd, pb, pc);
    if (!(rm_dot(n1, nf) > 0.0f) || !(rm_dot(n1, ng) > 0.0f) || !(rm_dot(n2, nf) > 0.0f) || !(rm_dot(n2, ng) > 0.0f)) return;
    key[h] = ((u64)(unsigned)(4 - gain) << 32) | (u64)(unsigned)h;
}
__global__ __launch_bounds__(BLOCK) void k_rm_flip_apply(int* __restrict__ faces, const int* __restrict__ twin, const int* __restrict__ win, int n) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n || !win[h]) return;
    const int t = twin[h];
    const int a = faces[h], b = faces[rm_next(h)], c = faces[rm_prev(h)], d = faces[rm_prev(t)];
    const int f = h / 3, g = t / 3;
    faces[3 * f] = c; faces[3 * f + 1] = a; faces[3 * f + 2] = d;
    faces[3 * g] = d; faces[3 * g + 1] = b; faces[3 * g + 2] = c;
}

// ---- relax ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_rm_relax(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ vptr,
                                                    const int* __restrict__ vcorner, const int* __restrict__ bnd, int V, float* __restrict__ Pn) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const float3 p = rm_ld(P, v);
    const int e0 = vptr[v], e1 = vptr[v + 1];
    if (bnd[v] || e1 == e0) { rm_st(Pn, v, p); return; }
    float3 q = make_float3(0.0f, 0.0f, 0.0f), nn = make_float3(0.0f, 0.0f, 0.0f);
    for (int e = e0; e < e1; ++e) {
        const int c = vcorner[e], f = c / 3;
        const float3 w = rm_ld(P, faces[rm_next(c)]);
        q.x = q.x + w.x; q.y = q.y + w.y; q.z = q.z + w.z;
        const float3 nf = rm_normal(rm_ld(P, faces[3 * f]), rm_ld(P, faces[3 * f + 1]), rm_ld(P, faces[3 * f + 2]));
        nn.x = nn.x + nf.x; nn.y = nn.y + nf.y; nn.z = nn.z + nf.z;
    }
    const float deg = (float)(e1 - e0);
    q.x = q.x / deg; q.y = q.y / deg; q.z = q.z / deg;
    const float nl = sqrtf((nn.x * nn.x + nn.y * nn.y) + nn.z * nn.z);
    if (!(nl > 0.0f)) { rm_st(Pn, v, q); return; }
    const float3 u = make_float3(nn.x / nl, nn.y / nl, nn.z / nl);
    const float3 r = make_float3(p.x - q.x, p.y - q.y, p.z - q.z);
    const float s = (u.x * r.x + u.y * r.y) + u.z * r.z;
    rm_st(Pn, v, make_float3(q.x + s * u.x, q.y + s * u.y, q.z + s * u.z));
}

// ---- projection: the LBVH of lbvh.h over the input mesh -----------------------------------------------------------------------
struct RmBest { double d2, r[3]; int tri; };
__device__ __forceinline__ void rm_test_leaf(const float* __restrict__ P0, const int* __restrict__ F0, int f, const double p[3], RmBest& best) {
    double a[3], b[3], c[3], r[3];
    for (int q = 0; q < 3; ++q) { a[q] = P0[3 * (size_t)F0[3 * f] + q]; b[q] = P0[3 * (size_t)F0[3 * f + 1] + q]; c[q] = P0[3 * (size_t)F0[3 * f + 2] + q]; }
    lbvh_point_tri(p, a, b, c, r);
    const double dx = p[0] - r[0], dy = p[1] - r[1], dz = p[2] - r[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < best.d2 || (d2 == best.d2 && f < best.tri)) { best.d2 = d2; best.tri = f; best.r[0] = r[0]; best.r[1] = r[1]; best.r[2] = r[2]; }
}
__device__ __forceinline__ float rm_box_d2(const float* __restrict__ bx, float px, float py, float pz) {
    const float x = fmaxf(fmaxf(bx[0] - px, 0.0f), px - bx[3]);
    const float y = fmaxf(fmaxf(bx[1] - py, 0.0f), py - bx[4]);
    const float z = fmaxf(fmaxf(bx[2] - pz, 0.0f), pz - bx[5]);
    return (x * x + y * y) + z * z;
}
// the projection's query of lbvh_walk: fp32 box distances (boxes inflated by the margin of rm_build_bvh), the fp64 leaf test
struct RmProject {
    const float* __restrict__ P0;
    const int* __restrict__ F0;
    const int* __restrict__ tri;
    const float* __restrict__ box;
    float px, py, pz;
    double p[3];
    RmBest b;
    __device__ __forceinline__ float bound(int node) const { return rm_box_d2(box + 6 * (size_t)node, px, py, pz); }
    __device__ __forceinline__ double best() const { return b.d2; }
    __device__ __forceinline__ void leaf(int i) { rm_test_leaf(P0, F0, tri[i], p, b); }
};
__global__ __launch_bounds__(BLOCK) void k_rm_project(float* __restrict__ P, const int* __restrict__ vptr, const int* __restrict__ bnd, int V,
                                                      const float* __restrict__ P0, const int* __restrict__ F0, int T, const int* __restrict__ tri,
                                                      const float* __restrict__ box, const int* __restrict__ left, const int* __restrict__ right,
                                                      const int* __restrict__ esc) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V || bnd[v] || vptr[v + 1] == vptr[v]) return;
    const float px = P[3 * (size_t)v], py = P[3 * (size_t)v + 1], pz = P[3 * (size_t)v + 2];
    const double p[3] = {px, py, pz};
    RmProject q{P0, F0, tri, box, px, py, pz, {p[0], p[1], p[2]}, {}};
    q.b.d2 = __longlong_as_double(0x7ff0000000000000ll);
    q.b.tri = 0x7fffffff;
    q.b.r[0] = p[0]; q.b.r[1] = p[1]; q.b.r[2] = p[2];
    lbvh_walk(left, right, esc, T, q);
    const RmBest& best = q.b;
    P[3 * (size_t)v] = (float)best.r[0]; P[3 * (size_t)v + 1] = (float)best.r[1]; P[3 * (size_t)v + 2] = (float)best.r[2];
}

// ---- the handle ----------------------------------------------------------------------------------------------------------------
struct RmBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct RemeshHandle {
    int device = 0;
    hipStream_t st = nullptr;
    float h = 0.0f, hi2 = 0.0f, lo2 = 0.0f;
    int project = 0;
    int V = 0, F = 0, V0 = 0, F0 = 0;
    bool bvh = false;
    int64_t counters[6] = {0, 0, 0, 0, 0, 0};
    double seconds[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // mesh (ping-pong), tables of a round, the input mesh and its BVH
    RmBuf pos, pos_b, faces, faces_b, cnt, vptr, cursor, vcorner, twin, bnd, flag, scan, key, mA, mB, remap, vkeep, vscan, fkeep, fscan,
        bsum, small, pos0, faces0, code, ord_a, sort, tri, scode, left, right, parent, esc, rflag, box;
    std::vector<RmBuf*> all() {
        return {&pos, &pos_b, &faces, &faces_b, &cnt, &vptr, &cursor, &vcorner, &twin, &bnd, &flag, &scan, &key, &mA, &mB, &remap, &vkeep,
                &vscan, &fkeep, &fscan, &bsum, &small, &pos0, &faces0, &code, &ord_a, &sort, &tri, &scode, &left, &right,
                &parent, &esc, &rflag, &box};
    }
};

static void rm_free(int device, RmBuf& b) {
    if (b.p && !pool_give(device, b.p, b.cap)) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}
// a buffer of at least `bytes` (the old contents are not kept); the stream is idle whenever this is called (every round ends with
// a synchronisation), so a replaced buffer can go back to the pool
static int rm_ensure(RemeshHandle* H, RmBuf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    if (b.cap >= bytes) return LS_OK;
    rm_free(H->device, b);
    const size_t want = bytes + bytes / 4;         // room for the next rounds' growth
    size_t cap = 0;
    void* p = pool_take(H->device, want, &cap);
    if (!p) { LS_HIP(pool_alloc(H->device, &p, want)); cap = want; }
    b.p = p;
    b.cap = cap;
    return LS_OK;
}
template <typename T> static T* rp(RmBuf& b) { return (T*)b.p; }
#define RM_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)
#define RM_GRID(n) dim3(div_up(std::max<int64_t>((int64_t)(n), 1), BLOCK)), dim3(BLOCK), 0, H->st

static int rm_read_int(RemeshHandle* H, const int* d, int* h) {
    LS_HIP(hipMemcpyAsync(h, d, sizeof(int), hipMemcpyDeviceToHost, H->st));
    LS_HIP(hipStreamSynchronize(H->st));
    return LS_OK;
}

// the tables of the current mesh; VALIDATE: small[1..3] get the manifold flags
template <bool VALIDATE>
static int rm_topo(RemeshHandle* H) {
    const int V = H->V, F = H->F, n = 3 * F;
    RM_TRY(rm_ensure(H, H->cnt, sizeof(int) * (V + 1)));
    RM_TRY(rm_ensure(H, H->vptr, sizeof(int) * (V + 1)));
    RM_TRY(rm_ensure(H, H->cursor, sizeof(int) * (V + 1)));
    RM_TRY(rm_ensure(H, H->vcorner, sizeof(int) * (n + 1)));
    RM_TRY(rm_ensure(H, H->twin, sizeof(int) * (n + 1)));
    RM_TRY(rm_ensure(H, H->bnd, sizeof(int) * (V + 1)));
    RM_TRY(rm_ensure(H, H->bsum, sizeof(int) * scan_scratch_ints(std::max(n, V))));
    LS_HIP(hipMemsetAsync(H->cnt.p, 0, sizeof(int) * (V + 1), H->st));
    LS_HIP(hipMemsetAsync(H->cursor.p, 0, sizeof(int) * (V + 1), H->st));
    const int* fc = rp<int>(H->faces);
    if (n) hipLaunchKernelGGL(k_rm_count, RM_GRID(n), fc, n, rp<int>(H->cnt));
    RM_TRY(exclusive_scan(rp<int>(H->cnt), V, rp<int>(H->vptr), rp<int>(H->bsum), H->st));
    if (n) {
        hipLaunchKernelGGL(k_rm_fill, RM_GRID(n), fc, n, (const int*)rp<int>(H->vptr), rp<int>(H->cursor), rp<int>(H->vcorner));
        hipLaunchKernelGGL(k_rm_sort, RM_GRID(V), (const int*)rp<int>(H->vptr), V, rp<int>(H->vcorner));
        hipLaunchKernelGGL(k_rm_twin, RM_GRID(n), fc, n, (const int*)rp<int>(H->vptr), (const int*)rp<int>(H->vcorner), rp<int>(H->twin),
                           rp<int>(H->small));
    }
    hipLaunchKernelGGL(k_rm_vflags<VALIDATE>, RM_GRID(V), (const int*)rp<int>(H->vptr), (const int*)rp<int>(H->vcorner), (const int*)rp<int>(H->twin),
                       V, rp<int>(H->bnd), rp<int>(H->small));
    LS_HIP(hipGetLastError());
    return LS_OK;
}

static void rm_swap(RmBuf& a, RmBuf& b) { std::swap(a, b); }

static int rm_split_round(RemeshHandle* H, int* ops) {
    RM_TRY(rm_topo<false>(H));
    const int V = H->V, F = H->F, n = 3 * F;
    RM_TRY(rm_ensure(H, H->flag, sizeof(int) * (n + 1)));
    RM_TRY(rm_ensure(H, H->scan, sizeof(int) * (n + 1)));
    hipLaunchKernelGGL(k_rm_split_mark, RM_GRID(n), (const float*)rp<float>(H->pos), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->twin), n,
                       H->hi2, rp<int>(H->flag));
    RM_TRY(exclusive_scan(rp<int>(H->flag), n, rp<int>(H->scan), rp<int>(H->bsum), H->st));
    int m = 0;
    RM_TRY(rm_read_int(H, rp<int>(H->scan) + n, &m));
    *ops = m;
    if (m == 0) return LS_OK;
    LS_REQUIRE((int64_t)V + m < INT32_MAX / 3 && 3 * ((int64_t)F + 2 * (int64_t)m) < INT32_MAX, LS_E_OVERFLOW, "ls_remesh: the mesh outgrows int32 indices");
    const int V2 = V + m, F2 = F + 2 * m;
    RM_TRY(rm_ensure(H, H->fkeep, sizeof(int) * (F + 1)));
    RM_TRY(rm_ensure(H, H->fscan, sizeof(int) * (F + 1)));
    RM_TRY(rm_ensure(H, H->pos_b, sizeof(float) * 3 * V2));
    RM_TRY(rm_ensure(H, H->faces_b, sizeof(int) * 3 * F2));
    hipLaunchKernelGGL(k_rm_split_count, RM_GRID(F), (const int*)rp<int>(H->twin), (const int*)rp<int>(H->flag), F, rp<int>(H->fkeep));
    RM_TRY(exclusive_scan(rp<int>(H->fkeep), F, rp<int>(H->fscan), rp<int>(H->bsum), H->st));
    LS_HIP(hipMemcpyAsync(H->pos_b.p, H->pos.p, sizeof(float) * 3 * V, hipMemcpyDeviceToDevice, H->st));
    hipLaunchKernelGGL(k_rm_split_verts, RM_GRID(n), (const float*)rp<float>(H->pos), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->flag),
                       (const int*)rp<int>(H->scan), n, V, rp<float>(H->pos_b));
    hipLaunchKernelGGL(k_rm_split_faces, RM_GRID(F), (const float*)rp<float>(H->pos_b), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->twin),
                       (const int*)rp<int>(H->flag), (const int*)rp<int>(H->scan), (const int*)rp<int>(H->fscan), F, V, rp<int>(H->faces_b));
    LS_HIP(hipGetLastError());
    rm_swap(H->pos, H->pos_b);
    rm_swap(H->faces, H->faces_b);
    H->V = V2;
    H->F = F2;
    return LS_OK;
}

// winners of the keys in H->key: 2 (collapse) or 4 (flip) endpoints each; H->flag = the winner flags, *ops = their count
static int rm_winners(RemeshHandle* H, bool four, int* ops) {
    const int V = H->V, n = 3 * H->F;
    RM_TRY(rm_ensure(H, H->mA, sizeof(u64) * (V + 1)));
    RM_TRY(rm_ensure(H, H->mB, sizeof(u64) * (V + 1)));
    RM_TRY(rm_ensure(H, H->flag, sizeof(int) * (n + 1)));
    LS_HIP(hipMemsetAsync(H->mA.p, 0xff, sizeof(u64) * V, H->st));
    const int* fc = rp<int>(H->faces);
    hipLaunchKernelGGL(k_rm_key_scatter, RM_GRID(n), fc, (const int*)rp<int>(H->twin), (const u64*)rp<u64>(H->key), n, (int)four, rp<u64>(H->mA));
    if (!four) {                                    // the minimum over distance 2 of either endpoint: two more passes over the edges
        for (int pass = 0; pass < 2; ++pass) {
            LS_HIP(hipMemcpyAsync(H->mB.p, H->mA.p, sizeof(u64) * V, hipMemcpyDeviceToDevice, H->st));
            hipLaunchKernelGGL(k_rm_ring_min, RM_GRID(n), fc, n, (const u64*)rp<u64>(H->mA), rp<u64>(H->mB));
            rm_swap(H->mA, H->mB);
        }
    }
    int* count = rp<int>(H->small) + 8;
    LS_HIP(hipMemsetAsync(count, 0, sizeof(int), H->st));
    hipLaunchKernelGGL(k_rm_winners, RM_GRID(n), fc, (const int*)rp<int>(H->twin), (const u64*)rp<u64>(H->key), n, (int)four, (const u64*)rp<u64>(H->mA),
                       rp<int>(H->flag), count);
    LS_HIP(hipGetLastError());
    return rm_read_int(H, count, ops);
}

static int rm_collapse_round(RemeshHandle* H, int* ops) {
    RM_TRY(rm_topo<false>(H));
    const int V = H->V, F = H->F, n = 3 * F;
    RM_TRY(rm_ensure(H, H->key, sizeof(u64) * (n + 1)));
    hipLaunchKernelGGL(k_rm_collapse_cand, RM_GRID(n), (const float*)rp<float>(H->pos), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->twin),
                       (const int*)rp<int>(H->vptr), (const int*)rp<int>(H->vcorner), (const int*)rp<int>(H->bnd), n, H->lo2, H->hi2, rp<u64>(H->key));
    int m = 0;
    RM_TRY(rm_winners(H, false, &m));
    *ops = m;
    if (m == 0) return LS_OK;
    RM_TRY(rm_ensure(H, H->remap, sizeof(int) * (V + 1)));
    RM_TRY(rm_ensure(H, H->vkeep, sizeof(int) * (V + 1)));
    RM_TRY(rm_ensure(H, H->vscan, sizeof(int) * (V + 1)));
    RM_TRY(rm_ensure(H, H->fkeep, sizeof(int) * (F + 1)));
    RM_TRY(rm_ensure(H, H->fscan, sizeof(int) * (F + 1)));
    RM_TRY(rm_ensure(H, H->pos_b, sizeof(float) * 3 * V));
    RM_TRY(rm_ensure(H, H->faces_b, sizeof(int) * 3 * F));
    hipLaunchKernelGGL(k_rm_iota, RM_GRID(V), rp<int>(H->remap), V);
    hipLaunchKernelGGL(k_rm_fill_int, RM_GRID(V), rp<int>(H->vkeep), V, 1);
    hipLaunchKernelGGL(k_rm_fill_int, RM_GRID(F), rp<int>(H->fkeep), F, 1);
    hipLaunchKernelGGL(k_rm_collapse_apply, RM_GRID(n), rp<float>(H->pos), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->twin),
                       (const int*)rp<int>(H->flag), n, rp<int>(H->remap), rp<int>(H->vkeep), rp<int>(H->fkeep));
    RM_TRY(exclusive_scan(rp<int>(H->vkeep), V, rp<int>(H->vscan), rp<int>(H->bsum), H->st));
    RM_TRY(exclusive_scan(rp<int>(H->fkeep), F, rp<int>(H->fscan), rp<int>(H->bsum), H->st));
    hipLaunchKernelGGL(k_rm_compact_verts, RM_GRID(V), (const float*)rp<float>(H->pos), (const int*)rp<int>(H->vkeep), (const int*)rp<int>(H->vscan), V,
                       rp<float>(H->pos_b));
    hipLaunchKernelGGL(k_rm_compact_faces, RM_GRID(F), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->fkeep), (const int*)rp<int>(H->fscan),
                       (const int*)rp<int>(H->remap), (const int*)rp<int>(H->vscan), F, rp<int>(H->faces_b));
    LS_HIP(hipGetLastError());
    rm_swap(H->pos, H->pos_b);
    rm_swap(H->faces, H->faces_b);
    H->V = V - m;
    H->F = F - 2 * m;
    return LS_OK;
}

static int rm_flip_round(RemeshHandle* H, int* ops) {
    RM_TRY(rm_topo<false>(H));
    const int n = 3 * H->F;
    RM_TRY(rm_ensure(H, H->key, sizeof(u64) * (n + 1)));
    hipLaunchKernelGGL(k_rm_flip_cand, RM_GRID(n), (const float*)rp<float>(H->pos), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->twin),
                       (const int*)rp<int>(H->vptr), (const int*)rp<int>(H->vcorner), (const int*)rp<int>(H->bnd), n, rp<u64>(H->key));
    int m = 0;
    RM_TRY(rm_winners(H, true, &m));
    *ops = m;
    if (m == 0) return LS_OK;
    hipLaunchKernelGGL(k_rm_flip_apply, RM_GRID(n), rp<int>(H->faces), (const int*)rp<int>(H->twin), (const int*)rp<int>(H->flag), n);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

static int rm_relax(RemeshHandle* H) {
    RM_TRY(rm_topo<false>(H));
    const int V = H->V;
    RM_TRY(rm_ensure(H, H->pos_b, sizeof(float) * 3 * V));
    hipLaunchKernelGGL(k_rm_relax, RM_GRID(V), (const float*)rp<float>(H->pos), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->vptr),
                       (const int*)rp<int>(H->vcorner), (const int*)rp<int>(H->bnd), V, rp<float>(H->pos_b));
    LS_HIP(hipGetLastError());
    rm_swap(H->pos, H->pos_b);
    return LS_OK;
}

static int rm_build_bvh(RemeshHandle* H) {
    const int T = H->F0, V0 = H->V0, N = 2 * T - 1;
    RM_TRY(rm_ensure(H, H->code, sizeof(int) * T));
    RM_TRY(rm_ensure(H, H->ord_a, sizeof(int) * T));
    RM_TRY(rm_ensure(H, H->sort, sort_scratch_bytes(T, false)));
    RM_TRY(rm_ensure(H, H->tri, sizeof(int) * T));
    RM_TRY(rm_ensure(H, H->scode, sizeof(unsigned) * T));
    RM_TRY(rm_ensure(H, H->left, sizeof(int) * T));
    RM_TRY(rm_ensure(H, H->right, sizeof(int) * T));
    RM_TRY(rm_ensure(H, H->parent, sizeof(int) * N));
    RM_TRY(rm_ensure(H, H->esc, sizeof(int) * N));
    RM_TRY(rm_ensure(H, H->rflag, sizeof(int) * T));
    RM_TRY(rm_ensure(H, H->box, sizeof(float) * 6 * (size_t)N));
    const Lbvh a{rp<int>(H->code), rp<int>(H->ord_a), sort_scratch_carve(H->sort.p, T, false), rp<int>(H->tri),
                 rp<unsigned>(H->scode), rp<int>(H->left), rp<int>(H->right), rp<int>(H->parent), rp<int>(H->esc), rp<int>(H->rflag),
                 rp<float>(H->box), (unsigned*)(rp<int>(H->small) + 16)};
    float lo[3], hi[3];
    RM_TRY(lbvh_bounds(rp<float>(H->pos0), V0, a, H->st, lo, hi));
    const double diag = sqrt((double)(hi[0] - lo[0]) * (hi[0] - lo[0]) + (double)(hi[1] - lo[1]) * (hi[1] - lo[1]) + (double)(hi[2] - lo[2]) * (hi[2] - lo[2]));
    const float margin = (float)(1e-5 * diag) + 1e-30f;
    RM_TRY(lbvh_build(rp<float>(H->pos0), rp<int>(H->faces0), T, margin, a, H->st));
    H->bvh = true;
    return LS_OK;
}

static int rm_project(RemeshHandle* H) {
    if (!H->bvh) RM_TRY(rm_build_bvh(H));
    RM_TRY(rm_topo<false>(H));
    hipLaunchKernelGGL(k_rm_project, RM_GRID(H->V), rp<float>(H->pos), (const int*)rp<int>(H->vptr), (const int*)rp<int>(H->bnd), H->V,
                       (const float*)rp<float>(H->pos0), (const int*)rp<int>(H->faces0), H->F0, (const int*)rp<int>(H->tri),
                       (const float*)rp<float>(H->box), (const int*)rp<int>(H->left), (const int*)rp<int>(H->right), (const int*)rp<int>(H->esc));
    LS_HIP(hipGetLastError());
    return LS_OK;
}

typedef int (*RmRound)(RemeshHandle*, int*);
// one phase: rounds until a round without an operation or the cap
static int rm_phase(RemeshHandle* H, int phase, int cap) {
    const auto t0 = std::chrono::steady_clock::now();
    if (phase <= LS_REMESH_FLIP) {
        const RmRound fn[3] = {rm_split_round, rm_collapse_round, rm_flip_round};
        for (int r = 0; r < cap; ++r) {
            int ops = 0;
            RM_TRY(fn[phase](H, &ops));
            H->counters[phase] += 1;
            H->counters[3 + phase] += ops;
            if (ops == 0) break;
        }
    } else if (phase == LS_REMESH_RELAX) RM_TRY(rm_relax(H));
    else RM_TRY(rm_project(H));
    LS_HIP(hipStreamSynchronize(H->st));
    H->seconds[phase] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return LS_OK;
}

}  // namespace ls

using namespace ls;

extern "C" int ls_remesh_create(const float* verts, int64_t V, const void* faces, int idx_bytes, int64_t F, float h, int project, int device,
                                void* stream, void** handle) {
    LS_REQUIRE(handle && verts && faces && (idx_bytes == 4 || idx_bytes == 8) && V > 0 && F > 0, LS_E_INVALID, "ls_remesh_create: bad argument");
    *handle = nullptr;
    LS_REQUIRE(V < INT32_MAX / 3 && 3 * F < INT32_MAX, LS_E_OVERFLOW, "ls_remesh_create: the mesh does not fit int32 indices");
    LS_REQUIRE(h > 0.0f && std::isfinite(h), LS_E_INVALID, "ls_remesh_create: the target edge length must be positive and finite (got %g)", (double)h);
    DeviceGuard g(device);
    LS_HIP(g.err);
    RemeshHandle* H = new (std::nothrow) RemeshHandle();
    LS_REQUIRE(H, LS_E_INVALID, "ls_remesh_create: out of host memory");
    H->device = device;
    H->st = (hipStream_t)stream;
    H->h = h;
    const float hi = (4.0f / 3.0f) * h, lo = (4.0f / 5.0f) * h;
    H->hi2 = hi * hi;
    H->lo2 = lo * lo;
    H->project = project != 0;
    H->V = (int)V;
    H->F = (int)F;
    auto fail = [&](int rc) { ls_remesh_destroy(H); return rc; };
    int rc = LS_OK;
    const int n = 3 * (int)F;
    if ((rc = rm_ensure(H, H->small, sizeof(int) * 64)) || (rc = rm_ensure(H, H->pos, sizeof(float) * 3 * V)) ||
        (rc = rm_ensure(H, H->faces, sizeof(int) * n)))
        return fail(rc);
    if (hipMemsetAsync(H->small.p, 0, sizeof(int) * 64, H->st) != hipSuccess ||
        hipMemcpyAsync(H->pos.p, verts, sizeof(float) * 3 * V, hipMemcpyDeviceToDevice, H->st) != hipSuccess)
        return fail(hip_fail(hipGetLastError(), "ls_remesh_create copies", __FILE__, __LINE__));
    int bad[4] = {0, 0, 0, 0};
    if (!faces_in(faces, idx_bytes, n, V, rp<int>(H->faces), rp<int>(H->small), H->st, &bad[0]))
        return fail(hip_fail(hipGetLastError(), "ls_remesh_create", __FILE__, __LINE__));
    if (bad[0]) { set_error("remesh_botsch: a face index is outside [0, %lld)", (long long)V); return fail(LS_E_INDEX); }
    if ((rc = rm_topo<true>(H))) return fail(rc);
    if (hipMemcpyAsync(bad, H->small.p, sizeof(bad), hipMemcpyDeviceToHost, H->st) != hipSuccess || hipStreamSynchronize(H->st) != hipSuccess)
        return fail(hip_fail(hipGetLastError(), "ls_remesh_create", __FILE__, __LINE__));
    if (bad[2]) { set_error("remesh_botsch: a face repeats a vertex"); return fail(LS_E_INVALID); }
    if (bad[1]) { set_error("remesh_botsch: an edge is traversed twice in the same direction (non-manifold or inconsistently oriented)"); return fail(LS_E_INVALID); }
    if (bad[3]) { set_error("remesh_botsch: the faces around a vertex form more than one fan"); return fail(LS_E_INVALID); }
    // drop the vertices no face references
    if ((rc = rm_ensure(H, H->vkeep, sizeof(int) * (V + 1))) || (rc = rm_ensure(H, H->vscan, sizeof(int) * (V + 1))) ||
        (rc = rm_ensure(H, H->remap, sizeof(int) * (V + 1))) || (rc = rm_ensure(H, H->fkeep, sizeof(int) * (F + 1))) ||
        (rc = rm_ensure(H, H->fscan, sizeof(int) * (F + 1))) || (rc = rm_ensure(H, H->pos_b, sizeof(float) * 3 * V)) ||
        (rc = rm_ensure(H, H->faces_b, sizeof(int) * n)))
        return fail(rc);
    hipLaunchKernelGGL(k_rm_used, RM_GRID(V), (const int*)rp<int>(H->vptr), (int)V, rp<int>(H->vkeep));
    hipLaunchKernelGGL(k_rm_iota, RM_GRID(V), rp<int>(H->remap), (int)V);
    hipLaunchKernelGGL(k_rm_fill_int, RM_GRID(F), rp<int>(H->fkeep), (int)F, 1);
    if ((rc = exclusive_scan(rp<int>(H->vkeep), V, rp<int>(H->vscan), rp<int>(H->bsum), H->st)) ||
        (rc = exclusive_scan(rp<int>(H->fkeep), F, rp<int>(H->fscan), rp<int>(H->bsum), H->st)))
        return fail(rc);
    hipLaunchKernelGGL(k_rm_compact_verts, RM_GRID(V), (const float*)rp<float>(H->pos), (const int*)rp<int>(H->vkeep), (const int*)rp<int>(H->vscan), (int)V,
                       rp<float>(H->pos_b));
    hipLaunchKernelGGL(k_rm_compact_faces, RM_GRID(F), (const int*)rp<int>(H->faces), (const int*)rp<int>(H->fkeep), (const int*)rp<int>(H->fscan),
                       (const int*)rp<int>(H->remap), (const int*)rp<int>(H->vscan), (int)F, rp<int>(H->faces_b));
    rm_swap(H->pos, H->pos_b);
    rm_swap(H->faces, H->faces_b);
    int used = 0;
    if ((rc = rm_read_int(H, rp<int>(H->vscan) + V, &used))) return fail(rc);
    H->V = used;
    // the input surface of the call (projection target)
    H->V0 = H->V;
    H->F0 = H->F;
    if ((rc = rm_ensure(H, H->pos0, sizeof(float) * 3 * H->V0)) || (rc = rm_ensure(H, H->faces0, sizeof(int) * n))) return fail(rc);
    if (hipMemcpyAsync(H->pos0.p, H->pos.p, sizeof(float) * 3 * H->V0, hipMemcpyDeviceToDevice, H->st) != hipSuccess ||
        hipMemcpyAsync(H->faces0.p, H->faces.p, sizeof(int) * n, hipMemcpyDeviceToDevice, H->st) != hipSuccess ||
        hipStreamSynchronize(H->st) != hipSuccess)
        return fail(hip_fail(hipGetLastError(), "ls_remesh_create copies", __FILE__, __LINE__));
    *handle = H;
    return LS_OK;
}

extern "C" int ls_remesh_run(void* handle, int iterations) {
    LS_REQUIRE(handle && iterations >= 0, LS_E_INVALID, "ls_remesh_run: bad argument");
    RemeshHandle* H = (RemeshHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    for (int it = 0; it < iterations; ++it) {
        RM_TRY(rm_phase(H, LS_REMESH_SPLIT, RM_SPLIT_ROUNDS));
        RM_TRY(rm_phase(H, LS_REMESH_COLLAPSE, RM_COLLAPSE_ROUNDS));
        RM_TRY(rm_phase(H, LS_REMESH_FLIP, RM_FLIP_ROUNDS));
        RM_TRY(rm_phase(H, LS_REMESH_RELAX, 1));
        if (H->project) RM_TRY(rm_phase(H, LS_REMESH_PROJECT, 1));
    }
    return LS_OK;
}

extern "C" int ls_remesh_phase(void* handle, int phase, int max_rounds) {
    LS_REQUIRE(handle && phase >= LS_REMESH_SPLIT && phase <= LS_REMESH_PROJECT && max_rounds >= 1, LS_E_INVALID, "ls_remesh_phase: bad argument");
    RemeshHandle* H = (RemeshHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    return rm_phase(H, phase, max_rounds);
}

extern "C" int ls_remesh_info(void* handle, int64_t* V, int64_t* F, int64_t* counters, double* seconds) {
    LS_REQUIRE(handle, LS_E_INVALID, "ls_remesh_info: null handle");
    RemeshHandle* H = (RemeshHandle*)handle;
    if (V) *V = H->V;
    if (F) *F = H->F;
    if (counters) for (int i = 0; i < 6; ++i) counters[i] = H->counters[i];
    if (seconds) for (int i = 0; i < 5; ++i) seconds[i] = H->seconds[i];
    return LS_OK;
}

extern "C" int ls_remesh_copy_out(void* handle, float* verts, void* faces, int idx_bytes) {
    LS_REQUIRE(handle && verts && faces && (idx_bytes == 4 || idx_bytes == 8), LS_E_INVALID, "ls_remesh_copy_out: bad argument");
    RemeshHandle* H = (RemeshHandle*)handle;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    LS_HIP(hipMemcpyAsync(verts, H->pos.p, sizeof(float) * 3 * (size_t)H->V, hipMemcpyDeviceToDevice, H->st));
    const int64_t n = 3 * (int64_t)H->F;
    if (idx_bytes == 4) LS_HIP(hipMemcpyAsync(faces, H->faces.p, sizeof(int) * n, hipMemcpyDeviceToDevice, H->st));
    else hipLaunchKernelGGL(k_rm_faces_out<int64_t>, RM_GRID(n), (const int*)rp<int>(H->faces), n, (int64_t*)faces);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_remesh_destroy(void* handle) {
    if (!handle) return LS_OK;
    RemeshHandle* H = (RemeshHandle*)handle;
    {
        DeviceGuard g(H->device);
        (void)hipStreamSynchronize(H->st);
        for (RmBuf* b : H->all()) rm_free(H->device, *b);
    }
    delete H;
    return LS_OK;
}
