// raycast.hip -- rays against the mesh of a mesh-distance handle (meshbvh.h) on the device (gfx950, wave64): the closest hit, any hit
// and the gradient of the hit distance -- libigl's ray_mesh_intersect and what ambient_occlusion is built from (DESIGN.md section 2.10,
// largesteps/raycast.py). tests/ray_statement.py restates the rule below as a brute force over all faces; the device answers with the
// same bits.
//
// The rule is Woop, Benthin and Wald's watertight test in fp64 from the fp32 inputs, no FMA contraction (-ffp-contract=off).
// Per ray (origin o, direction d, widened to fp64; d need not be unit): a d with a non-finite component, or all zero, hits nothing.
// Otherwise kz is the axis of largest |d| (the lowest on a tie), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky swapped when d[kz] < 0;
// Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
// Per face (a, b, c): A = a - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], B and C likewise; U = Cx By - Cy Bx, V = Ax Cy - Ay Cx,
// W = Bx Ay - By Ax, det = (U + V) + W. The face is hit iff U, V, W are all >= 0 or all <= 0 and det != 0 (edges and vertices count; a
// NaN fails every comparison, so a zero-area or repeated-index face is never hit); t = ((U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz])) / det;
// the hit is accepted iff tmin <= t <= tmax; the weights of (a, b, c) are (U / det, V / det, W / det).
// Closest hit: the accepted face of smallest t, the lowest id on equal t; a miss is t = +inf, I = -1, W = 0. Any hit: some face is accepted.
// An edge function depends on the ray and the two sheared ends only, and swapping the ends negates it exactly: two faces that share an edge
// cannot both reject a ray that passes between them.
//
// The walk. One thread per ray, the pre-order of the LBVH through its escape links: no stack, no LDS, no scratch, and a result that
// cannot depend on the order because every face the rule accepts is visited or provably worse. A subtree is skipped only when
//   (a) the ray misses its box widened by e on every side (the three slab intervals do not meet), or
//   (b) the slab of the axis kz -- the only one that bounds the computed t, see DESIGN.md -- is entered after the best t so far
//       (strictly: an equal t with a lower id behind it is still found) or left before tmin.
// e = 2^-40 (M + max |o|), M the largest coordinate of the mesh (the handle's slack): 8192 roundings of the largest difference a - o the
// rule can form, where the rule's own error is below 8 of them (the margin argument is in DESIGN.md section 2.10). The slab products use
// 1 / d per axis: a zero component gives infinities of the right sign, 0 x inf gives a NaN that fmin / fmax drop, and every comparison
// that skips a subtree is false on a NaN, so a non-finite origin only costs time. A greedy descent to one leaf (the child entered first)
// gives the closest hit a first bound before the pre-order.
//
// The gradient of t (first order, the face held fixed; W and I carry none). With n = (b - a) x (c - a), q = n / (n . d) in fp64 from the
// fp32 inputs and g the incoming gradient: dt/do = -q, dt/dd = -t q, dt/dV[F[I, k]] = w_k q; the terms -(g q), -((g t) q) and (g w_k) q are
// rounded to fp32 once. A miss adds nothing; n . d = 0 gives what IEEE gives. The vertex gradient is summed exactly as the distance's
// (md_vertex_grad of meshbvh.h): rays grouped by face, seg_sum<9>, a thread per vertex in corner-rank order. No float atomics, no host synchronisation.
#include "common.h"
#include "groupby.h"
#include "lbvh.h"
#include "meshbvh.h"
#include <algorithm>
#include <cmath>

namespace ls {

constexpr int RC_NONE = 0x7fffffff;
__device__ __forceinline__ double rc_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// the ray of the rule and of the walk
struct RcRay {
    double o[3];                    // the origin, permuted: (kx, ky, kz)
    double Sx, Sy, Sz;
    int kx, ky, kz;
    bool ok;                        // d finite and not all zero
    double ow[3], inv[3], e;        // the origin and 1 / d in world order, the widening of the boxes
};
__device__ __forceinline__ RcRay rc_ray(const float* __restrict__ O, const float* __restrict__ D, size_t i, double slack) {
    RcRay r;
    const double d0 = D[3 * i], d1 = D[3 * i + 1], d2 = D[3 * i + 2];
    const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
    r.ok = isfinite(d0) && isfinite(d1) && isfinite(d2) && (a0 > 0.0 || a1 > 0.0 || a2 > 0.0);
    r.kz = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
    const double dz = r.kz == 0 ? d0 : r.kz == 1 ? d1 : d2;
    r.kx = r.kz == 2 ? 0 : r.kz + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    if (dz < 0.0) { const int s = r.kx; r.kx = r.ky; r.ky = s; }
    const double dx = r.kx == 0 ? d0 : r.kx == 1 ? d1 : d2, dy = r.ky == 0 ? d0 : r.ky == 1 ? d1 : d2;
    r.Sx = dx / dz; r.Sy = dy / dz; r.Sz = 1.0 / dz;
    r.ow[0] = O[3 * i]; r.ow[1] = O[3 * i + 1]; r.ow[2] = O[3 * i + 2];
    r.o[0] = O[3 * i + r.kx]; r.o[1] = O[3 * i + r.ky]; r.o[2] = O[3 * i + r.kz];
    r.inv[0] = 1.0 / d0; r.inv[1] = 1.0 / d1; r.inv[2] = 1.0 / d2;
    r.e = slack + MD_SLACK * fmax(fmax(fabs(r.ow[0]), fabs(r.ow[1])), fabs(r.ow[2]));
    return r;
}
// the rule on face f: true iff the face is hit (before the range test); t and the three edge functions over det
__device__ __forceinline__ bool rc_face(const RcRay& r, const MeshView& m, int f, double& t, double& U, double& V, double& W, double& det) {
    const float* __restrict__ P = m.P;
    const int* __restrict__ faces = m.faces;
    const size_t va = 3 * (size_t)faces[3 * (size_t)f], vb = 3 * (size_t)faces[3 * (size_t)f + 1], vc = 3 * (size_t)faces[3 * (size_t)f + 2];
    const double Akx = (double)P[va + r.kx] - r.o[0], Aky = (double)P[va + r.ky] - r.o[1], Akz = (double)P[va + r.kz] - r.o[2];
    const double Bkx = (double)P[vb + r.kx] - r.o[0], Bky = (double)P[vb + r.ky] - r.o[1], Bkz = (double)P[vb + r.kz] - r.o[2];
    const double Ckx = (double)P[vc + r.kx] - r.o[0], Cky = (double)P[vc + r.ky] - r.o[1], Ckz = (double)P[vc + r.kz] - r.o[2];
    const double Ax = Akx - r.Sx * Akz, Ay = Aky - r.Sy * Akz;
    const double Bx = Bkx - r.Sx * Bkz, By = Bky - r.Sy * Bkz;
    const double Cx = Ckx - r.Sx * Ckz, Cy = Cky - r.Sy * Ckz;
    U = Cx * By - Cy * Bx;
    V = Ax * Cy - Ay * Cx;
    W = Bx * Ay - By * Ax;
    det = (U + V) + W;
    if (!(((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0)) && det != 0.0)) return false;
    t = ((U * (r.Sz * Akz) + V * (r.Sz * Bkz)) + W * (r.Sz * Ckz)) / det;
    return true;
}
// the ray against the box of a node widened by e: false when the three slab intervals do not meet (comparisons false on NaN keep the
// node); zn / zf: where the ray enters and leaves the slab of the axis kz, n3: where it enters the box
__device__ __forceinline__ bool rc_box(const RcRay& r, const float* __restrict__ box, int node, double& zn, double& zf, double& n3) {
    const float* bx = box + 6 * (size_t)node;
    double tn[3], tf[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double t1 = (((double)bx[q] - r.ow[q]) - r.e) * r.inv[q], t2 = (((double)bx[3 + q] - r.ow[q]) + r.e) * r.inv[q];
        tn[q] = fmin(t1, t2); tf[q] = fmax(t1, t2);
    }
    zn = r.kz == 0 ? tn[0] : r.kz == 1 ? tn[1] : tn[2];
    zf = r.kz == 0 ? tf[0] : r.kz == 1 ? tf[1] : tf[2];
    n3 = fmax(fmax(tn[0], tn[1]), tn[2]);
    return !(n3 > fmin(fmin(tf[0], tf[1]), tf[2]));
}

// the walk of ray i. ANY: hit[i] = some face is accepted (the walk stops at the first); else t, I, W of the closest hit, any may be null
template <bool ANY>
__device__ __forceinline__ void rc_walk(const float* __restrict__ O, const float* __restrict__ D, int n, const double* __restrict__ trange,
                                        const MeshView& m, double* __restrict__ tout, int64_t* __restrict__ I, double* __restrict__ Wout,
                                        unsigned char* __restrict__ hit) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int* __restrict__ left = m.left;
    const int* __restrict__ right = m.right;
    const int* __restrict__ esc = m.esc;
    const float* __restrict__ box = m.box;
    const RcRay r = rc_ray(O, D, (size_t)i, m.slack);
    const double tmin = trange ? trange[2 * (size_t)i] : 0.0, tmax = trange ? trange[2 * (size_t)i + 1] : rc_inf();
    const int leaf0 = m.T - 1;
    double best = tmax, w0 = 0.0, w1 = 0.0, w2 = 0.0;
    int id = RC_NONE;
    auto leaf = [&](int node) {
        const int f = m.tri[node - leaf0];
        double t, U, V, W, det;
        if (!rc_face(r, m, f, t, U, V, W, det)) return;
        if (!(t >= tmin && t <= tmax)) return;
        if (t < best || (t == best && f < id)) { best = t; id = f; w0 = U / det; w1 = V / det; w2 = W / det; }
    };
    if (r.ok) {
        double zn, zf, n3;
        if (!ANY) {                                   // a first bound: down to one leaf, into the child the ray enters first
            int node = 0;
            while (node < leaf0) {
                const int l = left[node], rr = right[node];
                double ln, rn;
                const bool lh = rc_box(r, box, l, zn, zf, ln) && !(zf < tmin) && !(zn > best);
                const bool rh = rc_box(r, box, rr, zn, zf, rn) && !(zf < tmin) && !(zn > best);
                if (!lh && !rh) break;
                node = (rh && (!lh || rn < ln)) ? rr : l;
            }
            if (node >= leaf0) leaf(node);
        }
        int node = 0;
        while (node >= 0) {
            if (!rc_box(r, box, node, zn, zf, n3) || zn > best || zf < tmin) { node = esc[node]; continue; }
            if (node >= leaf0) {
                leaf(node);
                if (ANY && id != RC_NONE) break;
                node = esc[node];
            } else node = left[node];
        }
    }
    const bool found = id != RC_NONE;
    if (ANY) { hit[i] = found ? 1 : 0; return; }
    if (tout) tout[i] = found ? best : rc_inf();
    if (I) I[i] = found ? id : -1;
    if (Wout) { Wout[3 * (size_t)i] = found ? w0 : 0.0; Wout[3 * (size_t)i + 1] = found ? w1 : 0.0; Wout[3 * (size_t)i + 2] = found ? w2 : 0.0; }
}
// one thread per ray: the closest hit (loose pointers, the view built here, for the reason given at k_md_query of distance.hip)
__global__ __launch_bounds__(BLOCK) void k_ray_closest(const float* __restrict__ O, const float* __restrict__ D, int n, const double* __restrict__ trange,
                                                       const float* __restrict__ P, const int* __restrict__ faces, int T, const int* __restrict__ tri,
                                                       const float* __restrict__ box, const int* __restrict__ left, const int* __restrict__ right,
                                                       const int* __restrict__ esc, double slack, double* __restrict__ t, int64_t* __restrict__ I,
                                                       double* __restrict__ W) {
    rc_walk<false>(O, D, n, trange, MeshView{P, faces, T, tri, box, left, right, esc, slack}, t, I, W, nullptr);
}
// one thread per ray: one byte, 1 iff some face is accepted
__global__ __launch_bounds__(BLOCK) void k_ray_any(const float* __restrict__ O, const float* __restrict__ D, int n, const double* __restrict__ trange,
                                                   const MeshView m, unsigned char* __restrict__ hit) {
    rc_walk<true>(O, D, n, trange, m, nullptr, nullptr, nullptr, hit);
}

// ---- the gradient ----------------------------------------------------------------------------------------------------------------
// n = (b - a) x (c - a) of face f, fp64
__device__ __forceinline__ void rc_normal(const MeshView& m, size_t f, double nrm[3]) {
    double y[9];
    mesh_corners(m, f, y);
    const double ab[3] = {y[3] - y[0], y[4] - y[1], y[5] - y[2]}, ac[3] = {y[6] - y[0], y[7] - y[1], y[8] - y[2]};
    nrm[0] = ab[1] * ac[2] - ab[2] * ac[1];
    nrm[1] = ab[2] * ac[0] - ab[0] * ac[2];
    nrm[2] = ab[0] * ac[1] - ab[1] * ac[0];
}
// q = n / (n . d) of ray i on face normal n
__device__ __forceinline__ void rc_q(const float* __restrict__ D, size_t i, const double nrm[3], double q[3]) {
    const double nd = (nrm[0] * (double)D[3 * i] + nrm[1] * (double)D[3 * i + 1]) + nrm[2] * (double)D[3 * i + 2];
    q[0] = nrm[0] / nd; q[1] = nrm[1] / nd; q[2] = nrm[2] / nd;
}
// gO[i] = fl32(-(g q)), gD[i] = fl32(-((g t) q)); zeros for a miss (an I outside [0, T))
__global__ __launch_bounds__(BLOCK) void k_ray_grad_rays(const float* __restrict__ D, int n, const MeshView m, const int64_t* __restrict__ I, const double* __restrict__ t, const double* __restrict__ g,
                                                         float* __restrict__ gO, float* __restrict__ gD) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t f = I[i];
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    if (f >= 0 && f < m.T) {
        double nrm[3], q[3];
        rc_normal(m, (size_t)f, nrm);
        rc_q(D, (size_t)i, nrm, q);
        const double gi = g[i], gt = gi * t[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = (float)(-(gi * q[k])); d[k] = (float)(-(gt * q[k])); }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (gO) gO[3 * (size_t)i + k] = o[k];
        if (gD) gD[3 * (size_t)i + k] = d[k];
    }
}
// rows[f][3 k + c] = sum over the rays of face f, in sorted order, of fl32((g w_k) q_c): the G of seg_sum
struct RcRows {
    const float* __restrict__ D; MeshView m; const double* __restrict__ g; const double* __restrict__ W;
    const int* __restrict__ order; const int* __restrict__ seg; float* __restrict__ rows;
    __device__ __forceinline__ int count(int64_t key) const { return seg[key + 1] - seg[key]; }
    __device__ __forceinline__ void walk(int64_t key, int start, int step, float (&acc)[9]) const {
        const int e = seg[key + 1];
        int j = seg[key] + start;
        if (j >= e) return;
        double nrm[3];
        rc_normal(m, (size_t)key, nrm);
        for (; j < e; j += step) {
            const size_t i = (size_t)order[j];
            double q[3];
            rc_q(D, i, nrm, q);
            const double gi = g[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double gw = gi * W[3 * i + k];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[3 * k + c] += (float)(gw * q[c]);
            }
        }
    }
    __device__ __forceinline__ void store(int64_t key, const float (&acc)[9]) const {
#pragma unroll
        for (int q = 0; q < 9; ++q) rows[key * 9 + q] = acc[q];
    }
};

}  // namespace ls

using namespace ls;

extern "C" int ls_mesh_ray_closest(void* handle, const float* O, const float* D, int64_t n, const double* trange, double* t, int64_t* I, double* W,
                                   void* stream) {
    LS_REQUIRE(handle && n >= 0 && (n == 0 || (O && D)), LS_E_INVALID, "ls_mesh_ray_closest: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_ray_closest: more than 2^31 rays");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    if (n == 0 || (!t && !I && !W)) return LS_OK;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    const MeshView v = H->view();
    hipLaunchKernelGGL(k_ray_closest, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, O, D, (int)n, trange, v.P, v.faces, v.T, v.tri, v.box,
                       v.left, v.right, v.esc, v.slack, t, I, W);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_ray_any(void* handle, const float* O, const float* D, int64_t n, const double* trange, unsigned char* hit, void* stream) {
    LS_REQUIRE(handle && n >= 0 && (n == 0 || (O && D && hit)), LS_E_INVALID, "ls_mesh_ray_any: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_ray_any: more than 2^31 rays");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    if (n == 0) return LS_OK;
    DeviceGuard g(H->device);
    LS_HIP(g.err);
    hipLaunchKernelGGL(k_ray_any, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, O, D, (int)n, trange, H->view(), hit);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mesh_ray_backward_workspace_bytes(int64_t n, int64_t F, size_t* bytes) {
    LS_REQUIRE(bytes && n >= 0 && F > 0, LS_E_INVALID, "ls_mesh_ray_backward_workspace_bytes: bad argument");
    LS_REQUIRE(n < INT32_MAX - BLOCK && 3 * F < INT32_MAX, LS_E_OVERFLOW, "ls_mesh_ray_backward_workspace_bytes: more than 2^31 rays or corners");
    *bytes = md_carve<float>(nullptr, n, F, false).total;
    return LS_OK;
}

extern "C" int ls_mesh_ray_backward(void* handle, const float* O, const float* D, int64_t n, const int64_t* I, const double* W, const double* t,
                                    const double* g, const int32_t* vptr, const int32_t* corner_order, float* gO, float* gD, float* gV, void* ws,
                                    size_t ws_bytes, void* stream) {
    LS_REQUIRE(handle && n >= 0 && (n == 0 || (O && D && I && t && g)), LS_E_INVALID, "ls_mesh_ray_backward: bad argument");
    LS_REQUIRE(!gV || (vptr && corner_order && ws && (n == 0 || W)), LS_E_INVALID,
               "ls_mesh_ray_backward: the vertex gradient needs W, the corner ranking and a workspace");
    LS_REQUIRE(n < INT32_MAX - BLOCK, LS_E_OVERFLOW, "ls_mesh_ray_backward: more than 2^31 rays");
    MeshDistanceHandle* H = (MeshDistanceHandle*)handle;
    const MdCarved<float> c = md_carve<float>(ws, n, H->T, false);
    LS_REQUIRE(!gV || ws_bytes >= c.total, LS_E_WORKSPACE, "ls_mesh_ray_backward: workspace too small (%zu < %zu bytes)", ws_bytes, c.total);
    DeviceGuard guard(H->device);
    LS_HIP(guard.err);
    const hipStream_t st = (hipStream_t)stream;
    if ((gO || gD) && n > 0)
        hipLaunchKernelGGL(k_ray_grad_rays, dim3(div_up(n, BLOCK)), dim3(BLOCK), 0, st, D, (int)n, H->view(), I, t, g, gO, gD);
    if (gV && n == 0) LS_HIP(hipMemsetAsync(gV, 0, sizeof(float) * 3 * (size_t)H->V, st));
    if (gV && n > 0)
        if (int rc = md_vertex_grad<float>(I, n, H->T, H->V, RcRows{D, H->view(), g, W, c.order, c.seg, c.rows}, vptr, corner_order, gV, c, st)) return rc;
    LS_HIP(hipGetLastError());
    return LS_OK;
}
