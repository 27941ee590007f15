// cube.hip -- differentiable cube-map lookup (gfx950, wave64): texture(..., boundary_mode='cube') of largesteps.render, nvdiffrast's
// cube mode without mipmaps. Restated in numpy by tests/cube_statement.py, described in DESIGN.md section 2.7.
//
// Rules. tex (Bt, 6, n, n, C) fp32 with Bt in {1, B}, 1 <= n <= 8192, 1 <= C <= 32; uv (B, H, W, 3) fp32: a direction d = (x, y, z) that
// need not be normalised; out (B, H, W, C).
//
// Face and coordinates (OpenGL / nvdiffrast order: faces 0..5 = +x, -x, +y, -y, +z, -z). Major axis: x if |x| >= |y| and |x| >= |z|,
// else y if |y| >= |z|, else z; the face is the major axis' sign.
//     face  sc  tc  ma        face  sc  tc  ma        face  sc  tc  ma
//      +x   -z  -y   x         +y   +x  +z   y         +z   +x  -y   z
//      -x   +z  -y   x         -y   +x  -z   y         -z   -x  -y   z
// s = (sc / |ma| + 1) * 0.5, t = (tc / |ma| + 1) * 0.5: one IEEE fp32 division, one add, one multiply, in that order (the build has
// -ffp-contract=off; the division is the plain `/`). A direction with a non-finite component, or with all components zero, gives
// output 0 and no gradient.
//
// Nearest: the texel (min(floor(s n), n - 1), min(floor(t n), n - 1)) of the face.
// Linear: x = s n - 0.5, i0 = floor(x), fx = x - i0, likewise j0, fy; i0, j0 go through tx_sat and an integer clamp to [-1, n - 1]
// before any address is formed. Taps (i0 + dx, j0 + dy), dx, dy in {0, 1}, tap id 2 dy + dx, weight w = wx wy with wx = fx or 1 - fx,
// wy = fy or 1 - fy.
//
// Seams. A tap with exactly one index out of range (-1 or n) reads the neighbouring face: the centre of that out-of-range texel on the
// extended plane of its face (|ma| = 1, sc or tc = +-(1 + 1 / n)) is a direction, and the tap is the texel that contains it. In units
// of 1 / n that direction has integer components (+-n for the old major axis, +-(n + 1) for the new one, 2 k + 1 - n along the edge),
// so cube_fold works in integers: the new coordinate (k + 1) n / (n + 1) along the edge lies strictly inside (k, k + 1), the one
// across it strictly inside (n - 1, n) or (0, 1). No table, no float.
//
// Corners. A tap with both indices out of range has no texel (at most one of the four): its weight w_c is split evenly over the other
// three, w'_k = w_k + w_c / 3 (OpenGL's seamless rule: the missing texel is the mean of the three).
//
// Arithmetic. No dropped tap: top = t00 + (t10 - t00) fx, bot = t01 + (t11 - t01) fx, out = top + (bot - top) fy -- tx_blend of
// textaps.h, the order of texture.hip, so a pixel whose four taps lie inside one face is bit for bit the 2-D linear + clamp lookup of
// that face at (s, t). With a dropped tap: out = sum of w'_k t_k over the three remaining taps in ascending tap id, from 0.
//
// Gradient to uv (linear only; zero for nearest), face choice held fixed. With the dropped tap's texel replaced by ((ta + tb) + tc) / 3
// of the other three (ascending tap id) the lookup is bilinear in all cases, so per channel du = (t10 - t00)(1 - fy) + (t11 - t01) fy,
// dv = (t01 - t00)(1 - fx) + (t11 - t10) fx; gs = n sum_c g_c du_c, gt likewise; g_sc = 0.5 gs / |ma|, g_tc = 0.5 gt / |ma|,
// g_ma = -(g_sc (sc / |ma|) + g_tc (tc / |ma|)) towards |ma|; the table above, read backwards, carries (g_sc, g_tc, g_ma) to (x, y, z).
// The result is perpendicular to d up to rounding.
//
// Gradient to tex: a many-to-one sum, without float atomics. Items are (pixel, tap) pairs, id 4 pixel + tap (nearest: one item per pixel,
// id = pixel); an item's key is its destination texel ((bt 6 + f) n + j) n + i, dropped taps and pixels without a gradient take the key
// 6 Bt n^2, which sorts last. ls_cube_order sorts the items stably by key (group_by_key of groupby.h); ls_cube_backward runs seg_sum
// with one thread per texel: term g w'_tap per item, items in sorted order, a texel with more than 64 items by its whole wave. For
// Bt = 1 the pixels of all images feed the one texture in ascending pixel index. 4 N items, no inverse seam map: the simple layout (it
// is mip.hip's 2 N items, doubled). Fixed order everywhere: bitwise reproducible. No entry point allocates or synchronises.
#include "textaps.h"

namespace ls {

struct CubeShape {
    int Bt, n, C;
    int64_t N, HW;              // pixels in all, per image
    int filter;
    int vec4;                   // as TxShape::vec4
};

// (sc, tc, ma) of face f -> (x, y, z), ma signed by the caller's convention (the table above read backwards: a signed permutation, so it
// also carries a gradient); T = float for directions and gradients, int for texel centres in units of 1 / n
template <class T>
__device__ __forceinline__ void cube_to_dir(int f, T sc, T tc, T ma, T& x, T& y, T& z) {
    switch (f) {
    case 0: x = ma; y = -tc; z = -sc; break;
    case 1: x = -ma; y = -tc; z = sc; break;
    case 2: x = sc; y = ma; z = tc; break;
    case 3: x = sc; y = -ma; z = -tc; break;
    case 4: x = sc; y = -tc; z = ma; break;
    default: x = -sc; y = -tc; z = -ma; break;
    }
}

template <class T>
__device__ __forceinline__ void cube_from_dir(int f, T x, T y, T z, T& sc, T& tc) {
    switch (f) {
    case 0: sc = -z; tc = -y; break;
    case 1: sc = z; tc = -y; break;
    case 2: sc = x; tc = z; break;
    case 3: sc = x; tc = -z; break;
    case 4: sc = x; tc = -y; break;
    default: sc = -x; tc = -y; break;
    }
}

// texel (i, j) of face f with exactly ONE index out of range (-1 or n), the other in [0, n): the neighbour's texel. Every result is
// clamped into its range, whatever came in.
__device__ __forceinline__ void cube_fold(int& f, int& i, int& j, int n) {
    int x, y, z;
    cube_to_dir<int>(f, 2 * i + 1 - n, 2 * j + 1 - n, n, x, y, z);       // the centre, times n: one component is +-(n + 1)
    const int a = abs(x) > n ? 0 : abs(y) > n ? 1 : 2;
    const int m = a == 0 ? x : a == 1 ? y : z;
    f = 2 * a + (m < 0 ? 1 : 0);
    int sc, tc;
    cube_from_dir<int>(f, x, y, z, sc, tc);
    // v = +-n: the old face's plane, the border row / column; v = 2 k + 1 - n: position k
    i = min(max((min(max(sc, -n), n) + n - 1) >> 1, 0), n - 1);
    j = min(max((min(max(tc, -n), n) + n - 1) >> 1, 0), n - 1);
}

// Everything a pixel's lookup is made of. Forward, the key kernel and both backward kernels go through cube_taps.
struct CubeTaps {
    bool finite;                // false: output 0, no gradient, no item
    int face;
    int drop;                   // the tap without a texel, -1 for none
    int texel[4];               // per tap 2 dy + dx: (f n + j) n + i within one batch entry (nearest: tap 0 only); the dropped tap's is 0
    float w[4];                 // w'_k; 0 for the dropped tap (nearest: w[0] = 1)
    float fx, fy;
    float qs, qt, ama;          // sc / |ma|, tc / |ma|, |ma|
};

__device__ __forceinline__ CubeTaps cube_taps(const float* __restrict__ uv, int64_t pix, const CubeShape& s) {
    CubeTaps r;
    const float* d = uv + 3 * (size_t)pix;
    const float x = d[0], y = d[1], z = d[2];
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    r.finite = isfinite(x) && isfinite(y) && isfinite(z) && (ax > 0.0f || ay > 0.0f || az > 0.0f);
    const int a = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float ma = a == 0 ? x : a == 1 ? y : z;
    r.face = 2 * a + (ma < 0.0f ? 1 : 0);
    r.ama = fabsf(ma);
    float sc, tc;
    cube_from_dir<float>(r.face, x, y, z, sc, tc);
    r.drop = -1;
    r.fx = r.fy = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { r.texel[k] = 0; r.w[k] = 0.0f; }
    if (!r.finite) {
        r.qs = r.qt = 0.0f;
        return r;
    }
    r.qs = sc / r.ama;
    r.qt = tc / r.ama;
    const float fs = (r.qs + 1.0f) * 0.5f, ft = (r.qt + 1.0f) * 0.5f;
    const int n = s.n;
    if (s.filter == TX_NEAREST) {
        const int i = min(max(tx_sat(floorf(fs * (float)n)), 0), n - 1);
        const int j = min(max(tx_sat(floorf(ft * (float)n)), 0), n - 1);
        r.texel[0] = (r.face * n + j) * n + i;
        r.w[0] = 1.0f;
        return r;
    }
    const float px = fs * (float)n - 0.5f, py = ft * (float)n - 0.5f;
    const float x0 = floorf(px), y0 = floorf(py);
    r.fx = px - x0;
    r.fy = py - y0;
    const int i0 = min(max(tx_sat(x0), -1), n - 1), j0 = min(max(tx_sat(y0), -1), n - 1);
    const float ofx = 1.0f - r.fx, ofy = 1.0f - r.fy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dx = k & 1, dy = k >> 1;
        int f = r.face, i = i0 + dx, j = j0 + dy;
        const bool ox = i < 0 || i >= n, oy = j < 0 || j >= n;
        r.w[k] = (dx ? r.fx : ofx) * (dy ? r.fy : ofy);
        if (ox && oy) {
            r.drop = k;
            continue;
        }
        if (ox || oy) cube_fold(f, i, j, n);
        r.texel[k] = (f * n + j) * n + i;
    }
    if (r.drop >= 0) {
        float wc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) wc = k == r.drop ? r.w[k] : wc;
        const float third = wc / 3.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) r.w[k] = k == r.drop ? 0.0f : r.w[k] + third;
    }
    return r;
}

__device__ __forceinline__ const float* cube_batch(const float* __restrict__ tex, int64_t pix, const CubeShape& s) {
    const int bt = s.Bt == 1 ? 0 : (int)(pix / s.HW);
    return tex + (size_t)bt * 6 * s.n * s.n * s.C;
}

// the texels of the taps (nearest: t[0] only); the dropped tap reads 0
template <int CT>
__device__ __forceinline__ void cube_read(const float* __restrict__ tex, const CubeTaps& q, int64_t pix, const CubeShape& s, int c0, float (&t)[4][CT]) {
    const float* base = cube_batch(tex, pix, s) + c0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != q.drop && (k == 0 || s.filter == TX_LINEAR)) tx_load<CT>(base + (size_t)q.texel[k] * s.C, s.vec4 != 0, t[k]);
        else {
#pragma unroll
            for (int c = 0; c < CT; ++c) t[k][c] = 0.0f;
        }
    }
}

// ---- forward: one thread per pixel, CT channels from c0 -------------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(256) void k_cube_forward(const float* __restrict__ tex, const float* __restrict__ uv, CubeShape s, int c0,
                                                      float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    const CubeTaps q = cube_taps(uv, pix, s);
    float o[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) o[c] = 0.0f;
    if (q.finite) {
        float t[4][CT];
        cube_read<CT>(tex, q, pix, s, c0, t);
        if (s.filter == TX_NEAREST) {
#pragma unroll
            for (int c = 0; c < CT; ++c) o[c] = t[0][c];
        } else if (q.drop < 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) o[c] = tx_blend(t[0][c], t[1][c], t[2][c], t[3][c], q.fx, q.fy);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k != q.drop) {
#pragma unroll
                    for (int c = 0; c < CT; ++c) o[c] = o[c] + q.w[k] * t[k][c];
                }
        }
    }
    tx_store<CT>(out + (size_t)pix * s.C + c0, s.vec4 != 0, o);
}

// ---- backward to uv: one thread per pixel; guv (N, 3) accumulates over the channel groups (first = the group that starts at channel 0) ----
template <int CT>
__global__ __launch_bounds__(256) void k_cube_backward_uv(const float* __restrict__ tex, const float* __restrict__ uv, const float* __restrict__ g,
                                                          CubeShape s, int c0, float* __restrict__ guv) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    float* o = guv + 3 * (size_t)pix;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (c0 != 0) { ax = o[0]; ay = o[1]; az = o[2]; }
    if (s.filter == TX_LINEAR) {
        const CubeTaps q = cube_taps(uv, pix, s);
        if (q.finite) {
            float t[4][CT], go[CT];
            cube_read<CT>(tex, q, pix, s, c0, t);
            tx_load<CT>(g + (size_t)pix * s.C + c0, s.vec4 != 0, go);
            if (q.drop >= 0) {                  // the missing texel is the mean of the other three
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    float sum = 0.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) sum = k == q.drop ? sum : sum + t[k][c];
                    const float mean = sum / 3.0f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) t[k][c] = k == q.drop ? mean : t[k][c];
                }
            }
            const float ofx = 1.0f - q.fx, ofy = 1.0f - q.fy;
            float su = 0.0f, sv = 0.0f;
#pragma unroll
            for (int c = 0; c < CT; ++c) tx_blend_grad(t[0][c], t[1][c], t[2][c], t[3][c], q.fx, ofx, q.fy, ofy, go[c], su, sv);
            const float gsc = 0.5f * ((float)s.n * su) / q.ama, gtc = 0.5f * ((float)s.n * sv) / q.ama;
            const float gma = -(gsc * q.qs + gtc * q.qt);
            float gx, gy, gz;
            cube_to_dir<float>(q.face, gsc, gtc, gma, gx, gy, gz);
            ax += gx; ay += gy; az += gz;
        }
    }
    o[0] = ax; o[1] = ay; o[2] = az;
}

// ---- the item order: one thread per pixel writes its four keys (nearest: one) ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cube_keys(const float* __restrict__ uv, CubeShape s, int nk, int* __restrict__ keys) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    const CubeTaps q = cube_taps(uv, pix, s);
    const int bt = s.Bt == 1 ? 0 : (int)(pix / s.HW);
    const int base = bt * 6 * s.n * s.n;
    if (s.filter == TX_NEAREST) {
        keys[pix] = q.finite ? base + q.texel[0] : nk;
        return;
    }
    int4 k4;
    k4.x = (q.finite && q.drop != 0) ? base + q.texel[0] : nk;
    k4.y = (q.finite && q.drop != 1) ? base + q.texel[1] : nk;
    k4.z = (q.finite && q.drop != 2) ? base + q.texel[2] : nk;
    k4.w = (q.finite && q.drop != 3) ? base + q.texel[3] : nk;
    *reinterpret_cast<int4*>(keys + 4 * (size_t)pix) = k4;          // (the key buffer is 256-byte aligned: tx_order_carve)
}

// ---- backward to tex: the gradient of one texel per key, summed by seg_sum of groupby.h ----------------------------------------------------
template <int CT>
struct CubeTexelSum {
    const float* __restrict__ uv; const float* __restrict__ g; const int* __restrict__ order; const int* __restrict__ seg;
    CubeShape s; int c0; float* __restrict__ gtex;
    __device__ __forceinline__ int64_t count(int64_t k) const { return seg[k + 1] - seg[k]; }
    __device__ __forceinline__ void walk(int64_t k, int start, int step, float (&acc)[CT]) const {
        const int e = seg[k + 1];
        for (int p = seg[k] + start; p < e; p += step) {
            const int item = order[p];
            int64_t pix = item;
            float w = 1.0f;
            if (s.filter == TX_LINEAR) {
                pix = item >> 2;
                const int tap = item & 3;
                const CubeTaps q = cube_taps(uv, pix, s);
                w = tap == 0 ? q.w[0] : tap == 1 ? q.w[1] : tap == 2 ? q.w[2] : q.w[3];
            }
            float go[CT];
            tx_load<CT>(g + (size_t)pix * s.C + c0, s.vec4 != 0, go);
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] += go[c] * w;
        }
    }
    __device__ __forceinline__ void store(int64_t k, const float (&acc)[CT]) const { tx_store<CT>(gtex + (size_t)k * s.C + c0, s.vec4 != 0, acc); }
};

template <int CT>
__global__ __launch_bounds__(256) void k_cube_backward_tex(const float* __restrict__ uv, const float* __restrict__ g, const int* __restrict__ order,
                                                           const int* __restrict__ seg, CubeShape s, int c0, float* __restrict__ gtex) {
    seg_sum<CT>((int64_t)s.Bt * 6 * s.n * s.n, CubeTexelSum<CT>{uv, g, order, seg, s, c0, gtex});
}

}  // namespace ls

using namespace ls;

namespace {

int cube_check(int64_t Bt, int n, int C, int64_t B, int H, int W, int filter, const char* who, CubeShape* s) {
    LS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (Bt == 1 || Bt == B) && n >= 1 && n <= TX_MAX_SIZE && C >= 1 && C <= TX_MAX_C, LS_E_INVALID,
               "%s: bad sizes (tex %lld x 6 x %d x %d x %d, uv %lld x %d x %d)", who, (long long)Bt, n, n, C, (long long)B, H, W);
    LS_REQUIRE(filter == TX_NEAREST || filter == TX_LINEAR, LS_E_INVALID, "%s: unknown filter mode %d", who, filter);
    const int64_t N = B * (int64_t)H * W;
    LS_REQUIRE(N < (((int64_t)1 << 31) - 1) / 4 && B < ((int64_t)1 << 31) && 6 * Bt * (int64_t)n * n < ((int64_t)1 << 31) - 2, LS_E_OVERFLOW,
               "%s: the problem does not fit the int32 index space (tex %lld x 6 x %d x %d, uv %lld x %d x %d)", who, (long long)Bt, n, n,
               (long long)B, H, W);
    *s = CubeShape{(int)Bt, n, C, N, (int64_t)H * W, filter, 0};
    return LS_OK;
}

}  // namespace

extern "C" int ls_cube_workspace_bytes(int64_t B, int H, int W, size_t* bytes) {
    LS_REQUIRE(bytes && B >= 1 && H >= 1 && W >= 1, LS_E_INVALID, "ls_cube_workspace_bytes: bad argument");
    LS_REQUIRE(B < ((int64_t)1 << 31) && B * (int64_t)H * W < (((int64_t)1 << 31) - 1) / 4, LS_E_OVERFLOW,
               "ls_cube_workspace_bytes: 4 B H W does not fit int32");
    *bytes = tx_order_carve(nullptr, 4 * B * (int64_t)H * W).total;
    return LS_OK;
}

extern "C" int ls_cube_forward(const float* tex, int64_t Bt, int n, int C, const float* uv, int64_t B, int H, int W, int filter, float* out,
                               int device, void* stream) {
    CubeShape s;
    int rc = cube_check(Bt, n, C, B, H, W, filter, "ls_cube_forward", &s);
    if (rc) return rc;
    LS_REQUIRE(tex && uv && out, LS_E_INVALID, "ls_cube_forward: null argument");
    s.vec4 = C == 4 && tx_aligned(tex, 16) && tx_aligned(out, 16);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(div_up(s.N, 256)), block(256);
    tx_groups(C, [&](int c0, auto ct) { hipLaunchKernelGGL(k_cube_forward<decltype(ct)::value>, grid, block, 0, st, tex, uv, s, c0, out); });
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_cube_order(const float* uv, int64_t B, int H, int W, int64_t Bt, int n, int filter, int32_t* order, int32_t* seg, void* ws,
                             size_t ws_bytes, int device, void* stream) {
    CubeShape s;
    int rc = cube_check(Bt, n, 1, B, H, W, filter, "ls_cube_order", &s);
    if (rc) return rc;
    const TxOrderWs L = tx_order_carve(ws, 4 * s.N);       // always sized for the four items per pixel of linear filtering
    LS_REQUIRE(uv && order && seg && ws, LS_E_INVALID, "ls_cube_order: null argument");
    LS_REQUIRE(tx_aligned(ws, 16), LS_E_INVALID, "ls_cube_order: the workspace must be 16-byte aligned");
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_cube_order: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = filter == TX_LINEAR ? 4 * s.N : s.N, nk = 6 * (int64_t)s.Bt * s.n * s.n;
    hipLaunchKernelGGL(k_cube_keys, dim3(div_up(s.N, 256)), dim3(256), 0, st, uv, s, (int)nk, L.keys);
    return tx_order_finish(L, items, nk, order, seg, st);
}

extern "C" int ls_cube_backward(const float* tex, int64_t Bt, int n, int C, const float* uv, int64_t B, int H, int W, int filter,
                                const float* grad_out, const int32_t* order, const int32_t* seg, float* grad_tex, float* grad_uv, int device,
                                void* stream) {
    CubeShape s;
    int rc = cube_check(Bt, n, C, B, H, W, filter, "ls_cube_backward", &s);
    if (rc) return rc;
    LS_REQUIRE(tex && uv && grad_out && (!grad_tex || (order && seg)), LS_E_INVALID, "ls_cube_backward: null argument");
    s.vec4 = C == 4 && tx_aligned(tex, 16) && tx_aligned(grad_out, 16) && (!grad_tex || tx_aligned(grad_tex, 16));
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    if (grad_uv) {
        const dim3 grid(div_up(s.N, 256)), block(256);
        tx_groups(C, [&](int c0, auto ct) { hipLaunchKernelGGL(k_cube_backward_uv<decltype(ct)::value>, grid, block, 0, st, tex, uv, grad_out, s, c0, grad_uv); });
    }
    if (grad_tex) {
        const dim3 grid(div_up((int64_t)s.Bt * 6 * s.n * s.n, 256)), block(256);
        tx_groups(C, [&](int c0, auto ct) { hipLaunchKernelGGL(k_cube_backward_tex<decltype(ct)::value>, grid, block, 0, st, uv, grad_out, order, seg, s, c0, grad_tex); });
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}
