// mip.hip -- mipmapped texture lookup and the pixel differentials that choose its level (gfx950, wave64): the rest of the nvdiffrast
// surface of largesteps.render (texture with filter_mode 'linear-mipmap-linear' / 'linear-mipmap-nearest', texture_construct_mip,
// interpolate(diff_attrs=...), pixel_differentials). Restated in fp64 numpy by tests/mip_statement.py, described in DESIGN.md section 2.7.
//
// Pyramid. Level 0 is tex (Bt, Ht, Wt, C) itself; level l + 1 has max(W_l / 2, 1) x max(H_l / 2, 1) texels (each of W_l, H_l is 1 or
// even: checked), the last level Lmax is given by the caller. A texel is ((c00 + c10) + (c01 + c11)) * 0.25f of its 2 x 2 children,
// (a + b) * 0.5f when one side is already 1. Levels 1 .. Lmax are packed level after level in ONE buffer, level l as (Bt, H_l, W_l, C).
//
// Level of detail per pixel, fp32 in this order: sx = da.x Wt, sy = da.y Wt, tx = da.z Ht, ty = da.w Ht for uv_da = (du/dX, du/dY,
// dv/dX, dv/dY); A = sx sx + tx tx, B = sy sy + ty ty, Cc = sx sy + tx ty; R = sqrt(0.25 ((A - B)(A - B)) + Cc Cc); m = 0.5 (A + B) + R;
// lod = 0.5 log2(m) + bias (bias alone when uv_da is NULL, 0.5 log2(m) alone when bias is NULL), clamped to [0, Lmax].
// linear-mipmap-linear: l0 = floor(lod), f = lod - l0, out = c0 + (c1 - c0) f with c_l the bilinear read of level l through textaps.h
// (the tap rules and operation order of texture.hip); when f == 0 or l0 == Lmax only l0 is read. linear-mipmap-nearest: the level
// min(floor(lod + 0.5), Lmax). A pixel with a non-finite uv_da, bias, lod or level-0 texel coordinate outputs 0 and gives no gradient.
//
// Gradients, no float atomics. Per pixel: to uv from both levels; d out / d lod = sum_c g_c (c1_c - c0_c) where two levels were read
// (zero where lod was clamped, where m == 0 and in nearest mode; c_l here is the sum of the four taps times their weights, see
// mip_level_grad), which is the bias gradient and, through d lod / d uv_da, the uv_da gradient (R == 0: d m / d A = d m / d B = 0.5,
// d m / d Cc = 0). To tex: every pixel is one item per level it read -- item p for l0,
// item N + p for l1 -- keyed by (level, base tap) as texture.hip keys a pixel by its base tap (tx_base, tx_base_key of textaps.h plus the
// keys of the levels before); ls_mip_order sorts the items (groupby.h) and ls_mip_backward runs one thread per texel of EVERY level
// over the sorted items of the base positions that touch it (tx_texel_walk of textaps.h, the walk of the plain texture), term
// g (wx wy) w_level, a texel with more than 64 items by its whole wave. ls_mip_fold then adds, top down, 0.25f (0.5f) of every parent's
// gradient to each of its children: a pure gather. Fixed order everywhere: bitwise reproducible. No entry point allocates or synchronises.
//
// Pixel differentials. For a covered pixel with clip-space corners p_k = (x_k, y_k, w_k): a_k = p_{k+1} x p_{k+2} are the rows of the
// adjugate, a_k(Xn, Yn) = a_k.x Xn + a_k.y Yn + a_k.z, s = a_0 + a_1 + a_2, u = a_0 / s, v = a_1 / s, and
// du/dXn = (a_0.x - u (a_0.x + a_1.x + a_2.x)) / s, likewise v and Yn; times 2 / W (2 / H) per pixel. Computed in fp64 like the coverage
// test of raster.hip, stored as fp32. Background and degenerate faces (s or the determinant zero or non-finite) give 0.
#include "meshface.h"
#include "textaps.h"

namespace ls {

constexpr int MIP_NEAREST = 0, MIP_LINEAR = 1;               // LS_MIP_* of the header
constexpr int MIP_MAX_LEVEL = 13;                            // 8192 = 2^13

struct MipShape {
    int Bt, Ht, Wt, C, Lmax;
    int64_t N, HW;              // pixels in all, per image
    int mode, boundary;
    int vec4;
};

__host__ __device__ __forceinline__ int mip_side(int n, int l) { return (n >> l) > 0 ? (n >> l) : 1; }

// the texels of levels [0, l), all batch entries
__host__ __device__ __forceinline__ int64_t mip_texels_before(const MipShape& s, int l) {
    int64_t t = 0;
    for (int k = 0; k < l; ++k) t += (int64_t)s.Bt * mip_side(s.Ht, k) * mip_side(s.Wt, k);
    return t;
}

// the keys of levels [0, l): level k has Bt (H_k + 1) (W_k + 1) base positions
__host__ __device__ __forceinline__ int64_t mip_keys_before(const MipShape& s, int l) {
    int64_t t = 0;
    for (int k = 0; k < l; ++k) t += (int64_t)s.Bt * (mip_side(s.Ht, k) + 1) * (mip_side(s.Wt, k) + 1);
    return t;
}

__device__ __forceinline__ TxShape mip_level_shape(const MipShape& s, int l) {
    return TxShape{s.Bt, mip_side(s.Ht, l), mip_side(s.Wt, l), s.C, s.N, s.HW, TX_LINEAR, s.boundary, s.vec4};
}

// level l as a (Bt, H_l, W_l, C) array
__device__ __forceinline__ const float* mip_level(const float* __restrict__ tex, const float* __restrict__ pyr, const MipShape& s, int l) {
    return l == 0 ? tex : pyr + (size_t)(mip_texels_before(s, l) - mip_texels_before(s, 1)) * s.C;
}

struct MipFoot {                // the footprint of a pixel in level-0 texels
    float sx, sy, tx, ty, A, B, Cc, R, m;
};

__device__ __forceinline__ MipFoot mip_foot(const float4& da, const MipShape& s) {
    MipFoot t;
    t.sx = da.x * (float)s.Wt; t.sy = da.y * (float)s.Wt;
    t.tx = da.z * (float)s.Ht; t.ty = da.w * (float)s.Ht;
    t.A = t.sx * t.sx + t.tx * t.tx;
    t.B = t.sy * t.sy + t.ty * t.ty;
    t.Cc = t.sx * t.sy + t.tx * t.ty;
    const float d = t.A - t.B;
    t.R = sqrtf(0.25f * (d * d) + t.Cc * t.Cc);
    t.m = 0.5f * (t.A + t.B) + t.R;
    return t;
}

struct MipLod {
    bool finite;                // false: the pixel outputs 0 and gives no gradient
    bool two;                   // two levels are read: l0 and l0 + 1, blended by f (then lod was not clamped: d out / d lod passes)
    int l0;
    float f;
};

__device__ __forceinline__ MipLod mip_lod(const float* __restrict__ uv, const float* __restrict__ uv_da, const float* __restrict__ bias,
                                          int64_t pix, const MipShape& s) {
    MipLod L;
    const float2 c = *reinterpret_cast<const float2*>(uv + 2 * (size_t)pix);
    bool fin = isfinite(c.x * (float)s.Wt - 0.5f) && isfinite(c.y * (float)s.Ht - 0.5f);
    float lod = 0.0f;
    if (uv_da) {
        const float4 da = *reinterpret_cast<const float4*>(uv_da + 4 * (size_t)pix);
        fin = fin && isfinite(da.x) && isfinite(da.y) && isfinite(da.z) && isfinite(da.w);
        lod = 0.5f * log2f(mip_foot(da, s).m);
    }
    if (bias) {
        const float b = bias[pix];
        fin = fin && isfinite(b);
        lod = uv_da ? lod + b : b;
    }
    fin = fin && !(lod != lod);
    const float lc = fin ? fminf(fmaxf(lod, 0.0f), (float)s.Lmax) : 0.0f;
    L.finite = fin;
    if (s.mode == MIP_LINEAR) {
        const float fl = floorf(lc);
        L.l0 = (int)fl;
        L.f = lc - fl;
        if (L.l0 >= s.Lmax) { L.l0 = s.Lmax; L.f = 0.0f; }
    } else {
        L.l0 = min((int)floorf(lc + 0.5f), s.Lmax);
        L.f = 0.0f;
    }
    L.two = L.f != 0.0f;
    return L;
}

// the bilinear read of one level: textaps.h's taps, texture.hip's operation order
template <int CT>
__device__ __forceinline__ void mip_sample(const float* __restrict__ level, const TxShape& sl, const float* __restrict__ uv, int64_t pix, int c0,
                                           float (&o)[CT]) {
    const TxCoord q = tx_coord(uv, pix, sl);
    const TxTaps<CT> a = tx_taps<CT>(level, q, pix, sl, c0);
#pragma unroll
    for (int c = 0; c < CT; ++c) o[c] = tx_blend(a.t[0][0][c], a.t[0][1][c], a.t[1][0][c], a.t[1][1][c], q.fx, q.fy);
}

// ---- pyramid: one thread per float of the coarser level (build) or of the finer level (fold) ---------------------------------------------
__global__ __launch_bounds__(256) void k_mip_down(const float* __restrict__ src, int Hs, int Ws, int C, int64_t n, float* __restrict__ dst) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int Hd = Hs > 1 ? Hs / 2 : 1, Wd = Ws > 1 ? Ws / 2 : 1;
    const int c = (int)(k % C);
    int64_t r = k / C;
    const int i = (int)(r % Wd); r /= Wd;
    const int j = (int)(r % Hd);
    const int64_t b = r / Hd;
    const int sj = Hs > 1 ? 2 * j : 0, si = Ws > 1 ? 2 * i : 0;
    const float* p = src + (((size_t)b * Hs + sj) * Ws + si) * C + c;
    const size_t dx = (size_t)C, dy = (size_t)Ws * C;
    float v;
    if (Hs > 1 && Ws > 1) v = ((p[0] + p[dx]) + (p[dy] + p[dy + dx])) * 0.25f;
    else if (Ws > 1) v = (p[0] + p[dx]) * 0.5f;
    else v = (p[0] + p[dy]) * 0.5f;
    dst[k] = v;
}

// child (b, j, i, c) of the finer level (Hs x Ws) += coef * its parent's gradient
__global__ __launch_bounds__(256) void k_mip_fold(float* __restrict__ fine, int Hs, int Ws, int C, int64_t n, const float* __restrict__ coarse) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int Hd = Hs > 1 ? Hs / 2 : 1, Wd = Ws > 1 ? Ws / 2 : 1;
    const int c = (int)(k % C);
    int64_t r = k / C;
    const int i = (int)(r % Ws); r /= Ws;
    const int j = (int)(r % Hs);
    const int64_t b = r / Hs;
    const int pj = Hs > 1 ? j >> 1 : 0, pi = Ws > 1 ? i >> 1 : 0;
    const float coef = (Hs > 1 && Ws > 1) ? 0.25f : 0.5f;
    fine[k] = fine[k] + coef * coarse[(((size_t)b * Hd + pj) * Wd + pi) * C + c];
}

// ---- pixel differentials ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mip_face_id(const float* __restrict__ rast, int64_t pix, int64_t F) {
    const float r = rast[pix * 4 + 3];
    return (r >= 1.0f && r <= (float)F) ? (int)r : 0;
}

__global__ __launch_bounds__(256) void k_mip_pixel_diff(const float* __restrict__ rast, const float* __restrict__ pos, const int* __restrict__ tri,
                                                        int B, int64_t V, int64_t F, int H, int W, float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    if (pix >= B * HW) return;
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int id = mip_face_id(rast, pix, F);
    if (id) {
        const int64_t b = pix / HW;
        const int64_t r = pix - b * HW;
        const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
        int v[3];
        ld_ids(tri, (int64_t)(id - 1), v);
        double p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 q = *reinterpret_cast<const float4*>(pos + ((size_t)b * V + v[k]) * 4);
            p[k][0] = q.x; p[k][1] = q.y; p[k][2] = q.w;
        }
        double a[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double(&q)[3] = p[(k + 1) % 3];
            const double(&t)[3] = p[(k + 2) % 3];
            a[k][0] = q[1] * t[2] - q[2] * t[1];
            a[k][1] = q[2] * t[0] - q[0] * t[2];
            a[k][2] = q[0] * t[1] - q[1] * t[0];
        }
        const double D = (p[0][0] * a[0][0] + p[0][1] * a[0][1]) + p[0][2] * a[0][2];
        const double Xn = (double)(2 * x + 1) / (double)W - 1.0, Yn = (double)(2 * y + 1) / (double)H - 1.0;
        double e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = (Xn * a[k][0] + Yn * a[k][1]) + a[k][2];
        const double s = (e[0] + e[1]) + e[2];
        if (s != 0.0 && D != 0.0 && isfinite(s) && isfinite(D)) {
            const double u = e[0] / s, w = e[1] / s;
            const double sa = (a[0][0] + a[1][0]) + a[2][0], sb = (a[0][1] + a[1][1]) + a[2][1];
            const double kx = 2.0 / (double)W, ky = 2.0 / (double)H;
            o.x = (float)((a[0][0] - u * sa) / s * kx);
            o.y = (float)((a[0][1] - u * sb) / s * ky);
            o.z = (float)((a[1][0] - w * sa) / s * kx);
            o.w = (float)((a[1][1] - w * sb) / s * ky);
            if (!(isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(o.w))) o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    *reinterpret_cast<float4*>(out + pix * 4) = o;
}

// attr_da (B, H, W, 2 C) = [da_c/dX, da_c/dY] per channel: du/dX (a0 - a2) + dv/dX (a1 - a2)
__global__ __launch_bounds__(256) void k_mip_interp_da(const float* __restrict__ attr, int Ba, int64_t V, int C, const float* __restrict__ rast,
                                                       const float* __restrict__ db, int B, int64_t HW, const int* __restrict__ tri, int64_t F,
                                                       float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= B * HW) return;
    const int id = mip_face_id(rast, pix, F);
    float2* o = reinterpret_cast<float2*>(out + (size_t)pix * 2 * C);
    if (!id) {
        for (int c = 0; c < C; ++c) o[c] = make_float2(0.0f, 0.0f);
        return;
    }
    const int64_t b = Ba == 1 ? 0 : pix / HW;
    int v[3];
    ld_ids(tri, (int64_t)(id - 1), v);
    const float* a0 = attr + ((size_t)b * V + v[0]) * C;
    const float* a1 = attr + ((size_t)b * V + v[1]) * C;
    const float* a2 = attr + ((size_t)b * V + v[2]) * C;
    const float4 d = *reinterpret_cast<const float4*>(db + pix * 4);
    for (int c = 0; c < C; ++c) {
        const float e0 = a0[c] - a2[c], e1 = a1[c] - a2[c];
        o[c] = make_float2(d.x * e0 + d.z * e1, d.y * e0 + d.w * e1);
    }
}

// ---- lookup forward: one thread per pixel, CT channels from c0 ---------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(256) void k_mip_forward(const float* __restrict__ tex, const float* __restrict__ pyr, const float* __restrict__ uv,
                                                     const float* __restrict__ uv_da, const float* __restrict__ bias, MipShape s, int c0,
                                                     float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    const MipLod L = mip_lod(uv, uv_da, bias, pix, s);
    float o[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) o[c] = 0.0f;
    if (L.finite) {
        mip_sample<CT>(mip_level(tex, pyr, s, L.l0), mip_level_shape(s, L.l0), uv, pix, c0, o);
        if (L.two) {
            float o1[CT];
            mip_sample<CT>(mip_level(tex, pyr, s, L.l0 + 1), mip_level_shape(s, L.l0 + 1), uv, pix, c0, o1);
#pragma unroll
            for (int c = 0; c < CT; ++c) o[c] = o[c] + (o1[c] - o[c]) * L.f;
        }
    }
    tx_store<CT>(out + (size_t)pix * s.C + c0, s.vec4 != 0, o);
}

// ---- per-pixel gradients: uv (N, 2) and d loss / d lod (N), both accumulated over the channel groups --------------------------------------
// the uv gradient of one level and its bilinear read. The read feeds d out / d lod = c1 - c0 and is summed by weights, not in the
// forward's order t00 + (t10 - t00) fx: that form errs by a rounding of the LARGEST tap (a tap that reads 0 in zero mode leaves
// t00 - t00 fx), the weighted sum by roundings of the weighted taps, which is what a difference of two reads needs.
template <int CT>
__device__ __forceinline__ void mip_level_grad(const float* __restrict__ level, const TxShape& sl, const float* __restrict__ uv, int64_t pix, int c0,
                                               const float (&go)[CT], float& gu, float& gv, float (&o)[CT]) {
    const TxCoord q = tx_coord(uv, pix, sl);
    const TxTaps<CT> a = tx_taps<CT>(level, q, pix, sl, c0);
    const float ofx = 1.0f - q.fx, ofy = 1.0f - q.fy;
    const float w00 = ofx * ofy, w10 = q.fx * ofy, w01 = ofx * q.fy, w11 = q.fx * q.fy;
    float su = 0.0f, sv = 0.0f;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        tx_blend_grad(a.t[0][0][c], a.t[0][1][c], a.t[1][0][c], a.t[1][1][c], q.fx, ofx, q.fy, ofy, go[c], su, sv);
        o[c] = (a.t[0][0][c] * w00 + a.t[0][1][c] * w10) + (a.t[1][0][c] * w01 + a.t[1][1][c] * w11);
    }
    gu = (float)sl.Wt * su;
    gv = (float)sl.Ht * sv;
}

template <int CT>
__global__ __launch_bounds__(256) void k_mip_backward_pixel(const float* __restrict__ tex, const float* __restrict__ pyr, const float* __restrict__ uv,
                                                            const float* __restrict__ uv_da, const float* __restrict__ bias,
                                                            const float* __restrict__ g, MipShape s, int c0, float* __restrict__ guv,
                                                            float* __restrict__ glod) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    float2 acc = make_float2(0.0f, 0.0f);
    float dl = 0.0f;
    if (c0 != 0) {
        if (guv) acc = *reinterpret_cast<const float2*>(guv + 2 * (size_t)pix);
        if (glod) dl = glod[pix];
    }
    const MipLod L = mip_lod(uv, uv_da, bias, pix, s);
    if (L.finite) {
        float go[CT], o0[CT];
        tx_load<CT>(g + (size_t)pix * s.C + c0, s.vec4 != 0, go);
        float gu0, gv0;
        mip_level_grad<CT>(mip_level(tex, pyr, s, L.l0), mip_level_shape(s, L.l0), uv, pix, c0, go, gu0, gv0, o0);
        if (L.two) {
            float o1[CT], gu1, gv1;
            mip_level_grad<CT>(mip_level(tex, pyr, s, L.l0 + 1), mip_level_shape(s, L.l0 + 1), uv, pix, c0, go, gu1, gv1, o1);
            const float of = 1.0f - L.f;
            acc.x += gu0 * of + gu1 * L.f;
            acc.y += gv0 * of + gv1 * L.f;
            float d = 0.0f;
#pragma unroll
            for (int c = 0; c < CT; ++c) d += go[c] * (o1[c] - o0[c]);
            dl += d;
        } else {
            acc.x += gu0;
            acc.y += gv0;
        }
    }
    if (guv) *reinterpret_cast<float2*>(guv + 2 * (size_t)pix) = acc;
    if (glod) glod[pix] = dl;
}

// grad_uv_da = d loss / d lod * d lod / d uv_da
__global__ __launch_bounds__(256) void k_mip_backward_da(const float* __restrict__ uv, const float* __restrict__ uv_da, const float* __restrict__ bias,
                                                         const float* __restrict__ glod, MipShape s, float* __restrict__ gda) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const MipLod L = mip_lod(uv, uv_da, bias, pix, s);
    if (L.finite && L.two) {
        const MipFoot t = mip_foot(*reinterpret_cast<const float4*>(uv_da + 4 * (size_t)pix), s);
        // lod = log2(m) / 2: d lod / d m = 1 / (2 ln 2 m); m = (A + B) / 2 + R
        const float dm = glod[pix] * (0.72134752044448170368f / t.m);
        float dA = 0.5f, dB = 0.5f, dC = 0.0f;
        if (t.R > 0.0f) {
            const float h = 0.25f * (t.A - t.B) / t.R;
            dA = 0.5f + h;
            dB = 0.5f - h;
            dC = t.Cc / t.R;
        }
        o.x = dm * (dA * (2.0f * t.sx) + dC * t.sy) * (float)s.Wt;
        o.y = dm * (dB * (2.0f * t.sy) + dC * t.sx) * (float)s.Wt;
        o.z = dm * (dA * (2.0f * t.tx) + dC * t.ty) * (float)s.Ht;
        o.w = dm * (dB * (2.0f * t.ty) + dC * t.tx) * (float)s.Ht;
    }
    *reinterpret_cast<float4*>(gda + 4 * (size_t)pix) = o;
}

// ---- the item order: item p < N is pixel p at its level l0, item N + p pixel p at l0 + 1 ------------------------------------------------
__global__ __launch_bounds__(256) void k_mip_keys(const float* __restrict__ uv, const float* __restrict__ uv_da, const float* __restrict__ bias,
                                                  MipShape s, int64_t nitems, int64_t nk, int* __restrict__ keys) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= nitems) return;
    const int which = it >= s.N ? 1 : 0;
    const int64_t pix = it - (which ? s.N : 0);
    const MipLod L = mip_lod(uv, uv_da, bias, pix, s);
    bool ok = L.finite && (which == 0 || L.two);
    int key = (int)nk;
    if (ok) {
        const int l = L.l0 + which;
        const TxShape sl = mip_level_shape(s, l);
        const TxCoord q = tx_coord(uv, pix, sl);
        int i = q.i0, j = q.j0;
        ok = tx_base(i, j, sl);
        const int bt = s.Bt == 1 ? 0 : (int)(pix / s.HW);
        if (ok) key = (int)(mip_keys_before(s, l) + tx_base_key(bt, j, i, sl));
    }
    keys[it] = key;
}

// ---- backward to the pyramid: one thread per texel of every level ------------------------------------------------------------------------
// item p < N is pixel p at its level l0, item N + p pixel p at l0 + 1: its weight has the factor 1 - f or f where two levels were read
struct MipItem {
    const float* __restrict__ uv; const float* __restrict__ uv_da; const float* __restrict__ bias;
    MipShape s;                 // (by value: through a reference the conversions of mip_lod are not hoisted out of the walk's loops)
    __device__ __forceinline__ bool operator()(int it, int64_t& pix, float& f) const {
        const bool which = it >= s.N;
        pix = which ? it - s.N : it;
        const MipLod L = mip_lod(uv, uv_da, bias, pix, s);
        f = which ? L.f : 1.0f - L.f;
        return L.two;
    }
};

// the gradient of one texel of one level per key: tx_texel_walk of textaps.h over the level's keys
template <int CT>
struct MipTexelSum {
    const float* __restrict__ uv; const float* __restrict__ uv_da; const float* __restrict__ bias; const float* __restrict__ g;
    const int* __restrict__ order; const int* __restrict__ seg;
    MipShape s; int c0; float* __restrict__ gtex; float* __restrict__ gpyr;

    template <bool COUNT>
    __device__ __forceinline__ int64_t visit(int64_t k, int start, int step, float (&acc)[CT]) const {
        int l = 0;
        int64_t n = (int64_t)s.Bt * s.Ht * s.Wt;
        while (k >= n && l < s.Lmax) {                 // (k < the texels of all levels: the loop ends at the texel's level)
            k -= n;
            ++l;
            n = (int64_t)s.Bt * mip_side(s.Ht, l) * mip_side(s.Wt, l);
        }
        const TxShape sl = mip_level_shape(s, l);
        return tx_texel_walk<CT, COUNT>(tx_texel(k, sl), sl, mip_keys_before(s, l), MipItem{uv, uv_da, bias, s}, uv, g, order, seg, c0, start,
                                        step, acc);
    }
    __device__ __forceinline__ int64_t count(int64_t k) const {
        float none[CT];
        return visit<true>(k, 0, 1, none);
    }
    __device__ __forceinline__ void walk(int64_t k, int start, int step, float (&acc)[CT]) const { visit<false>(k, start, step, acc); }
    __device__ __forceinline__ void store(int64_t k, const float (&acc)[CT]) const {
        const int64_t n0 = (int64_t)s.Bt * s.Ht * s.Wt;
        float* p = k < n0 ? gtex + (size_t)k * s.C + c0 : gpyr + (size_t)(k - n0) * s.C + c0;
        tx_store<CT>(p, s.vec4 != 0, acc);
    }
};

template <int CT>
__global__ __launch_bounds__(256) void k_mip_backward_tex(const float* __restrict__ uv, const float* __restrict__ uv_da, const float* __restrict__ bias,
                                                          const float* __restrict__ g, const int* __restrict__ order, const int* __restrict__ seg,
                                                          MipShape s, int c0, int64_t ntexels, float* __restrict__ gtex, float* __restrict__ gpyr) {
    seg_sum<CT>(ntexels, MipTexelSum<CT>{uv, uv_da, bias, g, order, seg, s, c0, gtex, gpyr});
}

}  // namespace ls

using namespace ls;

namespace {

int mip_check_tex(int64_t Bt, int Ht, int Wt, int C, int Lmax, const char* who) {
    LS_REQUIRE(Bt >= 1 && Ht >= 1 && Wt >= 1 && Ht <= TX_MAX_SIZE && Wt <= TX_MAX_SIZE && C >= 1 && C <= TX_MAX_C && Bt < ((int64_t)1 << 31),
               LS_E_INVALID, "%s: bad sizes (tex %lld x %d x %d x %d)", who, (long long)Bt, Ht, Wt, C);
    LS_REQUIRE(Lmax >= 0 && Lmax <= MIP_MAX_LEVEL, LS_E_INVALID, "%s: the last level %d is outside [0, %d]", who, Lmax, MIP_MAX_LEVEL);
    int h = Ht, w = Wt;
    for (int l = 0; l < Lmax; ++l) {
        LS_REQUIRE(h > 1 || w > 1, LS_E_INVALID, "%s: level %d is 1 x 1, there is no level %d", who, l, Lmax);
        LS_REQUIRE((h == 1 || h % 2 == 0) && (w == 1 || w % 2 == 0), LS_E_INVALID, "%s: level %d is %d x %d: each side must be 1 or even", who, l,
                   h, w);
        h = std::max(h / 2, 1);
        w = std::max(w / 2, 1);
    }
    return LS_OK;
}

int mip_check(int64_t Bt, int Ht, int Wt, int C, int Lmax, int64_t B, int H, int W, int mode, int boundary, const char* who, MipShape* s) {
    int rc = mip_check_tex(Bt, Ht, Wt, C, Lmax, who);
    if (rc) return rc;
    LS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (Bt == 1 || Bt == B), LS_E_INVALID, "%s: bad sizes (tex batch %lld, uv %lld x %d x %d)", who,
               (long long)Bt, (long long)B, H, W);
    LS_REQUIRE((mode == MIP_NEAREST || mode == MIP_LINEAR) && (boundary == TX_WRAP || boundary == TX_CLAMP || boundary == TX_ZERO), LS_E_INVALID,
               "%s: unknown mip mode %d or boundary mode %d", who, mode, boundary);
    const int64_t N = B * (int64_t)H * W;
    *s = MipShape{(int)Bt, Ht, Wt, C, Lmax, N, (int64_t)H * W, mode, boundary, 0};
    LS_REQUIRE(2 * N < ((int64_t)1 << 31) - 1 && mip_keys_before(*s, Lmax + 1) < ((int64_t)1 << 31) - 2, LS_E_OVERFLOW,
               "%s: the problem does not fit the int32 index space (tex %lld x %d x %d, uv %lld x %d x %d)", who, (long long)Bt, Ht, Wt,
               (long long)B, H, W);
    return LS_OK;
}

int mip_check_raster(int64_t B, int64_t V, int64_t F, int H, int W, const char* who) {
    LS_REQUIRE(B >= 1 && V >= 0 && F >= 0 && H >= 1 && W >= 1 && H <= 4096 && W <= 4096, LS_E_INVALID, "%s: bad sizes (B %lld V %lld F %lld H %d W %d)",
               who, (long long)B, (long long)V, (long long)F, H, W);
    LS_REQUIRE(B * H * W < ((int64_t)1 << 31) - 1 && F < ((int64_t)1 << 24) && B * V < ((int64_t)1 << 31), LS_E_OVERFLOW,
               "%s: the problem does not fit the int32 index space (B %lld V %lld F %lld H %d W %d)", who, (long long)B, (long long)V, (long long)F, H, W);
    return LS_OK;
}

}  // namespace

extern "C" int ls_mip_workspace_bytes(int64_t B, int H, int W, size_t* bytes) {
    LS_REQUIRE(bytes && B >= 1 && H >= 1 && W >= 1, LS_E_INVALID, "ls_mip_workspace_bytes: bad argument");
    LS_REQUIRE(2 * B * (int64_t)H * W < ((int64_t)1 << 31) - 1, LS_E_OVERFLOW, "ls_mip_workspace_bytes: 2 B H W does not fit int32");
    *bytes = tx_order_carve(nullptr, 2 * B * (int64_t)H * W).total;
    return LS_OK;
}

extern "C" int ls_mip_build(const float* tex, int64_t Bt, int Ht, int Wt, int C, int Lmax, float* pyr, int device, void* stream) {
    int rc = mip_check_tex(Bt, Ht, Wt, C, Lmax, "ls_mip_build");
    if (rc) return rc;
    LS_REQUIRE(tex && (pyr || Lmax == 0), LS_E_INVALID, "ls_mip_build: null argument");
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const float* src = tex;
    float* dst = pyr;
    int h = Ht, w = Wt;
    for (int l = 0; l < Lmax; ++l) {
        const int hd = std::max(h / 2, 1), wd = std::max(w / 2, 1);
        const int64_t n = Bt * (int64_t)hd * wd * C;
        hipLaunchKernelGGL(k_mip_down, dim3(div_up(n, 256)), dim3(256), 0, st, src, h, w, C, n, dst);
        src = dst;
        dst += n;
        h = hd; w = wd;
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mip_fold(float* grad_tex, int64_t Bt, int Ht, int Wt, int C, int Lmax, float* grad_pyr, int device, void* stream) {
    int rc = mip_check_tex(Bt, Ht, Wt, C, Lmax, "ls_mip_fold");
    if (rc) return rc;
    LS_REQUIRE(grad_tex && (grad_pyr || Lmax == 0), LS_E_INVALID, "ls_mip_fold: null argument");
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const MipShape s{(int)Bt, Ht, Wt, C, Lmax, 0, 0, 0, 0, 0};
    const int64_t t1 = mip_texels_before(s, 1);
    for (int l = Lmax - 1; l >= 0; --l) {
        float* fine = l == 0 ? grad_tex : grad_pyr + (size_t)(mip_texels_before(s, l) - t1) * C;
        const float* coarse = grad_pyr + (size_t)(mip_texels_before(s, l + 1) - t1) * C;
        const int h = mip_side(Ht, l), w = mip_side(Wt, l);
        const int64_t n = Bt * (int64_t)h * w * C;
        hipLaunchKernelGGL(k_mip_fold, dim3(div_up(n, 256)), dim3(256), 0, st, fine, h, w, C, n, coarse);
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mip_pixel_differentials(const float* rast, const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W,
                                          float* out, int device, void* stream) {
    int rc = mip_check_raster(B, V, F, H, W, "ls_mip_pixel_differentials");
    if (rc) return rc;
    LS_REQUIRE(rast && out && (pos || V == 0) && (tri || F == 0), LS_E_INVALID, "ls_mip_pixel_differentials: null argument");
    LS_REQUIRE(tx_aligned(pos, 16) && tx_aligned(out, 16), LS_E_INVALID, "ls_mip_pixel_differentials: pos and out must be 16-byte aligned");
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipLaunchKernelGGL(k_mip_pixel_diff, dim3(div_up(B * (int64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, rast, pos, tri, (int)B, V, F, H, W,
                       out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mip_interpolate_da(const float* attr, int64_t attr_batch, int64_t V, int C, const float* rast, const float* rast_db, int64_t B,
                                     int H, int W, const int32_t* tri, int64_t F, float* out, int device, void* stream) {
    int rc = mip_check_raster(B, V, F, H, W, "ls_mip_interpolate_da");
    if (rc) return rc;
    LS_REQUIRE(C >= 1 && (attr_batch == 1 || attr_batch == B), LS_E_INVALID, "ls_mip_interpolate_da: C %d, attribute batch %lld of %lld", C,
               (long long)attr_batch, (long long)B);
    LS_REQUIRE(rast && rast_db && out && (attr || V == 0) && (tri || F == 0), LS_E_INVALID, "ls_mip_interpolate_da: null argument");
    LS_REQUIRE(tx_aligned(rast_db, 16) && tx_aligned(out, 8), LS_E_INVALID, "ls_mip_interpolate_da: rast_db must be 16-byte, out 8-byte aligned");
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipLaunchKernelGGL(k_mip_interp_da, dim3(div_up(B * (int64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, attr, (int)attr_batch, V, C, rast,
                       rast_db, (int)B, (int64_t)H * W, tri, F, out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mip_forward(const float* tex, const float* pyr, int64_t Bt, int Ht, int Wt, int C, int Lmax, const float* uv, const float* uv_da,
                              const float* bias, int64_t B, int H, int W, int mode, int boundary, float* out, int device, void* stream) {
    MipShape s;
    int rc = mip_check(Bt, Ht, Wt, C, Lmax, B, H, W, mode, boundary, "ls_mip_forward", &s);
    if (rc) return rc;
    LS_REQUIRE(tex && (pyr || Lmax == 0) && uv && out && (uv_da || bias), LS_E_INVALID, "ls_mip_forward: null argument");
    LS_REQUIRE(tx_aligned(uv, 8) && tx_aligned(uv_da, 16), LS_E_INVALID, "ls_mip_forward: uv must be 8-byte, uv_da 16-byte aligned");
    s.vec4 = C == 4 && tx_aligned(tex, 16) && tx_aligned(pyr, 16) && tx_aligned(out, 16);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(div_up(s.N, 256)), block(256);
    tx_groups(C, [&](int c0, auto ct) {
        hipLaunchKernelGGL(k_mip_forward<decltype(ct)::value>, grid, block, 0, st, tex, pyr, uv, uv_da, bias, s, c0, out);
    });
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_mip_order(const float* uv, const float* uv_da, const float* bias, int64_t B, int H, int W, int64_t Bt, int Ht, int Wt, int Lmax,
                            int mode, int boundary, int32_t* order, int32_t* seg, void* ws, size_t ws_bytes, int device, void* stream) {
    MipShape s;
    int rc = mip_check(Bt, Ht, Wt, 1, Lmax, B, H, W, mode, boundary, "ls_mip_order", &s);
    if (rc) return rc;
    const TxOrderWs L = tx_order_carve(ws, 2 * s.N);       // always sized for the two items per pixel of linear-mipmap-linear
    LS_REQUIRE(uv && (uv_da || bias) && order && seg && ws, LS_E_INVALID, "ls_mip_order: null argument");
    LS_REQUIRE(tx_aligned(uv, 8) && tx_aligned(uv_da, 16), LS_E_INVALID, "ls_mip_order: uv must be 8-byte, uv_da 16-byte aligned");
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_mip_order: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = mode == MIP_LINEAR ? 2 * s.N : s.N, nk = mip_keys_before(s, Lmax + 1);
    hipLaunchKernelGGL(k_mip_keys, dim3(div_up(n, 256)), dim3(256), 0, st, uv, uv_da, bias, s, n, nk, L.keys);
    return tx_order_finish(L, n, nk, order, seg, st);
}

extern "C" int ls_mip_backward(const float* tex, const float* pyr, int64_t Bt, int Ht, int Wt, int C, int Lmax, const float* uv, const float* uv_da,
                               const float* bias, int64_t B, int H, int W, int mode, int boundary, const float* grad_out, const int32_t* order,
                               const int32_t* seg, float* grad_tex, float* grad_pyr, float* grad_uv, float* grad_lod, float* grad_uv_da, int device,
                               void* stream) {
    MipShape s;
    int rc = mip_check(Bt, Ht, Wt, C, Lmax, B, H, W, mode, boundary, "ls_mip_backward", &s);
    if (rc) return rc;
    LS_REQUIRE(tex && (pyr || Lmax == 0) && uv && grad_out && (uv_da || bias), LS_E_INVALID, "ls_mip_backward: null argument");
    LS_REQUIRE(!grad_tex || (order && seg && (grad_pyr || Lmax == 0)), LS_E_INVALID, "ls_mip_backward: grad_tex needs order, seg and grad_pyr");
    LS_REQUIRE(!grad_uv_da || (grad_lod && uv_da), LS_E_INVALID, "ls_mip_backward: grad_uv_da needs uv_da and grad_lod");
    LS_REQUIRE(tx_aligned(uv, 8) && tx_aligned(uv_da, 16) && tx_aligned(grad_uv, 8) && tx_aligned(grad_uv_da, 16), LS_E_INVALID,
               "ls_mip_backward: uv and grad_uv must be 8-byte, uv_da and grad_uv_da 16-byte aligned");
    s.vec4 = C == 4 && tx_aligned(tex, 16) && tx_aligned(pyr, 16) && tx_aligned(grad_out, 16) && tx_aligned(grad_tex, 16) && tx_aligned(grad_pyr, 16);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    if (grad_uv || grad_lod) {
        const dim3 grid(div_up(s.N, 256)), block(256);
        tx_groups(C, [&](int c0, auto ct) {
            hipLaunchKernelGGL(k_mip_backward_pixel<decltype(ct)::value>, grid, block, 0, st, tex, pyr, uv, uv_da, bias, grad_out, s, c0, grad_uv, grad_lod);
        });
        if (grad_uv_da)
            hipLaunchKernelGGL(k_mip_backward_da, grid, block, 0, st, uv, uv_da, bias, (const float*)grad_lod, s, grad_uv_da);
    }
    if (grad_tex) {
        const int64_t nt = mip_texels_before(s, Lmax + 1);
        const dim3 grid(div_up(nt, 256)), block(256);
        tx_groups(C, [&](int c0, auto ct) {
            hipLaunchKernelGGL(k_mip_backward_tex<decltype(ct)::value>, grid, block, 0, st, uv, uv_da, bias, grad_out, order, seg, s, c0, nt, grad_tex,
                               grad_pyr);
        });
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}
