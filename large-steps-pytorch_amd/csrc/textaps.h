// textaps.h -- the tap rules of the texture lookup, shared by texture.hip (one level) and mip.hip (a pyramid of levels): the texel-space
// coordinate of a pixel, the saturating conversion, the boundary rule per tap index and the four taps of a bilinear read. The rules and
// their operation order are stated at the top of texture.hip and in DESIGN.md section 2.7; both files sample a level through these
// functions, so a level of a pyramid is read exactly as a plain texture of its size is.
#pragma once
#include "common.h"

namespace ls {

constexpr int TX_LINEAR = 1, TX_NEAREST = 0;                 // LS_TEXTURE_* of the header
constexpr int TX_WRAP = 0, TX_CLAMP = 1, TX_ZERO = 2;
constexpr int TX_MAX_SIZE = 8192, TX_MAX_C = 32;

struct TxShape {
    int Bt, Ht, Wt, C;          // texture
    int64_t N, HW;              // pixels in all, per image
    int filter, boundary;
    int vec4;                   // C == 4 and every channel-row pointer of the call is 16-byte aligned: rows move as one float4
};

// float -> int32, saturating: the clamp happens on the float, whose bounds are exactly representable; x is finite
__device__ __forceinline__ int tx_sat(float x) { return (int)fminf(fmaxf(x, -2147483648.0f), 2147483520.0f); }

// tap index -> [0, n) by the boundary rule; zero mode: returns false when the tap lies outside (i is then unused)
__device__ __forceinline__ bool tx_fold(int& i, int n, int boundary) {
    if (boundary == TX_WRAP) {
        int r = i % n;
        i = r < 0 ? r + n : r;
        return true;
    }
    if (boundary == TX_CLAMP) {
        i = min(max(i, 0), n - 1);
        return true;
    }
    return i >= 0 && i < n;
}

// the texel after tap `i` (already in [0, n)) by the boundary rule: i + 1 without overflow
__device__ __forceinline__ bool tx_next(int i, int n, int boundary, int& i1) {
    if (boundary == TX_WRAP) { i1 = i + 1 == n ? 0 : i + 1; return true; }
    if (boundary == TX_CLAMP) { i1 = min(i + 1, n - 1); return true; }
    i1 = i + 1;
    return i1 < n;
}

struct TxCoord {
    bool finite;
    int i0, j0;                 // saturated floor
    float fx, fy;
};

__device__ __forceinline__ TxCoord tx_coord(const float* __restrict__ uv, int64_t pix, const TxShape& s) {
    const float2 c = *reinterpret_cast<const float2*>(uv + 2 * (size_t)pix);
    TxCoord t;
    float x = c.x * (float)s.Wt, y = c.y * (float)s.Ht;
    if (s.filter == TX_LINEAR) { x = x - 0.5f; y = y - 0.5f; }
    t.finite = isfinite(x) && isfinite(y);
    const float x0 = floorf(x), y0 = floorf(y);
    t.fx = x - x0;
    t.fy = y - y0;
    t.i0 = t.finite ? tx_sat(x0) : 0;
    t.j0 = t.finite ? tx_sat(y0) : 0;
    return t;
}

template <int CT>
__device__ __forceinline__ void tx_load(const float* __restrict__ p, bool vec4, float (&t)[CT]) {
    if constexpr (CT == 4) {
        if (vec4) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) t[c] = p[c];
}

template <int CT>
__device__ __forceinline__ void tx_store(float* __restrict__ p, bool vec4, const float (&t)[CT]) {
    if constexpr (CT == 4) {
        if (vec4) {
            *reinterpret_cast<float4*>(p) = make_float4(t[0], t[1], t[2], t[3]);
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) p[c] = t[c];
}

// the four taps of a pixel (linear) or its one texel (nearest: only t[0][0], ok[0][0]); a tap that is not ok reads 0
template <int CT>
struct TxTaps {
    float t[2][2][CT];          // [dy][dx]
    bool ok[2][2];
};

template <int CT>
__device__ __forceinline__ TxTaps<CT> tx_taps(const float* __restrict__ tex, const TxCoord& q, int64_t pix, const TxShape& s, int c0) {
    TxTaps<CT> r;
    const int bt = s.Bt == 1 ? 0 : (int)(pix / s.HW);
    const bool vec4 = s.vec4 != 0;
    int ix[2], jy[2];
    bool okx[2], oky[2];
    ix[0] = q.i0; jy[0] = q.j0;
    okx[0] = tx_fold(ix[0], s.Wt, s.boundary);
    oky[0] = tx_fold(jy[0], s.Ht, s.boundary);
    if (s.filter == TX_LINEAR) {
        if (s.boundary == TX_ZERO) {         // i0 + 1: no overflow, tx_sat stops below 2^31 - 1
            ix[1] = q.i0 + 1; jy[1] = q.j0 + 1;
            okx[1] = ix[1] >= 0 && ix[1] < s.Wt;
            oky[1] = jy[1] >= 0 && jy[1] < s.Ht;
        } else if (s.boundary == TX_CLAMP) {
            ix[1] = min(max(q.i0 + 1, 0), s.Wt - 1); jy[1] = min(max(q.j0 + 1, 0), s.Ht - 1);
            okx[1] = oky[1] = true;
        } else {
            okx[1] = tx_next(ix[0], s.Wt, TX_WRAP, ix[1]);
            oky[1] = tx_next(jy[0], s.Ht, TX_WRAP, jy[1]);
        }
    } else {
        ix[1] = jy[1] = 0;
        okx[1] = oky[1] = false;
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const bool ok = q.finite && okx[dx] && oky[dy];
            r.ok[dy][dx] = ok;
            if (ok) tx_load<CT>(tex + (((size_t)bt * s.Ht + jy[dy]) * s.Wt + ix[dx]) * s.C + c0, vec4, r.t[dy][dx]);
            else {
#pragma unroll
                for (int c = 0; c < CT; ++c) r.t[dy][dx][c] = 0.0f;
            }
        }
    return r;
}

}  // namespace ls
