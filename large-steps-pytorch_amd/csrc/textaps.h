// textaps.h -- what the three texture lookups share: texture.hip (one level), mip.hip (a pyramid of levels) and cube.hip (six faces).
// Device: the texel-space coordinate of a pixel, the saturating conversion, the boundary rule per tap index, the four taps of a
// bilinear read, the bilinear blend and its (du, dv) per channel, the base tap a linear pixel is keyed by and the key of a base
// position, and the walk of one texel over the sorted items of the base positions that touch it. Host: the channel-group dispatcher,
// the alignment predicate, and the layout and group-by tail of the item order. The rules and their operation order are stated at the
// top of texture.hip and in DESIGN.md section 2.7; all three files go through these functions, so a level of a pyramid is read
// exactly as a plain texture of its size is, and a pixel inside a cube face exactly as the 2D linear + clamp lookup of that face.
#pragma once
#include "common.h"
#include "groupby.h"
#include <algorithm>
#include <type_traits>

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

// the bilinear read of one channel's taps t[dy][dx] = tYX in the operation order stated at the top of texture.hip
__device__ __forceinline__ float tx_blend(float t00, float t10, float t01, float t11, float fx, float fy) {
    const float top = t00 + (t10 - t00) * fx;
    const float bot = t01 + (t11 - t01) * fx;
    return top + (bot - top) * fy;
}

// d blend / d fx, d blend / d fy of one channel, times its upstream gradient, added to su, sv (ofx = 1 - fx, ofy = 1 - fy)
__device__ __forceinline__ void tx_blend_grad(float t00, float t10, float t01, float t11, float fx, float ofx, float fy, float ofy, float go,
                                              float& su, float& sv) {
    const float du = (t10 - t00) * ofy + (t11 - t01) * fy;
    const float dv = (t01 - t00) * ofx + (t11 - t10) * fx;
    su += go * du;
    sv += go * dv;
}

// ---- the order of the gradient to tex: a linear pixel is keyed by its base tap -------------------------------------------------------------
// (i, j) = the saturated floor -> the base tap after the part of the boundary rule that cannot change which texels the pixel touches:
// wrap folds, clamp goes to [-1, size - 1], zero keeps a tap only inside [-1, size - 1] (false: the pixel has no key)
__device__ __forceinline__ bool tx_base(int& i, int& j, const TxShape& s) {
    if (s.boundary == TX_WRAP) {
        tx_fold(i, s.Wt, TX_WRAP);
        tx_fold(j, s.Ht, TX_WRAP);
        return true;
    }
    if (s.boundary == TX_CLAMP) {
        i = min(max(i, -1), s.Wt - 1);
        j = min(max(j, -1), s.Ht - 1);
        return true;
    }
    return i >= -1 && i < s.Wt && j >= -1 && j < s.Ht;
}

// the key of base position (i, j) in [-1, size - 1]^2 of batch entry bt; a level of a pyramid adds the keys of the levels before it
__device__ __forceinline__ int64_t tx_base_key(int bt, int j, int i, const TxShape& s) {
    return ((int64_t)bt * (s.Ht + 1) + (j + 1)) * (s.Wt + 1) + (i + 1);
}

// slot q < 4 of the base positions along one axis whose tap falls on texel i of n: (base, tap); false = the slot is empty
__device__ __forceinline__ bool tx_slot(int q, int i, int n, int filter, int boundary, int& base, int& tap) {
    if (q == 0) { base = i; tap = 0; return true; }
    if (filter == TX_NEAREST) return false;
    if (q == 1) { base = (boundary == TX_WRAP && i == 0) ? n - 1 : i - 1; tap = 1; return true; }
    if (boundary != TX_CLAMP) return false;
    if (q == 2) { base = -1; tap = 0; return i == 0; }
    base = n - 1; tap = 1;
    return i == n - 1;
}

struct TxTexel { int bt, j, i; };

// texel k of a (Bt, Ht, Wt) array
__device__ __forceinline__ TxTexel tx_texel(int64_t k, const TxShape& s) {
    TxTexel t;
    const int64_t row = k / s.Wt;
    t.i = (int)(k - row * s.Wt);
    t.bt = (int)(row / s.Ht);
    t.j = (int)(row - (int64_t)t.bt * s.Ht);
    return t;
}

// the plain texture's items are its pixels, with no further factor in the weight
struct TxPixelItem {
    __device__ __forceinline__ bool operator()(int it, int64_t& pix, float& f) const { pix = it; return false; }
};

// the items of the texel's up to 16 base positions in the (Bt, Ht, Wt) array s, whose keys start at k0: their number (COUNT) or their
// weighted gradients added to acc, items start, start + step, ... of every position. item(id, pix, f) gives the pixel of an item and
// returns whether f is one more factor of its weight.
template <int CT, bool COUNT, class Item>
__device__ __forceinline__ int64_t tx_texel_walk(const TxTexel& t, const TxShape& s, int64_t k0, const Item& item, const float* __restrict__ uv,
                                                 const float* __restrict__ g, const int* __restrict__ order, const int* __restrict__ seg, int c0,
                                                 int start, int step, float (&acc)[CT]) {
    int64_t total = 0;
#pragma unroll
    for (int qy = 0; qy < 4; ++qy) {
        int by, ty;
        if (!tx_slot(qy, t.j, s.Ht, s.filter, s.boundary, by, ty)) continue;
#pragma unroll
        for (int qx = 0; qx < 4; ++qx) {
            int bx, tx;
            if (!tx_slot(qx, t.i, s.Wt, s.filter, s.boundary, bx, tx)) continue;
            const int64_t key = k0 + tx_base_key(t.bt, by, bx, s);
            const int b = seg[key], e = seg[key + 1];
            if constexpr (COUNT) total += e - b;
            else {
                for (int p = b + start; p < e; p += step) {
                    int64_t pix;
                    float f;
                    const bool more = item(order[p], pix, f);
                    float w = 1.0f;
                    if (s.filter == TX_LINEAR) {
                        const TxCoord q = tx_coord(uv, pix, s);
                        w = (tx ? q.fx : 1.0f - q.fx) * (ty ? q.fy : 1.0f - q.fy);
                    }
                    if (more) w = w * f;
                    float go[CT];
                    tx_load<CT>(g + (size_t)pix * s.C + c0, s.vec4 != 0, go);
#pragma unroll
                    for (int c = 0; c < CT; ++c) acc[c] += go[c] * w;
                }
            }
        }
    }
    return total;
}

}  // namespace ls

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// the channels in groups of at most four: one launch per group, launch(c0, std::integral_constant<int, CT>) for its CT channels from c0
template <class Launch>
static inline void tx_groups(int C, Launch launch) {
    for (int c0 = 0; c0 < C; c0 += 4)
        switch (std::min(4, C - c0)) {
        case 1: launch(c0, std::integral_constant<int, 1>()); break;
        case 2: launch(c0, std::integral_constant<int, 2>()); break;
        case 3: launch(c0, std::integral_constant<int, 3>()); break;
        default: launch(c0, std::integral_constant<int, 4>()); break;
        }
}

static inline bool tx_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the workspace of an item order: the keys and the scratch of the sort with carried keys, both 256-byte aligned. The plain texture has
// one item per pixel; the mipmapped lookup is always sized for the two of linear-mipmap-linear, the cube lookup for the four of linear.
struct TxOrderWs {
    int* keys;
    char* sort;             // sort_scratch_bytes(items, true): carved for the n <= items keys a call sorts (tx_order_finish)
    size_t total;
};

static inline TxOrderWs tx_order_carve(void* ws, int64_t items) {
    ls::WsWalk w(ws);
    int* keys = w.take<int>((size_t)items);
    char* sort = w.take<char>(sort_scratch_bytes(items, true));
    return {keys, sort, w.bytes()};
}

// the tail of the three *_order entry points: the n keys in [0, nk] that a key kernel wrote on st -> order, seg (groupby.h)
static inline int tx_order_finish(const TxOrderWs& w, int64_t n, int64_t nk, int* order, int* seg, hipStream_t st) {
    return group_by_key<true>(w.keys, n, nk, order, seg, sort_scratch_carve(w.sort, n, true), st);
}
