// texture.hip -- differentiable 2D texture lookup (gfx950, wave64): the fourth nvdiffrast primitive the reference's renderer calls
// (rgl-epfl/large-steps-pytorch scripts/render.py: dr.texture), restated in numpy by tests/texture_statement.py and described in
// DESIGN.md section 2.7.
//
// Rules. tex (Bt, Ht, Wt, C) fp32 with Bt in {1, B}, uv (B, H, W, 2) fp32, out (B, H, W, C). Texel (i, j) has its centre at
// ((i + 0.5) / Wt, (j + 0.5) / Ht). Linear: x = u Wt - 0.5, y = v Ht - 0.5 (one fp32 multiply, one fp32 subtract: the build has
// -ffp-contract=off), i0 = floor(x), fx = x - i0, likewise j0, fy; top = t00 + (t10 - t00) fx, bot = t01 + (t11 - t01) fx,
// out = top + (bot - top) fy -- the operation order of the plain-torch lookup this kernel replaced, so the results are the same bits.
// Nearest: the texel (floor(u Wt), floor(v Ht)). Boundary per tap index: wrap = modulo the size, clamp = clamped to [0, size - 1],
// zero = a tap outside reads 0 and receives no gradient. A non-finite u or v gives output 0 and no gradient.
//
// Range safety. floor(x) becomes an int32 through tx_sat (clamped IN FLOAT to [-2^31, 2^31 - 128], both representable, before the
// conversion; a NaN never reaches it) and is then reduced by tx_fold (integer remainder made non-negative, or an integer clamp) to
// [0, size) -- or, in zero mode, compared against [0, size) and the tap dropped. No address is formed from anything else.
//
// Gradient to uv (linear only; zero for nearest): per pixel, d out / d u = Wt ((t10 - t00)(1 - fy) + (t11 - t01) fy), likewise v.
//
// Gradient to tex: a many-to-one sum, without float atomics. ls_texture_order sorts the N = B H W pixels stably (radix.h) by ONE key
// each, the pixel's base tap after the part of the boundary rule that cannot change which texels it touches:
//     linear   wrap: (i0 mod Wt, j0 mod Ht)   clamp: (clamp(i0, -1, Wt - 1), clamp(j0, -1, Ht - 1))   zero: (i0, j0) if both lie
//              in [-1, size - 1], else none
//     nearest  the texel itself after wrap / clamp; zero: none when outside
// as key = (bt (Ht + 1) + j + 1) (Wt + 1) + i + 1, "none" (and non-finite uv) = Bt (Ht + 1) (Wt + 1), sorted last; seg[k] = the first
// sorted position with key >= k. The order depends on uv alone. ls_texture_backward then runs one thread per texel: it walks the base
// positions whose taps fall on it -- per axis (i, tap 0) and (i - 1, tap 1) (wrapped in wrap mode), plus (-1, tap 0) for texel 0 and
// (size - 1, tap 1) for the last texel in clamp mode -- and adds g (wx wy) over each position's pixels in sorted order. A texel with
// more than 64 pixels in all is summed by its whole wave, lane-strided per position, then an xor butterfly: a fixed order either way,
// so every gradient is bitwise reproducible. No entry point allocates or synchronises.
//
// The taps, the blend and its (du, dv), the base tap and its key, the texel walk and the host side of the order (channel groups,
// workspace layout, group-by tail) are in textaps.h, shared with mip.hip and cube.hip; this file keeps the kernels, the nearest
// branch of the key and the entry points.
#include "textaps.h"

namespace ls {

// ---- forward: one thread per pixel, CT channels from c0 -------------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(256) void k_tx_forward(const float* __restrict__ tex, const float* __restrict__ uv, TxShape s, int c0,
                                                    float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    const TxCoord q = tx_coord(uv, pix, s);
    const TxTaps<CT> a = tx_taps<CT>(tex, q, pix, s, c0);
    float o[CT];
    if (s.filter == TX_LINEAR) {
#pragma unroll
        for (int c = 0; c < CT; ++c) o[c] = q.finite ? tx_blend(a.t[0][0][c], a.t[0][1][c], a.t[1][0][c], a.t[1][1][c], q.fx, q.fy) : 0.0f;
    } else {
#pragma unroll
        for (int c = 0; c < CT; ++c) o[c] = a.t[0][0][c];
    }
    tx_store<CT>(out + (size_t)pix * s.C + c0, s.vec4 != 0, o);
}

// ---- backward to uv: one thread per pixel; gu (N, 2) accumulates over the channel groups (first = the group that starts at channel 0) ----
template <int CT>
__global__ __launch_bounds__(256) void k_tx_backward_uv(const float* __restrict__ tex, const float* __restrict__ uv, const float* __restrict__ g,
                                                        TxShape s, int c0, float* __restrict__ guv) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    float2 acc = c0 == 0 ? make_float2(0.0f, 0.0f) : *reinterpret_cast<const float2*>(guv + 2 * (size_t)pix);
    if (s.filter == TX_LINEAR) {
        const TxCoord q = tx_coord(uv, pix, s);
        if (q.finite) {
            const TxTaps<CT> a = tx_taps<CT>(tex, q, pix, s, c0);
            float go[CT];
            tx_load<CT>(g + (size_t)pix * s.C + c0, s.vec4 != 0, go);
            const float ofx = 1.0f - q.fx, ofy = 1.0f - q.fy;
            float su = 0.0f, sv = 0.0f;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                tx_blend_grad(a.t[0][0][c], a.t[0][1][c], a.t[1][0][c], a.t[1][1][c], q.fx, ofx, q.fy, ofy, go[c], su, sv);
            acc.x += (float)s.Wt * su;
            acc.y += (float)s.Ht * sv;
        }
    }
    *reinterpret_cast<float2*>(guv + 2 * (size_t)pix) = acc;
}

// ---- the pixel order -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t tx_nkeys(const TxShape& s) { return (int64_t)s.Bt * (s.Ht + 1) * (s.Wt + 1); }

__global__ __launch_bounds__(256) void k_tx_keys(const float* __restrict__ uv, TxShape s, int* __restrict__ keys) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= s.N) return;
    const TxCoord q = tx_coord(uv, pix, s);
    int i = q.i0, j = q.j0;
    bool ok = q.finite;
    if (s.filter == TX_NEAREST) {
        ok = tx_fold(i, s.Wt, s.boundary) && ok;
        ok = tx_fold(j, s.Ht, s.boundary) && ok;
    } else {
        ok = tx_base(i, j, s) && ok;
    }
    const int bt = s.Bt == 1 ? 0 : (int)(pix / s.HW);
    keys[pix] = ok ? (int)tx_base_key(bt, j, i, s) : (int)tx_nkeys(s);
}

// ---- backward to tex: one thread per texel ------------------------------------------------------------------------------------------------
// the gradient of one texel per key, summed by seg_sum of groupby.h: a texel's items are the pixels of up to 16 base positions, walked
// by tx_texel_walk of textaps.h (no key offset, no further factor in the weight)
template <int CT>
struct TxTexelSum {
    const float* __restrict__ uv; const float* __restrict__ g; const int* __restrict__ order; const int* __restrict__ seg;
    TxShape s; int c0; float* __restrict__ gtex;
    __device__ __forceinline__ int64_t count(int64_t k) const {
        float none[CT];
        return tx_texel_walk<CT, true>(tx_texel(k, s), s, 0, TxPixelItem(), uv, g, order, seg, c0, 0, 1, none);
    }
    __device__ __forceinline__ void walk(int64_t k, int start, int step, float (&acc)[CT]) const {
        tx_texel_walk<CT, false>(tx_texel(k, s), s, 0, TxPixelItem(), uv, g, order, seg, c0, start, step, acc);
    }
    __device__ __forceinline__ void store(int64_t k, const float (&acc)[CT]) const { tx_store<CT>(gtex + (size_t)k * s.C + c0, s.vec4 != 0, acc); }
};

template <int CT>
__global__ __launch_bounds__(256) void k_tx_backward_tex(const float* __restrict__ uv, const float* __restrict__ g, const int* __restrict__ order,
                                                         const int* __restrict__ seg, TxShape s, int c0, float* __restrict__ gtex) {
    seg_sum<CT>((int64_t)s.Bt * s.Ht * s.Wt, TxTexelSum<CT>{uv, g, order, seg, s, c0, gtex});
}

}  // namespace ls

using namespace ls;

namespace {

int tx_check(int64_t Bt, int Ht, int Wt, int C, int64_t B, int H, int W, int filter, int boundary, const char* who, TxShape* s) {
    LS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (Bt == 1 || Bt == B) && Ht >= 1 && Wt >= 1 && Ht <= TX_MAX_SIZE && Wt <= TX_MAX_SIZE && C >= 1 &&
                   C <= TX_MAX_C,
               LS_E_INVALID, "%s: bad sizes (tex %lld x %d x %d x %d, uv %lld x %d x %d)", who, (long long)Bt, Ht, Wt, C, (long long)B, H, W);
    LS_REQUIRE((filter == TX_NEAREST || filter == TX_LINEAR) && (boundary == TX_WRAP || boundary == TX_CLAMP || boundary == TX_ZERO), LS_E_INVALID,
               "%s: unknown filter mode %d or boundary mode %d", who, filter, boundary);
    const int64_t N = B * (int64_t)H * W;
    LS_REQUIRE(N < ((int64_t)1 << 31) - 1 && Bt * (int64_t)(Ht + 1) * (Wt + 1) < ((int64_t)1 << 31) - 2, LS_E_OVERFLOW,
               "%s: the problem does not fit the int32 index space (tex %lld x %d x %d, uv %lld x %d x %d)", who, (long long)Bt, Ht, Wt,
               (long long)B, H, W);
    *s = TxShape{(int)Bt, Ht, Wt, C, N, (int64_t)H * W, filter, boundary, 0};
    return LS_OK;
}

}  // namespace

extern "C" int ls_texture_workspace_bytes(int64_t B, int H, int W, size_t* bytes) {
    LS_REQUIRE(bytes && B >= 1 && H >= 1 && W >= 1, LS_E_INVALID, "ls_texture_workspace_bytes: bad argument");
    LS_REQUIRE(B * (int64_t)H * W < ((int64_t)1 << 31) - 1, LS_E_OVERFLOW, "ls_texture_workspace_bytes: B H W does not fit int32");
    *bytes = tx_order_carve(nullptr, B * (int64_t)H * W).total;
    return LS_OK;
}

extern "C" int ls_texture_forward(const float* tex, int64_t Bt, int Ht, int Wt, int C, const float* uv, int64_t B, int H, int W, int filter,
                                  int boundary, float* out, int device, void* stream) {
    TxShape s;
    int rc = tx_check(Bt, Ht, Wt, C, B, H, W, filter, boundary, "ls_texture_forward", &s);
    if (rc) return rc;
    LS_REQUIRE(tex && uv && out, LS_E_INVALID, "ls_texture_forward: null argument");
    LS_REQUIRE(tx_aligned(uv, 8), LS_E_INVALID, "ls_texture_forward: uv must be 8-byte aligned");
    s.vec4 = C == 4 && tx_aligned(tex, 16) && tx_aligned(out, 16);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(div_up(s.N, 256)), block(256);
    tx_groups(C, [&](int c0, auto ct) { hipLaunchKernelGGL(k_tx_forward<decltype(ct)::value>, grid, block, 0, st, tex, uv, s, c0, out); });
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_texture_order(const float* uv, int64_t B, int H, int W, int64_t Bt, int Ht, int Wt, int filter, int boundary, int32_t* order,
                                int32_t* seg, void* ws, size_t ws_bytes, int device, void* stream) {
    TxShape s;
    int rc = tx_check(Bt, Ht, Wt, 1, B, H, W, filter, boundary, "ls_texture_order", &s);
    if (rc) return rc;
    const TxOrderWs L = tx_order_carve(ws, s.N);
    LS_REQUIRE(uv && order && seg && ws, LS_E_INVALID, "ls_texture_order: null argument");
    LS_REQUIRE(tx_aligned(uv, 8), LS_E_INVALID, "ls_texture_order: uv must be 8-byte aligned");
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_texture_order: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tx_keys, dim3(div_up(s.N, 256)), dim3(256), 0, st, uv, s, L.keys);
    return tx_order_finish(L, s.N, (int64_t)s.Bt * (s.Ht + 1) * (s.Wt + 1), order, seg, st);
}

extern "C" int ls_texture_backward(const float* tex, int64_t Bt, int Ht, int Wt, int C, const float* uv, int64_t B, int H, int W, int filter,
                                   int boundary, const float* grad_out, const int32_t* order, const int32_t* seg, float* grad_tex, float* grad_uv,
                                   int device, void* stream) {
    TxShape s;
    int rc = tx_check(Bt, Ht, Wt, C, B, H, W, filter, boundary, "ls_texture_backward", &s);
    if (rc) return rc;
    LS_REQUIRE(tex && uv && grad_out && (!grad_tex || (order && seg)), LS_E_INVALID, "ls_texture_backward: null argument");
    LS_REQUIRE(tx_aligned(uv, 8) && (!grad_uv || tx_aligned(grad_uv, 8)), LS_E_INVALID, "ls_texture_backward: uv and grad_uv must be 8-byte aligned");
    s.vec4 = C == 4 && tx_aligned(tex, 16) && tx_aligned(grad_out, 16) && (!grad_tex || tx_aligned(grad_tex, 16));
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    if (grad_uv) {
        const dim3 grid(div_up(s.N, 256)), block(256);
        tx_groups(C, [&](int c0, auto ct) { hipLaunchKernelGGL(k_tx_backward_uv<decltype(ct)::value>, grid, block, 0, st, tex, uv, grad_out, s, c0, grad_uv); });
    }
    if (grad_tex) {
        const dim3 grid(div_up((int64_t)s.Bt * s.Ht * s.Wt, 256)), block(256);
        tx_groups(C, [&](int c0, auto ct) { hipLaunchKernelGGL(k_tx_backward_tex<decltype(ct)::value>, grid, block, 0, st, uv, grad_out, order, seg, s, c0, grad_tex); });
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}
