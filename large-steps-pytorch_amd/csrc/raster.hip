// raster.hip -- differentiable triangle rasterization, barycentric interpolation and analytic silhouette antialiasing (gfx950,
// wave64): the three nvdiffrast primitives the reference's renderer calls (rgl-epfl/large-steps-pytorch scripts/render.py), restated
// in numpy by tests/render_statement.py and described in DESIGN.md section 2.7.
//
// Coverage (exact rule; the statement reproduces the decision bit for bit). Clip-space vertices q_i = (x_i, y_i, w_i) are read as fp32
// and widened to fp64. Edge function of corner i at the pixel centre p = (px, py, 1), px = (2 x + 1) / W - 1, py = (2 y + 1) / H - 1:
//   c_i = q_{i+1} x q_{i+2} (fp64 cross product),  E_i(p) = (px c_i.x + py c_i.y) + c_i.z,  D = (x_0 c_0.x + y_0 c_0.y) + w_0 c_0.z.
// These are the homogeneous (2DH) edge functions: E_i / (E_0 + E_1 + E_2) are the perspective-correct barycentrics of the point of the
// triangle that projects to p, and sum_i E_i q_i = D p, so z/w = (E_0 z_0 + E_1 z_1 + E_2 z_2) / D. A pixel is covered iff s E_i >= 0
// for all three corners with s = sign(D) (a zero E_i counts iff s c_i.x > 0, or s c_i.x == 0 and s c_i.y > 0: the top-left rule, i.e.
// p perturbed by (eps, eps^2)), s (E_0 + E_1 + E_2) > 0 (the point lies in front, w > 0) and z/w, rounded to fp32, lies in [-1, 1]
// (the near and far clip planes). c computed for an edge from the other side is bitwise the negation (fp products commute, a - b =
// -(b - a)), so two triangles that share an edge decide every pixel centre on it oppositely: coverage is watertight along shared
// edges, and exact (also at shared vertices) whenever the fp64 arithmetic is, e.g. for dyadic inputs. No triangle setup crosses w = 0
// specially: the same rule covers triangles behind, across and in front of the eye. D == 0 (zero area or edge-on) covers nothing.
//
// Depth: 64-bit integer atomicMin of (order-preserving bits of fp32 z/w) << 32 | face id per pixel (ties: lower face id). Triangles whose
// pixel bounding box holds at most RS_SMALL pixels are rasterized by one thread each; the others (and every triangle with a vertex at
// w <= 0, whose box is the whole image) get 16 x 16-pixel tiles numbered by an exclusive scan of their tile counts: a fixed grid of
// workgroups walks the tile numbers (total read on the device), one pixel per thread. A resolve pass writes (u, v, z/w, id + 1) fp32.
//
// Backward passes use no float atomics. Pixels are sorted once per rasterized frame (stable radix sort by key b F + face, background
// last: ls_raster_pixel_order) and every backward recomputes a pixel's contribution row in that order and sums each face's rows in a
// fixed order (a thread per face; a face with more than 64 pixels is summed by the whole wave, lane-strided, then a butterfly): face rows
// [B F][9] (the x, y, w gradient of each corner) or [B F][C][3] (attribute gradients). A per-vertex pass adds a vertex's face rows in the
// corner ranking of the normals (ls_corner_ranks): every output and gradient is bitwise reproducible.
//
// Range mode (ls_range_*): pos (V, 4) is shared and image b draws the faces tri[start_b : start_b + count_b] of a range table
// (B, 3) = (start, count, item_ptr). The slice law: image b is, bit for bit, the instanced frame of pos[None] and that slice with start_b
// added to the ids of covered pixels, and every gradient is the sum of the B slice calls' gradients added in ascending b. An ITEM is a
// pair (b, f), f in range b, numbered item_ptr[b] + f - start_b, N = sum count_b of them: the depth pass, the tile scan, the pixel-order
// keys, seg, the face rows and the edge adjacency (per image: the neighbour across an edge WITHIN the slice) are all indexed by item.
// Both modes run the same device functions and kernels, through a mapping (MapInst, MapRange) from keys to (image, face, pos batch).
//
// Depth peeling (ls_peel_*): the depth pass with a floor per pixel. The previous layer's rast holds, bit for bit, the z/w and the id its
// pixel won with, i.e. its depth key; a covering fragment enters the minimum only if its key is STRICTLY GREATER than that key, and
// nothing enters where the previous layer is background (or holds an id foreign to the image): background stays background. The law:
// layer l of a pixel is the l-th of its covering fragments in ascending key order, (order bits of z/w, face id) -- exact depth ties
// peel in face order, no epsilon. The peeling kernels are the two depth kernels instantiated with Peel<Map>; resolve is shared.
#include "common.h"
#include "groupby.h"
#include <algorithm>
#include <type_traits>

namespace ls {

constexpr int RS_SMALL = 256;                 // bounding-box pixels up to which one thread rasterizes a triangle
constexpr int RS_TILE = 16;                   // tile edge of the cooperative path (one 256-thread workgroup per tile)
constexpr int RS_LARGE_GRID = 2048;           // workgroups of the cooperative path
typedef unsigned long long u64;

struct RTri {
    float4 q[3];                              // (x, y, z, w) of the three corners
    double c[3][3];                           // edge vectors c_i = q_{i+1} x q_{i+2} over (x, y, w)
    double D;
};

__device__ __forceinline__ void rs_cross(const float4& a, const float4& b, double (&c)[3]) {
    const double ax = a.x, ay = a.y, aw = a.w, bx = b.x, by = b.y, bw = b.w;
    c[0] = ay * bw - aw * by;
    c[1] = aw * bx - ax * bw;
    c[2] = ax * by - ay * bx;
}

__device__ __forceinline__ RTri rs_setup(const float* __restrict__ pos, const int* __restrict__ tri, int64_t b, int64_t V, int64_t f) {
    RTri t;
#pragma unroll
    for (int i = 0; i < 3; ++i) t.q[i] = *reinterpret_cast<const float4*>(pos + ((size_t)b * V + tri[3 * f + i]) * 4);
    rs_cross(t.q[1], t.q[2], t.c[0]);
    rs_cross(t.q[2], t.q[0], t.c[1]);
    rs_cross(t.q[0], t.q[1], t.c[2]);
    t.D = ((double)t.q[0].x * t.c[0][0] + (double)t.q[0].y * t.c[0][1]) + (double)t.q[0].w * t.c[0][2];
    return t;
}

__device__ __forceinline__ double rs_det(const float4& a, const float4& b, const float4& c) {
    double x[3];
    rs_cross(b, c, x);
    return ((double)a.x * x[0] + (double)a.y * x[1]) + (double)a.w * x[2];
}

__device__ __forceinline__ double rs_centre(int i, int n) { return (double)(2 * i + 1) / (double)n - 1.0; }

__device__ __forceinline__ bool rs_edge_in(double E, const double (&c)[3], double s) {
    const double e = s * E;
    if (e > 0.0) return true;
    if (e < 0.0) return false;
    if (!(e == 0.0)) return false;             // NaN
    const double cx = s * c[0], cy = s * c[1];
    return cx > 0.0 || (cx == 0.0 && cy > 0.0);
}

// coverage of the pixel centre (px, py); E = the three edge functions, zf = z/w in fp32
__device__ __forceinline__ bool rs_cover(const RTri& t, double px, double py, double (&E)[3], float& zf) {
    const double s = t.D > 0.0 ? 1.0 : -1.0;
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        E[i] = (px * t.c[i][0] + py * t.c[i][1]) + t.c[i][2];
        in = in && rs_edge_in(E[i], t.c[i], s);
    }
    if (!in) return false;
    const double S = (E[0] + E[1]) + E[2];
    if (!(s * S > 0.0)) return false;
    const double zw = (((double)t.q[0].z * E[0] + (double)t.q[1].z * E[1]) + (double)t.q[2].z * E[2]) / t.D;
    zf = (float)zw;
    return zf >= -1.0f && zf <= 1.0f;
}

// false: the triangle can cover nothing (D == 0 or NaN, all w <= 0, or all corners outside one clip plane)
__device__ __forceinline__ bool rs_visible(const RTri& t) {
    if (!(t.D != 0.0) || t.D != t.D) return false;
    bool allw = true, xp = true, xn = true, yp = true, yn = true, zp = true, zn = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 q = t.q[i];
        allw = allw && !(q.w > 0.0f);
        xp = xp && q.x > q.w; xn = xn && q.x < -q.w;
        yp = yp && q.y > q.w; yn = yn && q.y < -q.w;
        zp = zp && q.z > q.w; zn = zn && q.z < -q.w;
    }
    return !(allw || xp || xn || yp || yn || zp || zn);
}

// pixel bounding box [x0, x1] x [y0, y1] (conservative; the coverage test decides); false when empty
__device__ __forceinline__ bool rs_bbox(const RTri& t, int H, int W, int& x0, int& x1, int& y0, int& y1) {
    bool front = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) front = front && t.q[i].w > 0.0f;
    if (!front) { x0 = 0; x1 = W - 1; y0 = 0; y1 = H - 1; return true; }
    double mnx = 1e300, mxx = -1e300, mny = 1e300, mxy = -1e300;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double X = (double)t.q[i].x / (double)t.q[i].w, Y = (double)t.q[i].y / (double)t.q[i].w;
        mnx = fmin(mnx, X); mxx = fmax(mxx, X); mny = fmin(mny, Y); mxy = fmax(mxy, Y);
    }
    // centre i lies in [lo, hi] iff ((lo + 1) W - 1) / 2 <= i <= ((hi + 1) W - 1) / 2; one pixel of margin for the rounding
    const double ax = fmax(floor(((mnx + 1.0) * W - 1.0) * 0.5) - 1.0, 0.0), bx = fmin(ceil(((mxx + 1.0) * W - 1.0) * 0.5) + 1.0, W - 1.0);
    const double ay = fmax(floor(((mny + 1.0) * H - 1.0) * 0.5) - 1.0, 0.0), by = fmin(ceil(((mxy + 1.0) * H - 1.0) * 0.5) + 1.0, H - 1.0);
    if (!(ax <= bx && ay <= by)) return false;
    x0 = (int)ax; x1 = (int)bx; y0 = (int)ay; y1 = (int)by;
    return true;
}

__device__ __forceinline__ u64 rs_key(float zf, int f) { return ((u64)key_of(zf) << 32) | (unsigned)f; }

// face id of a pixel from the fourth rast channel: 0 for background and for anything that is not an id in [1, F]
__device__ __forceinline__ int rs_id(const float* __restrict__ rast, int64_t pix, int64_t F) {
    const float r = rast[pix * 4 + 3];
    return (r >= 1.0f && r <= (float)F) ? (int)r : 0;
}

// ---- the two modes ------------------------------------------------------------------------------------------------------------------
// What a kernel asks of its mode: the image and the face of a key, the key of (image, face), the pos batch an image reads, the id of a
// pixel (0: background for this image), and where the adjacency keeps a face's row and what its entries mean.
struct MapInst {       // instanced: every image draws all F faces from its own pos batch; key = b F + f
    __device__ __forceinline__ int64_t image(int64_t key, int64_t F) const { return key / F; }
    __device__ __forceinline__ int64_t face(int64_t key, int64_t b, int64_t F) const { return key - b * F; }
    __device__ __forceinline__ int64_t key(int64_t b, int64_t f, int64_t F) const { return b * F + f; }
    __device__ __forceinline__ int64_t pos_batch(int64_t b) const { return b; }
    __device__ __forceinline__ int id(const float* __restrict__ rast, int64_t pix, int64_t, int64_t F) const { return rs_id(rast, pix, F); }
    __device__ __forceinline__ size_t adj_row(int64_t, int t) const { return (size_t)t; }
    __device__ __forceinline__ int adj_face(int64_t, int opp) const { return opp; }
};

struct MapRange {      // range mode: image b draws faces [start_b, start_b + count_b) from the one pos; key = the item
    const int* __restrict__ rt;               // (B, 3): start, count, item_ptr
    int B;
    __device__ __forceinline__ int64_t image(int64_t key, int64_t) const {        // the last image whose item_ptr is <= key (empty ranges are passed over)
        int lo = 0, hi = B;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rt[3 * mid + 2] <= key) lo = mid; else hi = mid;
        }
        return lo;
    }
    __device__ __forceinline__ int64_t face(int64_t key, int64_t b, int64_t) const { return rt[3 * b] + (key - rt[3 * b + 2]); }
    __device__ __forceinline__ int64_t key(int64_t b, int64_t f, int64_t) const { return rt[3 * b + 2] + (f - rt[3 * b]); }
    __device__ __forceinline__ int64_t pos_batch(int64_t) const { return 0; }
    // an id outside [start_b + 1, start_b + count_b] (a rast edited by the caller, or of another call) is background
    __device__ __forceinline__ int id(const float* __restrict__ rast, int64_t pix, int64_t b, int64_t) const {
        const float r = rast[pix * 4 + 3];
        const int s = rt[3 * b], c = rt[3 * b + 1];
        return (r >= (float)(s + 1) && r <= (float)(s + c)) ? (int)r : 0;
    }
    __device__ __forceinline__ size_t adj_row(int64_t b, int t) const { return (size_t)(rt[3 * b + 2] + (t - rt[3 * b])); }
    __device__ __forceinline__ int adj_face(int64_t b, int opp) const { return rt[3 * b] + (opp - rt[3 * b + 2]); }      // entries are items
};

// Depth peeling: a mode's map together with the previous layer, given to the two depth kernels in place of the map itself. floor_key:
// the key that the previous layer's pixel won with (key_of maps -0 and +0 to one key and rast keeps z/w bit for bit), ~0 -- above every key --
// where that pixel is background for image b; it reads the (z/w, id) half of the pixel's rast row. The kernels submit a fragment only
// above the floor of its pixel; with a plain map the `if constexpr` is discarded and their source is what it was.
template <class Map>
struct Peel : Map {
    const float* __restrict__ prev;
    __device__ __forceinline__ u64 floor_key(int64_t pix, int64_t b, int64_t F) const {
        const int id = this->id(prev, pix, b, F);
        return id ? rs_key(prev[pix * 4 + 2], id - 1) : ~0ull;
    }
};
template <class Map> struct is_peel { static constexpr bool value = false; };
template <class Map> struct is_peel<Peel<Map>> { static constexpr bool value = true; };

// one thread per key (b, f): small triangles rasterized here, large ones only counted in tiles
template <class Map>
__global__ __launch_bounds__(256) void k_rs_small(Map map, const float* __restrict__ pos, const int* __restrict__ tri, int64_t nk, int64_t V,
                                                  int64_t F, int H, int W, u64* __restrict__ depth, int* __restrict__ tiles) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nk) return;
    const int64_t b = map.image(k, F), f = map.face(k, b, F);
    const RTri t = rs_setup(pos, tri, map.pos_batch(b), V, f);
    int x0, x1, y0, y1, nt = 0;
    if (rs_visible(t) && rs_bbox(t, H, W, x0, x1, y0, y1)) {
        const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
        if ((int64_t)bw * bh > RS_SMALL) {
            nt = ((bw + RS_TILE - 1) / RS_TILE) * ((bh + RS_TILE - 1) / RS_TILE);
        } else {
            u64* img = depth + (size_t)b * H * W;
            for (int y = y0; y <= y1; ++y) {
                const double py = rs_centre(y, H);
                for (int x = x0; x <= x1; ++x) {
                    double E[3];
                    float zf;
                    if (rs_cover(t, rs_centre(x, W), py, E, zf)) {
                        if constexpr (is_peel<Map>::value)
                            if (!(rs_key(zf, (int)f) > map.floor_key((b * H + y) * W + x, b, F))) continue;
                        atomicMin(&img[(size_t)y * W + x], rs_key(zf, (int)f));
                    }
                }
            }
        }
    }
    tiles[k] = nt;
}

// the cooperative path: tile number t -> key k (toff[k] <= t < toff[k + 1]) and tile t - toff[k] of its box, a pixel per thread
template <class Map>
__global__ __launch_bounds__(256) void k_rs_large(Map map, const float* __restrict__ pos, const int* __restrict__ tri, int64_t nk, int64_t V,
                                                  int64_t F, int H, int W, const int* __restrict__ toff, u64* __restrict__ depth) {
    const int total = toff[nk];
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
        int64_t lo = 0, hi = nk;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (toff[mid] <= tile) lo = mid; else hi = mid;
        }
        const int64_t b = map.image(lo, F), f = map.face(lo, b, F);
        const RTri t = rs_setup(pos, tri, map.pos_batch(b), V, f);
        int x0, x1, y0, y1;
        if (!rs_bbox(t, H, W, x0, x1, y0, y1)) continue;
        const int per_row = (x1 - x0 + RS_TILE) / RS_TILE;
        const int j = tile - toff[lo];
        const int x = x0 + (j % per_row) * RS_TILE + (int)(threadIdx.x % RS_TILE);
        const int y = y0 + (j / per_row) * RS_TILE + (int)(threadIdx.x / RS_TILE);
        if (x > x1 || y > y1) continue;
        double E[3];
        float zf;
        if (rs_cover(t, rs_centre(x, W), rs_centre(y, H), E, zf)) {
            if constexpr (is_peel<Map>::value)
                if (!(rs_key(zf, (int)f) > map.floor_key((b * H + y) * W + x, b, F))) continue;
            atomicMin(&depth[((size_t)b * H + y) * W + x], rs_key(zf, (int)f));
        }
    }
}

template <class Map>
__global__ __launch_bounds__(256) void k_rs_resolve(Map map, const float* __restrict__ pos, const int* __restrict__ tri, int B, int64_t V, int64_t F,
                                                    int H, int W, const u64* __restrict__ depth, float* __restrict__ rast) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    if (pix >= B * HW) return;
    const u64 key = depth[pix];
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (key != ~0ull) {
        const int64_t b = pix / HW, r = pix - b * HW, y = r / W, x = r - y * W;
        const int f = (int)(unsigned)(key & 0xffffffffull);
        const RTri t = rs_setup(pos, tri, map.pos_batch(b), V, f);
        double E[3];
        float zf = 0.0f;
        rs_cover(t, rs_centre((int)x, W), rs_centre((int)y, H), E, zf);
        const double S = (E[0] + E[1]) + E[2];
        out = make_float4((float)(E[0] / S), (float)(E[1] / S), zf, (float)(f + 1));
    }
    *reinterpret_cast<float4*>(rast + pix * 4) = out;
}

template <class Map>
__global__ __launch_bounds__(256) void k_rs_keys(Map map, const float* __restrict__ rast, int64_t N, int64_t HW, int64_t F, int64_t nk,
                                                 int* __restrict__ keys) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= N) return;
    const int64_t b = pix / HW;
    const int id = map.id(rast, pix, b, F);
    keys[pix] = id ? (int)map.key(b, id - 1, F) : (int)nk;
}

// ---- sums in pixel order ---------------------------------------------------------------------------------------------------------
// rows[key * stride + off + q] (q < K) = the sum of R::add over the pixels of `key` in sorted order, by seg_sum of groupby.h (a fixed
// order of additions)
template <class R>
struct RsRows {
    R r;
    const int* __restrict__ order; const int* __restrict__ seg; int stride, off; float* __restrict__ rows;
    __device__ __forceinline__ int count(int64_t key) const { return seg[key + 1] - seg[key]; }
    __device__ __forceinline__ void walk(int64_t key, int start, int step, float (&acc)[R::K]) const {
        const int e = seg[key + 1];
        for (int i = seg[key] + start; i < e; i += step) r.add(order[i], key, acc);
    }
    __device__ __forceinline__ void store(int64_t key, const float (&acc)[R::K]) const {
#pragma unroll
        for (int q = 0; q < R::K; ++q) rows[key * stride + off + q] = acc[q];
    }
};

template <class R>
__global__ __launch_bounds__(256) void k_rs_seg_sum(R r, const int* __restrict__ order, const int* __restrict__ seg, int64_t nk, int stride, int off,
                                                    float* __restrict__ rows) {
    seg_sum<R::K>(nk, RsRows<R>{r, order, seg, stride, off, rows});
}

// rasterize backward: d (gu u + gv v) / d (x, y, w) of the three corners, u = E_0 / S, v = E_1 / S
template <class Map>
struct RowRaster {
    static constexpr int K = 9;
    Map map; const float* pos; const int* tri; const float* grad; int64_t V, F; int H, W;
    __device__ __forceinline__ void add(int pix, int64_t key, float (&acc)[K]) const {
        const int64_t b = map.image(key, F), f = map.face(key, b, F), HW = (int64_t)H * W, rr = pix - b * HW, y = rr / W, x = rr - y * W;
        const RTri t = rs_setup(pos, tri, map.pos_batch(b), V, f);
        const double px = rs_centre((int)x, W), py = rs_centre((int)y, H);
        double E[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) E[i] = (px * t.c[i][0] + py * t.c[i][1]) + t.c[i][2];
        const double S = (E[0] + E[1]) + E[2];
        const double gu = grad[(size_t)pix * 4], gv = grad[(size_t)pix * 4 + 1];
        const double dot = gu * (E[0] / S) + gv * (E[1] / S);
        const double dE[3] = {(gu - dot) / S, (gv - dot) / S, -dot / S};
        const double p[3] = {px, py, 1.0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 a = t.q[(j + 1) % 3], c = t.q[(j + 2) % 3];        // q_{j+1}, q_{j-1}
            const double qa[3] = {a.x, a.y, a.w}, qc[3] = {c.x, c.y, c.w};
            // dE_{j-1}/dq_j = q_{j+1} x p ; dE_{j+1}/dq_j = p x q_{j-1}
            const double m1 = dE[(j + 2) % 3], m2 = dE[(j + 1) % 3];
            const double g0 = m1 * (qa[1] * p[2] - qa[2] * p[1]) + m2 * (p[1] * qc[2] - p[2] * qc[1]);
            const double g1 = m1 * (qa[2] * p[0] - qa[0] * p[2]) + m2 * (p[2] * qc[0] - p[0] * qc[2]);
            const double g2 = m1 * (qa[0] * p[1] - qa[1] * p[0]) + m2 * (p[0] * qc[1] - p[1] * qc[0]);
            acc[3 * j] += (float)g0;
            acc[3 * j + 1] += (float)g1;
            acc[3 * j + 2] += (float)g2;
        }
    }
};

// interpolate backward, channel c: (u g, v g, (1 - u - v) g) for the three corners
struct RowInterp {
    static constexpr int K = 3;
    const float* rast; const float* grad; int C, c;
    __device__ __forceinline__ void add(int pix, int64_t, float (&acc)[K]) const {
        const float u = rast[(size_t)pix * 4], v = rast[(size_t)pix * 4 + 1], w = (1.0f - u) - v;
        const float g = grad[(size_t)pix * C + c];
        acc[0] += u * g;
        acc[1] += v * g;
        acc[2] += w * g;
    }
};

// ---- antialias -----------------------------------------------------------------------------------------------------------------------
// The pair (P, Q), Q the right (axis 0) or upper (axis 1) neighbour of P, with different ids. The nearer pixel n (smaller z/w; background
// is infinitely far; equal depths: P) owns triangle t. Among t's silhouette edges (no neighbour face, or one whose D has the other sign
// in this view) with both ends at w > 0 and of the pair's orientation (an edge with |dY| > |dX| in pixels belongs to horizontal pairs, any
// other to vertical pairs, as in Laine et al. 2020: a pixel is then never blended across one edge in both directions), the first in
// corner order whose screen projection crosses the line through the two centres between them gives alpha in [0, 1], the distance from
// n's centre to the crossing in pixels. The blend, with the other pixel o:
//   alpha > 1/2: o += (alpha - 1/2) (c_n - c_o);  alpha < 1/2: n += (1/2 - alpha) (c_o - c_n)
// i.e. the receiving pixel r gains fac (c_other - c_r), fac = |alpha - 1/2|.
struct AAHit {
    bool found;
    int near;        // 0: P, 1: Q
    int e;           // edge of t: corners e and e + 1
    int t;
    float alpha;
    float dA[3], dB[3];   // d alpha / d (x, y, w) of corners e and e + 1
};

template <class Map>
struct AAMesh {
    Map map; const float* pos; const int* tri; const int* adj; const float* rast; int64_t V, F; int H, W;
};

template <class Map>
__device__ __forceinline__ AAHit aa_pair(const AAMesh<Map>& m, int64_t b, int64_t pixP, int64_t pixQ, int xP, int yP, int axis) {
    AAHit h;
    h.found = false;
    const int idP = m.map.id(m.rast, pixP, b, m.F), idQ = m.map.id(m.rast, pixQ, b, m.F);
    const size_t pb = (size_t)m.map.pos_batch(b) * m.V;
    h.near = 0; h.e = 0; h.t = 0; h.alpha = 0.0f;
    if (idP == idQ) return h;
    const float zP = idP ? m.rast[pixP * 4 + 2] : __int_as_float(0x7f800000), zQ = idQ ? m.rast[pixQ * 4 + 2] : __int_as_float(0x7f800000);
    h.near = (zP <= zQ) ? 0 : 1;
    const int t = (h.near ? idQ : idP) - 1;
    h.t = t;
    const float xn = (float)(xP + (h.near && axis == 0 ? 1 : 0)) + 0.5f, yn = (float)(yP + (h.near && axis == 1 ? 1 : 0)) + 0.5f;
    const float dir = h.near ? -1.0f : 1.0f;
    float4 q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = *reinterpret_cast<const float4*>(m.pos + (pb + m.tri[3 * (size_t)t + i]) * 4);
    const bool st = rs_det(q[0], q[1], q[2]) > 0.0;
    const float hw = 0.5f * (float)m.W, hh = 0.5f * (float)m.H;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (h.found) continue;
        const float4 A = q[e], Bv = q[(e + 1) % 3];
        if (!(A.w > 0.0f && Bv.w > 0.0f)) continue;
        const int across = m.adj[3 * m.map.adj_row(b, t) + e];
        if (across >= 0) {
            const int opp = m.map.adj_face(b, across);
            float4 o[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = *reinterpret_cast<const float4*>(m.pos + (pb + m.tri[3 * (size_t)opp + i]) * 4);
            if ((rs_det(o[0], o[1], o[2]) > 0.0) == st) continue;
        }
        const float XA = (A.x / A.w + 1.0f) * hw, YA = (A.y / A.w + 1.0f) * hh;
        const float XB = (Bv.x / Bv.w + 1.0f) * hw, YB = (Bv.y / Bv.w + 1.0f) * hh;
        const bool steep = fabsf(YB - YA) > fabsf(XB - XA);          // mostly vertical: horizontal pairs only; else vertical pairs only
        if (steep == (axis == 1)) continue;
        const float alA = axis ? YA : XA, alB = axis ? YB : XB, acA = axis ? XA : YA, acB = axis ? XB : YB;
        const float line = axis ? xn : yn, start = axis ? yn : xn;
        if ((acA < line) == (acB < line)) continue;
        const float d = acB - acA;
        const float tt = (line - acA) / d;
        const float hit = alA + tt * (alB - alA);
        const float alpha = (hit - start) * dir;
        if (!(alpha >= 0.0f && alpha <= 1.0f)) continue;
        h.found = true;
        h.e = e;
        h.alpha = alpha;
        const float d_alA = dir * (1.0f - tt), d_alB = dir * tt;
        const float d_acA = dir * (alB - alA) * (tt - 1.0f) / d, d_acB = dir * (alB - alA) * (-tt / d);
        const float dXA = axis ? d_acA : d_alA, dYA = axis ? d_alA : d_acA, dXB = axis ? d_acB : d_alB, dYB = axis ? d_alB : d_acB;
        h.dA[0] = dXA * hw / A.w; h.dA[1] = dYA * hh / A.w; h.dA[2] = -(dXA * hw * A.x + dYA * hh * A.y) / (A.w * A.w);
        h.dB[0] = dXB * hw / Bv.w; h.dB[1] = dYB * hh / Bv.w; h.dB[2] = -(dXB * hw * Bv.x + dYB * hh * Bv.y) / (Bv.w * Bv.w);
    }
    return h;
}

// pair d of a pixel, in the fixed order left, right, below, above (false: outside the image); selfP: the pixel is P of the pair
template <class Map>
__device__ __forceinline__ bool aa_neighbour(const AAMesh<Map>& m, int64_t b, int x, int y, int d, AAHit& h, bool& selfP, int64_t& other) {
    const int64_t pix = ((int64_t)b * m.H + y) * m.W + x;
    if (d == 0) { if (x == 0) return false; other = pix - 1; selfP = false; h = aa_pair(m, b, other, pix, x - 1, y, 0); }
    else if (d == 1) { if (x + 1 >= m.W) return false; other = pix + 1; selfP = true; h = aa_pair(m, b, pix, other, x, y, 0); }
    else if (d == 2) { if (y == 0) return false; other = pix - m.W; selfP = false; h = aa_pair(m, b, other, pix, x, y - 1, 1); }
    else { if (y + 1 >= m.H) return false; other = pix + m.W; selfP = true; h = aa_pair(m, b, pix, other, x, y, 1); }
    return h.found;
}

__device__ __forceinline__ bool aa_receiver(const AAHit& h, bool selfP) {
    const bool self_near = (h.near == 0) == selfP;
    return h.alpha > 0.5f ? !self_near : self_near;
}

template <class Map>
__global__ __launch_bounds__(256) void k_aa_forward(AAMesh<Map> m, int B, const float* __restrict__ color, int C, float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)m.H * m.W;
    if (pix >= B * HW) return;
    const int64_t b = pix / HW, r = pix - b * HW;
    const int y = (int)(r / m.W), x = (int)(r - (int64_t)y * m.W);
    for (int c = 0; c < C; ++c) out[pix * C + c] = color[pix * C + c];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        AAHit h;
        bool selfP;
        int64_t other;
        if (!aa_neighbour(m, b, x, y, d, h, selfP, other) || !aa_receiver(h, selfP)) continue;
        const float fac = h.alpha > 0.5f ? h.alpha - 0.5f : 0.5f - h.alpha;
        for (int c = 0; c < C; ++c) out[pix * C + c] = out[pix * C + c] + fac * (color[other * C + c] - color[pix * C + c]);
    }
}

// gradient of the colour: g_col[p] = g[p] + per pair (p receives: -fac g[p]; the other receives: +fac g[other])
template <class Map>
__global__ __launch_bounds__(256) void k_aa_grad_color(AAMesh<Map> m, int B, const float* __restrict__ g, int C, float* __restrict__ gcol) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)m.H * m.W;
    if (pix >= B * HW) return;
    const int64_t b = pix / HW, r = pix - b * HW;
    const int y = (int)(r / m.W), x = (int)(r - (int64_t)y * m.W);
    for (int c = 0; c < C; ++c) gcol[pix * C + c] = g[pix * C + c];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        AAHit h;
        bool selfP;
        int64_t other;
        if (!aa_neighbour(m, b, x, y, d, h, selfP, other)) continue;
        const float fac = h.alpha > 0.5f ? h.alpha - 0.5f : 0.5f - h.alpha;
        const bool mine = aa_receiver(h, selfP);
        for (int c = 0; c < C; ++c) {
            const float dg = mine ? -fac * g[pix * C + c] : fac * g[other * C + c];
            gcol[pix * C + c] = gcol[pix * C + c] + dg;
        }
    }
}

// antialias backward, position rows: the pairs in which this pixel is the nearer one (its own triangle t = key's face)
template <class Map>
struct RowAA {
    static constexpr int K = 9;
    AAMesh<Map> m; const float* color; const float* g; int C; float boost;
    __device__ __forceinline__ void add(int pix, int64_t key, float (&acc)[K]) const {
        const int64_t HW = (int64_t)m.H * m.W, b = m.map.image(key, m.F), r = pix - b * HW;
        const int y = (int)(r / m.W), x = (int)(r - (int64_t)y * m.W);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            AAHit h;
            bool selfP;
            int64_t other;
            if (!aa_neighbour(m, b, x, y, d, h, selfP, other) || (h.near == 0) != selfP) continue;
            const bool far_gets = h.alpha > 0.5f;          // receiver: the other pixel (far) or this one (near)
            const int64_t rcv = far_gets ? other : pix, src = far_gets ? pix : other;
            float dl = 0.0f;                               // d L / d fac * d fac / d alpha
            for (int c = 0; c < C; ++c) dl += g[rcv * C + c] * (color[src * C + c] - color[rcv * C + c]);
            dl = (far_gets ? dl : -dl) * boost;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                if (h.e != e) continue;
                const int a = e, bb = (e + 1) % 3;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    acc[3 * a + q] += dl * h.dA[q];
                    acc[3 * bb + q] += dl * h.dB[q];
                }
            }
        }
    }
};

// ---- per vertex ------------------------------------------------------------------------------------------------------------------------
// grad_pos (B, V, 4) = the vertex's corners' (x, y, w) rows in rank order, z = 0
__global__ __launch_bounds__(256) void k_rs_gather_pos(const float* __restrict__ rows, const int* __restrict__ vptr, const int* __restrict__ order,
                                                       int B, int64_t V, int64_t F, float* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)B * V) return;
    const int64_t b = k / V, v = k - b * V;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int r = vptr[v]; r < vptr[v + 1]; ++r) {
        const int c = order[r];
        const float* row = rows + ((size_t)b * F + c / 3) * 9 + 3 * (c % 3);
        s0 += row[0]; s1 += row[1]; s2 += row[2];
    }
    *reinterpret_cast<float4*>(out + k * 4) = make_float4(s0, s1, 0.0f, s2);
}

// grad_attr (Ba, V, C): Ba == B per batch; Ba == 1 the batches summed in order b = 0 .. B - 1
__global__ __launch_bounds__(256) void k_rs_gather_attr(const float* __restrict__ rows, const int* __restrict__ vptr, const int* __restrict__ order,
                                                        int B, int Ba, int64_t V, int64_t F, int C, float* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)Ba * V * C) return;
    const int64_t c = k % C, kv = k / C, ba = kv / V, v = kv - ba * V;
    const int b0 = Ba == 1 ? 0 : (int)ba, b1 = Ba == 1 ? B : (int)ba + 1;
    float s = 0.0f;
    for (int b = b0; b < b1; ++b)
        for (int r = vptr[v]; r < vptr[v + 1]; ++r) {
            const int cr = order[r];
            s += rows[((size_t)b * F + cr / 3) * (3 * (size_t)C) + 3 * c + (cr % 3)];
        }
    out[k] = s;
}

// Range mode: grad_pos (V, 4) and grad_attr (V, C). Per image b a partial sum from zero over the vertex's corners whose face lies in range
// b, in rank order (they are in the relative order of the slice's own ranking: ls_corner_ranks ranks by ascending corner id) -- bit for
// bit the gradient of the slice call -- and the partial sums added in ascending b, starting from image 0's.
__global__ __launch_bounds__(256) void k_rg_gather_pos(const float* __restrict__ rows, const int* __restrict__ vptr, const int* __restrict__ order,
                                                       const int* __restrict__ rt, int B, int64_t V, float* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int r0 = vptr[v], r1 = vptr[v + 1];
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
    for (int b = 0; b < B; ++b) {
        const int start = rt[3 * b], count = rt[3 * b + 1], ptr = rt[3 * b + 2];
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int r = r0; r < r1; ++r) {
            const int c = order[r], f = c / 3;
            if (f < start || f - start >= count) continue;
            const float* row = rows + (size_t)(ptr + (f - start)) * 9 + 3 * (c % 3);
            s0 += row[0]; s1 += row[1]; s2 += row[2];
        }
        if (b == 0) { t0 = s0; t1 = s1; t2 = s2; }
        else { t0 = t0 + s0; t1 = t1 + s1; t2 = t2 + s2; }
    }
    *reinterpret_cast<float4*>(out + v * 4) = make_float4(t0, t1, 0.0f, t2);
}

__global__ __launch_bounds__(256) void k_rg_gather_attr(const float* __restrict__ rows, const int* __restrict__ vptr, const int* __restrict__ order,
                                                        const int* __restrict__ rt, int B, int64_t V, int C, float* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= V * C) return;
    const int64_t c = k % C, v = k / C;
    const int r0 = vptr[v], r1 = vptr[v + 1];
    float t = 0.0f;
    for (int b = 0; b < B; ++b) {
        const int start = rt[3 * b], count = rt[3 * b + 1], ptr = rt[3 * b + 2];
        float s = 0.0f;
        for (int r = r0; r < r1; ++r) {
            const int cr = order[r], f = cr / 3;
            if (f < start || f - start >= count) continue;
            s += rows[(size_t)(ptr + (f - start)) * (3 * (size_t)C) + 3 * c + (cr % 3)];
        }
        t = b == 0 ? s : t + s;
    }
    out[k] = t;
}

// ---- interpolate forward and the rast gradient -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rs_interp(const float* __restrict__ attr, int Ba, int64_t V, int C, const float* __restrict__ rast,
                                                   int B, int64_t HW, const int* __restrict__ tri, int64_t F, float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= B * HW) return;
    const int id = rs_id(rast, pix, F);
    if (!id) {
        for (int c = 0; c < C; ++c) out[pix * C + c] = 0.0f;
        return;
    }
    const int64_t b = Ba == 1 ? 0 : pix / HW;
    const float u = rast[pix * 4], v = rast[pix * 4 + 1], w = (1.0f - u) - v;
    const float* a0 = attr + ((size_t)b * V + tri[3 * (size_t)(id - 1)]) * C;
    const float* a1 = attr + ((size_t)b * V + tri[3 * (size_t)(id - 1) + 1]) * C;
    const float* a2 = attr + ((size_t)b * V + tri[3 * (size_t)(id - 1) + 2]) * C;
    for (int c = 0; c < C; ++c) out[pix * C + c] = (u * a0[c] + v * a1[c]) + w * a2[c];
}

__global__ __launch_bounds__(256) void k_rs_interp_grad_rast(const float* __restrict__ attr, int Ba, int64_t V, int C, const float* __restrict__ rast,
                                                             int B, int64_t HW, const int* __restrict__ tri, int64_t F, const float* __restrict__ g,
                                                             float* __restrict__ grast) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= B * HW) return;
    const int id = rs_id(rast, pix, F);
    float du = 0.0f, dv = 0.0f;
    if (id) {
        const int64_t b = Ba == 1 ? 0 : pix / HW;
        const float* a0 = attr + ((size_t)b * V + tri[3 * (size_t)(id - 1)]) * C;
        const float* a1 = attr + ((size_t)b * V + tri[3 * (size_t)(id - 1) + 1]) * C;
        const float* a2 = attr + ((size_t)b * V + tri[3 * (size_t)(id - 1) + 2]) * C;
        for (int c = 0; c < C; ++c) {
            const float gc = g[pix * C + c];
            du += gc * (a0[c] - a2[c]);
            dv += gc * (a1[c] - a2[c]);
        }
    }
    *reinterpret_cast<float4*>(grast + pix * 4) = make_float4(du, dv, 0.0f, 0.0f);
}

// ---- edge adjacency ---------------------------------------------------------------------------------------------------------------------
// (KeyEdge, the two-word key of a half-edge, is in radix.h: subdiv.hip sorts by it too)

// range mode: half-edge h = 3 n + e of item n = (b, f): KeyEdge's two words over face f, and the image as word 2 -- an edge pairs its
// half-edges within one image only
struct KeyItemEdge {
    const int* tri; MapRange map;
    __device__ __forceinline__ unsigned word(int h, int w) const {
        const int n = h / 3, e = h - 3 * n;
        const int64_t b = map.image(n, 0);
        if (w == 2) return (unsigned)b;
        const int64_t f = map.face(n, b, 0);
        const unsigned a = (unsigned)tri[3 * f + e], c = (unsigned)tri[3 * f + (e + 1) % 3];
        return w == 0 ? min(a, c) : max(a, c);
    }
};

// sorted half-edges: an edge with exactly two half-edges pairs them; any other count leaves -1 (boundary or non-manifold). adj holds the
// face (instanced) or the item (range mode) of the other half-edge.
template <class Key, int WORDS>
__global__ __launch_bounds__(256) void k_rs_adjacency(Key key, const int* __restrict__ sorted, int64_t n, int* __restrict__ adj) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int h = sorted[i];
    unsigned a[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) a[w] = key.word(h, w);
    auto same = [&](int64_t j) {
        if (j < 0 || j >= n) return false;
        bool eq = true;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) eq = eq && key.word(sorted[j], w) == a[w];
        return eq;
    };
    int other = -1;
    if (same(i + 1) && !same(i - 1) && !same(i + 2)) other = sorted[i + 1];
    if (same(i - 1) && !same(i - 2) && !same(i + 1)) other = sorted[i - 1];
    adj[h] = other >= 0 ? other / 3 : -1;
}

}  // namespace ls

using namespace ls;

namespace {

struct RsWs {          // the workspace's regions (sized from the shapes alone)
    u64* depth;
    int *tiles, *toff, *bsum, *keys;
    SortScratch sort;
    float* rows;
    size_t total;
};

// N pixels, nk keys (B F faces of an instanced frame, the items of a range-mode one)
RsWs rs_carve_keys(void* ws, int64_t N, int64_t nk, int64_t C) {
    WsWalk w(ws);
    u64* depth = w.take<u64>((size_t)N);
    int* tiles = w.take<int>((size_t)(nk + 1));
    int* toff = w.take<int>((size_t)(nk + 2));
    int* bsum = w.take<int>((size_t)scan_scratch_ints(nk));
    int* keys = w.take<int>((size_t)N);
    const SortScratch sort = sort_scratch_take(w, N, false);   // the pixel order sorts by gathered key bytes
    float* rows = w.take<float>((size_t)nk * (size_t)std::max<int64_t>(9, 3 * C));
    return {depth, tiles, toff, bsum, keys, sort, rows, w.bytes()};
}

RsWs rs_carve(void* ws, int64_t B, int64_t F, int64_t H, int64_t W, int64_t C) { return rs_carve_keys(ws, B * H * W, B * F, C); }

int rs_check(int64_t B, int64_t V, int64_t F, int H, int W, const char* who) {
    LS_REQUIRE(B >= 1 && V >= 0 && F >= 0 && H >= 1 && W >= 1 && H <= 4096 && W <= 4096, LS_E_INVALID, "%s: bad sizes (B %lld V %lld F %lld H %d W %d)",
               who, (long long)B, (long long)V, (long long)F, H, W);
    LS_REQUIRE(B * H * W < ((int64_t)1 << 31) - 1 && B * F < ((int64_t)1 << 31) - 1 && F < ((int64_t)1 << 24) && B * V < ((int64_t)1 << 31),
               LS_E_OVERFLOW, "%s: the problem does not fit the int32 index space (B %lld V %lld F %lld H %d W %d)", who, (long long)B,
               (long long)V, (long long)F, H, W);
    return LS_OK;
}

// range mode: B images, N items over F faces and V shared vertices
int rg_check(int64_t B, int64_t N, int64_t V, int64_t F, int H, int W, const char* who) {
    LS_REQUIRE(B >= 1 && N >= 0 && V >= 0 && F >= 0 && H >= 1 && W >= 1 && H <= 4096 && W <= 4096, LS_E_INVALID,
               "%s: bad sizes (B %lld N %lld V %lld F %lld H %d W %d)", who, (long long)B, (long long)N, (long long)V, (long long)F, H, W);
    LS_REQUIRE(B * H * W < ((int64_t)1 << 31) - 1 && 3 * N < ((int64_t)1 << 31) - 1 && F < ((int64_t)1 << 24) && V < ((int64_t)1 << 31),
               LS_E_OVERFLOW, "%s: the problem does not fit the int32 index space (B %lld N %lld V %lld F %lld H %d W %d)", who, (long long)B,
               (long long)N, (long long)V, (long long)F, H, W);
    return LS_OK;
}

// ---- a mode above the kernels: its key map, B images, nk keys (the workspace is rs_carve_keys(ws, B H W, nk, C)), V vertices (per image when
// instanced) and F faces -- and, by overload, its size check and the launches of its two gather kernels (whose summation orders differ: the
// slice law). Each extern "C" function below hands its mode `m`, its name `who` and its pointer test `ok` to a body written once -------------
template <class Map>
struct Mode {
    Map map;
    int64_t B, nk, V, F;
};
using Inst = Mode<MapInst>;
using Range = Mode<MapRange>;

Inst inst(int64_t B, int64_t V, int64_t F) { return {MapInst{}, B, B * F, V, F}; }
Range range(const int32_t* ranges, int64_t B, int64_t N, int64_t V, int64_t F) { return {MapRange{ranges, (int)B}, B, N, V, F}; }

int rs_check(const Inst& m, int H, int W, const char* who) { return rs_check(m.B, m.V, m.F, H, W, who); }
int rs_check(const Range& m, int H, int W, const char* who) { return rg_check(m.B, m.nk, m.V, m.F, H, W, who); }

void rs_gather_pos(const Inst& m, const float* rows, const int32_t* vptr, const int32_t* corner_order, float* grad_pos, hipStream_t st) {
    if (m.B * m.V > 0)
        hipLaunchKernelGGL(k_rs_gather_pos, dim3(div_up(m.B * m.V, 256)), dim3(256), 0, st, rows, vptr, corner_order, (int)m.B, m.V, m.F, grad_pos);
}
void rs_gather_pos(const Range& m, const float* rows, const int32_t* vptr, const int32_t* corner_order, float* grad_pos, hipStream_t st) {
    if (m.V > 0)
        hipLaunchKernelGGL(k_rg_gather_pos, dim3(div_up(m.V, 256)), dim3(256), 0, st, rows, vptr, corner_order, m.map.rt, m.map.B, m.V, grad_pos);
}

void rs_gather_attr(const Inst& m, const float* rows, const int32_t* vptr, const int32_t* corner_order, int64_t attr_batch, int C, float* grad_attr,
                    hipStream_t st) {
    if (attr_batch * m.V * C > 0)
        hipLaunchKernelGGL(k_rs_gather_attr, dim3(div_up(attr_batch * m.V * C, 256)), dim3(256), 0, st, rows, vptr, corner_order, (int)m.B,
                           (int)attr_batch, m.V, m.F, C, grad_attr);
}
void rs_gather_attr(const Range& m, const float* rows, const int32_t* vptr, const int32_t* corner_order, int64_t, int C, float* grad_attr,
                    hipStream_t st) {
    if (m.V * C > 0)
        hipLaunchKernelGGL(k_rg_gather_attr, dim3(div_up(m.V * C, 256)), dim3(256), 0, st, rows, vptr, corner_order, m.map.rt, m.map.B, m.V, C,
                           grad_attr);
}

// PEEL: the layer behind `prev` (the rast of the layer before, of the same mode and sizes): the depth kernels get Peel<Map>; otherwise
// prev is not looked at
template <bool PEEL, class Map>
int rs_forward(const Mode<Map>& m, const char* who, bool ok, const float* pos, const int32_t* tri, int H, int W, const float* prev, float* rast,
               void* ws, size_t ws_bytes, int device, void* stream) {
    int rc = rs_check(m, H, W, who);
    if (rc) return rc;
    const RsWs L = rs_carve_keys(ws, m.B * H * W, m.nk, 0);
    LS_REQUIRE(ok, LS_E_INVALID, "%s: null argument", who);
    LS_REQUIRE(!PEEL || prev != rast, LS_E_INVALID, "%s: prev_rast and rast are the same buffer (the layer before is read while this one is written)",
               who);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    u64* depth = L.depth;
    const int64_t N = m.B * H * W, nk = m.nk;
    LS_HIP(hipMemsetAsync(depth, 0xff, 8 * (size_t)N, st));
    if (nk > 0) {
        const auto dmap = [&] {
            if constexpr (PEEL) return Peel<Map>{m.map, prev};
            else return m.map;
        }();
        using DepthMap = std::remove_const_t<decltype(dmap)>;
        hipLaunchKernelGGL(k_rs_small<DepthMap>, dim3(div_up(nk, 256)), dim3(256), 0, st, dmap, pos, tri, nk, m.V, m.F, H, W, depth, L.tiles);
        rc = exclusive_scan(L.tiles, nk, L.toff, L.bsum, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_rs_large<DepthMap>, dim3(RS_LARGE_GRID), dim3(256), 0, st, dmap, pos, tri, nk, m.V, m.F, H, W, (const int*)L.toff, depth);
    }
    hipLaunchKernelGGL(k_rs_resolve<Map>, dim3(div_up(N, 256)), dim3(256), 0, st, m.map, pos, tri, (int)m.B, m.V, m.F, H, W, (const u64*)depth,
                       rast);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

template <class Map>
int rs_pixel_order(const Mode<Map>& m, const char* who, bool ok, const float* rast, int H, int W, int32_t* order, int32_t* seg, void* ws,
                   size_t ws_bytes, int device, void* stream) {
    int rc = rs_check(m, H, W, who);
    if (rc) return rc;
    const RsWs L = rs_carve_keys(ws, m.B * H * W, m.nk, 0);
    LS_REQUIRE(ok, LS_E_INVALID, "%s: null argument", who);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = m.B * H * W, nk = m.nk;
    hipLaunchKernelGGL(k_rs_keys<Map>, dim3(div_up(N, 256)), dim3(256), 0, st, m.map, rast, N, (int64_t)H * W, m.F, nk, L.keys);
    return group_by_key<false>(L.keys, N, nk, order, seg, L.sort, st);
}

template <class Map>
int rs_backward(const Mode<Map>& m, const char* who, bool ok, const float* pos, const int32_t* tri, int H, int W, const float* grad_rast,
                const int32_t* order, const int32_t* seg, const int32_t* vptr, const int32_t* corner_order, float* grad_pos, void* ws,
                size_t ws_bytes, int device, void* stream) {
    int rc = rs_check(m, H, W, who);
    if (rc) return rc;
    const RsWs L = rs_carve_keys(ws, m.B * H * W, m.nk, 0);
    LS_REQUIRE(ok, LS_E_INVALID, "%s: null argument", who);
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nk = m.nk;
    if (nk > 0) {
        RowRaster<Map> r{m.map, pos, tri, grad_rast, m.V, m.F, H, W};
        hipLaunchKernelGGL(k_rs_seg_sum<RowRaster<Map>>, dim3(div_up(nk, 256)), dim3(256), 0, st, r, order, seg, nk, 9, 0, L.rows);
    }
    rs_gather_pos(m, L.rows, vptr, corner_order, grad_pos, st);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// the grad_attr half of interpolate's backward, after its entry point's checks
template <class Map>
void rs_interp_grad_attr(const Mode<Map>& m, const float* rast, int64_t attr_batch, int C, const float* grad_out, const int32_t* order,
                         const int32_t* seg, const int32_t* vptr, const int32_t* corner_order, float* grad_attr, float* rows, hipStream_t st) {
    const int64_t nk = m.nk;
    if (nk > 0)
        for (int c = 0; c < C; ++c) {
            RowInterp r{rast, grad_out, C, c};
            hipLaunchKernelGGL(k_rs_seg_sum<RowInterp>, dim3(div_up(nk, 256)), dim3(256), 0, st, r, order, seg, nk, 3 * C, 3 * c, rows);
        }
    rs_gather_attr(m, rows, vptr, corner_order, attr_batch, C, grad_attr, st);
}

// the ids of n half-edges, the sort's scratch behind them: packed at 4 bytes
struct AdjWs { int* ord_a; SortScratch sort; size_t total; };
AdjWs rs_adjacency_carve(void* ws, int64_t n) {
    WsWalk w(ws);
    int* ord_a = w.take<int>((size_t)n, 4);
    const SortScratch sort = sort_scratch_take(w, n, true, 0, 4);
    return {ord_a, sort, w.bytes()};
}
size_t rs_adjacency_bytes(int64_t nk) { return rs_adjacency_carve(nullptr, 3 * nk).total; }      // nk faces or items

// the n half-edges sorted by the WORDS words of `key` (the last one `last_bytes` wide), each paired with the other one of its edge
template <class Key, int WORDS>
int rs_adjacency(Key key, int64_t n, int last_bytes, int32_t* adj, void* ws, int device, void* stream) {
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const AdjWs w = rs_adjacency_carve(ws, n);
    const int* sorted = nullptr;
    int rc = radix_argsort_words(key, n, WORDS, w.ord_a, w.sort, st, &sorted, last_bytes);
    if (rc) return rc;
    hipLaunchKernelGGL((k_rs_adjacency<Key, WORDS>), dim3(div_up(n, 256)), dim3(256), 0, st, key, sorted, n, adj);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

template <class Map>
int rs_antialias(const Mode<Map>& m, const char* who, bool ok, const float* color, int C, const float* rast, const float* pos, const int32_t* tri,
                 const int32_t* adj, int H, int W, float* out, int device, void* stream) {
    int rc = rs_check(m, H, W, who);
    if (rc) return rc;
    LS_REQUIRE(ok, LS_E_INVALID, "%s: bad argument", who);
    DeviceGuard g(device);
    LS_HIP(g.err);
    AAMesh<Map> mesh{m.map, pos, tri, adj, rast, m.V, m.F, H, W};
    hipLaunchKernelGGL(k_aa_forward<Map>, dim3(div_up(m.B * H * W, 256)), dim3(256), 0, (hipStream_t)stream, mesh, (int)m.B, color, C, out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

template <class Map>
int rs_antialias_backward(const Mode<Map>& m, const char* who, bool ok, const float* color, int C, const float* rast, const float* pos,
                          const int32_t* tri, const int32_t* adj, int H, int W, const float* grad_out, float boost, const int32_t* order,
                          const int32_t* seg, const int32_t* vptr, const int32_t* corner_order, float* grad_color, float* grad_pos, void* ws,
                          size_t ws_bytes, int device, void* stream) {
    int rc = rs_check(m, H, W, who);
    if (rc) return rc;
    const int64_t N = m.B * H * W, nk = m.nk;
    const RsWs L = rs_carve_keys(ws, N, nk, 0);
    LS_REQUIRE(ok, LS_E_INVALID, "%s: bad argument", who);
    LS_REQUIRE(!grad_pos || (order && seg && vptr && ws && (corner_order || m.F == 0)), LS_E_INVALID,
               "%s: grad_pos needs the pixel order, the corner ranking and a workspace", who);
    LS_REQUIRE(!grad_pos || ws_bytes >= L.total, LS_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    AAMesh<Map> mesh{m.map, pos, tri, adj, rast, m.V, m.F, H, W};
    if (grad_color) hipLaunchKernelGGL(k_aa_grad_color<Map>, dim3(div_up(N, 256)), dim3(256), 0, st, mesh, (int)m.B, grad_out, C, grad_color);
    if (grad_pos) {
        if (nk > 0) {
            RowAA<Map> r{mesh, color, grad_out, C, boost};
            hipLaunchKernelGGL(k_rs_seg_sum<RowAA<Map>>, dim3(div_up(nk, 256)), dim3(256), 0, st, r, order, seg, nk, 9, 0, L.rows);
        }
        rs_gather_pos(m, L.rows, vptr, corner_order, grad_pos, st);
    }
    LS_HIP(hipGetLastError());
    return LS_OK;
}

}  // namespace

extern "C" int ls_raster_workspace_bytes(int64_t B, int64_t F, int H, int W, int C, size_t* bytes) {
    int rc = rs_check(B, 0, F, H, W, "ls_raster_workspace_bytes");
    if (rc) return rc;
    LS_REQUIRE(bytes && C >= 0, LS_E_INVALID, "ls_raster_workspace_bytes: bad argument");
    *bytes = rs_carve(nullptr, B, F, H, W, C).total;
    return LS_OK;
}

extern "C" int ls_raster_forward(const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W, float* rast, void* ws,
                                 size_t ws_bytes, int device, void* stream) {
    return rs_forward<false>(inst(B, V, F), "ls_raster_forward", rast && ws && (pos || V == 0) && (tri || F == 0), pos, tri, H, W, nullptr, rast,
                             ws, ws_bytes, device, stream);
}

extern "C" int ls_raster_pixel_order(const float* rast, int64_t B, int64_t F, int H, int W, int32_t* order, int32_t* seg, void* ws,
                                     size_t ws_bytes, int device, void* stream) {
    return rs_pixel_order(inst(B, 0, F), "ls_raster_pixel_order", rast && order && seg && ws, rast, H, W, order, seg, ws, ws_bytes, device, stream);
}

extern "C" int ls_raster_backward(const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W, const float* grad_rast,
                                  const int32_t* order, const int32_t* seg, const int32_t* vptr, const int32_t* corner_order, float* grad_pos,
                                  void* ws, size_t ws_bytes, int device, void* stream) {
    const bool ok = grad_rast && order && seg && vptr && grad_pos && ws && (pos || V == 0) && (tri || F == 0) && (corner_order || F == 0);
    return rs_backward(inst(B, V, F), "ls_raster_backward", ok, pos, tri, H, W, grad_rast, order, seg, vptr, corner_order, grad_pos, ws, ws_bytes,
                       device, stream);
}

extern "C" int ls_raster_interpolate(const float* attr, int64_t attr_batch, int64_t V, int C, const float* rast, int64_t B, int H, int W,
                                     const int32_t* tri, int64_t F, float* out, int device, void* stream) {
    int rc = rs_check(B, V, F, H, W, "ls_raster_interpolate");
    if (rc) return rc;
    LS_REQUIRE(C >= 1 && (attr_batch == 1 || attr_batch == B), LS_E_INVALID, "ls_raster_interpolate: C %d, attribute batch %lld of %lld", C,
               (long long)attr_batch, (long long)B);
    LS_REQUIRE(rast && out && (attr || V == 0) && (tri || F == 0), LS_E_INVALID, "ls_raster_interpolate: null argument");
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = B * H * W;
    hipLaunchKernelGGL(k_rs_interp, dim3(div_up(N, 256)), dim3(256), 0, st, attr, (int)attr_batch, V, C, rast, (int)B, (int64_t)H * W, tri, F, out);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_raster_interpolate_backward(const float* attr, int64_t attr_batch, int64_t V, int C, const float* rast, int64_t B, int H, int W,
                                              const int32_t* tri, int64_t F, const float* grad_out, const int32_t* order, const int32_t* seg,
                                              const int32_t* vptr, const int32_t* corner_order, float* grad_attr, float* grad_rast, void* ws,
                                              size_t ws_bytes, int device, void* stream) {
    int rc = rs_check(B, V, F, H, W, "ls_raster_interpolate_backward");
    if (rc) return rc;
    LS_REQUIRE(C >= 1 && (attr_batch == 1 || attr_batch == B), LS_E_INVALID, "ls_raster_interpolate_backward: C %d, attribute batch %lld of %lld",
               C, (long long)attr_batch, (long long)B);
    const RsWs L = rs_carve(ws, B, F, H, W, C);
    LS_REQUIRE(rast && grad_out && (attr || V == 0) && (tri || F == 0), LS_E_INVALID, "ls_raster_interpolate_backward: null argument");
    LS_REQUIRE(!grad_attr || (order && seg && vptr && ws && (corner_order || F == 0)), LS_E_INVALID,
               "ls_raster_interpolate_backward: grad_attr needs the pixel order, the corner ranking and a workspace");
    LS_REQUIRE(!grad_attr || ws_bytes >= L.total, LS_E_WORKSPACE, "ls_raster_interpolate_backward: workspace too small (%zu < %zu bytes)", ws_bytes,
               L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    hipStream_t st = (hipStream_t)stream;
    if (grad_rast)
        hipLaunchKernelGGL(k_rs_interp_grad_rast, dim3(div_up(B * H * W, 256)), dim3(256), 0, st, attr, (int)attr_batch, V, C, rast, (int)B,
                           (int64_t)H * W, tri, F, grad_out, grad_rast);
    if (grad_attr)
        rs_interp_grad_attr(inst(B, V, F), rast, attr_batch, C, grad_out, order, seg, vptr, corner_order, grad_attr, L.rows, st);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_raster_adjacency_workspace_bytes(int64_t F, size_t* bytes) {
    LS_REQUIRE(bytes && F >= 0 && 3 * F < ((int64_t)1 << 31) - 1, LS_E_INVALID, "ls_raster_adjacency_workspace_bytes: bad argument");
    *bytes = rs_adjacency_bytes(F);
    return LS_OK;
}

extern "C" int ls_raster_adjacency(const int32_t* tri, int64_t F, int32_t* adj, void* ws, size_t ws_bytes, int device, void* stream) {
    size_t need = 0;
    int rc = ls_raster_adjacency_workspace_bytes(F, &need);
    if (rc) return rc;
    LS_REQUIRE(adj && ws && (tri || F == 0), LS_E_INVALID, "ls_raster_adjacency: null argument");
    LS_REQUIRE(ws_bytes >= need, LS_E_WORKSPACE, "ls_raster_adjacency: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    if (F == 0) return LS_OK;
    return rs_adjacency<KeyEdge, 2>(KeyEdge{tri}, 3 * F, 4, adj, ws, device, stream);
}

extern "C" int ls_raster_antialias(const float* color, int C, const float* rast, const float* pos, int64_t B, int64_t V, int H, int W,
                                   const int32_t* tri, int64_t F, const int32_t* adj, float* out, int device, void* stream) {
    const bool ok = C >= 1 && color && rast && out && (pos || V == 0) && ((tri && adj) || F == 0);
    return rs_antialias(inst(B, V, F), "ls_raster_antialias", ok, color, C, rast, pos, tri, adj, H, W, out, device, stream);
}

extern "C" int ls_raster_antialias_backward(const float* color, int C, const float* rast, const float* pos, int64_t B, int64_t V, int H, int W,
                                            const int32_t* tri, int64_t F, const int32_t* adj, const float* grad_out, float boost,
                                            const int32_t* order, const int32_t* seg, const int32_t* vptr, const int32_t* corner_order,
                                            float* grad_color, float* grad_pos, void* ws, size_t ws_bytes, int device, void* stream) {
    const bool ok = C >= 1 && color && rast && grad_out && (pos || V == 0) && ((tri && adj) || F == 0);
    return rs_antialias_backward(inst(B, V, F), "ls_raster_antialias_backward", ok, color, C, rast, pos, tri, adj, H, W, grad_out, boost, order, seg,
                                 vptr, corner_order, grad_color, grad_pos, ws, ws_bytes, device, stream);
}

// ---- range mode ---------------------------------------------------------------------------------------------------------------------------
extern "C" int ls_range_workspace_bytes(int64_t B, int64_t N, int H, int W, int C, size_t* bytes) {
    int rc = rg_check(B, N, 0, 0, H, W, "ls_range_workspace_bytes");
    if (rc) return rc;
    LS_REQUIRE(bytes && C >= 0, LS_E_INVALID, "ls_range_workspace_bytes: bad argument");
    *bytes = rs_carve_keys(nullptr, B * H * W, N, C).total;
    return LS_OK;
}

extern "C" int ls_range_forward(const float* pos, int64_t V, const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N, int H,
                                int W, float* rast, void* ws, size_t ws_bytes, int device, void* stream) {
    return rs_forward<false>(range(ranges, B, N, V, F), "ls_range_forward", rast && ws && ranges && ((pos && tri) || N == 0), pos, tri, H, W,
                             nullptr, rast, ws, ws_bytes, device, stream);
}

extern "C" int ls_range_pixel_order(const float* rast, const int32_t* ranges, int64_t B, int64_t N, int64_t F, int H, int W, int32_t* order,
                                    int32_t* seg, void* ws, size_t ws_bytes, int device, void* stream) {
    return rs_pixel_order(range(ranges, B, N, 0, F), "ls_range_pixel_order", rast && ranges && order && seg && ws, rast, H, W, order, seg, ws,
                          ws_bytes, device, stream);
}

extern "C" int ls_range_backward(const float* pos, int64_t V, const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N, int H,
                                 int W, const float* grad_rast, const int32_t* order, const int32_t* seg, const int32_t* vptr,
                                 const int32_t* corner_order, float* grad_pos, void* ws, size_t ws_bytes, int device, void* stream) {
    const bool ok = grad_rast && ranges && order && seg && vptr && grad_pos && ws && (pos || V == 0) && ((tri && corner_order) || F == 0);
    return rs_backward(range(ranges, B, N, V, F), "ls_range_backward", ok, pos, tri, H, W, grad_rast, order, seg, vptr, corner_order, grad_pos, ws,
                       ws_bytes, device, stream);
}

extern "C" int ls_range_interpolate_backward(const float* rast, const int32_t* ranges, int64_t B, int64_t N, int H, int W, int64_t V, int C,
                                             const float* grad_out, const int32_t* order, const int32_t* seg, const int32_t* vptr,
                                             const int32_t* corner_order, float* grad_attr, void* ws, size_t ws_bytes, int device, void* stream) {
    int rc = rg_check(B, N, V, 0, H, W, "ls_range_interpolate_backward");
    if (rc) return rc;
    LS_REQUIRE(C >= 1, LS_E_INVALID, "ls_range_interpolate_backward: C %d", C);
    const RsWs L = rs_carve_keys(ws, B * H * W, N, C);
    LS_REQUIRE(rast && ranges && grad_out && order && seg && vptr && grad_attr && ws && (corner_order || N == 0), LS_E_INVALID,
               "ls_range_interpolate_backward: null argument");
    LS_REQUIRE(ws_bytes >= L.total, LS_E_WORKSPACE, "ls_range_interpolate_backward: workspace too small (%zu < %zu bytes)", ws_bytes, L.total);
    DeviceGuard g(device);
    LS_HIP(g.err);
    rs_interp_grad_attr(range(ranges, B, N, V, 0), rast, 1, C, grad_out, order, seg, vptr, corner_order, grad_attr, L.rows, (hipStream_t)stream);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

extern "C" int ls_range_adjacency_workspace_bytes(int64_t N, size_t* bytes) {
    LS_REQUIRE(bytes && N >= 0 && 3 * N < ((int64_t)1 << 31) - 1, LS_E_INVALID, "ls_range_adjacency_workspace_bytes: bad argument");
    *bytes = rs_adjacency_bytes(N);
    return LS_OK;
}

extern "C" int ls_range_adjacency(const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N, int32_t* adj, void* ws,
                                  size_t ws_bytes, int device, void* stream) {
    size_t need = 0;
    int rc = ls_range_adjacency_workspace_bytes(N, &need);
    if (rc) return rc;
    LS_REQUIRE(B >= 1 && F >= 0 && adj && ws && ranges && (tri || N == 0), LS_E_INVALID, "ls_range_adjacency: bad argument");
    LS_REQUIRE(ws_bytes >= need, LS_E_WORKSPACE, "ls_range_adjacency: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    if (N == 0) return LS_OK;
    return rs_adjacency<KeyItemEdge, 3>(KeyItemEdge{tri, MapRange{ranges, (int)B}}, 3 * N, radix_passes(B - 1), adj, ws, device, stream);
}

extern "C" int ls_range_antialias(const float* color, int C, const float* rast, const float* pos, int64_t V, const int32_t* tri, int64_t F,
                                  const int32_t* ranges, int64_t B, int64_t N, int H, int W, const int32_t* adj, float* out, int device,
                                  void* stream) {
    const bool ok = C >= 1 && color && rast && out && ranges && ((pos && tri && adj) || N == 0);
    return rs_antialias(range(ranges, B, N, V, F), "ls_range_antialias", ok, color, C, rast, pos, tri, adj, H, W, out, device, stream);
}

extern "C" int ls_range_antialias_backward(const float* color, int C, const float* rast, const float* pos, int64_t V, const int32_t* tri, int64_t F,
                                           const int32_t* ranges, int64_t B, int64_t N, int H, int W, const int32_t* adj, const float* grad_out,
                                           float boost, const int32_t* order, const int32_t* seg, const int32_t* vptr,
                                           const int32_t* corner_order, float* grad_color, float* grad_pos, void* ws, size_t ws_bytes, int device,
                                           void* stream) {
    const bool ok = C >= 1 && color && rast && grad_out && ranges && ((pos && tri && adj) || N == 0);
    return rs_antialias_backward(range(ranges, B, N, V, F), "ls_range_antialias_backward", ok, color, C, rast, pos, tri, adj, H, W, grad_out, boost,
                                 order, seg, vptr, corner_order, grad_color, grad_pos, ws, ws_bytes, device, stream);
}

// ---- depth peeling: the layer behind prev_rast, both modes (the workspaces are ls_raster_workspace_bytes / ls_range_workspace_bytes) --------
extern "C" int ls_peel_forward(const float* pos, int64_t B, int64_t V, const int32_t* tri, int64_t F, int H, int W, const float* prev_rast,
                               float* rast, void* ws, size_t ws_bytes, int device, void* stream) {
    const bool ok = prev_rast && rast && ws && (pos || V == 0) && (tri || F == 0);
    return rs_forward<true>(inst(B, V, F), "ls_peel_forward", ok, pos, tri, H, W, prev_rast, rast, ws, ws_bytes, device, stream);
}

extern "C" int ls_peel_range_forward(const float* pos, int64_t V, const int32_t* tri, int64_t F, const int32_t* ranges, int64_t B, int64_t N,
                                     int H, int W, const float* prev_rast, float* rast, void* ws, size_t ws_bytes, int device, void* stream) {
    const bool ok = prev_rast && rast && ws && ranges && ((pos && tri) || N == 0);
    return rs_forward<true>(range(ranges, B, N, V, F), "ls_peel_range_forward", ok, pos, tri, H, W, prev_rast, rast, ws, ws_bytes, device, stream);
}
