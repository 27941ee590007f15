"""
The inputs of tests/test_texture_scale_gpu.py and tests/test_mip_scale_gpu.py: textures past one workgroup of texels and past two byte
passes of the pixel sort, and clusters of pixels at the lengths where groupby.h's seg_sum changes from one thread to a whole wave.
Plain seeded numpy, no device: tests/test_texture_cpu.py and tests/test_mip_cpu.py check here that every case meets the conditions it
was built for.

Byte passes. The pixel order sorts keys in [0, nk], nk = Bt (Ht + 1) (Wt + 1) for a plain texture and the sum of that over the levels for
a pyramid, by the fewest bytes that hold nk: passes = the smallest p in 1 .. 4 with nk < 256^p. An odd number of passes leaves the
order in the caller's buffer, an even number in the scratch's second buffer, which is copied and then reused for the sorted keys.

Workgroups. The texture gradient runs one thread per texel (of every level, level after level, for a pyramid) in workgroups of 256 =
four waves of 64 texels in row-major order; a texel with more than 64 items in all is summed by its whole wave.
"""
import numpy as np

import mip_statement as ms

FILTERS = ("nearest", "linear")
BOUNDARIES = ("wrap", "clamp", "zero")
ALL_MODES = tuple((f, b) for f in FILTERS for b in BOUNDARIES)
MIP_COMBOS = tuple((m, b) for m in ms.MODES for b in BOUNDARIES)


def radix_passes(nk):
    """the smallest p in 1 .. 4 with nk < 256^p (the module docstring)"""
    return next((p for p in (1, 2, 3) if nk < 256 ** p), 4)


def texture_keys(tex_shape):
    Bt, Ht, Wt, _ = tex_shape
    return Bt * (Ht + 1) * (Wt + 1)


def mip_keys(tex_shape, Lmax):
    Bt, Ht, Wt, _ = tex_shape
    return Bt * sum((max(Ht >> l, 1) + 1) * (max(Wt >> l, 1) + 1) for l in range(Lmax + 1))


def _seed(name):
    return sum(map(ord, name))


def scaled_da(rng, shape, Ht, Wt, lo, hi):
    """uv_da whose lod (without bias) is uniform in [lo, hi): a random direction scaled to the wanted footprint"""
    d = rng.standard_normal(shape + (4,))
    want = rng.uniform(lo, hi, shape)
    m = ms.footprint(d, Ht, Wt)[0]
    return (d * np.sqrt(4.0 ** want / m)[..., None]).astype(np.float32)


# ---- clusters at the lengths around seg_sum's threshold ----------------------------------------------------------------------------------
# (pixels, i0, j0): `pixels` pixels strictly inside the cell whose base tap is texel (i0, j0): in linear mode each of the texels (i0, j0),
# (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1) gains that many items from ONE base position. Cells are at least two texels apart and away
# from the border, so no other cluster and no boundary rule adds to these texels -- but for the two PAIRS of side-by-side cells, whose
# shared texels (i0 + 1, j0) and (i0 + 1, j0 + 1) collect 40 + 25 = 65 and 40 + 24 = 64 items from two base positions.
THRESHOLD_SHAPE = (1, 24, 40, 3)            # 960 texels: three workgroups and 192 texels
THRESHOLD_CLUSTERS = (
    (64, 2, 0), (65, 6, 0), (129, 10, 0), (1, 14, 0),       # rows 0 and 1 up to column 23: texels 0 .. 63, the first wave
    (63, 4, 4), (66, 10, 4), (127, 20, 4), (128, 30, 4),
    (700, 5, 9),
    (40, 20, 10), (25, 21, 10),                             # shared texels (21, 10), (21, 11): 65 items
    (40, 30, 14), (24, 31, 14),                             # shared texels (31, 14), (31, 15): 64 items
    (65, 20, 21),                                           # texels 860, 861, 900, 901 of the last workgroup (768 .. 959)
)
MIP_THRESHOLD_SHAPE = (1, 16, 32, 3)        # level 0: 512 texels = two workgroups; levels 1 .. 5 (171 texels) are the third
MIP_THRESHOLD_CLUSTERS = (
    (128, 2, 0), (129, 6, 0), (700, 10, 0), (1, 14, 0), (64, 18, 0), (65, 22, 0),       # rows 0 and 1: the first wave
    (63, 2, 4), (66, 8, 4), (127, 14, 4),
    (40, 20, 4), (25, 21, 4),
    (40, 26, 8), (24, 27, 8),
    (130, 20, 12),
)
# Half of every cluster (the larger half of an odd one) reads level 0 alone, the other half levels 1 and 2 (level 2 alone in
# linear-mipmap-nearest). The biases are 0.0 and 1.5 moved by 2^-10, the smallest step that keeps the flag rule of tests/mip_statement.py
# quiet: lod = 0.0 exactly is "within 64 U of an integer" in linear mode and lod + 1/2 = 2.0 exactly in nearest mode, which would flag
# half the pixels of the case. -2^-10 clamps to lod 0: the very lookup of bias 0.0. Because that half is clamped its bias gradient is
# identically zero: this case has no bias gradient at l0 = 0 with f > 0 (the cases with uv_da, whose lod is spread over every level, do).
MIP_THRESHOLD_BIAS = (np.float32(-2.0 ** -10), np.float32(1.5 + 2.0 ** -10))


def _cluster_pixels(rng, clusters, Ht, Wt, linear):
    """(uv (P, 2) fp32, cluster id (P), rank within the cluster (P)) in a shuffled pixel order: the sort has work to do. Linear: a random
    offset in [0.1, 0.9) of the cell; nearest: the centre of texel (i0, j0)"""
    uv, cid, rank = [], [], []
    for k, (m, i0, j0) in enumerate(clusters):
        ox, oy = (rng.uniform(0.1, 0.9, m), rng.uniform(0.1, 0.9, m)) if linear else (np.zeros(m), np.zeros(m))
        uv.append(np.stack([(i0 + ox + 0.5) / Wt, (j0 + oy + 0.5) / Ht], -1))
        cid.append(np.full(m, k))
        rank.append(np.arange(m))
    uv, cid, rank = np.concatenate(uv), np.concatenate(cid), np.concatenate(rank)
    p = rng.permutation(len(uv))
    return uv[p].astype(np.float32), cid[p], rank[p]


def _as_image(a):
    """(P, ...) -> (1, H, W, ...) with H W = P, H the largest divisor up to sqrt(P)"""
    P = a.shape[0]
    H = max(h for h in range(1, int(P ** 0.5) + 1) if P % h == 0)
    return a.reshape((1, H, P // H) + a.shape[1:])


def threshold_counts(clusters, Ht, Wt):
    """the items per texel (Ht, Wt) the clusters give in linear mode, counted from the layout alone"""
    n = np.zeros((Ht, Wt), np.int64)
    for m, i0, j0 in clusters:
        n[j0:j0 + 2, i0:i0 + 2] += m
    return n


# ---- plain texture ----------------------------------------------------------------------------------------------------------------------------
# name -> (tex shape, uv shape, modes)
TEXTURE_CASES = {
    "wide_300x5_c3": ((1, 5, 300, 3), (2, 48, 48), ALL_MODES),                  # Wt + 1 = 301 > 255; 1500 texels = 5 workgroups + 220
    "three_pass_255x257_c3": ((1, 255, 257, 3), (2, 64, 64), ALL_MODES),        # 256 x 258 = 66 048 keys
    "three_pass_own_b4_128x128_c4": ((4, 128, 128, 4), (4, 40, 40), ALL_MODES),  # 4 x 129^2 = 66 564 keys, float4 rows
    "four_pass_4096_c1": ((1, 4096, 4096, 1), (1, 64, 64), (("linear", "wrap"), ("linear", "clamp"))),      # 4097^2 > 2^24
    "threshold": (THRESHOLD_SHAPE, (1, 29, 53), ALL_MODES),
    "c32": ((1, 6, 10, 32), (2, 8, 8), ALL_MODES),                              # TX_MAX_C: eight channel groups
    "c5": ((2, 4, 6, 5), (2, 8, 8), ALL_MODES),                                 # 4 + 1 channels
}


def texture_case(name, filt="linear"):
    """(tex, uv, g) fp32 arrays. Only `threshold` depends on the filter: its pixels sit inside cells (linear) or on texel centres (nearest)"""
    tex_shape, uv_shape, _ = TEXTURE_CASES[name]
    rng = np.random.default_rng(_seed(name))
    tex = rng.standard_normal(tex_shape, dtype=np.float32)
    if name == "threshold":
        uv = _as_image(_cluster_pixels(rng, THRESHOLD_CLUSTERS, tex_shape[1], tex_shape[2], filt != "nearest")[0])
        assert uv.shape[:3] == uv_shape
    else:
        uv = rng.uniform(-1.5, 2.5, uv_shape + (2,)).astype(np.float32)
    g = rng.standard_normal(uv.shape[:3] + (tex_shape[3],), dtype=np.float32)
    return tex, uv, g


# ---- mipmapped ----------------------------------------------------------------------------------------------------------------------------------
# name -> (tex shape, uv shape, max_mip_level)
MIP_CASES = {
    "levels_straddle_40x72_c3_max3": ((1, 40, 72, 3), (2, 40, 40), 3),          # level offsets 2880, 3600, 3780, 3825 texels
    "deep_64x512_c3": ((1, 64, 512, 3), (2, 32, 32), None),                     # Lmax 9, levels 6 .. 9 one texel high
    "deep_512x2_c2": ((1, 512, 2, 2), (2, 32, 32), None),                       # Lmax 9, levels 1 .. 9 one texel wide
    "three_pass_256x256_c4": ((1, 256, 256, 4), (2, 96, 96), None),             # level 0 alone: 257^2 = 66 049 keys
    "three_pass_own_b2_128x256_c1": ((2, 128, 256, 1), (2, 48, 48), None),      # level 0: 2 x 129 x 257 = 66 306 keys
    "mip_threshold": (MIP_THRESHOLD_SHAPE, (1, 18, 89), None),
}


def mip_case(name):
    """(tex, uv, uv_da or None, bias, max_mip_level, g) fp32 arrays; lod is spread over [-1, Lmax + 1], so both clamps are hit"""
    tex_shape, uv_shape, max_level = MIP_CASES[name]
    rng = np.random.default_rng(_seed(name))
    Bt, Ht, Wt, C = tex_shape
    tex = rng.standard_normal(tex_shape, dtype=np.float32)
    if name == "mip_threshold":
        uv, _, rank = _cluster_pixels(rng, MIP_THRESHOLD_CLUSTERS, Ht, Wt, True)
        uv, da = _as_image(uv), None
        bias = _as_image(np.where(rank % 2 == 0, MIP_THRESHOLD_BIAS[0], MIP_THRESHOLD_BIAS[1]).astype(np.float32))
        assert uv.shape[:3] == uv_shape
    else:
        Lmax = ms.last_level(Ht, Wt, max_level)
        uv = rng.uniform(-1.5, 2.5, uv_shape + (2,)).astype(np.float32)
        da = scaled_da(rng, uv_shape, Ht, Wt, -0.8, Lmax + 0.8)
        bias = rng.uniform(-0.2, 0.2, uv_shape).astype(np.float32)
    g = rng.standard_normal(uv_shape + (C,), dtype=np.float32)
    return tex, uv, da, bias, max_level, g
