"""
The inputs of tests/test_distance_grad_scale_gpu.py: the gradient of largesteps.distance to the mesh vertices (csrc/distance.hip: weights,
keys, the group-by of groupby.h over the sort of radix.h, the face rows of seg_sum, the vertex gather) at the sizes where that chain
changes its path. Plain seeded numpy, no device: tests/test_distance_grad_cases_cpu.py checks here that every case meets the conditions it
was built for.

Sort workgroups. The n points are sorted in workgroups of rs_chunk(n) points: 1024 up to n = 2 * 2^20, 2048 up to 4 * 2^20, 4096 beyond.
The histogram, its scan and the scatter have one table of 256 counters per workgroup in the caller's workspace.

Byte passes. The keys lie in [0, T] (T faces; T itself means "no face"), sorted by the fewest bytes that hold T: passes = the smallest p in
1 .. 4 with T < 256^p. An odd number of passes leaves the order in the caller's buffer; an even number leaves it in the scratch's second
buffer, from where it is copied before that buffer is reused for the sorted keys. One, two and three passes all occur below, each over
more than one sort workgroup.

Face rows. One thread per face in workgroups of 256 = four waves of 64 faces; a face with more than 64 points is summed by its whole wave,
the waves' long faces one after the other.

Two kinds of case. A *walked* case holds a mesh and query points; I and C come from the device's own query. A *fabricated* case chooses I
freely: C is an fp64 point of face I (random barycentric coordinates), P is C plus an offset, rounded to fp32, and g is uniform in
[-1, 2]. The kernels take I and C as given, so the statement on the same (P, I, C, g) is the exact reference. An I outside [0, T) gets a
C inside the mesh's box.
"""
import numpy as np

from largesteps import synthetic

F32 = np.float32


def rs_chunk(n):
    """points per sort workgroup (the module docstring)"""
    return 4096 if n > 4 << 20 else 2048 if n > 2 << 20 else 1024


def sort_workgroups(n):
    return -(-n // rs_chunk(n))


def radix_passes(T):
    """the smallest p in 1 .. 4 with T < 256^p (the module docstring)"""
    return next((p for p in (1, 2, 3) if T < 256 ** p), 4)


def _seed(name):
    return sum(map(ord, name))


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------------
_meshes = {}


def sphere(freq):
    """icosphere(freq), radially perturbed by 5 %: (v fp32, f int64)"""
    if freq not in _meshes:
        v, f = synthetic.icosphere(freq)
        _meshes[freq] = (synthetic.perturb(v, radial=0.05, seed=2).astype(F32), np.asarray(f, dtype=np.int64))
    return _meshes[freq]


HUB_FACES = 1200
HUB_VERTEX = 700
HUB_LONG = {5: 65, 600: 130, 1199: 200}          # fan face -> points; every other face i gets 1 + i % 4


def fan():
    """a closed cone of HUB_FACES faces around one vertex: the hub is vertex HUB_VERTEX and a corner of every face, at corner
    position i % 3 of face i; the rim vertices (two faces each) take the other ids in order"""
    R = HUB_FACES
    w = 2.0 * np.pi * np.arange(R) / R
    rim = np.stack([np.cos(w), np.sin(w), 0.1 * np.sin(5.0 * w)], -1)
    ids = np.arange(R + 1)
    ids = ids[ids != HUB_VERTEX]
    v = np.zeros((R + 1, 3))
    v[ids], v[HUB_VERTEX] = rim, (0.0, 0.0, 0.6)
    i = np.arange(R)
    f = np.stack([np.full(R, HUB_VERTEX), ids[i], ids[(i + 1) % R]], -1)
    f = np.stack([np.roll(row, k % 3) for k, row in enumerate(f)])
    return v.astype(F32), f.astype(np.int64)


# ---- the per-face counts of `thresholds` ---------------------------------------------------------------------------------------------------------
# icosphere(6): T = 720 faces = workgroups of 256, 256 and 208 faces; the last wave holds faces 704 .. 719, 16 lanes.
THRESHOLD_FREQ = 6
THRESHOLD_LONG = {
    0: 65,                              # lane 0 of the first wave
    63: 129,                            # lane 63 of the first wave
    100: 66, 101: 700, 102: 128,        # three in a row inside the second wave (lanes 36 .. 38)
    127: 65,                            # lane 63 of the second wave
    128: 4097,                          # lane 0 of the third wave: 65 turns of the lane chains, the last with one item
    300: 127,                           # alone in its wave, in the second workgroup
    710: 129,                           # in the final 16-lane wave
    719: 65,                            # face T - 1
}
THRESHOLD_SHORT = {1: 64, 2: 63, 62: 64, 64: 0, 99: 64, 103: 64, 104: 63, 129: 64, 301: 0, 709: 64, 711: 63, 718: 64}
THRESHOLD_COUNTS = (0, 1, 63, 64, 65, 66, 127, 128, 129, 700, 4097)


THRESHOLD_BARE = 3


def threshold_counts():
    """points per face (720,): the long and short faces above; every other face f is empty when f % 5 == 0 and has one point otherwise,
    so empty and short faces sit between the long ones; and every face around the first THRESHOLD_BARE vertices that touch none of
    the faces above is empty, so those vertices receive nothing"""
    f = sphere(THRESHOLD_FREQ)[1]
    m = np.where(np.arange(f.shape[0]) % 5 == 0, 0, 1)
    placed = {**THRESHOLD_LONG, **THRESHOLD_SHORT}
    for a, c in placed.items():
        m[a] = c
    bare = 0
    for u in range(int(f.max()) + 1):
        around = np.nonzero((f == u).any(1))[0]
        if bare < THRESHOLD_BARE and not set(around.tolist()) & set(placed):
            m[around], bare = 0, bare + 1
    return m


# ---- fabrication ----------------------------------------------------------------------------------------------------------------------------
def scattered(counts, rng):
    """I with counts[f] points on face f, in shuffled order: the points of a face are spread through the array"""
    return rng.permutation(np.repeat(np.arange(len(counts)), counts))


def fabricate(v, f, I, rng):
    """(P (n, 3) fp32, C (n, 3) fp64, g (n,) fp64) for the face ids I (the module docstring)"""
    n, T = len(I), f.shape[0]
    v64 = v.astype(np.float64)
    lo, hi = v64.min(0), v64.max(0)
    ok = (I >= 0) & (I < T)
    b = rng.dirichlet(np.ones(3), n)
    corners = v64[f[np.where(ok, I, 0)]]                                   # (n, 3 corners, 3)
    C = np.where(ok[:, None], (b[:, :, None] * corners).sum(1), rng.uniform(lo, hi, (n, 3)))
    P = (C + rng.normal(scale=0.05 * float(np.linalg.norm(hi - lo)), size=(n, 3))).astype(F32)
    return P, C, rng.uniform(-1.0, 2.0, n)


def out_of_range_ids(T):
    """the four ids outside [0, T) that `out_of_range` plants in turn"""
    return np.array([-1, T, T + 1, 2 ** 40], dtype=np.int64)


FABRICATED = ("one_pass_many_blocks", "thresholds", "hub", "out_of_range", "chunk_1024_last", "chunk_2048_first", "chunk_4096_first")
CHUNK_N = {"chunk_1024_last": 2 << 20, "chunk_2048_first": (2 << 20) + 1, "chunk_4096_first": (4 << 20) + 1}
SMALL_FABRICATED = tuple(c for c in FABRICATED if c not in CHUNK_N)


def fabricated_mesh(name):
    if name == "one_pass_many_blocks":
        return sphere(3)
    if name in ("thresholds", "out_of_range"):
        return sphere(THRESHOLD_FREQ)
    if name == "hub":
        return fan()
    return sphere(58)


def fabricated_ids(name):
    """the face ids I (n,) int64 of a fabricated case"""
    rng = np.random.default_rng(_seed(name))
    T = fabricated_mesh(name)[1].shape[0]
    if name == "one_pass_many_blocks":
        return rng.integers(0, T, 5000)
    if name == "thresholds":
        return scattered(threshold_counts(), rng)
    if name == "hub":
        m = 1 + np.arange(T) % 4
        for f, c in HUB_LONG.items():
            m[f] = c
        return scattered(m, rng)
    if name == "out_of_range":
        I = fabricated_ids("thresholds").copy()
        at = rng.choice(len(I), len(I) // 100, replace=False)
        I[at] = out_of_range_ids(T)[np.arange(len(at)) % 4]
        return I
    return rng.integers(0, T, CHUNK_N[name])


def fabricated(name):
    """(v, f, P, I, C, g) of a fabricated case. `out_of_range` is `thresholds` with one point in a hundred sent outside [0, T): the
    same P, C and g, so removing those points gives a sub-sequence of the `thresholds` case"""
    v, f = fabricated_mesh(name)
    I = fabricated_ids(name)
    src = "thresholds" if name == "out_of_range" else name
    P, C, g = fabricate(v, f, fabricated_ids(src), np.random.default_rng(_seed(src) + 1))
    return v, f, P, I, C, g


def walked_three_pass():
    """(v, f, p): the perturbed icosphere(58) (67 280 faces: three byte passes), queried with the vertices of a differently perturbed copy
    and the probes of tests/test_distance_gpu.py (points on vertices and edges, near, far and very far): 34 sort workgroups"""
    from test_distance_gpu import probes
    v, f = sphere(58)
    base = synthetic.icosphere(58)[0]
    other = synthetic.perturb(base, radial=0.03, seed=11).astype(F32)
    return v, f, np.concatenate([other, probes(v, f, 64, seed=58)])
