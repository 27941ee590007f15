"""
The meshes of tests/test_normals_scale_gpu.py and what they cross in csrc/normals.hip. Shared with tests/golden/make_golden_normals.py
(--scale: the reference's own fp32 error on these meshes, measured once on the CPU), which is why it is not inside the test file.

The constants that set the thresholds are READ from the sources the library is compiled from (csrc/common.h, csrc/meshface.h,
csrc/normals.hip), not restated: SIZES below holds the counts the issue's meshes must give with them, and
tests/test_normals.py::test_scale_meshes_cross_the_compiled_thresholds (CPU) and every Case of the GPU test assert them -- a change of
PF, FIN, FIN_U, BLOCK or MESH_MAXG fails those tests instead of silently un-testing the second slot / second trip / second pass.
"""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "large-steps-pytorch_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def compiled_int(name, const):
    """the value of `constexpr int ... CONST = <integer literal>` in csrc/<name>; exactly one definition, or an error"""
    found = re.findall(r"constexpr\s+int\b[^;]*?\b%s\s*=\s*(\d+)\s*[,;]" % const, source(name))
    if len(found) != 1:
        raise AssertionError(f"{name}: expected one `constexpr int {const} = <literal>`, found {len(found)}")
    return int(found[0])


BLOCK = compiled_int("common.h", "BLOCK")
MESH_MAXG = compiled_int("meshface.h", "MESH_MAXG")  # the grid cap of the looping reductions (k_edge_norm_partials, k_vertex_normals_bwd1)
PF = compiled_int("normals.hip", "PF")               # faces per thread of the pair's reducing passes -> one partial per PF * BLOCK faces
FIN = compiled_int("normals.hip", "FIN")             # k_finish3's threads ...
FIN_U = compiled_int("normals.hip", "FIN_U")         # ... and partials per thread per trip of its loop
PAIR_FACES = PF * BLOCK        # faces per partial of the pair path
GENERAL_SWEEP = MESH_MAXG * BLOCK     # faces one sweep of the general path's grid covers
# how the sources use them: the statements the formulas of this file (pair_G, tail_start, GENERAL_SWEEP) stand for
USES = {"normals.hip": ["const int G = (int)div_up(F, (int64_t)PF * BLOCK)",                     # pair_G
                        "for (int g0 = threadIdx.x; g0 < G; g0 += FIN * FIN_U)",                # a trip of k_finish3 takes FIN * FIN_U
                        "const int g = g0 + u * FIN;",                                          # ... slot u of a thread is FIN further
                        "f0 = blk * (PF * BLOCK) + threadIdx.x",                                # partial blk = faces [blk, blk + 1) * PF * BLOCK
                        "part[(size_t)i * P + blk] = acc[i]", "part[(size_t)i * P + blk] = gN[i]",
                        "f += (int64_t)gridDim.x * BLOCK"],                                     # the general path's sweep
        "meshface.h": ["std::min<int64_t>(MESH_MAXG, std::max<int64_t>(1, div_up(F, BLOCK)))"]}

# the sizes at which the END-TO-END part (numpy fp64 backward: 1 s and 3 s) runs; its measured tolerances are keyed by these
END_TO_END = (364, 726)

# n -> (F, V, pair G): plane(n) has 2 (n - 1)^2 faces
SIZES = {364: (263538, 132496, 258), 726: (1051250, 527076, 1027), 1450: (4199202, 2102500, 4101)}


def pair_G(F):
    return -(-F // PAIR_FACES)


def jittered_plane(n, seed=5):
    """synthetic.plane(n) with every vertex moved by a seeded uniform jitter of +-0.2 cell in x and y and +-0.1 cell in z (cell =
    1 / (n - 1)): without it every face is congruent and the corner terms are the same everywhere. fp32 verts, int64 faces."""
    from largesteps import synthetic
    v, f = synthetic.plane(n)
    cell = 1.0 / (n - 1)
    d = np.random.default_rng(seed + n).uniform(-1.0, 1.0, size=v.shape) * (np.array([0.2, 0.2, 0.1]) * cell)
    return (v.astype(np.float64) + d).astype(np.float32), f


def tail_start(n):
    """first face whose pair partial k_finish3 reads past its first slot (G <= FIN_U * FIN) or past its first trip; None where neither"""
    G = pair_G(SIZES[n][0])
    if G > FIN * FIN_U:
        return FIN * FIN_U * PAIR_FACES
    return FIN * PAIR_FACES if G > FIN else None


def tail_vertices(n, f):
    """the vertices of the faces from tail_start(n) on (none where there is no tail)"""
    t = tail_start(n)
    return np.unique(f[t:]) if t is not None else np.zeros(0, dtype=np.int64)


def tail_weights(n, V, f, seed=7):
    """g_out (V, 3) fp32: seeded normal values, times 1000 on the vertices of the faces from tail_start(n) on -- the tail of the
    reduction then carries the sum (the device of test_adam_uniform_finds_the_largest_gradient_wherever_it_sits)"""
    w = np.random.default_rng(seed + n).standard_normal((V, 3)).astype(np.float32)
    w[tail_vertices(n, f)] *= 1000.0
    return w


def tail_raw(n, V, seed=9):
    """raw (V, 3) fp32 for the same entry point, where it is an input like g_out: seeded vectors of the size the forward gives on these
    meshes (six corners of angle ~ pi / 2 around +z), built directly -- the fp64 forward of 4.2M faces would cost the test 3 s"""
    return (np.random.default_rng(seed + n).normal(size=(V, 3)) * 0.5 + np.array([0.0, 0.0, 9.4])).astype(np.float32)


def plain_weights(n, V):
    """the output gradient of the end-to-end cases (and of the reference's run in tests/golden/make_golden_normals.py --scale)"""
    return np.random.default_rng(n).standard_normal((V, 3)).astype(np.float32)
