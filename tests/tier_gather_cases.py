"""
Cases of tests/test_tier_gather_gpu.py (TEST helper; also run by tools/record_tier_gather_bits.py, which writes the record the test
compares against): the smallest meshes on which every gather of the tier kernels (csrc/nd_tier.h) runs.

    plane     synthetic.plane(250), 62 500 vertices, uniform Laplacian lambda = 19: a tree of 6 levels at arity 4 (1024 leaves, 256 tier
              workgroups), of 5 levels at arity 8 (4096 leaves, 512 tier workgroups). Arity 4 runs the in-register pull lists (pull_request / pull_sum) in its 4-, 8- and 16-wave
              shape, arity 8 runs pull_compact for every row.
    rough     synthetic.icosphere(40) with 30 % radial noise, 16 002 vertices: the smallest closed sphere of the family (searched over the
              frequencies 20 .. 163 at 5, 15 and 30 % noise with the host planner) that has a leaf with MORE THAN 64 boundary rows
              (71; tests assert it) and rows with more than TIER_SPE = 4 sparse entries in both sweeps. tests/irregular_meshes.py has
              no closed mesh, and at the benchmark's 5 % noise no sphere below 270k vertices has such a leaf.

Every solver is built with leaf_size = 64 and ordering = 'longest-axis' given explicitly: the plan, and with it every bit of x, is then a
function of the mesh alone and not of what the process solved before.
"""
import hashlib

import numpy as np

from largesteps import synthetic

LAMBDA = 19.0
KS = (1, 2, 3, 4)
# (mesh, arity, tier_waves)
SHAPES = [("plane", 4, 4), ("plane", 4, 8), ("plane", 4, 16), ("plane", 8, 4), ("plane", 8, 8), ("rough", 4, 4), ("rough", 4, 16)]
GOLDEN = "tier_gather_bits.npz"


def mesh(name):
    if name == "plane":
        return synthetic.plane(250)
    v, f = synthetic.icosphere(40)
    return synthetic.perturb(v, radial=0.3, tangential=0.25, edge=1.2 / 40, seed=0), f


def pattern(f, V):
    """(rowptr, col) of the system matrix' pattern: the mesh edges in both directions and the diagonal"""
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.concatenate([e, e[:, ::-1], np.stack([np.arange(V), np.arange(V)], 1)])
    key = np.unique(e[:, 0].astype(np.int64) * V + e[:, 1])
    rowptr = np.zeros(V + 1, np.int64)
    np.add.at(rowptr, key // V + 1, 1)
    return np.cumsum(rowptr), key % V


def rhs(V):
    """(V, 4) white right-hand side; the k-column case solves its first k columns"""
    return np.random.default_rng(20).standard_normal((V, 4)).astype(np.float32)


def case_id(name, arity, waves, k):
    return f"{name}-a{arity}-w{waves}-k{k}"


def digest(x):
    """sha256 of the fp32 bits of x (a contiguous (V, k) array) as 32 bytes"""
    a = np.ascontiguousarray(x, dtype=np.float32)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def solver(M, arity, waves):
    from largesteps.solvers import NestedDissectionSolver
    return NestedDissectionSolver(M, arity=arity, leaf_size=64, tier_waves=waves, ordering="longest-axis")
