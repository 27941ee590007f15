"""
The gathers of the tier kernels (csrc/nd_tier.h: pull_request / pull_sum, pull_compact, the right-hand-side gather at the kernel's head,
the tail of sparse_row, the rows past the 64th of a leaf's boundary) on the smallest meshes on which each of them runs
(tests/tier_gather_cases.py), for k = 1 .. 4 right-hand sides and every workgroup shape of the kernel:

    bits       x is, bit for bit, what the commit BEFORE the gathers were rewritten computed (tests/golden/tier_gather_bits.npz,
               recorded with that commit's library by tools/record_tier_gather_bits.py): the rewrite loads every child's row
               unconditionally and sums by a select in child order -- same operands, same order
    accuracy   forward error against the fp64 oracle's solution <= 1e-4 relative; the workgroup shapes agree to <= 2e-5 (the project's
               criteria for this solver, tests/test_gpu_parity.py)
    no leaks   the rows loaded for ABSENT children (row 0 of the hand-over array, whatever it holds) never reach a result: after a solve
               with 1e30-sized entries the same handle gives a normal right-hand side the bits a fresh handle gives it
"""
import os

import numpy as np
import pytest
import torch

import tier_gather_cases as tc
from oracle import solve as osv

gpu = pytest.mark.gpu
CASES = [(n, a, w, k) for (n, a, w) in tc.SHAPES for k in tc.KS]
IDS = [tc.case_id(*c) for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()          # fail loudly if the extension is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def record():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", tc.GOLDEN))


class _Systems:
    """matrix, right-hand side and fp64 solution per mesh; x and the solver's shape per (mesh, arity, waves), each computed once"""

    def __init__(self, dev):
        self.dev, self.sys, self.sol = dev, {}, {}

    def system(self, name):
        if name not in self.sys:
            from largesteps.geometry import compute_matrix
            v, f = tc.mesh(name)
            tv, tf = torch.from_numpy(v).to(self.dev), torch.from_numpy(f).to(self.dev)
            M = compute_matrix(tv, tf, tc.LAMBDA)
            B = tc.rhs(v.shape[0])
            idx, val = M.indices().cpu().numpy(), M.values().cpu().numpy()
            x64 = osv.DirectSolver(idx[0], idx[1], val, v.shape[0]).solve(B)
            self.sys[name] = (M, torch.from_numpy(B).to(self.dev), x64)
        return self.sys[name]

    def solutions(self, name, arity, waves):
        key = (name, arity, waves)
        if key not in self.sol:
            M, B, _ = self.system(name)
            s = tc.solver(M, arity, waves)
            inf = s.info()
            xs = {k: s.solve(B[:, :k].contiguous()).cpu().numpy() for k in tc.KS}
            s.close()
            self.sol[key] = (inf, xs)
        return self.sol[key]


@pytest.fixture(scope="module")
def systems(dev):
    return _Systems(dev)


def _ran_a_tier(inf, waves):
    if inf["tier_levels"] < 1 or inf["tier_workgroups"] < 1:
        pytest.skip(f"the library ran no tier on this mesh (info: {inf}); tier_waves={waves} was not exercised")


@gpu
@pytest.mark.parametrize("name,arity,waves,k", CASES, ids=IDS)
def test_bits_are_the_parent_commits(systems, record, name, arity, waves, k):
    inf, xs = systems.solutions(name, arity, waves)
    _ran_a_tier(inf, waves)
    cid = tc.case_id(name, arity, waves, k)
    shape = [inf["launches"], inf["tier_levels"], inf["tier_workgroups"], inf["levels"]]
    got, want = tc.digest(xs[k]), record[cid]
    print(cid, "shape", shape, "recorded", record[cid + "/shape"].tolist(), "sha256", got.tobytes().hex()[:16], "recorded", want.tobytes().hex()[:16])
    assert shape == record[cid + "/shape"].tolist(), "the solver's shape (launches, tier levels, tier workgroups, levels) is not the recorded one"
    assert np.array_equal(got, want), "x differs from the record in at least one bit"


@gpu
@pytest.mark.parametrize("name,arity,waves,k", CASES, ids=IDS)
def test_forward_error_against_the_fp64_oracle(systems, name, arity, waves, k):
    inf, xs = systems.solutions(name, arity, waves)
    _ran_a_tier(inf, waves)
    x64 = systems.system(name)[2][:, :k]
    err, scale = float(np.abs(xs[k] - x64).max()), float(np.abs(x64).max())
    print(tc.case_id(name, arity, waves, k), "forward error", err / scale)
    assert np.isfinite(xs[k]).all()
    assert err <= 1e-4 * scale


@gpu
@pytest.mark.parametrize("name,arity", sorted({(n, a) for (n, a, w) in tc.SHAPES}))
def test_workgroup_shapes_agree(systems, name, arity):
    widths = [w for (n, a, w) in tc.SHAPES if (n, a) == (name, arity)]
    x64 = systems.system(name)[2]
    first = systems.solutions(name, arity, widths[0])[1]
    for w in widths[1:]:
        inf, xs = systems.solutions(name, arity, w)
        _ran_a_tier(inf, w)
        for k in tc.KS:
            diff, scale = float(np.abs(xs[k] - first[k]).max()), float(np.abs(x64[:, :k]).max())
            print(name, arity, "waves", widths[0], "vs", w, "k", k, "difference", diff / scale)
            assert diff <= 2e-5 * scale


@gpu
@pytest.mark.parametrize("name,arity,waves", tc.SHAPES, ids=[f"{n}-a{a}-w{w}" for (n, a, w) in tc.SHAPES])
def test_a_huge_right_hand_side_leaves_nothing_behind(systems, name, arity, waves):
    """One handle: a solve with entries of size 1e30 (the hand-over arrays then hold such numbers, row 0 -- what an absent child's load
    reads -- included), then a normal right-hand side. A fresh handle gives the normal one the same bits."""
    M, B, _ = systems.system(name)
    b = B[:, :3].contiguous()
    s = tc.solver(M, arity, waves)
    _ran_a_tier(s.info(), waves)
    huge = s.solve((b * 1e30).contiguous())
    after = s.solve(b)
    s.close()
    fresh = systems.solutions(name, arity, waves)[1][3]
    print(name, arity, waves, "max |x| of the huge solve", float(huge.abs().max()))
    assert np.array_equal(after.cpu().numpy().view(np.uint32), fresh.view(np.uint32))


def test_the_rough_sphere_reaches_the_long_paths():
    """Host only (the planner through the C ABI): the rough sphere has a leaf with more than 64 boundary rows and, in both sweeps, sparse
    rows with more than TIER_SPE = 4 entries -- the loops of leaf_up_compute / leaf_down_head and the tail of sparse_row run on it."""
    from native_plan import native_plan
    v, f = tc.mesh("rough")
    V = v.shape[0]
    assert V == 16002
    rowptr, col = tc.pattern(f, V)
    p = native_plan(rowptr, col, v, leaf_size=64, arity=4, ordering=0)
    leaves = np.arange(p.level_off[p.levels - 1], p.level_off[p.levels])
    print("leaves", len(leaves), "largest boundary", int(p.b[leaves].max()), "largest leaf", int(p.s[leaves].max()))
    assert p.s[leaves].max() <= 64 and p.b[leaves].max() > 64
    # entries of the leaves' sparse blocks: (row, column) pairs of the matrix with exactly one end inside a leaf, in the tree's numbering
    rows = np.repeat(np.arange(V), np.diff(rowptr))
    rn, cn = p.inv[rows], p.inv[col]
    nr, nc = p.node_of_new[rn], p.node_of_new[cn]
    up = (nc >= leaves[0]) & (nr != nc)              # boundary row rn of leaf nc
    up_len = np.unique(nc[up] * V + rn[up], return_counts=True)[1]
    down_len = np.bincount(rn[(nr >= leaves[0]) & (nr != nc)], minlength=V)   # own row rn of its leaf
    print("longest sparse row: up", int(up_len.max()), "down", int(down_len.max()))
    assert up_len.max() > 4 and down_len.max() > 4
