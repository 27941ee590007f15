"""
csrc/meshgeom.hip and k_gather_corners (csrc/meshface.h) BIT FOR BIT against the fp32 statement in the kernels' order
(tests/meshgeom_ordered.py; the forward mass against tests/meshgeom_statement.py in fp32), on the cases of tests/meshgeom_scale_cases.py:
past one and two sweeps of the average's capped grid, around a wave and a workgroup, on valences of every remainder modulo the two
request groups and far past them, and with V around one workgroup of the per-vertex kernels. What each case crosses, why the average
is exactly predictable and that the ordered statement is the fp64 statement's function are asserted on the CPU
(tests/test_meshgeom_scale_cpu.py).

"rank order is summation order, so every gradient is bitwise reproducible" (csrc/meshface.h): no tolerance anywhere below. Every output is
taken through the public functions with int32 and with int64 faces, the int32 run twice. Every case prints how many values differ (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import meshgeom_ordered as mo
import meshgeom_scale_cases as mc
import meshgeom_statement as ms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # a copy: the cases are read-only arrays


class Reference:
    """the statements on one case: computed once per module on first use, read-only"""

    def __init__(self, name):
        self.name = name
        self.v, self.f = mc.mesh(name)
        self.V, self.F = self.v.shape[0], self.f.shape[0]
        self.unreferenced = mc.valence(name) == 0

    def _frozen(self, a):
        a = np.asarray(a)
        a.setflags(write=False)
        return a

    @functools.cached_property
    def terms(self):
        return ms.face_terms(self.v, self.f, np.float32)

    @functools.cached_property
    def average(self):
        return self._frozen(mo.average(self.v, self.f, self.terms))

    @functools.cached_property
    def average_backward(self):
        return {g: self._frozen(mo.gather(mo.corner_rows_avg(self.v, self.f, g, self.terms), self.f, self.V)) for g in mc.AVG_WEIGHTS}

    @functools.cached_property
    def mass(self):
        return self._frozen(ms.massmatrix_voronoi(self.v, self.f, np.float32))

    @functools.cached_property
    def mass_backward(self):
        return self._frozen(mo.gather(mo.corner_rows_mass(self.v, self.f, mc.mass_weights(self.name), self.terms), self.f, self.V))


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(name)


def same_bits(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    g, w = got.reshape(-1), want.reshape(-1)
    diff = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
    line = f"{what}: {diff.size} of {g.size} values differ"
    if diff.size:
        i = int(diff[0])
        ulp = np.abs(g[diff].astype(np.float64) - w[diff]) / np.spacing(np.abs(w[diff])).astype(np.float64)
        line += f"; first at {i}: device {g[i]!r} ({g[i:i + 1].view(np.int32)[0]:#010x}), statement {w[i]!r} " \
                f"({w[i:i + 1].view(np.int32)[0]:#010x}); largest distance {np.nanmax(ulp):.3g} ulp"
    print(line)
    assert diff.size == 0, line


def runs(dev, name, fn):
    """fn(verts, faces) -> numpy result, with int32 faces twice and with int64 faces once"""
    r = reference(name)
    out = []
    for idx in (np.int32, np.int32, np.int64):
        tv, tf = _t(r.v, dev).requires_grad_(True), _t(r.f.astype(idx), dev)
        out.append((idx.__name__, fn(tv, tf).detach().cpu().numpy()))
    return out


@pytest.mark.parametrize("name", mc.CASES)
def test_average_edge_length_bits(dev, name):
    from largesteps.meshops import average_edge_length
    for idx, avg in runs(dev, name, average_edge_length):
        same_bits(f"average {name} {idx}", avg, reference(name).average)


@pytest.mark.parametrize("name", mc.CASES)
def test_average_edge_length_backward_bits(dev, name):
    from largesteps.meshops import average_edge_length
    r = reference(name)
    for g in mc.AVG_WEIGHTS:
        def grad(tv, tf):
            return torch.autograd.grad(average_edge_length(tv, tf), tv, grad_outputs=torch.tensor(g, dtype=torch.float32, device=dev))[0]

        for idx, gv in runs(dev, name, grad):
            same_bits(f"average backward {name} g={g} {idx}", gv, r.average_backward[g])
            assert not gv[r.unreferenced].view(np.int32).any(), "an unreferenced vertex has a gradient that is not +0"
    assert np.abs(r.average_backward[1.0]).max() > 0


@pytest.mark.parametrize("name", mc.CASES)
def test_massmatrix_voronoi_bits(dev, name):
    from largesteps.meshops import massmatrix_voronoi
    r = reference(name)
    for idx, mass in runs(dev, name, massmatrix_voronoi):
        same_bits(f"mass {name} {idx}", mass, r.mass)
        assert not mass[r.unreferenced].view(np.int32).any()
    assert np.isfinite(r.mass).all() and (r.mass[~r.unreferenced] > 0).all()


@pytest.mark.parametrize("name", mc.CASES)
def test_massmatrix_voronoi_backward_bits(dev, name):
    from largesteps.meshops import massmatrix_voronoi
    r = reference(name)
    w = _t(mc.mass_weights(name), dev)

    def grad(tv, tf):
        return torch.autograd.grad(massmatrix_voronoi(tv, tf), tv, grad_outputs=w)[0]

    for idx, gv in runs(dev, name, grad):
        same_bits(f"mass backward {name} {idx}", gv, r.mass_backward)
        assert not gv[r.unreferenced].view(np.int32).any()
    assert np.isfinite(r.mass_backward).all() and np.abs(r.mass_backward).max() > 0
