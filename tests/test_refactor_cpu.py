"""
Same-pattern refactorisation without a device: the three entry points are declared, exported and bound, their argument checks run on
the host, and NestedDissectionSolver.refactor / CholeskySolver.refactor / parameterize.update_matrix / DifferentiableSolve validate
before anything reaches the device.
"""
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ls_direct_factor_refactorable", "ls_direct_refactor", "ls_direct_refactorable")


@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


def test_entry_points_are_declared_exported_and_bound(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", native.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in exported and name in native.EXPORTED_SYMBOLS, name
        assert getattr(native.lib(), name).restype is ctypes.c_int


def test_host_side_argument_checks(native):
    lib = native.lib()
    yes, kept = ctypes.c_int(7), ctypes.c_size_t(7)
    assert lib.ls_direct_refactorable(None, ctypes.byref(yes), ctypes.byref(kept)) == native.LS_E_INVALID
    assert lib.ls_direct_refactor(None, None, None, None, 10, 40, None) == native.LS_E_INVALID
    assert "ls_direct_refactor" in native.last_error()
    h = ctypes.c_void_p()
    assert lib.ls_direct_factor_refactorable(None, None, None, 10, 40, None, None, 0, None, ctypes.byref(h)) == native.LS_E_INVALID
    assert not h.value
    opt = native.DirectOptions()
    assert lib.ls_direct_options_default(ctypes.byref(opt)) == 0
    opt.struct_bytes = 0
    assert lib.ls_direct_factor_refactorable(None, None, None, 10, 40, None, ctypes.byref(opt), 0, None, ctypes.byref(h)) == native.LS_E_INVALID
    assert "struct_bytes" in native.last_error()


def _cpu_matrix(V):
    i = torch.arange(V)
    return torch.sparse_coo_tensor(torch.stack([i, i]), torch.ones(V), (V, V)).coalesce()


def _fake_direct(V=10, nnz=10, refactorable=True):
    """A NestedDissectionSolver as it looks from Python, with no native handle behind it (nothing here may reach one)."""
    from largesteps.solvers import NestedDissectionSolver
    s = NestedDissectionSolver.__new__(NestedDissectionSolver)
    s._csr = types.SimpleNamespace(V=V, nnz=nnz, device=torch.device("cuda", 0))
    s.refactorable, s.generation, s._direct = refactorable, 0, None
    return s


def test_refactor_validates_before_the_device(native):
    from largesteps.solvers import CholeskySolver
    s = _fake_direct()
    with pytest.raises(TypeError):
        s.refactor(torch.eye(10))                           # dense
    with pytest.raises(ValueError, match="new solver"):
        s.refactor(_cpu_matrix(11))                         # wrong V
    with pytest.raises(RuntimeError, match="HIP device"):
        s.refactor(_cpu_matrix(10))                         # a CPU matrix
    assert s.generation == 0
    c = CholeskySolver.__new__(CholeskySolver)
    c.refactorable, c.generation, c._impl = True, 0, s
    with pytest.raises(ValueError, match="new solver"):
        c.refactor(_cpu_matrix(9))
    c.refactorable = False
    with pytest.raises(RuntimeError, match="refactorable=False"):
        c.refactor(_cpu_matrix(10))
    assert c.generation == 0


def test_update_matrix_validates_before_the_device(native):
    from largesteps.parameterize import update_matrix
    L = _cpu_matrix(10)
    with pytest.raises(ValueError, match="Unknown solver type"):
        update_matrix(L, L, method="LU")
    with pytest.raises(TypeError):
        update_matrix(L, torch.eye(10))
    with pytest.raises(RuntimeError, match="HIP device"):
        update_matrix(L, _cpu_matrix(10))
    with pytest.raises(RuntimeError, match="HIP device"):
        update_matrix(L, _cpu_matrix(10), method="CG")


def test_backward_after_a_refactor_raises():
    """DifferentiableSolve records the solver's generation in forward; a refactor in between makes backward raise."""
    from largesteps.solvers import Solver, solve

    class Doubling(Solver):
        def solve(self, b, backward=False):
            return 2.0 * b

    s = Doubling(None)
    b = torch.ones(4, 3, requires_grad=True)
    solve(s, b).sum().backward()
    assert torch.equal(b.grad, torch.full((4, 3), 2.0))
    x = solve(s, b)
    s.generation += 1
    with pytest.raises(RuntimeError, match="refactored"):
        x.sum().backward()
