"""
Range mode of largesteps.render without a device: the host validation of `ranges`, the errors CPU tensors get, and the native surface
(the ls_range_* entry points declared in the header, exported and bound; the library's version; no float atomics in their source).
"""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

RANGE_ENTRY_POINTS = ["ls_range_workspace_bytes", "ls_range_forward", "ls_range_pixel_order", "ls_range_backward",
                      "ls_range_interpolate_backward", "ls_range_adjacency_workspace_bytes", "ls_range_adjacency", "ls_range_antialias",
                      "ls_range_antialias_backward"]


def _ranges(rows, dtype=torch.int32):
    return torch.tensor(rows, dtype=dtype).reshape(-1, 2)


def _call(ranges, pos=None, F=6):
    import largesteps.render as dr
    pos = torch.zeros(5, 4) if pos is None else pos
    return dr.rasterize(None, pos, torch.zeros((F, 3), dtype=torch.int32), (8, 8), ranges=ranges)


def test_valid_ranges_on_cpu_tensors_say_that_range_mode_needs_a_device():
    for rows in ([(0, 6)], [(0, 0)], [(6, 0)], [(2, 3), (0, 6), (5, 1)], [(3, 3), (0, 3)]):      # whole, empty, overlapping, unsorted
        with pytest.raises(NotImplementedError, match="range mode.*needs a HIP device"):
            _call(_ranges(rows))


def test_ranges_are_validated_on_the_host():
    import largesteps.render as dr
    assert dr._check_ranges(_ranges([(2, 3), (0, 6), (4, 0)]), 6) == (3, 9)
    for rows in ([(0, 7)], [(-1, 2)], [(2, -1)], [(5, 2)], [(0, 6), (7, 0)]):
        with pytest.raises(ValueError, match="outside the 6 faces"):
            _call(_ranges(rows))
    with pytest.raises(TypeError, match="int32"):
        _call(_ranges([(0, 6)], torch.int64))
    with pytest.raises(TypeError, match="int32"):
        _call(_ranges([(0, 6)]).float())
    with pytest.raises(TypeError, match="torch.Tensor"):
        _call([(0, 6)])
    for shape in ((2, 3), (4,), (0, 2), (1, 2, 2)):
        with pytest.raises(ValueError, match=r"\(B, 2\)"):
            _call(torch.zeros(shape, dtype=torch.int32))
    with pytest.raises(ValueError, match="instanced"):          # a batched pos is instanced mode
        _call(_ranges([(0, 6)]), pos=torch.zeros(2, 5, 4))
    with pytest.raises(ValueError, match=r"\(V, 4\)"):
        _call(_ranges([(0, 6)]), pos=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="resolution"):
        dr.rasterize(None, torch.zeros(5, 4), torch.zeros((6, 3), dtype=torch.int32), (8, 5000), ranges=_ranges([(0, 6)]))


def test_a_flat_pos_without_a_range_table_is_refused():
    import largesteps.render as dr
    rast, tri = torch.zeros(1, 8, 8, 4), torch.zeros((6, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="rasterize"):
        dr.antialias(torch.zeros(1, 8, 8, 3), rast, torch.zeros(5, 4), tri)
    with pytest.raises(NotImplementedError, match="range mode"):
        dr.pixel_differentials(rast, torch.zeros(5, 4), tri)


def test_range_entry_points_are_declared_exported_and_bound():
    from largesteps import _native
    names = [n for n in _native.EXPORTED_SYMBOLS if n.startswith("ls_range_")]
    assert sorted(names) == sorted(RANGE_ENTRY_POINTS)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ls_range_[a-z_0-9]+)\s*\(", header))
    assert declared == set(RANGE_ENTRY_POINTS)
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _native.lib()
    for n in RANGE_ENTRY_POINTS:
        assert getattr(lib, n).argtypes == _native._SIGNATURES[n][1]
    assert lib.ls_version() == 110


def test_range_workspace_sizes_and_limits_without_a_device():
    import ctypes
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _native.lib()
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.ls_range_workspace_bytes(4, 1000, 32, 32, 3, ctypes.byref(n)) == 0
    assert lib.ls_raster_workspace_bytes(4, 250, 32, 32, 3, ctypes.byref(m)) == 0
    assert n.value == m.value > 0                                  # the same layout: N items in place of B F faces
    assert lib.ls_range_workspace_bytes(64, 2 * 10 ** 6, 256, 256, 3, ctypes.byref(n)) == 0
    assert n.value < 2 ** 31                                       # sized by items, not by B F (131 M rows at these sizes)
    assert lib.ls_range_workspace_bytes(0, 10, 32, 32, 3, ctypes.byref(n)) == _native.LS_E_INVALID
    assert lib.ls_range_workspace_bytes(1, 10, 32, 5000, 3, ctypes.byref(n)) == _native.LS_E_INVALID
    assert lib.ls_range_workspace_bytes(1, 2 ** 30, 32, 32, 3, ctypes.byref(n)) == _native.LS_E_OVERFLOW
    assert lib.ls_range_workspace_bytes(1024, 10, 2048, 2048, 3, ctypes.byref(n)) == _native.LS_E_OVERFLOW
    assert lib.ls_range_adjacency_workspace_bytes(1000, ctypes.byref(n)) == 0 and n.value > 4 * 3000
    assert lib.ls_range_adjacency_workspace_bytes(-1, ctypes.byref(n)) == _native.LS_E_INVALID


def test_no_float_atomics_in_the_source_of_the_range_kernels():
    src = open(os.path.join(ROOT, "large-steps-pytorch_amd", "csrc", "raster.hip")).read()
    assert "ls_range_forward" in src and "k_rg_gather_pos" in src
    assert "atomicAdd" not in src and "unsafeAtomicAdd" not in src
    assert src.count("atomicMin(") == 2                            # the depth pass's 64-bit integer minimum: the small and the tile path
