"""
Depth peeling of largesteps.render without a device: the numpy statement (tests/peel_statement.py) against render_statement.py and
against itself (depth complexity, exact depth ties, strictly increasing keys), the two ls_peel_* entry points (declared, exported, bound,
and their argument checks, which run before the device is touched), and the public surface of `DepthPeeler`.
"""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import peel_statement as ps  # noqa: E402
import render_statement as rs  # noqa: E402
from render_scenes import random_soup, scene  # noqa: E402

PEEL_ENTRY_POINTS = ["ls_peel_forward", "ls_peel_range_forward"]
# scene -> (largest depth complexity, pixels with an exact z/w tie between two consecutive layers: the soups duplicate faces)
CASES = {"sphere": (2, 0), "sphere_b3": (4, 0), "folded": (2, 0), "near_plane": (1, 0), "quad": (1, 0),
         "soup0": (14, 822), "soup1": (12, 852), "soup2": (14, 955)}


def _scene(name):
    return random_soup(int(name[4:])) if name.startswith("soup") else scene(name)


@pytest.fixture(scope="module")
def peeled():
    """name -> (pos, tri, H, W, every layer of the statement up to the last non-empty one)"""
    out = {}
    for name in CASES:
        pos, tri, H, W = _scene(name)
        out[name] = (pos, tri, H, W, ps.peel(pos, tri, H, W))
    return out


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_layer_zero_of_the_statement_is_rasterize(peeled, name):
    pos, tri, H, W, layers = peeled[name]
    ref = rs.rasterize(pos, tri, H, W)
    assert np.array_equal(layers[0][..., 3], ref[..., 3])
    assert np.array_equal(layers[0].view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", list(CASES))
def test_depth_complexity_and_exact_ties_of_the_scenes(peeled, name):
    pos, tri, H, W, layers = peeled[name]
    depth, ties = CASES[name]
    count = ps.depth_complexity(pos, tri, H, W)
    assert count.max() == depth == layers.shape[0]
    for l in range(depth):                                     # a layer covers exactly the pixels with more than l fragments
        assert np.array_equal(layers[l][..., 3] > 0, count > l)
    both = (layers[1:][..., 3] > 0) & (layers[:-1][..., 3] > 0)
    same_z = both & (layers[1:][..., 2].view(np.uint32) == layers[:-1][..., 2].view(np.uint32))
    assert int(same_z.any(0).sum()) == ties
    if name == "sphere":
        assert int((count == 2).sum()) == 534 and count.size == 768


@pytest.mark.parametrize("name", list(CASES))
def test_keys_of_successive_layers_increase_strictly(peeled, name):
    layers = peeled[name][4]
    keys = ps.layer_keys(layers)
    for l in range(1, layers.shape[0]):
        covered = layers[l][..., 3] > 0
        assert np.all(keys[l][covered] > keys[l - 1][covered])
        assert np.all((layers[l - 1][..., 3] > 0)[covered])          # nothing appears behind background
    assert not ps.peel(peeled[name][0], peeled[name][1], peeled[name][2], peeled[name][3], layers.shape[0] + 1)[-1].any()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _lib():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native.lib()


def test_peel_entry_points_are_declared_exported_and_bound():
    from largesteps import _native
    names = [n for n in _native.EXPORTED_SYMBOLS if n.startswith("ls_peel_")]
    assert sorted(names) == sorted(PEEL_ENTRY_POINTS)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "largesteps_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(ls_peel_[a-z_0-9]+)\s*\(", header)) == set(PEEL_ENTRY_POINTS)
    lib = _lib()
    for n in PEEL_ENTRY_POINTS:
        assert getattr(lib, n).argtypes == _native._SIGNATURES[n][1]
    # the forward's arguments with prev_rast in front of rast
    fwd, peel = _native._SIGNATURES["ls_raster_forward"][1], _native._SIGNATURES["ls_peel_forward"][1]
    assert peel == fwd[:7] + [ctypes.c_void_p] + fwd[7:]
    fwd, peel = _native._SIGNATURES["ls_range_forward"][1], _native._SIGNATURES["ls_peel_range_forward"][1]
    assert peel == fwd[:9] + [ctypes.c_void_p] + fwd[9:]


def test_peel_argument_checks_run_without_a_device():
    """pointers are only compared, never followed: the checks come before the device is touched"""
    from largesteps import _native
    lib = _lib()
    B, V, F, N, H, W = 2, 5, 4, 6, 8, 8
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.ls_raster_workspace_bytes(B, F, H, W, 0, ctypes.byref(n)) == 0
    assert lib.ls_range_workspace_bytes(B, N, H, W, 0, ctypes.byref(m)) == 0
    pos, tri, ranges, prev, rast, ws = (ctypes.c_void_p(4096 * k) for k in range(1, 7))
    null = ctypes.c_void_p(0)

    def inst(prev=prev, rast=rast, ws_bytes=n.value, H=H):
        return lib.ls_peel_forward(pos, B, V, tri, F, H, W, prev, rast, ws, ws_bytes, 0, null)

    def rng(prev=prev, rast=rast, ws_bytes=m.value, H=H):
        return lib.ls_peel_range_forward(pos, V, tri, F, ranges, B, N, H, W, prev, rast, ws, ws_bytes, 0, null)

    for call in (inst, rng):
        assert call(prev=null) == _native.LS_E_INVALID
        assert "null argument" in _native.last_error()
        assert call(prev=rast) == _native.LS_E_INVALID
        assert "same buffer" in _native.last_error()
        assert call(rast=null) == _native.LS_E_INVALID
        assert call(ws_bytes=call.__defaults__[2] - 1) == _native.LS_E_WORKSPACE
        assert call(H=5000) == _native.LS_E_INVALID
        assert call(H=0) == _native.LS_E_INVALID
    assert lib.ls_peel_forward(pos, 1, V, tri, 2 ** 24, H, W, prev, rast, ws, n.value, 0, null) == _native.LS_E_OVERFLOW
    assert lib.ls_peel_range_forward(pos, V, tri, F, ranges, B, 2 ** 30, H, W, prev, rast, ws, m.value, 0, null) == _native.LS_E_OVERFLOW
    assert lib.ls_version() == 110


def test_the_peel_adds_no_depth_kernel_of_its_own():
    """the peeling kernels are instantiations of the two depth kernels (still two atomicMin sites, no float atomics)"""
    src = open(os.path.join(ROOT, "large-steps-pytorch_amd", "csrc", "raster.hip")).read()
    assert "ls_peel_forward" in src and "ls_peel_range_forward" in src
    assert src.count("atomicMin(") == 2 and "atomicAdd" not in src and "atomicMax" not in src
    assert len(re.findall(r"__global__[^;{]*\bk_rs_(?:small|large)\b", src)) == 2


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_depth_peeler_surface():
    import largesteps.render as dr
    assert "DepthPeeler" in dr.__all__
    assert list(inspect.signature(dr.DepthPeeler).parameters) == ["glctx", "pos", "tri", "resolution", "ranges", "grad_db"]
    assert list(inspect.signature(dr.DepthPeeler).parameters) == list(inspect.signature(dr.rasterize).parameters)
    assert inspect.signature(dr.DepthPeeler).parameters["ranges"].default is None
    assert list(inspect.signature(dr.DepthPeeler.rasterize_next_layer).parameters) == ["self"]
    for frame in (dr._InstancedFrame, dr._RangeFrame):
        assert callable(frame.rasterize) and callable(frame.rasterize_layer)


def test_rasterize_next_layer_outside_the_with_block_raises():
    """a peeler cannot be constructed without a device, so this one is allocated and given the state the constructor leaves: no `with`
    block entered (the GPU tests call a constructed one before `with` and after it)"""
    import largesteps.render as dr
    peeler = dr.DepthPeeler.__new__(dr.DepthPeeler)
    peeler._active = False
    with pytest.raises(RuntimeError, match="`with` block"):
        peeler.rasterize_next_layer()


def test_cpu_tensors_raise_what_rasterize_raises():
    import largesteps.render as dr
    tri = torch.zeros((1, 3), dtype=torch.int32)
    cases = [
        (dict(pos=torch.zeros(1, 3, 4), tri=tri, resolution=(8, 8)), RuntimeError),                               # no CPU path
        (dict(pos=torch.zeros(1, 3, 4), tri=tri, resolution=(8, 5000)), ValueError),
        (dict(pos=torch.zeros(4, 4), tri=tri, resolution=(8, 8), ranges=torch.zeros((1, 2), dtype=torch.int32)), NotImplementedError),
        (dict(pos=torch.zeros(4, 4), tri=tri, resolution=(8, 8), ranges=torch.tensor([[0, 2]], dtype=torch.int32)), ValueError),
        (dict(pos=torch.zeros(4, 4), tri=tri, resolution=(8, 8), ranges=torch.zeros((1, 2), dtype=torch.int64)), TypeError),
        (dict(pos=torch.zeros(2, 4, 4), tri=tri, resolution=(8, 8), ranges=torch.zeros((1, 2), dtype=torch.int32)), ValueError),
        (dict(pos=[[0.0] * 4], tri=tri, resolution=(8, 8)), TypeError),
    ]
    for kw, exc in cases:
        with pytest.raises(exc) as want:
            dr.rasterize(None, **kw)
        with pytest.raises(exc) as got:
            dr.DepthPeeler(None, **kw)
        assert str(got.value) == str(want.value)
