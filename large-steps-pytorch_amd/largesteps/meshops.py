"""
Mesh bookkeeping the optimisation loop needs around a remesh, on the MI355X.

`remove_duplicates` is the reference's scripts/geometry.py:3-11 with the same name, argument order and return values
(unique vertices in the order torch.unique(dim=0) gives them, re-indexed faces, inverse map) -- one native call
(`ls_remove_duplicates`: hand-written radix sort + compaction) instead of torch.unique's library sort.

`average_edge_length` (scripts/geometry.py:13-33; scripts/main.py:146 takes the remesher's target edge length from it) and
`massmatrix_voronoi` (:35-89, the Voronoi area of every vertex) keep the reference's names, argument order and shapes (a 0-dim
tensor, a (V,) tensor) and are differentiable with respect to the vertices (autograd Functions over csrc/meshgeom.hip: a
hand-written forward and backward each, no atomics, bitwise reproducible, no host synchronisation once the face tensor's corner
ranking is cached -- so they can sit in a captured graph). The results are float32, as the reference's are for fp32 vertices.
Faces may be int32 or int64 (the reference needs int64 for scatter_add_). The reference's quirks are kept:
  * a face with a zero-length edge has NaN cells (0 / 0 in its cosines), so its vertices' mass is NaN;
  * an unreferenced vertex has mass 0;
  * the obtuse-triangle rule tests `cos < 0` on the fp32 cosine: a right angle whose cosine rounds to a slightly negative value
    takes the obtuse branch (same cells at exactly 90 degrees, a different gradient) -- the branch follows the reference's fp32
    arithmetic, which the kernel reproduces operation for operation;
  * average_edge_length counts an interior edge twice and a boundary edge once (it averages over the 3 F face edges); F == 0
    gives NaN, and massmatrix_voronoi then returns zeros.
There is no CPU path.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _native
from .normals import _mesh, _on, _prep, _tail, _workspace_of


def remove_duplicates(v, f):
    """
    Generate a mesh representation with no duplicates and
    return it along with the mapping to the original mesh layout.

    Returns (unique_verts (U, 3), new_faces (F, 3) int64, inverse (V,) int64) with v == unique_verts[inverse].
    """
    _native.require_device(v, "v")
    _native.require_device(f, "f")
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"v must be (V, 3), got {tuple(v.shape)}")
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"f must be (F, 3), got {tuple(f.shape)}")
    if v.dtype != torch.float32:
        raise TypeError(f"v must be float32, got {v.dtype}")
    if f.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"f must be int32 or int64, got {f.dtype}")
    if f.device != v.device:
        raise RuntimeError(f"v ({v.device}) and f ({f.device}) must be on the same device")
    vc, fc = v.detach().contiguous(), f.contiguous()
    V, F, dev = vc.shape[0], fc.shape[0], vc.device
    lib = _native.lib()
    ws = _native.workspace("ls_remove_duplicates_workspace_bytes", (V,), dev)
    unique = torch.empty((V, 3), dtype=torch.float32, device=dev)
    inverse = torch.empty(V, dtype=torch.int64, device=dev)
    new_faces = torch.empty((F, 3), dtype=torch.int64, device=dev)
    nu = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        _native.check(lib.ls_remove_duplicates(_native.ptr(vc), V, _native.ptr(fc), fc.element_size(), F, _native.ptr(unique), _native.ptr(inverse),
                                               _native.ptr(new_faces), ctypes.byref(nu), *_tail(ws, dev)))
    return unique[: nu.value], new_faces, inverse


_workspace = _workspace_of("ls_meshgeom_workspace_bytes")


# Both Functions validate the faces through the corner ranking of normals._prep (built once per face tensor: the range check
# raises IndexError and is the only host synchronisation); the kernels trust that plan.
class _AverageEdgeLength(Function):
    @staticmethod
    def forward(ctx, verts, faces):
        v, f, vptr, vcorner, _ = _prep(verts, faces)
        F, V, dev = f.shape[0], v.shape[0], v.device
        out = torch.empty((), dtype=torch.float32, device=dev)
        ws = _workspace(F, V, dev)
        with _on(dev):
            _native.check(_native.lib().ls_average_edge_length(*_mesh(v, f), _native.ptr(out), *_tail(ws, dev)))
        ctx.save_for_backward(v, f, vptr, vcorner)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        v, f, vptr, vcorner = ctx.saved_tensors
        F, V, dev = f.shape[0], v.shape[0], v.device
        g = g.to(torch.float32).contiguous()
        gv = torch.empty_like(v)
        ws = _workspace(F, V, dev)
        with _on(dev):
            _native.check(_native.lib().ls_average_edge_length_backward(*_mesh(v, f), _native.ptr(vptr), _native.ptr(vcorner), _native.ptr(g),
                                                                        _native.ptr(gv), *_tail(ws, dev)))
        return gv, None


class _MassmatrixVoronoi(Function):
    @staticmethod
    def forward(ctx, verts, faces):
        v, f, vptr, vcorner, order = _prep(verts, faces)
        F, V, dev = f.shape[0], v.shape[0], v.device
        mass = torch.empty(V, dtype=torch.float32, device=dev)
        with _on(dev):
            _native.check(_native.lib().ls_massmatrix_voronoi(*_mesh(v, f), _native.ptr(vptr), _native.ptr(order), _native.ptr(mass), dev.index,
                                                              _native.stream_of(dev)))
        ctx.save_for_backward(v, f, vptr, vcorner)
        return mass

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        v, f, vptr, vcorner = ctx.saved_tensors
        F, V, dev = f.shape[0], v.shape[0], v.device
        g = g.to(torch.float32).contiguous()
        gv = torch.empty_like(v)
        ws = _workspace(F, V, dev)
        with _on(dev):
            _native.check(_native.lib().ls_massmatrix_voronoi_backward(*_mesh(v, f), _native.ptr(vptr), _native.ptr(vcorner), _native.ptr(g),
                                                                       _native.ptr(gv), *_tail(ws, dev)))
        return gv, None


@_native.retry_on_oom
def average_edge_length(verts, faces):
    """
    Compute the average length of all edges in a given mesh (scripts/geometry.py:13-33). Returns a 0-dim float32 tensor.

    Parameters
    ----------
    verts : torch.Tensor
        Vertex positions (V, 3), on a HIP device.
    faces : torch.Tensor
        array of triangle faces (F, 3), int32 or int64.
    """
    return _AverageEdgeLength.apply(verts, faces)


@_native.retry_on_oom
def massmatrix_voronoi(verts, faces):
    """
    Compute the area of the Voronoi cell around each vertex in the mesh (scripts/geometry.py:35-89). Returns a (V,) float32
    tensor.

    params
    ------

    verts: vertex positions (V, 3), on a HIP device
    faces: triangle indices (F, 3), int32 or int64
    """
    return _MassmatrixVoronoi.apply(verts, faces)
