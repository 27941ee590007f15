"""
From a field back to a mesh on the MI355X: a deterministic, differentiable isosurface extractor, and level-set remeshing on top of it.

    from largesteps.levelset import isosurface             # igl.marching_tets on a regular grid; MeshSDF / DMTet style extraction
    from largesteps.levelset import remesh_level_set       # a self-intersecting mesh -> a closed one without crossings

`isosurface(S, iso)` returns the level set S = iso of a scalar field on a regular grid as a triangle mesh (csrc/isosurf.hip, DESIGN.md
section 2.13; tests/isosurf_statement.py restates the rule in numpy and the device returns the same bits). The rule is marching
tetrahedra on the Kuhn split: every cube of 8 nodes is cut into the same 6 tets, whose face diagonals agree between neighbours, so the
level set of the piecewise-linear interpolant is a closed, consistently oriented 2-manifold wherever it does not leave the grid -- no
ambiguous cases, no 256-entry table. S is (nx, ny, nz); node (i, j, k) lies at origin + spacing * (i, j, k). A node is low iff S < iso
(a NaN counts as high); there is one vertex on every grid edge (along 100, 010, 001, 110, 011, 101 or 111) whose two ends are finite and
of which exactly one is low, at the linear interpolant's crossing; a cube with a NaN or infinite corner emits nothing; a grid with
a side of 1 gives nothing. Every face's normal points from the low side to the high side: outward for a field that is negative inside.
Vertices are ordered by (node, direction) and faces by (cube, tet) through two prefix sums -- no sort, no atomics -- so the result
depends on (S, iso, origin, spacing) alone and is bitwise reproducible.

S == iso exactly at a node is legal and follows the low / high rule (the node is high): the vertices of the live edges at that node
coincide with it (t = 0) and the faces between them have zero area. Move iso by a rounding error if that matters downstream.

Autograd. With a tensor S that requires grad, V is differentiable in S: a vertex on the edge a -> b at t = (iso - S[a]) / (S[b] - S[a])
moves along the edge, dV / dS[a] = -(1 - t) / (S[b] - S[a]) (p_b - p_a) and dV / dS[b] = -t / (S[b] - S[a]) (p_b - p_a). The backward is a
gather per node over its 14 incident edges in a fixed order, every term formed in float64 and the sum rounded to float32 once:
no float atomics, bitwise reproducible, no host synchronisation, capturable in a torch.cuda.graph. F and E are not differentiable; iso,
origin and spacing are Python numbers and get no gradient. The connectivity is held fixed, as in MeshSDF.

The forward reads the two totals (vertices, faces) on the host to size its outputs: one synchronisation, so `isosurface` itself is
not capturable (like `MeshDistance.self_intersections`).

Input conventions follow largesteps.distance: a numpy S (any real dtype, converted to fp32) runs on the current HIP device and returns
numpy; a tensor S (fp32, on a HIP device) returns tensors on that device. CPU tensors raise.
"""
import ctypes
import math

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from .distance import MeshDistance, _as_beta, _as_faces, _as_points, _current_device


def _fits(shape):
    """the int32 limits of csrc/isosurf.hip: 8 x the nodes and 12 x the cubes stay below 2^31"""
    nx, ny, nz = (int(s) for s in shape)
    return 8 * nx * ny * nz < 2 ** 31 and 12 * (nx - 1) * (ny - 1) * (nz - 1) < 2 ** 31


def _real(x, what):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what} must be a real number, got {type(x).__name__}")
    return float(x)


def _triple(x, what):
    if isinstance(x, (tuple, list, np.ndarray)) and len(x) == 3:
        return tuple(_real(v.item() if isinstance(v, np.generic) else v, what) for v in x)
    raise ValueError(f"{what} must have 3 entries, got {x!r}")


def _as_spacing(spacing):
    sp = _triple(spacing, "spacing") if isinstance(spacing, (tuple, list, np.ndarray)) else (_real(spacing, "spacing"),) * 3
    if not all(math.isfinite(s) and s > 0 for s in sp):
        raise ValueError(f"spacing must be positive and finite, got {spacing!r}")
    return sp


def _as_field(S):
    """(tensor (nx, ny, nz) fp32, or a contiguous fp32 numpy array; was_numpy); raises before any device work"""
    if isinstance(S, torch.Tensor):
        _native.require_device(S, "S")
        if S.dtype != torch.float32:
            raise TypeError(f"S must be float32, got {S.dtype}")
        if S.dim() != 3:
            raise ValueError(f"S must be (nx, ny, nz), got {tuple(S.shape)}")
        Sn = S
    else:
        Sn = np.asarray(S)
        if not (np.issubdtype(Sn.dtype, np.floating) or np.issubdtype(Sn.dtype, np.integer)):
            raise TypeError(f"S must hold real numbers, got {Sn.dtype}")
        if Sn.ndim != 3:
            raise ValueError(f"S must be (nx, ny, nz), got {Sn.shape}")
    if min(Sn.shape) < 1:
        raise ValueError(f"S must have at least one node along every axis, got {tuple(Sn.shape)}")
    _check_grid(Sn.shape)
    if isinstance(S, torch.Tensor):
        return S, False
    return np.ascontiguousarray(Sn, dtype=np.float32), True


def _check_grid(shape):
    if not _fits(shape):
        raise OverflowError(f"isosurface: a grid of {' x '.join(str(int(s)) for s in shape)} nodes passes the int32 limits of the kernels "
                            "(8 x nodes and 12 x cubes below 2^31)")


def _floats(x):
    return (ctypes.c_float * 3)(*x)


class _Isosurface(Function):
    """V, F, E of the field S; the workspace with the masks and offsets is kept for the backward"""

    @staticmethod
    def forward(ctx, S, iso, origin, spacing):
        s = S.detach().contiguous()
        dev = s.device
        nx, ny, nz = s.shape
        lib = _native.lib()
        with torch.cuda.device(dev):
            ws = _native.workspace("ls_iso_workspace_bytes", (nx, ny, nz), dev)
            totals = torch.empty(2, dtype=torch.int64, device=dev)
            _native.check(lib.ls_iso_count(_native.ptr(s), nx, ny, nz, iso, _native.ptr(ws), ws.numel(), _native.ptr(totals), dev.index,
                                           _native.stream_of(dev)))
            n, m = (int(x) for x in totals.cpu())              # the one synchronisation
            V = torch.empty((n, 3), dtype=torch.float32, device=dev)
            E = torch.empty(n, dtype=torch.int64, device=dev)
            F = torch.empty((m, 3), dtype=torch.int64, device=dev)
            _native.check(lib.ls_iso_fill(_native.ptr(s), nx, ny, nz, iso, _floats(origin), _floats(spacing), _native.ptr(ws), ws.numel(), n, m,
                                          _native.ptr(V), _native.ptr(E), _native.ptr(F), dev.index, _native.stream_of(dev)))
        ctx.args = (iso, origin, spacing)
        ctx.save_for_backward(s, ws)
        ctx.mark_non_differentiable(F, E)
        return V, F, E

    @staticmethod
    @once_differentiable
    def backward(ctx, gV, _gF, _gE):
        s, ws = ctx.saved_tensors
        iso, origin, spacing = ctx.args
        dev = s.device
        nx, ny, nz = s.shape
        g = gV.to(torch.float32).contiguous()
        gS = torch.empty_like(s)
        with torch.cuda.device(dev):
            _native.check(_native.lib().ls_iso_backward(_native.ptr(s), nx, ny, nz, iso, _floats(origin), _floats(spacing), _native.ptr(ws),
                                                        ws.numel(), g.shape[0], _native.ptr(g), _native.ptr(gS), dev.index,
                                                        _native.stream_of(dev)))
        return gS, None, None, None


@_native.retry_on_oom
def isosurface(S, iso=0.0, origin=(0.0, 0.0, 0.0), spacing=1.0, return_edges=False):
    """(V (n, 3) float32, F (m, 3) int64[, E (n,) int64]): the level set S = iso of the field S (nx, ny, nz) on the grid whose node
    (i, j, k) lies at origin + spacing * (i, j, k), by marching tetrahedra on the Kuhn split (module docstring). `spacing` is a
    positive number or three of them. Faces are oriented with their normals from S < iso to S >= iso. With return_edges, E[v] =
    8 * node + direction names the grid edge vertex v lies on (node = (i * ny + j) * nz + k; directions 100, 010, 001, 110, 011, 101,
    111 = 0..6): libigl's marching_tets returns the same as J. Nothing crossing gives (0, 3) arrays.

    S == iso exactly at a node is legal: the node counts as high, the vertices of its live edges coincide with it and the faces
    between them have zero area. NaN and infinite nodes remove the cubes around them, which leaves a boundary.

    V is differentiable in a tensor S that requires grad; F and E are not. The call synchronises once (it reads the two totals to
    size the outputs) and is not capturable; its backward does not synchronise and is. numpy S gives numpy results, a tensor gives
    tensors; a non-contiguous S is copied. Bitwise reproducible."""
    iso = _real(iso, "iso")
    origin = _triple(origin, "origin")
    spacing = _as_spacing(spacing)
    s, s_np = _as_field(S)
    if s_np:
        s = torch.from_numpy(s).to(_current_device())
    V, F, E = _Isosurface.apply(s, iso, origin, spacing)
    if s_np:
        V, F, E = V.cpu().numpy(), F.cpu().numpy(), E.cpu().numpy()
    return (V, F, E) if return_edges else (V, F)


def _grid_over(lo, hi, h, pad):
    """(origin (3,) float64, dims (3,) int) of the grid of spacing h over the box [lo, hi] padded by pad * h"""
    origin = lo - pad * h
    dims = np.ceil((hi - lo) / h + 2 * pad).astype(np.int64) + 1
    return origin, dims


@_native.retry_on_oom
def remesh_level_set(V, F, h, field="winding", offset=0.0, pad=2, beta=2.0):
    """(V2, F2): the mesh (V, F) rebuilt as a level set of its own inside / outside field on a grid of spacing `h` -- the repair of a
    mesh that cuts through itself (Barill et al. 2018). The grid covers the bounding box of V padded by `pad` * h; at its nodes
    field='winding' evaluates S = 0.5 - winding_number(P, beta) and field='signed_distance' S = signed_distance(P, beta), both
    negative inside, and `isosurface(S, iso=offset)` extracts the mesh, oriented outward. With 'signed_distance' a positive `offset`
    dilates the shape by that distance (choose `pad` * h above it, or the surface leaves the grid and comes back open) and a negative
    one erodes it; with 'winding' the offset moves the threshold 0.5 of the winding number. beta = math.inf sums the winding number exactly.

    The result is closed (the padding keeps the level set inside the grid) and free of crossings between triangles of distinct
    tets: each piece lies in its own tet of the grid. It is as fine as h, whatever the input's resolution, and features below h are
    lost. Its triangles include poorly shaped ones (slivers where the surface passes near a node): follow with `remesh_botsch`
    before compute_matrix. Not differentiable in V. numpy input gives numpy, tensors give tensors on their device.

    The level set has every closed sheet of the field: the outer skin, the inward-facing shells around enclosed voids, specks of a noisy
    winding field. largesteps.topology filters them on the device: keep_outer_components(V2, F2) drops every facet component whose
    signed volume is <= 0 (the shells around voids), keep_largest_component(V2, F2, by='volume') keeps the one of largest |volume|.

    ValueError when the grid would pass the int32 limits of the kernels; the message names the smallest h that fits."""
    h = _real(h, "h")
    offset = _real(offset, "offset")
    beta = _as_beta(beta)
    if not (math.isfinite(h) and h > 0):
        raise ValueError(f"remesh_level_set: h must be positive and finite, got {h}")
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or pad < 1:
        raise ValueError(f"remesh_level_set: pad must be an integer of at least 1, got {pad!r}")
    if field not in ("winding", "signed_distance"):
        raise ValueError(f"remesh_level_set: field must be 'winding' or 'signed_distance', got {field!r}")
    v, v_np = _as_points(V, "V")
    _as_faces(F)
    with MeshDistance(V, F) as mesh:
        vt = mesh.V
        lo, hi = vt.min(0).values.double().cpu().numpy(), vt.max(0).values.double().cpu().numpy()
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("remesh_level_set: V has a non-finite coordinate")
        origin, dims = _grid_over(lo, hi, h, pad)
        if not _fits(dims):
            a, b = h, h * 2.0
            while not _fits(_grid_over(lo, hi, b, pad)[1]):
                a, b = b, b * 2.0
            for _ in range(60):                                  # the grid shrinks as h grows: bisect for the smallest h that fits
                mid = 0.5 * (a + b)
                a, b = (a, mid) if _fits(_grid_over(lo, hi, mid, pad)[1]) else (mid, b)
            raise ValueError(f"remesh_level_set: a grid of {dims[0]} x {dims[1]} x {dims[2]} nodes passes the int32 limits of the kernels "
                             f"(8 x nodes and 12 x cubes below 2^31); the smallest h that fits is {b:.6g}")
        dev = mesh.device
        axes = [torch.arange(int(d), dtype=torch.float64, device=dev) * h + float(o) for d, o in zip(dims, origin)]
        P = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).to(torch.float32)
        with torch.no_grad():
            if field == "winding":
                S = 0.5 - mesh.winding_number(P, beta)
            else:
                S = mesh.signed_distance(P, beta)[0]
        S = S.to(torch.float32).reshape(tuple(int(d) for d in dims))
    # the nodes were placed in float64 and rounded; the extractor places them as origin + h * i in float32 (a rounding error of the
    # coordinates, far below h)
    V2, F2 = isosurface(S, iso=offset, origin=tuple(float(o) for o in origin), spacing=h)
    if v_np:
        return V2.cpu().numpy(), F2.cpu().numpy()
    return V2, F2
