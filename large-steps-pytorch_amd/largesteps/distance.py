"""
Point-to-mesh distance and libigl's Hausdorff distance on the MI355X: the error column of the reference's figures.

figures/comparison/generate_data.py scores every 10th recorded step as ``hausdorff(verts[it], fa, vb, fb) + hausdorff(vb, fb, verts[it],
fa)`` with libigl's CPU implementation; the `influence` and `viewpoints` notebooks make the same call. Here it runs on the device
(csrc/distance.hip, over the LBVH that the remesher's projection uses):

    from largesteps.distance import hausdorff                              # instead of: from igl import hausdorff
    from largesteps.distance import point_mesh_squared_distance            # igl.point_mesh_squared_distance

The arithmetic is fp64 from fp32 coordinates; ties of the squared distance go to the lowest face id; a degenerate face (its area term
|ab x ac|^2 is not positive) is measured as its closest edge segment. DESIGN.md section 2.8 states the rules, tests/distance_statement.py
restates them as a brute force, and the device answers with the same bits. Results are bitwise reproducible.

Autograd. With tensor input, `MeshDistance.squared_distance(P)` and `point_mesh_squared_distance(P, V, F)` return a differentiable
sqrD (float64) when grad mode is on and P, or the tensor V the handle was built from (or last updated with), requires grad; I and C
are marked non-differentiable. The closest point is C = sum_k w_k V[F[I, k]] with the weights w of the same region tests; C minimises
over the face, so with d = p - C the gradient of sqrD is 2 d to p and -2 w_k d to corner k (first derivatives only). Where the
distance is not differentiable -- a point equidistant from several faces, a point on a vertex or an edge -- this is the gradient of
the face the tie rule chose: the chosen subgradient. Gradients are float32 like their inputs, every term formed in float64 and rounded
once, summed per vertex without float atomics in a fixed order (csrc/distance.hip): bitwise reproducible. `max_squared_distance` and
`hausdorff` stay non-differentiable; numpy input, or input that requires no grad, takes exactly the non-differentiable path.

A handle holds a copy of the positions. `MeshDistance.update(V)` moves the mesh (same faces, same vertex count) in place of destroying
and rebuilding the handle; a backward whose forward ran before an `update`, or after an in-place change of the source V that no
`update` followed, raises RuntimeError, because the handle no longer holds the positions of that forward.

Stream capture (torch.cuda.graph): queries and both gradients against a handle that is not updated inside the captured body are
capturable, after one eager warm-up pass (the first gradient to V builds the corner ranking of the faces, which synchronises).
Construction, `update` and `point_mesh_squared_distance` itself (it builds and destroys a handle) synchronise and are not. A
differentiable result of `point_mesh_squared_distance` keeps its handle until its graph is freed, and releasing a handle synchronises
the device: let that graph go (drop the result and the tensors computed from it) outside any capture. A `MeshDistance` of your
own is released by `close()` or its `with` block, when you choose.

Inside or outside. `MeshDistance.winding_number(P, beta)` is the generalized winding number (Jacobson et al. 2013) by the tree walk of
Barill et al. 2018 over the same LBVH (csrc/winding.hip), `signed_distance` the distance with its sign
(negative inside): igl.fast_winding_number, igl.winding_number (beta = math.inf) and igl.signed_distance. Unlike ray parity or a
pseudonormal sign it degrades gracefully on self-intersecting, folded and open meshes. The handle prepares the walk's node moments on
the first winding query after construction or `update`; a handle that never asks pays nothing. Prepared, both queries are capturable.

Does the mesh cut through itself? `MeshDistance.self_intersections()` lists the pairs of faces that do, `self_intersecting_faces()` marks
their faces and `count_self_intersections()` counts the pairs without synchronising (a per-step metric): igl.fast_find_self_intersections
(csrc/selfx.hip; tests/selfx_statement.py restates the rule). A pair of faces that share no vertex index is
reported iff an edge of one crosses the other, by the watertight segment test of the ray queries in fp64; a pair that shares one index
iff the edge opposite the shared corner of one crosses the other; a pair that shares two or three never. And a pair is reported only if
the corner boxes of its two faces come within 2 e of each other on every axis, e = 2^-40 x the largest |coordinate| of V: a real crossing
always does, and the clause leaves out what the segment test accepts on rounding alone between far-apart faces of an exactly flat
sheet. Consequences:
  * coplanar overlaps are not reported, a sheet folded flat onto itself included: a segment in a face's plane has det == 0. That is
    exact where the arithmetic is (a plane along the axes, coordinates on a grid); in a tilted plane whose shear rounds, det is a
    rounding error and coplanar faces with near boxes can be reported on it, the same ones on every run and in any face order;
  * two faces that touch at a point or along a segment ARE reported when they share no index: run the query on the de-duplicated mesh
    (largesteps.meshops.remove_duplicates, the reference's function of that name);
  * an edge that passes exactly through the common edge of two faces is reported against at least one of them.
The result depends on the mesh alone and is bitwise reproducible; none of the three is differentiable.

Input conventions follow remesh_botsch: numpy input (V float64 or float32, converted to fp32; F integer) runs on the current HIP device
and returns numpy; tensor input (V and query points fp32, F int32 / int64, all on one HIP device) returns tensors on that device. CPU
tensors raise.
"""
import ctypes
import math

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from .normals import _plan


def _as_points(P, what):
    """(tensor (n, 3) fp32 on a HIP device, was_numpy)"""
    if isinstance(P, torch.Tensor):
        _native.require_device(P, what)
        if P.dtype != torch.float32:
            raise TypeError(f"{what} must be float32, got {P.dtype}")
        if P.dim() != 2 or P.shape[1] != 3:
            raise ValueError(f"{what} must be (n, 3), got {tuple(P.shape)}")
        return P.detach().contiguous(), False
    Pn = np.asarray(P)
    if Pn.ndim != 2 or Pn.shape[1] != 3:
        raise ValueError(f"{what} must be (n, 3), got {Pn.shape}")
    if not (np.issubdtype(Pn.dtype, np.floating) or np.issubdtype(Pn.dtype, np.integer)):
        raise TypeError(f"{what} must hold real numbers, got {Pn.dtype}")
    return np.ascontiguousarray(Pn, dtype=np.float32), True


def _as_faces(F):
    if isinstance(F, torch.Tensor):
        _native.require_device(F, "F")
        if F.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"F must be int32 or int64, got {F.dtype}")
        if F.dim() != 2 or F.shape[1] != 3:
            raise ValueError(f"F must be (m, 3), got {tuple(F.shape)}")
        return F.contiguous()
    Fn = np.asarray(F)
    if Fn.ndim != 2 or Fn.shape[1] != 3:
        raise ValueError(f"F must be (m, 3), got {Fn.shape}")
    if not np.issubdtype(Fn.dtype, np.integer):
        raise TypeError(f"F must hold integers, got {Fn.dtype}")
    return np.ascontiguousarray(Fn, dtype=np.int64 if Fn.dtype.itemsize > 4 else np.int32)


def _current_device():
    if not torch.cuda.is_available():
        raise RuntimeError("largesteps (MI355X build): the mesh distance needs a HIP device; there is no CPU path in this package.")
    return torch.device("cuda", torch.cuda.current_device())


def _on(x, device):
    """a numpy array moved to `device`, or a tensor checked to be there"""
    if isinstance(x, torch.Tensor):
        if x.device != device:
            raise RuntimeError(f"all tensors must be on one device: got {x.device} and {device}")
        return x
    return torch.from_numpy(x).to(device)


@_native.retry_on_oom
def _gradients(m, p, I, C, g, need_p, need_v):
    """(gP or None, gV or None) of one backward pass: its allocations and the native call"""
    n = p.shape[0]
    g = g.to(torch.float64).contiguous()
    gP = torch.empty_like(p) if need_p else None
    gV, vptr, order, ws = m._vertex_grad_buffers("ls_mesh_distance_backward_workspace_bytes", n, need_v)
    m._call("ls_mesh_distance_backward", _native.ptr(p), n, _native.ptr(I), _native.ptr(C), _native.ptr(g), _native.ptr(vptr), _native.ptr(order),
            _native.ptr(gP), _native.ptr(gV), _native.ptr(ws), ws.numel() if ws is not None else 0)
    return gP, gV


class _SquaredDistance(Function):
    """sqrD, I, C of the points P against the handle m; V is m's source tensor (or None): the positions the handle holds"""

    @staticmethod
    def forward(ctx, P, V, m):
        p = P.detach().contiguous()
        sqrD, I, C = m._query(p)
        ctx.m, ctx.version = m, m._version
        if ctx.needs_input_grad[1]:
            m._corner_ranks()              # once per handle (synchronises): every later forward and backward finds it
        ctx.save_for_backward(p, I, C)
        ctx.mark_non_differentiable(I, C)
        return sqrD, I, C

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gI, _gC):
        p, I, C = ctx.saved_tensors
        m = ctx.m
        m._check_backward(ctx.version, "mesh distance", "distances", "MeshDistance")
        gP, gV = _gradients(m, p, I, C, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gP, gV, None


def _as_beta(beta):
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)):
        raise TypeError(f"beta must be a real number, got {type(beta).__name__}")
    beta = float(beta)
    if not beta >= 1.0:
        raise ValueError(f"winding number: beta must be at least 1, got {beta}")
    return beta


class _SignedRoot(Function):
    """S = s sqrt(sqrD), computed by the caller, with dS = coef dsqrD (coef = s / (2 sqrt(sqrD)), 0 where sqrD == 0)"""

    @staticmethod
    def forward(ctx, sqrD, S, coef):
        ctx.save_for_backward(coef)
        return S.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        coef, = ctx.saved_tensors
        return g * coef, None, None


class MeshDistance:
    """The LBVH of one mesh (V, F) on a HIP device, for distance queries from any number of point sets: the figure's target mesh,
    built once and queried at every recorded step, or a moving mesh whose positions `update` replaces at every step. numpy (V, F) go
    to the current HIP device; tensors stay on theirs. Built from a tensor V, the handle remembers it: a query is differentiable in
    it (module docstring)."""

    def __init__(self, V, F):
        v, v_np = _as_points(V, "V")
        f = _as_faces(F)
        if f.shape[0] == 0:
            raise ValueError("mesh distance: the mesh has no faces")
        if v.shape[0] == 0:
            raise ValueError("mesh distance: the mesh has no vertices")
        self.device = _current_device() if v_np else v.device
        self._numpy = v_np                 # the queries that take no points return numpy for a handle built from numpy; update keeps it
        self.V = _on(v, self.device)
        f = _on(f, self.device)
        self._f = f
        self._ranks = None
        self._version = 0                  # bumped by update: a backward pass belongs to the positions of its forward pass
        self._wn, self._wn_version = None, -1      # the winding walk's moments and the version they were prepared for
        self._remember(V)
        self._h = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().ls_mesh_distance_create(_native.ptr(self.V), self.V.shape[0], _native.ptr(f), f.element_size(), f.shape[0],
                                                                self.device.index, _native.stream_of(self.device), ctypes.byref(self._h)))

    def _remember(self, V):
        """the tensor the positions came from, and its version: what a gradient to V flows into"""
        self._src = V if isinstance(V, torch.Tensor) else None
        self._src_version = V._version if self._src is not None else 0

    def _check_source(self):
        if self._src is not None and self._src._version != self._src_version:
            raise RuntimeError("mesh distance: the tensor V this handle was built from was changed in place; the handle still holds the "
                               "old positions. Call MeshDistance.update(V) after changing V")

    def _check_backward(self, version, what, results, cls):
        """the fences of a backward pass whose forward pass saw this handle at `version`: the handle still open, not updated since, its
        source tensor not changed in place. `what`, `results` and `cls` are the words of the caller's messages"""
        if not self._h:
            raise RuntimeError(f"{what}: the handle of this forward pass was closed before its backward pass")
        if self._version != version:
            raise RuntimeError(f"{what}: the handle was updated after this forward pass; it no longer holds the positions the "
                               f"{results} were computed from. Run the backward pass before {cls}.update")
        self._check_source()

    def _call(self, name, *args):
        """the native function `name`(handle, *args, stream) on the handle's device and its current stream; raises what its status means"""
        with torch.cuda.device(self.device):
            _native.check(getattr(_native.lib(), name)(self._h, *args, _native.stream_of(self.device)))

    @classmethod
    def _for_call(cls, V, F, query):
        """query(m) for a handle m built for this one call. The handle is closed on return unless the first result is a tensor that
        requires grad: its graph then keeps the handle, which is released with the graph"""
        m = cls(V, F)
        out = None
        try:
            out = query(m)
            return out
        finally:
            if not (out is not None and isinstance(out[0], torch.Tensor) and out[0].requires_grad):
                m.close()

    def _vertex_grad_buffers(self, size_fn_name, n, need_v):
        """(gV, vptr, order, ws) of a backward pass over n items: the gradient to V, the corner ranking and the native workspace, or
        four None when V needs no gradient"""
        if not need_v:
            return None, None, None, None
        gV = torch.empty_like(self.V)
        vptr, order = self._corner_ranks()
        return gV, vptr, order, _native.workspace(size_fn_name, (n, self._f.shape[0]), self.device)

    def _corner_ranks(self):
        """(vptr, rank -> corner) of the faces, the summation order of the gradient to V (largesteps.normals._plan)"""
        if self._ranks is None:
            vptr, _, _, order = _plan(self._f, self.V.shape[0])
            self._ranks = (vptr, order)
        return self._ranks

    @_native.retry_on_oom
    def update(self, V):
        """New positions V (the same vertex count; the faces stay) in place of destroying and rebuilding the handle: afterwards it
        answers exactly as MeshDistance(V, F) would, and V is the tensor its gradient flows into. Synchronises the stream."""
        v, v_np = _as_points(V, "V")
        if v.shape[0] != self.V.shape[0]:
            raise ValueError(f"mesh distance: update needs the handle's {self.V.shape[0]} vertices, got {v.shape[0]}")
        if not self._h:
            raise RuntimeError("mesh distance: update of a closed handle")
        v = _on(v, self.device)
        self._call("ls_mesh_distance_update", _native.ptr(v))
        self.V = v
        self._version += 1
        self._remember(V)

    def _points(self, P):
        p, p_np = _as_points(P, "P")
        return _on(p, self.device), p_np

    @_native.retry_on_oom
    def squared_distance(self, P):
        """(sqrD (n,) float64, I (n,) int64, C (n, 3) float64): for every row of P its squared distance to the mesh, the id of the
        nearest face (the lowest on a tie) and the closest point on it. numpy P gives numpy results, a tensor gives tensors. With a
        tensor P, grad mode on and P or the handle's source V requiring grad, sqrD is differentiable (module docstring)."""
        if isinstance(P, torch.Tensor) and torch.is_grad_enabled() and (P.requires_grad or (self._src is not None and self._src.requires_grad)):
            _on(_as_points(P, "P")[0], self.device)            # the argument checks of the plain path
            self._check_source()
            return _SquaredDistance.apply(P, self._src, self)
        p, p_np = self._points(P)
        sqrD, I, C = self._query(p)
        if p_np:
            return sqrD.cpu().numpy(), I.cpu().numpy(), C.cpu().numpy()
        return sqrD, I, C

    def _query(self, p):
        n = p.shape[0]
        sqrD = torch.empty(n, dtype=torch.float64, device=self.device)
        I = torch.empty(n, dtype=torch.int64, device=self.device)
        C = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        self._call("ls_mesh_distance_query", _native.ptr(p), n, _native.ptr(sqrD), _native.ptr(I), _native.ptr(C))
        return sqrD, I, C

    def max_squared_distance(self, P):
        """max over the rows of P of their squared distance to the mesh (0 for no rows): a float for numpy P, a 0-dim float64 tensor on
        the device for a tensor (no synchronisation)."""
        p, p_np = self._points(P)
        out = torch.empty((), dtype=torch.float64, device=self.device)
        self._call("ls_mesh_distance_max", _native.ptr(p), p.shape[0], _native.ptr(out))
        return float(out) if p_np else out

    def _moments(self):
        """the moment buffer of the winding walk, prepared on the first winding query after construction or `update`"""
        if self._wn_version != self._version:
            if self._wn is None:
                self._wn = _native.workspace("ls_mesh_winding_bytes", (self._f.shape[0],), self.device)
            self._call("ls_mesh_winding_prepare", _native.ptr(self._wn))
            self._wn_version = self._version
        return self._wn

    def _winding(self, p, beta):
        if not self._h:
            raise RuntimeError("mesh distance: query of a closed handle")
        w = torch.empty(p.shape[0], dtype=torch.float64, device=self.device)
        mom = None if beta == math.inf else self._moments()
        self._call("ls_mesh_winding_query", _native.ptr(mom), _native.ptr(p), p.shape[0], beta, _native.ptr(w))
        return w

    @_native.retry_on_oom
    def winding_number(self, P, beta=2.0):
        """w (n,) float64: the generalized winding number of the mesh around every row of P (libigl's fast_winding_number): 1 inside a
        closed, outward-oriented mesh, 0 outside, -1 for the flipped orientation, k inside k nested copies, a fraction near an open
        boundary; NaN for a row with a non-finite component. `beta` >= 1 is the accuracy of the tree walk: a node of the handle's LBVH
        farther than beta times its radius answers with a three-term expansion of its faces (DESIGN.md section 2.11 has measured
        errors; the default 2.0 is libigl's). beta = math.inf sums every face exactly (libigl's winding_number). A query lying in
        the plane of a face, on an edge or on a vertex takes 0 from that face. Bitwise reproducible; not differentiable."""
        beta = _as_beta(beta)
        p, p_np = self._points(P)
        w = self._winding(p, beta)
        return w.cpu().numpy() if p_np else w

    @_native.retry_on_oom
    def signed_distance(self, P, beta=2.0):
        """(S (n,) float64, I (n,) int64, C (n, 3) float64): libigl's signed_distance with the winding-number sign. I and C are those of
        `squared_distance`; S = s sqrt(sqrD) with s = -1 where winding_number(P, beta) >= 0.5 (inside: negative, libigl's convention)
        and +1 elsewhere; S is NaN where the winding number is. libigl scales the distance by 1 - 2 w instead; here |S| is the distance.
        S is differentiable in P and in the handle's source V exactly as sqrD is, dS = s / (2 sqrt(sqrD)) dsqrD, and zero where
        sqrD == 0; the winding number and the sign carry no gradient."""
        beta = _as_beta(beta)
        sqrD, I, C = self.squared_distance(P)
        if isinstance(sqrD, torch.Tensor):
            with torch.no_grad():
                w = self._winding(_on(_as_points(P, "P")[0], self.device), beta)
                d = torch.sqrt(sqrD.detach())
                s = torch.where(w >= 0.5, -1.0, 1.0).to(torch.float64)
                S = torch.where(torch.isnan(w), w, s * d)
            if sqrD.requires_grad:
                coef = torch.where(d > 0, s / (2.0 * d), torch.zeros_like(d))
                S = _SignedRoot.apply(sqrD, S, coef)
            return S, I, C
        w = self.winding_number(P, beta)
        S = np.where(w >= 0.5, -1.0, 1.0) * np.sqrt(sqrD)
        return np.where(np.isnan(w), w, S), I, C

    def _selfx_count(self, with_flags):
        """(counts (F,) int32, total 0-dim int64, flags (F,) uint8 or None) of the count pass; no synchronisation"""
        if not self._h:
            raise RuntimeError("mesh distance: query of a closed handle")
        F = self._f.shape[0]
        counts = torch.empty(F, dtype=torch.int32, device=self.device)
        total = torch.empty((), dtype=torch.int64, device=self.device)
        flags = torch.empty(F, dtype=torch.uint8, device=self.device) if with_flags else None
        self._call("ls_mesh_selfx_count", _native.ptr(counts), _native.ptr(total), _native.ptr(flags))
        return counts, total, flags

    @_native.retry_on_oom
    def count_self_intersections(self):
        """The number of pairs of faces that cut through each other (module docstring; `self_intersections` lists them): a 0-dim int64
        tensor on the handle's device, an int for a handle built from numpy. With a tensor handle it does not synchronise and, after
        one eager warm-up call, can be captured in a torch.cuda.graph: a metric to read at every step. Not differentiable."""
        total = self._selfx_count(False)[1]
        return int(total) if self._numpy else total

    @_native.retry_on_oom
    def self_intersecting_faces(self):
        """(F,) bool: True for every face in some pair of `self_intersections` -- the `intersect` vector of libigl's
        fast_find_self_intersections. A tensor on the handle's device (no synchronisation), numpy for a handle built from numpy.
        Not differentiable."""
        flags = self._selfx_count(True)[2].to(torch.bool)
        return flags.cpu().numpy() if self._numpy else flags

    @_native.retry_on_oom
    def self_intersections(self):
        """IF (k, 2) int64: the pairs of faces (f, g), f < g, that cut through each other, sorted lexicographically; (0, 2) when there
        are none. The rule and what follows from it (coplanar overlaps are not reported, touching faces without a common index are)
        is in the module docstring. One count pass, one host read of k (synchronises), one fill pass. A tensor on the handle's device,
        numpy for a handle built from numpy (`update` with either kind of V does not change that). Bitwise reproducible;
        not differentiable."""
        counts, total, _ = self._selfx_count(False)
        k = int(total)
        pairs = torch.empty((k, 2), dtype=torch.int64, device=self.device)
        if k:
            ws = _native.workspace("ls_mesh_selfx_workspace_bytes", (self._f.shape[0], k), self.device)
            self._call("ls_mesh_selfx_pairs", _native.ptr(counts), k, _native.ptr(pairs), _native.ptr(ws), ws.numel())
        return pairs.cpu().numpy() if self._numpy else pairs

    def hausdorff(self, VA, FA):
        """hausdorff(VA, FA, V, F) of this mesh (V, F): only the other mesh's LBVH is built."""
        if (VA.shape[0] if isinstance(VA, torch.Tensor) else np.asarray(VA).shape[0]) == 0:
            raise ValueError("hausdorff: VA has no vertices")
        with torch.cuda.device(self.device), MeshDistance(VA, FA) as other:
            if other.device != self.device:
                raise RuntimeError(f"the meshes must be on one device: got {other.device} and {self.device}")
            ab = self.max_squared_distance(other.V)
            ba = other.max_squared_distance(self.V)
            return math.sqrt(float(torch.maximum(ab, ba)))

    def close(self):
        if self._h:
            _native.lib().ls_mesh_distance_destroy(self._h)
            self._h = ctypes.c_void_p(0)
            self._wn, self._wn_version = None, -1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@_native.retry_on_oom
def point_mesh_squared_distance(P, V, F):
    """libigl's point_mesh_squared_distance(P, V, F) -> (sqrD, I, C): for every row of P the squared distance to the mesh (V, F), the id
    of the nearest face (the lowest on a tie) and the closest point. sqrD and C are float64, I int64; numpy input gives numpy, tensors
    give tensors on their device. sqrD is differentiable in tensors P and V that require grad (module docstring); its graph then keeps
    the handle, which is released with the graph instead of on return. The release synchronises the device, so let the graph go (drop sqrD
    and the tensors computed from it) outside any stream capture; with a MeshDistance of your own, `close()` decides the moment."""
    return MeshDistance._for_call(V, F, lambda m: m.squared_distance(P))


@_native.retry_on_oom
def winding_number(V, F, P, beta=2.0):
    """libigl's fast_winding_number(V, F, P) (and winding_number with beta = math.inf) -> w (n,) float64: MeshDistance.winding_number of
    a handle built for this call. numpy input gives numpy, tensors give a tensor on their device."""
    _as_beta(beta)
    for name, X in (("V", V), ("P", P)):                # the type, dtype and shape checks, before any device work
        _as_points(X, name)
    _as_faces(F)
    with MeshDistance(V, F) as m:
        return m.winding_number(P, beta)


@_native.retry_on_oom
def signed_distance(P, V, F, beta=2.0):
    """libigl's signed_distance(P, V, F) with the winding-number sign -> (S, I, C): MeshDistance.signed_distance of a handle built for
    this call; negative inside. S is differentiable in tensors P and V that require grad; its graph then keeps the handle, as
    point_mesh_squared_distance's does."""
    _as_beta(beta)
    for name, X in (("P", P), ("V", V)):
        _as_points(X, name)
    _as_faces(F)
    return MeshDistance._for_call(V, F, lambda m: m.signed_distance(P, beta))


def _mesh_checks(V, F):
    """the type, dtype and shape checks of a mesh, before any device work"""
    _as_points(V, "V")
    _as_faces(F)


@_native.retry_on_oom
def self_intersections(V, F):
    """IF (k, 2) int64, the pairs of faces of the mesh (V, F) that cut through each other: MeshDistance.self_intersections of a handle
    built for this call. numpy input gives numpy, tensors give a tensor on their device. Not differentiable."""
    _mesh_checks(V, F)
    return MeshDistance._for_call(V, F, lambda m: (m.self_intersections(),))[0]


@_native.retry_on_oom
def count_self_intersections(V, F):
    """The number of pairs of `self_intersections(V, F)` without listing them: MeshDistance.count_self_intersections of a handle built
    for this call (building it synchronises; keep a handle and `update` it for a per-step metric). An int for numpy input, a 0-dim
    int64 tensor for tensors. Not differentiable."""
    _mesh_checks(V, F)
    return MeshDistance._for_call(V, F, lambda m: (m.count_self_intersections(),))[0]


@_native.retry_on_oom
def fast_find_self_intersections(V, F):
    """libigl's fast_find_self_intersections(V, F) -> (found, intersect): found is a bool, True iff some pair of faces cut through each
    other, and intersect (F,) bool marks every face of such a pair (numpy for numpy input, a tensor on their device for tensors).
    Synchronises (found comes to the host). Not differentiable."""
    _mesh_checks(V, F)
    intersect = MeshDistance._for_call(V, F, lambda m: (m.self_intersecting_faces(),))[0]
    return bool(intersect.any()), intersect


@_native.retry_on_oom
def chamfer_distance(VA, FA, VB, FB, n, seed=0):
    """mean_a d^2(a, B) + mean_b d^2(b, A) over n area-weighted surface samples a of mesh A (largesteps.sampling.sample_surface with
    `seed`, stream 0) and n samples b of mesh B (stream 1): a mesh-to-mesh measure that does not depend on where the vertices lie. A
    0-dim float64 tensor on the meshes' device for tensor input, a float for numpy; NaN when a mesh has no face of positive area.
    Bitwise reproducible.

    With tensor input it is differentiable in VA and VB, each through both paths: through its own samples (their gradient to the
    corners of the drawn faces) and through the faces closest to the other mesh's samples (module docstring). The face choice of the
    sampler carries no gradient.

    It builds two MeshDistance handles and releases them, so like point_mesh_squared_distance it synchronises and is not capturable;
    a differentiable result keeps the handles until its graph is freed. In a loop keep the handles instead:

        a, b = MeshDistance(VA, FA), MeshDistance(VB, FB)            # once
        for it in range(steps):
            a.update(VA)                                            # the mesh that moves
            PA, _, _ = sample_surface(VA, FA, n, seed=it, stream=0)
            PB, _, _ = sample_surface(VB, FB, n, seed=it, stream=1)
            loss = b.squared_distance(PA)[0].mean() + a.squared_distance(PB)[0].mean()
    """
    from .sampling import _uint, sample_surface
    if _uint(n, "n", 63) < 1:
        raise ValueError("chamfer_distance: n must be at least 1")
    _uint(seed, "seed", 64)
    for name, X in (("VA", VA), ("FA", FA), ("VB", VB), ("FB", FB)):        # the type, dtype and shape checks, before any device work
        (_as_faces(X) if name[0] == "F" else _as_points(X, name))
    a = MeshDistance(VA, FA)
    b = out = None
    try:
        b = MeshDistance(VB, FB)
        if a.device != b.device:
            raise RuntimeError(f"the meshes must be on one device: got {a.device} and {b.device}")
        with torch.cuda.device(a.device):
            # numpy positions: the handles' device copies, so that either kind of input takes one path to one value
            PA, _, _ = sample_surface(VA if isinstance(VA, torch.Tensor) else a.V, a._f, n, seed=seed, stream=0)
            PB, _, _ = sample_surface(VB if isinstance(VB, torch.Tensor) else b.V, b._f, n, seed=seed, stream=1)
            out = b.squared_distance(PA)[0].mean() + a.squared_distance(PB)[0].mean()
        if not (isinstance(VA, torch.Tensor) or isinstance(VB, torch.Tensor)):
            out = float(out)
        return out
    finally:
        if not (isinstance(out, torch.Tensor) and out.requires_grad):
            a.close()
            if b is not None:
                b.close()


@_native.retry_on_oom
def hausdorff(VA, FA, VB, FB):
    """libigl's hausdorff(VA, FA, VB, FB): sqrt(max(max_a d^2(a, B), max_b d^2(b, A))) over every row of VA and VB as query points, a
    Python float. As in libigl this is vertex-to-surface (its documented known issue): a surface point that is not a vertex is not
    a query, so the value can be below the surfaces' true Hausdorff distance."""
    for name, X in (("VA", VA), ("VB", VB)):
        if (X.shape[0] if isinstance(X, torch.Tensor) else np.asarray(X).shape[0]) == 0:
            raise ValueError(f"hausdorff: {name} has no vertices")
    with MeshDistance(VB, FB) as b:
        return b.hausdorff(VA, FA)
