"""
Rays against a mesh on the MI355X: closest hit, any hit, the gradient of the hit distance, and ambient occlusion on top of them.

    from largesteps.raycast import ray_mesh_intersect                      # instead of: igl.ray_mesh_intersect
    from largesteps.raycast import ambient_occlusion                       # igl.ambient_occlusion

`RayMesh(V, F)` is a `distance.MeshDistance`: one handle, one LBVH, answers "how far is this point" and "what does this ray hit", and
`update(V)` moves both. The kernels are csrc/raycast.hip.

The rule (tests/ray_statement.py restates it as a numpy brute force and the device returns the same bits) is
Woop, Benthin and Wald's watertight ray-triangle test evaluated in float64 from the float32 inputs. A direction need not be unit: t is
in units of |D|. A hit is accepted when tmin <= t <= tmax, both ends inclusive; the closest hit is the accepted face of smallest t and,
on equal t, of lowest id. Edges and vertices count as hits, and two faces that share an edge can never both reject a ray that passes
between them. A zero-area face is never hit; a direction with a non-finite component, or all zero, hits nothing. A ray that starts on
the surface with tmin = 0 returns that surface at t = 0 (the self-hit): start such rays a little off it, as `ambient_occlusion` does,
or pass a positive tmin. A miss is t = +inf, I = -1, W = 0.

Autograd. With tensor input, `intersect` returns a differentiable t (float64) when grad mode is on and O, D, or the tensor V the handle
was built from (or last updated with), requires grad. The face is held fixed: with n = (b - a) x (c - a) of the hit face and
q = n / (n . d), dt/dO = -q, dt/dD = -t q and dt/dV[F[I, k]] = W[k] q (first derivatives only; a miss contributes nothing). I and W carry
no gradient: a differentiable hit point is O + t[:, None] * D, not W-weighted corners. Gradients are float32 like their inputs, every
term formed in float64 and rounded once, the vertex gradient summed without float atomics in a fixed order: bitwise reproducible.
`occluded` and `ambient_occlusion` are not differentiable. The fences of `distance` apply: a backward after `update`, or after an
in-place change of the source V that no `update` followed, raises RuntimeError.

Stream capture: `intersect`, `occluded` and the gradients are capturable against a handle that is not updated inside the captured
body, after one eager warm-up pass (the first gradient to V builds the corner ranking, which synchronises). Construction, `update`,
`ray_mesh_intersect` (it builds and destroys a handle) and `ambient_occlusion` synchronise.

Input conventions are those of `distance`: numpy input runs on the current HIP device and returns numpy; tensors (O, D, V float32, F
int32 / int64, on one HIP device) return tensors on that device. CPU tensors raise.
"""
import math

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from .distance import MeshDistance, _as_faces, _as_points, _on


def _as_bound(x, what, n):
    """a scalar or (n,) bound of the ray parameter -> float, numpy (n,) float64 or tensor (n,); checked before any device work"""
    if isinstance(x, torch.Tensor):
        _native.require_device(x, what)
        if not x.dtype.is_floating_point:
            raise TypeError(f"{what} must hold real numbers, got {x.dtype}")
        if x.dim() == 0:
            return x.detach()
        if x.dim() != 1 or x.shape[0] != n:
            raise ValueError(f"{what} must be a scalar or ({n},), got {tuple(x.shape)}")
        return x.detach()
    if isinstance(x, (bool, np.bool_)):
        raise TypeError(f"{what} must be a real number, got {type(x).__name__}")
    if isinstance(x, (int, float, np.integer, np.floating)):
        return float(x)
    a = np.asarray(x)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise TypeError(f"{what} must hold real numbers, got {a.dtype}")
    if a.ndim == 0:
        return float(a)
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError(f"{what} must be a scalar or ({n},), got {a.shape}")
    return a.astype(np.float64)


def _as_rays(O, D, tmin, tmax):
    """(o, d, tmin, tmax, was_numpy): the type, dtype and shape checks of a ray set, before any device work"""
    o, o_np = _as_points(O, "O")
    d, d_np = _as_points(D, "D")
    if o_np != d_np:
        raise TypeError("O and D must both be numpy arrays or both be tensors")
    if o.shape[0] != d.shape[0]:
        raise ValueError(f"O and D must have one row per ray, got {o.shape[0]} and {d.shape[0]}")
    return o, d, _as_bound(tmin, "tmin", o.shape[0]), _as_bound(tmax, "tmax", o.shape[0]), o_np


def _trange(tmin, tmax, n, dev):
    """(n, 2) float64 on the device, or None for the default [0, +inf]"""
    if isinstance(tmin, float) and isinstance(tmax, float) and tmin == 0.0 and tmax == math.inf:
        return None
    tr = torch.empty((n, 2), dtype=torch.float64, device=dev)
    for k, x in enumerate((tmin, tmax)):
        tr[:, k] = x if isinstance(x, float) else _on(x if isinstance(x, torch.Tensor) else np.ascontiguousarray(x), dev).to(torch.float64)
    return tr


@_native.retry_on_oom
def _gradients(m, o, d, I, W, t, g, need_o, need_d, need_v):
    """(gO, gD, gV), each or None, of one backward pass: its allocations and the native call"""
    n = o.shape[0]
    g = g.to(torch.float64).contiguous()
    gO = torch.empty_like(o) if need_o else None
    gD = torch.empty_like(d) if need_d else None
    gV, vptr, order, ws = m._vertex_grad_buffers("ls_mesh_ray_backward_workspace_bytes", n, need_v)
    m._call("ls_mesh_ray_backward", _native.ptr(o), _native.ptr(d), n, _native.ptr(I), _native.ptr(W), _native.ptr(t), _native.ptr(g),
            _native.ptr(vptr), _native.ptr(order), _native.ptr(gO), _native.ptr(gD), _native.ptr(gV), _native.ptr(ws),
            ws.numel() if ws is not None else 0)
    return gO, gD, gV


class _Intersect(Function):
    """t, I, W of the rays (O, D) against the handle m; V is m's source tensor (or None): the positions the handle holds"""

    @staticmethod
    def forward(ctx, O, D, V, m, trange):
        o, d = O.detach().contiguous(), D.detach().contiguous()
        t, I, W = m._cast(o, d, trange)
        ctx.m, ctx.version = m, m._version
        if ctx.needs_input_grad[2]:
            m._corner_ranks()              # once per handle (synchronises): every later forward and backward finds it
        ctx.save_for_backward(o, d, t, I, W)
        ctx.mark_non_differentiable(I, W)
        return t, I, W

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gI, _gW):
        o, d, t, I, W = ctx.saved_tensors
        m = ctx.m
        m._check_backward(ctx.version, "ray mesh", "hits", "RayMesh")
        gO, gD, gV = _gradients(m, o, d, I, W, t, g, *ctx.needs_input_grad[:3])
        return gO, gD, gV, None, None


class RayMesh(MeshDistance):
    """The mesh (V, F) and its LBVH on a HIP device, for rays and for the distance queries of MeshDistance, from one handle. `update`,
    `close`, the `with` block and the fences against a moved mesh are MeshDistance's."""

    def _rays(self, O, D, tmin, tmax):
        o, d, tmin, tmax, was_np = _as_rays(O, D, tmin, tmax)
        if not self._h:
            raise RuntimeError("ray mesh: query of a closed handle")
        o, d = _on(o, self.device), _on(d, self.device)
        return o, d, _trange(tmin, tmax, o.shape[0], self.device), was_np

    def _cast(self, o, d, trange):
        n = o.shape[0]
        t = torch.empty(n, dtype=torch.float64, device=self.device)
        I = torch.empty(n, dtype=torch.int64, device=self.device)
        W = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        self._call("ls_mesh_ray_closest", _native.ptr(o), _native.ptr(d), n, _native.ptr(trange), _native.ptr(t), _native.ptr(I), _native.ptr(W))
        return t, I, W

    @_native.retry_on_oom
    def intersect(self, O, D, tmin=0.0, tmax=math.inf):
        """(t (n,) float64, I (n,) int64, W (n, 3) float64): for every ray O[i] + t D[i] its closest hit with tmin <= t <= tmax -- the
        parameter t, the face (the lowest id on equal t) and the barycentric weights of the hit on the face's corners; t = +inf,
        I = -1, W = 0 for a miss. tmin and tmax are scalars or (n,). An origin on the surface with tmin = 0 returns that surface at
        t = 0. numpy rays give numpy results, tensors give tensors. With tensors, grad mode on and O, D or the handle's source V
        requiring grad, t is differentiable with the face held fixed (module docstring); I and W carry no gradient: a differentiable
        hit point is O + t[:, None] * D."""
        tensors = isinstance(O, torch.Tensor) and isinstance(D, torch.Tensor)
        if tensors and torch.is_grad_enabled() and (O.requires_grad or D.requires_grad or (self._src is not None and self._src.requires_grad)):
            _, _, trange, _ = self._rays(O, D, tmin, tmax)            # the argument checks of the plain path
            self._check_source()
            return _Intersect.apply(O, D, self._src, self, trange)
        o, d, trange, was_np = self._rays(O, D, tmin, tmax)
        t, I, W = self._cast(o, d, trange)
        if was_np:
            return t.cpu().numpy(), I.cpu().numpy(), W.cpu().numpy()
        return t, I, W

    @_native.retry_on_oom
    def occluded(self, O, D, tmin=0.0, tmax=math.inf):
        """(n,) bool: whether the ray O[i] + t D[i] hits any face with tmin <= t <= tmax, which is I >= 0 of `intersect` over the same
        range, found by a walk that stops at the first accepted face. Not differentiable."""
        o, d, trange, was_np = self._rays(O, D, tmin, tmax)
        hit = torch.empty(o.shape[0], dtype=torch.bool, device=self.device)
        self._call("ls_mesh_ray_any", _native.ptr(o), _native.ptr(d), o.shape[0], _native.ptr(trange), _native.ptr(hit))
        return hit.cpu().numpy() if was_np else hit


@_native.retry_on_oom
def ray_mesh_intersect(O, D, V, F, tmin=0.0, tmax=math.inf):
    """The closest hit of every ray O[i] + t D[i] on the mesh (V, F) -> (t, I, W) as `RayMesh.intersect` returns them: libigl's
    ray_mesh_intersect for many rays at once (its first hit; igl's (u, v) are W[:, 1:]). t is differentiable in tensors O, D and V that
    require grad; its graph then keeps the handle, which is released with the graph instead of on return. The release synchronises the
    device, so let the graph go outside any stream capture; with a RayMesh of your own, `close()` decides the moment."""
    _as_rays(O, D, tmin, tmax)                                        # the ray checks, before the handle is built
    return RayMesh._for_call(V, F, lambda m: m.intersect(O, D, tmin, tmax))


@_native.retry_on_oom
def ambient_occlusion(V, F, P, N, n_rays, seed=0, eps=1e-4):
    """libigl's ambient_occlusion(V, F, P, N, num_samples): for every point P[i] with unit normal N[i] the fraction of n_rays rays that
    the mesh (V, F) blocks, (len(P),) float32, 0 for an unoccluded point and 1 for one that sees no sky. The directions are
    cosine-weighted around N[i] (Malley's method in a frame around the normal), drawn from a torch.Generator on the device seeded with
    `seed`: the same seed gives the same values. The origins are P + eps * diag * N, diag the diagonal of the mesh's box, so that a
    point on the surface does not hit its own face. numpy input gives numpy. Plain torch on top of `RayMesh.occluded`; it builds and
    releases a handle, so it synchronises and is not capturable. Not differentiable."""
    from .sampling import _uint
    if _uint(n_rays, "n_rays", 31) < 1:
        raise ValueError("ambient_occlusion: n_rays must be at least 1")
    _uint(seed, "seed", 63)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not math.isfinite(eps) or eps < 0:
        raise ValueError(f"ambient_occlusion: eps must be a finite non-negative number, got {eps!r}")
    p, p_np = _as_points(P, "P")
    nrm, n_np = _as_points(N, "N")
    if p_np != n_np:
        raise TypeError("P and N must both be numpy arrays or both be tensors")
    if p.shape[0] != nrm.shape[0]:
        raise ValueError(f"P and N must have one row per point, got {p.shape[0]} and {nrm.shape[0]}")
    _as_points(V, "V")
    _as_faces(F)
    with RayMesh(V, F) as m, torch.cuda.device(m.device), torch.no_grad():
        dev = m.device
        p, nrm = _on(p, dev), _on(nrm, dev)
        npts = p.shape[0]
        if npts == 0:
            out = torch.zeros(0, dtype=torch.float32, device=dev)
            return out.cpu().numpy() if p_np else out
        diag = (m.V.max(0).values.double() - m.V.min(0).values.double()).norm()
        origin = (p.double() + (eps * diag) * nrm.double()).float()
        # a frame (t1, t2, n) around every normal: t1 from the axis the normal is least aligned with
        axis = torch.nn.functional.one_hot(nrm.abs().argmin(1), 3).to(nrm.dtype)
        t1 = torch.nn.functional.normalize(torch.linalg.cross(nrm, axis), dim=1)
        t2 = torch.linalg.cross(nrm, t1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        u = torch.rand((npts, int(n_rays), 2), generator=gen, device=dev, dtype=torch.float32)
        r, phi = u[..., 0].sqrt(), (2.0 * math.pi) * u[..., 1]
        x, y, z = r * phi.cos(), r * phi.sin(), (1.0 - u[..., 0]).clamp_min(0.0).sqrt()
        d = x[..., None] * t1[:, None, :] + y[..., None] * t2[:, None, :] + z[..., None] * nrm[:, None, :]
        hit = m.occluded(origin[:, None, :].expand(-1, int(n_rays), -1).reshape(-1, 3), d.reshape(-1, 3))
        out = hit.view(npts, int(n_rays)).float().mean(1)
        return out.cpu().numpy() if p_np else out
