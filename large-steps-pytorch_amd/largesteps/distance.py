"""
Point-to-mesh distance and libigl's Hausdorff distance on the MI355X: the error column of the reference's figures.

figures/comparison/generate_data.py scores every 10th recorded step as ``hausdorff(verts[it], fa, vb, fb) + hausdorff(vb, fb, verts[it],
fa)`` with libigl's CPU implementation; the `influence` and `viewpoints` notebooks make the same call. Here it runs on the device
(csrc/distance.hip, over the LBVH that the remesher's projection uses):

    from largesteps.distance import hausdorff                              # instead of: from igl import hausdorff
    from largesteps.distance import point_mesh_squared_distance            # igl.point_mesh_squared_distance

The arithmetic is fp64 from fp32 coordinates; ties of the squared distance go to the lowest face id; a degenerate face (its area term
|ab x ac|^2 is not positive) is measured as its closest edge segment. DESIGN.md section 2.8 states the rules, tests/distance_statement.py
restates them as a brute force, and the device answers with the same bits. Results are bitwise reproducible. No autograd.

Input conventions follow remesh_botsch: numpy input (V float64 or float32, converted to fp32; F integer) runs on the current HIP device
and returns numpy; tensor input (V and query points fp32, F int32 / int64, all on one HIP device) returns tensors on that device. CPU
tensors raise.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native


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


class MeshDistance:
    """The LBVH of one fixed mesh (V, F) on a HIP device, for distance queries from any number of point sets: the figure's target mesh,
    built once and queried at every recorded step. numpy (V, F) go to the current HIP device; tensors stay on theirs."""

    def __init__(self, V, F):
        v, v_np = _as_points(V, "V")
        f = _as_faces(F)
        if f.shape[0] == 0:
            raise ValueError("mesh distance: the mesh has no faces")
        if v.shape[0] == 0:
            raise ValueError("mesh distance: the mesh has no vertices")
        self.device = _current_device() if v_np else v.device
        self.V = _on(v, self.device)
        f = _on(f, self.device)
        self._h = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().ls_mesh_distance_create(_native.ptr(self.V), self.V.shape[0], _native.ptr(f), f.element_size(), f.shape[0],
                                                                self.device.index, _native.stream_of(self.device), ctypes.byref(self._h)))

    def _points(self, P):
        p, p_np = _as_points(P, "P")
        return _on(p, self.device), p_np

    def squared_distance(self, P):
        """(sqrD (n,) float64, I (n,) int64, C (n, 3) float64): for every row of P its squared distance to the mesh, the id of the
        nearest face (the lowest on a tie) and the closest point on it. numpy P gives numpy results, a tensor gives tensors."""
        p, p_np = self._points(P)
        n = p.shape[0]
        sqrD = torch.empty(n, dtype=torch.float64, device=self.device)
        I = torch.empty(n, dtype=torch.int64, device=self.device)
        C = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().ls_mesh_distance_query(self._h, _native.ptr(p), n, _native.ptr(sqrD), _native.ptr(I), _native.ptr(C),
                                                               _native.stream_of(self.device)))
        if p_np:
            return sqrD.cpu().numpy(), I.cpu().numpy(), C.cpu().numpy()
        return sqrD, I, C

    def max_squared_distance(self, P):
        """max over the rows of P of their squared distance to the mesh (0 for no rows): a float for numpy P, a 0-dim float64 tensor on
        the device for a tensor (no synchronisation)."""
        p, p_np = self._points(P)
        out = torch.empty((), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().ls_mesh_distance_max(self._h, _native.ptr(p), p.shape[0], _native.ptr(out), _native.stream_of(self.device)))
        return float(out) if p_np else out

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
    give tensors on their device."""
    with MeshDistance(V, F) as m:
        return m.squared_distance(P)


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
