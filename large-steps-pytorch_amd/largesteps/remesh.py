"""
Botsch-Kobbelt isotropic remeshing on the MI355X: the remesh step of the reference's optimisation loop.

scripts/main.py:137-169 calls ``remesh_botsch(v, f, 5, h, True)`` from ``pyremesh`` (an external C++ / libigl CPU build) on
``.cpu().numpy()`` copies, with ``h = 0.5 * average_edge_length``. Here the same call runs on the device (csrc/remesh.hip):

    from largesteps.remesh import remesh_botsch      # instead of: from pyremesh import remesh_botsch

One iteration is split -> collapse -> flip -> relax -> project ("Isotropic remeshing"; tests/remesh_statement.py states
every rule). Boundary edges and vertices are locked. The output is bitwise reproducible.
"""
import ctypes

import numpy as np
import torch

from . import _native

PHASES = {"split": 0, "collapse": 1, "flip": 2, "relax": 3, "project": 4}


class RemeshHandle:
    """A mesh being remeshed on one device (the C handle of ls_remesh_create). Faces come back in `index_dtype`."""

    def __init__(self, V, F, h, project=True):
        _native.require_device(V, "V")
        _native.require_device(F, "F")
        if V.dtype != torch.float32:
            raise TypeError(f"V must be float32, got {V.dtype}")
        if F.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"F must be int32 or int64, got {F.dtype}")
        if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
            raise ValueError(f"V must be (n, 3) and F (m, 3), got {tuple(V.shape)} and {tuple(F.shape)}")
        if F.device != V.device:
            raise RuntimeError(f"V ({V.device}) and F ({F.device}) must be on the same device")
        if V.shape[0] == 0 or F.shape[0] == 0:
            raise ValueError("remesh_botsch: the mesh has no faces")
        self.device, self.index_dtype = V.device, F.dtype
        v, f = V.detach().contiguous(), F.contiguous()
        self._h = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().ls_remesh_create(_native.ptr(v), v.shape[0], _native.ptr(f), f.element_size(), f.shape[0], float(h),
                                                         int(bool(project)), self.device.index, _native.stream_of(self.device),
                                                         ctypes.byref(self._h)))

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            _native.check(getattr(_native.lib(), name)(self._h, *args))

    def run(self, iterations):
        self._call("ls_remesh_run", int(iterations))

    def phase(self, name, max_rounds=1):
        """one phase on the current mesh: split / collapse / flip (up to max_rounds rounds), relax, project"""
        self._call("ls_remesh_phase", PHASES[name], int(max_rounds))

    def info(self):
        V, F = ctypes.c_int64(0), ctypes.c_int64(0)
        c, s = (ctypes.c_int64 * 6)(), (ctypes.c_double * 5)()
        _native.check(_native.lib().ls_remesh_info(self._h, ctypes.byref(V), ctypes.byref(F), ctypes.byref(c), ctypes.byref(s)))
        return {"V": V.value, "F": F.value, "rounds": dict(split=c[0], collapse=c[1], flip=c[2]),
                "ops": dict(split=c[3], collapse=c[4], flip=c[5]),
                "seconds": dict(zip(("split", "collapse", "flip", "relax", "project"), list(s)))}

    def result(self):
        n = self.info()
        v = torch.empty((n["V"], 3), dtype=torch.float32, device=self.device)
        f = torch.empty((n["F"], 3), dtype=self.index_dtype, device=self.device)
        self._call("ls_remesh_copy_out", _native.ptr(v), _native.ptr(f), f.element_size())
        return v, f

    def close(self):
        if self._h:
            _native.lib().ls_remesh_destroy(self._h)
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


def _scalar(h):
    if isinstance(h, torch.Tensor):
        if h.numel() != 1:
            raise ValueError("h must be a scalar")
        return float(h.item())
    return float(np.asarray(h).reshape(()))


@_native.retry_on_oom
def remesh_botsch(V, F, i, h, project):
    """
    Isotropic remeshing of a triangle mesh to the target edge length h (the call form of pyremesh's remesh_botsch,
    scripts/main.py:149): `i` iterations of split (edges longer than 4/3 h) -> collapse (shorter than 4/5 h) -> flip (towards
    valence 6, 4 on the boundary) -> tangential relaxation -> projection onto the input surface (when `project`).

    * numpy input (V float64 (n, 3), F int32 (m, 3), h a float or 0-dim array): the mesh is copied to the current HIP device,
      remeshed there, and returned as numpy (V' float64, F' int32) -- a drop-in for ``from pyremesh import remesh_botsch``.
    * tensor input (V float32, F int32 or int64 on one HIP device, h a float or 0-dim tensor): tensors on that device come back,
      F' in F's dtype; the mesh makes no host round trip. CPU tensors raise, as everywhere in this package.

    The device computes in fp32 (the reference's remesher computes in double; scripts/main.py casts its result to float at once).
    Boundary edges and vertices stay as they are; vertices no face references are dropped. The input must be an edge-manifold,
    consistently oriented triangle mesh whose vertices' faces form one fan each: anything else raises ValueError (for tensor
    input the check runs on the device, before any remeshing). The call reads sizes on the host every round, so it cannot be
    captured in a graph.
    """
    hval = _scalar(h)
    if isinstance(V, np.ndarray) or isinstance(F, np.ndarray):
        Vn, Fn = np.asarray(V), np.asarray(F)
        if Vn.ndim != 2 or Vn.shape[1] != 3 or Fn.ndim != 2 or Fn.shape[1] != 3:
            raise ValueError(f"V must be (n, 3) and F (m, 3), got {Vn.shape} and {Fn.shape}")
        if not np.issubdtype(Fn.dtype, np.integer):
            raise TypeError(f"F must hold integers, got {Fn.dtype}")
        if not torch.cuda.is_available():
            raise RuntimeError("largesteps (MI355X build): remesh_botsch needs a HIP device; there is no CPU path in this package.")
        dev = torch.device("cuda", torch.cuda.current_device())
        tv = torch.from_numpy(np.ascontiguousarray(Vn, dtype=np.float32)).to(dev)
        tf = torch.from_numpy(np.ascontiguousarray(Fn, dtype=np.int64 if Fn.dtype.itemsize > 4 else np.int32)).to(dev)
        v, f = remesh_botsch(tv, tf, i, hval, project)
        return v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int32)
    with RemeshHandle(V, F, hval, project) as r:
        r.run(int(i))
        return r.result()
