"""
Area-weighted points on a mesh surface, on the MI355X (csrc/sample.hip): the step that turns the point-to-mesh distance of
largesteps.distance into a mesh-to-mesh measure -- a chamfer or dense-Hausdorff curve, or a fit of one mesh to another or to a scan.

    from largesteps.sampling import sample_surface
    P, I, W = sample_surface(V, F, n, seed=0, stream=0, offset=0)

P (n, 3) float32 are the points, I (n,) int64 their faces (the dtype of point_mesh_squared_distance's face ids), W (n, 3) float32 their
barycentric weights: P[i] = sum_k W[i, k] V[F[I[i], k]]. The rule (tests/sample_statement.py restates it in
numpy and the device answers with the same bits):

  * Weights, recomputed on every call. With the fp32 corners a, b, c widened to fp64, area = 0.5 sqrt(|(b - a) x (c - a)|^2). A face
    whose area is not finite or not positive has weight 0. amax is the largest area, q_f = floor((area_f / amax) 2^32) as uint64, cumq
    the inclusive prefix sum of q and Q its last entry. Faces smaller than amax * 2^-32 are therefore NEVER drawn; every other face is
    drawn in proportion to its area to 32 bits.
  * Sample i (i counts from `offset`) takes the four words x0 .. x3 of Philox4x32-10 for the counter (i_lo, i_hi, stream, 0) under
    the key (seed_lo, seed_hi). Its face is the first f with cumq[f] > (x0 2^32 + x1) Q >> 64; with u1 = (x2 + 0.5) 2^-32,
    u2 = (x3 + 0.5) 2^-32 and s = sqrt(u1), W = fp32(1 - s, s (1 - u2), s u2), and P = fp32((W0 a + W1 b) + W2 c) in fp64 from the
    ROUNDED weights, so autograd over the returned W describes P exactly.
  * When no face can be drawn (no face of positive area, or no face at all) every P is NaN, every I is -1 and every W is 0; nothing
    is raised, because finding out would synchronise.

The slice law: samples [o, o + m) of a call are, bit for bit, what the call with offset=o, n=m returns. `stream` names an independent
sequence under one seed (chamfer_distance draws from A on stream 0 and from B on stream 1). Results are bitwise reproducible.

Autograd. P is differentiable in a tensor V that requires grad; I and W are marked non-differentiable. The face choice is discrete
and carries no gradient, and W is held fixed: gV[v] = sum_i W[i, k] gP[i] over the samples whose face has v at corner k, every term
formed in float64 and the sum rounded to float32 once, added without float atomics in one fixed order (the samples of a face in
ascending i, a vertex's corners in the rank order of largesteps.normals): bitwise reproducible.

Stream capture (torch.cuda.graph): the forward and the gradient are capturable, after one eager warm-up pass (the first gradient to V
builds the corner ranking of the faces, which synchronises -- and it is there that a face index outside [0, V) raises; the sampler
itself never follows such an index: the face just is not drawn).

Input conventions follow largesteps.distance: tensor input (V float32, F int32 / int64, on one HIP device) returns tensors on that
device; numpy input (V real, converted to float32; F integer) runs on the current HIP device and returns numpy. CPU tensors raise.
"""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from .distance import _as_faces, _as_points, _current_device, _on
from .normals import _plan

SCAN_TILE = 2048            # LS_SAMPLE_SCAN_TILE of the header: the faces one workgroup of the 64-bit scan owns


def _uint(x, what, bits):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"{what} must be an integer, got {type(x).__name__}")
    x = int(x)
    if x < 0 or x >= 1 << bits:
        raise ValueError(f"{what} must be in [0, 2^{bits}), got {x}")
    return x


@_native.retry_on_oom
def _forward(v, f, n, seed, stream, offset):
    dev = v.device
    P = torch.empty((n, 3), dtype=torch.float32, device=dev)
    I = torch.empty(n, dtype=torch.int64, device=dev)
    W = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n:
        ws = _native.workspace("ls_sample_workspace_bytes", (f.shape[0], n), dev)
        with torch.cuda.device(dev):
            _native.check(_native.lib().ls_sample_surface(_native.ptr(v), _native.ptr(f), f.element_size(), f.shape[0], v.shape[0], n, seed, stream,
                                                          offset, _native.ptr(P), _native.ptr(I), _native.ptr(W), _native.ptr(ws), ws.numel(),
                                                          dev.index, _native.stream_of(dev)))
    return P, I, W


@_native.retry_on_oom
def _backward(f, nv, I, W, gP):
    dev, n = f.device, I.shape[0]
    if nv == 0 or f.shape[0] == 0:
        return torch.zeros((nv, 3), dtype=torch.float32, device=dev)
    gV = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    vptr, _, _, order = _plan(f, nv)
    ws = _native.workspace("ls_sample_workspace_bytes", (f.shape[0], n), dev)
    gP = gP.to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        _native.check(_native.lib().ls_sample_surface_backward(_native.ptr(f), f.element_size(), f.shape[0], nv, n, _native.ptr(I), _native.ptr(W),
                                                               _native.ptr(gP), _native.ptr(vptr), _native.ptr(order), _native.ptr(gV),
                                                               _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))
    return gV


class _SampleSurface(Function):
    @staticmethod
    def forward(ctx, V, f, n, seed, stream, offset):
        v = V.detach().contiguous()
        if f.shape[0] and v.shape[0]:
            _plan(f, v.shape[0])            # once per face tensor (synchronises; a bad index raises here): the backward finds it
        P, I, W = _forward(v, f, n, seed, stream, offset)
        ctx.f, ctx.nv = f, v.shape[0]
        ctx.save_for_backward(I, W)
        ctx.mark_non_differentiable(I, W)
        return P, I, W

    @staticmethod
    @once_differentiable
    def backward(ctx, gP, _gI, _gW):
        I, W = ctx.saved_tensors
        return _backward(ctx.f, ctx.nv, I, W, gP), None, None, None, None, None


def sample_surface(V, F, n, seed=0, stream=0, offset=0):
    """(P (n, 3) float32, I (n,) int64, W (n, 3) float32): samples offset .. offset + n - 1 of the area-weighted sequence (seed, stream)
    on the mesh (V, F) -- the rule, the slice law, the gradient to V and the capture conditions are in the module docstring. Faces
    smaller than 2^-32 of the largest one are never drawn. TypeError for wrong types and dtypes; ValueError for wrong shapes, n < 0,
    seed outside [0, 2^64) and stream outside [0, 2^32); OverflowError when n + offset or the number of faces reaches 2^31. n == 0
    returns empty results."""
    v, v_np = _as_points(V, "V")
    f = _as_faces(F)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError(f"n must be an integer, got {type(n).__name__}")
    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    seed, stream, offset = _uint(seed, "seed", 64), _uint(stream, "stream", 32), _uint(offset, "offset", 64)
    if n + offset >= 1 << 31:
        raise OverflowError(f"sample_surface: n + offset must be below 2^31, got {n + offset}")
    if f.shape[0] >= 1 << 31:
        raise OverflowError(f"sample_surface: the mesh must have fewer than 2^31 faces, got {f.shape[0]}")
    dev = _current_device() if v_np else v.device
    v, f = _on(v, dev), _on(f, dev)
    if isinstance(V, torch.Tensor) and torch.is_grad_enabled() and V.requires_grad:
        return _SampleSurface.apply(V, f, n, seed, stream, offset)
    P, I, W = _forward(v, f, n, seed, stream, offset)
    if v_np:
        return P.cpu().numpy(), I.cpu().numpy(), W.cpu().numpy()
    return P, I, W
