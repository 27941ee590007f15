"""
Midpoint and Loop subdivision on the MI355X (csrc/subdiv.hip): a finer mesh that keeps its correspondence with the coarse one. The
topology is built once per connectivity and level; after that V_fine = S V_coarse is one gather per step, and its gradient the
transposed gather -- a control cage optimised through its refined surface (from_differential -> Subdivision.apply -> normals ->
render), or u, Adam moments and per-vertex attributes carried from one resolution to the next without a closest-point search.

    from largesteps.subdivide import Subdivision, loop, upsample
    sub = Subdivision(F, num_vertices, scheme='loop', levels=1)     # topology only; synchronises once per level
    sub.faces           # (4^levels F, 3), dtype of F, on F's device
    sub.num_vertices    # of the finest level
    sub.edges           # one (E_l, 2) tensor per level: the coarse ends (lower id first) of the new vertex V_l + e
    X_fine = sub.apply(X)     # X (V, C) float32, 1 <= C <= 32 -> (V_fine, C); differentiable in X; no synchronisation
    NV, NF = loop(V, F, number_of_subdivs=1)        # libigl's igl.loop
    NV, NF = upsample(V, F, number_of_subdivs=1)    # libigl's igl.upsample: scheme='midpoint'

The rule (tests/subdiv_statement.py restates it in numpy and the device answers with the same bits):

  * Half-edge h = 3 f + e runs from F[f, e] to F[f, (e + 1) % 3]; the half-edges of one unordered vertex pair form an edge, owned by
    the one of lowest id; edges are numbered by ascending owner, and the new vertex of edge e is V + e. An edge of one half-edge is a
    boundary edge. Orientation need not be consistent. Face f becomes 4 f .. 4 f + 3 = (F[f,0], m_0, m_2), (F[f,1], m_1, m_0),
    (F[f,2], m_2, m_1), (m_0, m_1, m_2) with m_e the new vertex of half-edge 3 f + e.
  * A vertex with no boundary edge is interior, with two a boundary vertex. ValueError for anything else, for an edge of more than
    two half-edges, a face that names a vertex twice and an index outside [0, V).
  * midpoint: an old vertex keeps its bits, an edge vertex is (a + b) / 2.
  * loop (Warren's weights): an edge vertex is 3/8 (a + b) + 1/8 (c + d), c and d the corners opposite the edge, or (a + b) / 2 on a
    boundary edge; an interior vertex of n edges becomes (1 - n beta) x + beta sum(neighbours), beta = 3/16 for n = 3 and 3 / (8 n)
    otherwise; a boundary vertex 3/4 x + 1/8 (p + q), p and q the far ends of its two boundary edges; a vertex in no face keeps its bits.
  * Every value is formed in float64 from the float32 inputs in one stated order and rounded to float32 once; the gradient
    gX = S^T g is a gather per coarse vertex over the same walk, float64, rounded once, without float atomics: forward and backward
    are bitwise reproducible. A vertex of more than 64 corners is summed by a whole wave in a second fixed order.

levels = k is k applications; levels = 0 is the identity (faces is F, apply returns X). Stream capture (torch.cuda.graph): apply and
its backward allocate nothing but their result and never synchronise; only the constructor does.

Input conventions follow largesteps.sampling and largesteps.distance: tensors stay on their HIP device; numpy in gives numpy out (on the
current HIP device); CPU tensors raise. TypeError for wrong types and dtypes, ValueError for wrong shapes, an unknown scheme and
levels < 0, OverflowError when 12 F or V + E of any level reaches 2^31.
"""
import ctypes

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native
from .distance import _as_faces, _as_points, _current_device, _on

SCHEMES = {"midpoint": 0, "loop": 1}            # LS_SUBDIV_MIDPOINT, LS_SUBDIV_LOOP
BAD_INDEX, REPEATED_VERTEX, NONMANIFOLD_EDGE, NONMANIFOLD_VERTEX = 1, 2, 4, 8      # LS_SUBDIV_* status flags
MAX_CHANNELS = 32


def _int(x, what):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"{what} must be an integer, got {type(x).__name__}")
    return int(x)


class _Level:
    """the arrays of one ls_subdiv_topology: F faces over V vertices -> 4 F faces over V + E"""
    __slots__ = ("F", "V", "E", "arrays", "faces", "edges")

    def args(self):
        return [_native.ptr(a) for a in self.arrays]


@_native.retry_on_oom
def _topology(f, V):
    dev, F = f.device, f.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    n = 3 * F
    tri, he, order = (torch.empty(n, **i32) for _ in range(3))
    edges, opp = torch.empty((n, 2), **i32), torch.empty((n, 2), **i32)
    valence, bnbr, vptr = torch.empty(V, **i32), torch.empty((V, 2), **i32), torch.empty(V + 1, **i32)
    bflag = torch.empty(V, dtype=torch.uint8, device=dev)
    fine = torch.empty((4 * F, 3), dtype=f.dtype, device=dev)
    ws = _native.workspace("ls_subdiv_workspace_bytes", (F, V), dev)
    E, status = ctypes.c_int64(0), ctypes.c_int(0)
    with torch.cuda.device(dev):
        _native.check(_native.lib().ls_subdiv_topology(_native.ptr(f), f.element_size(), F, V, _native.ptr(tri), _native.ptr(he), _native.ptr(edges),
                                                       _native.ptr(opp), _native.ptr(valence), _native.ptr(bflag), _native.ptr(bnbr),
                                                       _native.ptr(vptr), _native.ptr(order), _native.ptr(fine), ctypes.byref(E),
                                                       ctypes.byref(status), _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))
    s = status.value
    if s & BAD_INDEX:
        raise ValueError(f"a face index is outside [0, {V})")
    if s & REPEATED_VERTEX:
        raise ValueError("a face names a vertex twice")
    if s & NONMANIFOLD_EDGE:
        raise ValueError("non-manifold edge")
    if s & NONMANIFOLD_VERTEX:
        raise ValueError("non-manifold vertex")
    L = _Level()
    L.F, L.V, L.E = F, V, int(E.value)
    edges, opp = edges[:L.E].clone(), opp[:L.E].clone()           # (the buffers had room for 3 F rows)
    L.arrays = (tri, he, edges, opp, valence, bflag, bnbr, vptr, order)
    L.faces, L.edges = fine, edges.to(f.dtype)
    return L


@_native.retry_on_oom
def _apply(L, scheme, x, backward):
    """S x (V + E, C) of the level, or S^T x (V, C)"""
    dev, C = x.device, x.shape[1]
    out = torch.empty((L.V if backward else L.V + L.E, C), dtype=torch.float32, device=dev)
    fn = _native.lib().ls_subdiv_apply_backward if backward else _native.lib().ls_subdiv_apply
    with torch.cuda.device(dev):
        _native.check(fn(_native.ptr(x), L.F, L.V, L.E, C, scheme, *L.args(), _native.ptr(out), dev.index, _native.stream_of(dev)))
    return out


class _Apply(Function):
    @staticmethod
    def forward(ctx, X, sub):
        ctx.sub = sub
        return sub._forward(X.detach().contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.to(torch.float32).contiguous()
        for L in reversed(ctx.sub._levels):
            g = _apply(L, ctx.sub._scheme, g, True)
        return g, None


class Subdivision:
    """`levels` levels of midpoint or Loop subdivision of the connectivity F (m, 3) over num_vertices vertices: the topology, built on
    the device once (one synchronisation per level), and the linear map it defines. See the module docstring for the rule."""

    def __init__(self, F, num_vertices, scheme="loop", levels=1):
        f = _as_faces(F)
        V = _int(num_vertices, "num_vertices")
        levels = _int(levels, "levels")
        if not isinstance(scheme, str):
            raise TypeError(f"scheme must be a string, got {type(scheme).__name__}")
        if scheme not in SCHEMES:
            raise ValueError(f"scheme must be 'loop' or 'midpoint', got {scheme!r}")
        if V < 0:
            raise ValueError(f"num_vertices must not be negative, got {V}")
        if levels < 0:
            raise ValueError(f"levels must not be negative, got {levels}")
        nf, nv = f.shape[0], V
        for _ in range(levels):                      # E <= 3 F: what cannot fit is refused before anything is built
            if 12 * nf >= 1 << 31 or nv >= 1 << 31:
                raise OverflowError(f"Subdivision: 12 F or V + E of a level reaches 2^31 ({nf} faces, at least {nv} vertices)")
            nf, nv = 4 * nf, nv + (3 * nf + 1) // 2
        self._numpy = not isinstance(f, torch.Tensor)
        dev = _current_device() if self._numpy else f.device
        f = _on(f, dev)
        self.scheme, self._scheme = scheme, SCHEMES[scheme]
        self.device = dev
        self.num_coarse_vertices = V
        self._levels = []
        for _ in range(levels):
            L = _topology(f, V)
            self._levels.append(L)
            f, V = L.faces, L.V + L.E
        self._faces = f
        self.num_vertices = V

    @property
    def faces(self):
        return self._faces.cpu().numpy() if self._numpy else self._faces

    @property
    def edges(self):
        return [L.edges.cpu().numpy() if self._numpy else L.edges for L in self._levels]

    def _forward(self, x):
        for L in self._levels:
            x = _apply(L, self._scheme, x, False)
        return x

    def apply(self, X):
        """X (V, C) float32, 1 <= C <= 32 -> (V_fine, C) = S X; differentiable in a tensor X; numpy in gives numpy out"""
        was_numpy = not isinstance(X, torch.Tensor)
        if was_numpy:
            Xn = np.asarray(X)
            if not (np.issubdtype(Xn.dtype, np.floating) or np.issubdtype(Xn.dtype, np.integer)):
                raise TypeError(f"X must hold real numbers, got {Xn.dtype}")
            if Xn.ndim != 2:
                raise ValueError(f"X must be (V, C), got {Xn.shape}")
            x = np.ascontiguousarray(Xn, dtype=np.float32)
        else:
            _native.require_device(X, "X")
            if X.dtype != torch.float32:
                raise TypeError(f"X must be float32, got {X.dtype}")
            if X.dim() != 2:
                raise ValueError(f"X must be (V, C), got {tuple(X.shape)}")
            x = X
        if x.shape[0] != self.num_coarse_vertices:
            raise ValueError(f"X must have {self.num_coarse_vertices} rows, got {x.shape[0]}")
        if not 1 <= x.shape[1] <= MAX_CHANNELS:
            raise ValueError(f"X must have 1 to {MAX_CHANNELS} columns, got {x.shape[1]}")
        x = _on(x, self.device)
        if not self._levels:
            return X
        if not was_numpy and torch.is_grad_enabled() and X.requires_grad:
            return _Apply.apply(X, self)
        out = self._forward(x.detach().contiguous())
        return out.cpu().numpy() if was_numpy else out


def _one_shot(V, F, number_of_subdivs, scheme):
    v, v_np = _as_points(V, "V")
    f = _as_faces(F)
    if not v_np and isinstance(f, torch.Tensor) and f.device != v.device:
        raise RuntimeError(f"all tensors must be on one device: got {v.device} and {f.device}")
    sub = Subdivision(f, v.shape[0], scheme, number_of_subdivs)            # (refuses what cannot be built before it asks for a device)
    NV, NF = sub.apply(v if v_np else V), sub._faces
    if v_np:
        return NV, NF.cpu().numpy()
    return NV, _on(NF, v.device)


def loop(V, F, number_of_subdivs=1):
    """libigl's igl.loop: (NV, NF) = number_of_subdivs levels of Loop subdivision of the mesh (V (n, 3), F (m, 3)), on a throw-away
    Subdivision; NV is differentiable in a tensor V."""
    return _one_shot(V, F, number_of_subdivs, "loop")


def upsample(V, F, number_of_subdivs=1):
    """libigl's igl.upsample: (NV, NF) = number_of_subdivs levels of midpoint subdivision (every face cut in four, positions in plane)."""
    return _one_shot(V, F, number_of_subdivs, "midpoint")
