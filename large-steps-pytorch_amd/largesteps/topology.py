"""
Mesh topology on the MI355X (csrc/topology.hip): how many pieces a mesh is, which piece is which, where its holes are, and the filter
that keeps some pieces -- without leaving the device. `remesh_level_set` returns every closed sheet of a level set (the outer skin, the
shells around enclosed voids, specks); `remesh_botsch` and `Subdivision` raise on what is not edge-manifold: this module is what stands
between them.

    from largesteps.topology import (MeshTopology, vertex_components, facet_components, boundary_loops, boundary_loop,
                                     is_edge_manifold, remove_unreferenced, keep_components, keep_largest_component,
                                     keep_outer_components)
    topo = MeshTopology(F, num_vertices)      # connectivity only, built on the device once; synchronises once
    topo.vertex_components   # (V,) dtype of F: igl.vertex_components
    topo.facet_components    # (F,) dtype of F: igl.facet_components
    topo.num_vertex_components, topo.num_facet_components          # Python ints
    topo.edges               # (E, 2) lower id first, numbered as Subdivision numbers them
    topo.edge_faces          # (E, 2) the two faces of an edge (lowest half-edge first); -1 for none; first two of a non-manifold edge
    topo.is_edge_manifold, topo.is_oriented, topo.is_closed        # Python bools
    topo.counts()            # per facet component, int64 (K, 6): faces, vertices, edges, boundary, non-manifold, misoriented edges
    topo.euler_characteristic()   # (K,) int64 = vertices - edges + faces
    topo.boundary_loops()    # (loops (B,), ptr (L + 1,)); loop l = loops[ptr[l]:ptr[l + 1]]
    topo.measures(V)         # (K, 2) float64: area and signed volume of every facet component; V (num_vertices, 3) fp32
    topo.keep(mask)          # mask (K,) bool over facet components -> (F2, I, J): compacted faces, I (V,) old->new or -1, J (V2,) new->old

The rule (tests/topology_statement.py restates it in numpy and the device returns the same arrays):

  * Edges. Half-edge h = 3 f + e runs from F[f, e] to F[f, (e + 1) % 3]; the half-edges of one unordered vertex pair form an edge, owned
    by the lowest h; edges are numbered by ascending owner -- Subdivision's rule, so topo.edges equals Subdivision(F, V).edges[0]. An
    edge of one half-edge is a boundary edge, of more than two a non-manifold edge, of exactly two that run the same way a misoriented
    edge. is_edge_manifold: no non-manifold edge; is_oriented: no misoriented and no non-manifold edge; is_closed: no boundary edge.
  * Vertex components. Vertices joined by an edge are in one component; components are numbered by ascending lowest vertex id; a vertex
    in no face is a component of its own.
  * Facet components. Faces that share an EDGE are in one component (two cones tip to tip: one vertex component, two facet components);
    all faces around a non-manifold edge are joined; components are numbered by ascending lowest face id. A component's vertex count is
    the number of distinct vertices its faces name, its edge counts those of the edges of its faces.
  * Boundary loops are defined when every vertex on a boundary edge has exactly one boundary half-edge leaving it and one entering;
    otherwise ValueError("boundary is not a set of oriented cycles"). A loop follows the boundary half-edges from its lowest vertex id;
    loops are ordered by ascending lowest vertex id.
  * Measures. Per face, in float64 from the float32 coordinates: n = (b - a) x (c - a), the area term 0.5 sqrt(nx^2 + ny^2 + nz^2), the
    volume term (ax (b x c)x + ay (b x c)y + az (b x c)z) / 6, every sum left to right. Per component the terms of its faces in ascending
    face id: at most 64 faces by one thread in order; more by a wave, lane l adding faces l, l + 64, ... and the xor butterfly 32, 16,
    ... 1 adding the lanes. No float atomics: bitwise reproducible. Not differentiable.
  * keep. Kept faces keep their order; kept vertices are those a kept face names, in ascending old id; F2 is renumbered through I.
    remove_unreferenced is keep with every component kept; unreferenced vertices get I = -1.

The components come from hooking (the larger root under the smaller, integer atomicMin) and one compression: no host loop, and the
labels do not depend on the order the device runs its threads in.

Input conventions follow largesteps.subdivide: tensors stay on their HIP device; numpy in gives numpy out (on the current HIP device);
CPU tensors raise. Faces are int32 or int64 and index outputs take the dtype of F. ValueError for an index outside [0, V) and for a face
that names a vertex twice; OverflowError when 3 F or V reaches 2^31. An empty F is legal: no facet component, V vertex components.
Stream capture (torch.cuda.graph): measures and keep allocate nothing but their results and never synchronise when keep is told the
sizes of its result (`sizes=`); only the constructor synchronises.
"""
import ctypes

import numpy as np
import torch

from . import _native
from .distance import _as_faces, _as_points, _current_device, _on
from .subdivide import _int

BAD_INDEX, REPEATED_VERTEX, BAD_BOUNDARY = 1, 2, 4          # LS_TOPO_* status flags
COUNT_COLUMNS = ("faces", "vertices", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges")


@_native.retry_on_oom
def _build(f, V):
    dev, F = f.device, f.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    n = 3 * F
    a = dict(tri=torch.empty(n, **i32), vcomp=torch.empty(V, **i32), fcomp=torch.empty(F, **i32), edges=torch.empty((n, 2), **i32),
             edge_faces=torch.empty((n, 2), **i32), eflag=torch.empty(n, dtype=torch.uint8, device=dev), corder=torch.empty(n, **i32),
             forder=torch.empty(F, **i32), fseg=torch.empty(F + 2, **i32), loops=torch.empty(V, **i32), loop_ptr=torch.empty(V + 1, **i32))
    ws = _native.workspace("ls_topo_workspace_bytes", (F, V), dev)
    sizes, status = (ctypes.c_int64 * 8)(), ctypes.c_int(0)
    with torch.cuda.device(dev):
        _native.check(_native.lib().ls_topo_build(_native.ptr(f), f.element_size(), F, V, *[_native.ptr(t) for t in a.values()],
                                                  ctypes.byref(sizes), ctypes.byref(status), _native.ptr(ws), ws.numel(), dev.index,
                                                  _native.stream_of(dev)))
    s = status.value
    if s & BAD_INDEX:
        raise ValueError(f"a face index is outside [0, {V})")
    if s & REPEATED_VERTEX:
        raise ValueError("a face names a vertex twice")
    return a, [int(x) for x in sizes], s


class MeshTopology:
    """The topology of the connectivity F (m, 3) over num_vertices vertices, built on the device once (one synchronisation). See the
    module docstring for the rule and the attributes."""

    def __init__(self, F, num_vertices):
        f = _as_faces(F)
        V = _int(num_vertices, "num_vertices")
        if V < 0:
            raise ValueError(f"num_vertices must not be negative, got {V}")
        if 3 * f.shape[0] >= 1 << 31 or V >= 1 << 31:
            raise OverflowError(f"MeshTopology: 3 F or V reaches 2^31 ({f.shape[0]} faces, {V} vertices)")
        self._numpy = not isinstance(f, torch.Tensor)
        dev = _current_device() if self._numpy else f.device
        f = _on(f, dev)
        self.device, self.dtype = dev, f.dtype
        self.num_faces, self.num_vertices = f.shape[0], V
        a, sizes, status = _build(f, V)
        E, KV, KF, B, L, nb, nnm, nmis = sizes
        self.num_edges, self.num_vertex_components, self.num_facet_components = E, KV, KF
        self.num_boundary_edges, self.num_nonmanifold_edges, self.num_misoriented_edges = nb, nnm, nmis
        self.is_edge_manifold, self.is_oriented, self.is_closed = nnm == 0, nnm == 0 and nmis == 0, nb == 0
        self._loops_defined = not status & BAD_BOUNDARY
        # (the buffers had room for 3 F edges and V loop vertices)
        self._tri, self._fcomp, self._corder, self._forder, self._fseg = a["tri"], a["fcomp"], a["corder"], a["forder"], a["fseg"]
        self._edge_faces, self._eflag = a["edge_faces"][:E].clone(), a["eflag"][:E].clone()
        self._vcomp = a["vcomp"]
        self._edges = a["edges"][:E].clone()
        self._loops = (a["loops"][:B].clone(), a["loop_ptr"][:L + 1].clone()) if self._loops_defined else None
        self._counts = None

    def _out(self, t, index=True):
        if index:
            t = t.to(self.dtype)
        return t.cpu().numpy() if self._numpy else t

    @property
    def vertex_components(self):
        return self._out(self._vcomp)

    @property
    def facet_components(self):
        return self._out(self._fcomp)

    @property
    def edges(self):
        return self._out(self._edges)

    @property
    def edge_faces(self):
        return self._out(self._edge_faces)

    def _counts_tensor(self):
        if self._counts is None:
            K = self.num_facet_components
            c = torch.empty((K, 6), dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                _native.check(_native.lib().ls_topo_counts(_native.ptr(self._tri), _native.ptr(self._fcomp), _native.ptr(self._edge_faces),
                                                           _native.ptr(self._eflag), _native.ptr(self._corder), self.num_faces, self.num_edges, K,
                                                           _native.ptr(c), self.device.index, _native.stream_of(self.device)))
            self._counts = c
        return self._counts

    def counts(self):
        """(K, 6) int64 per facet component: faces, vertices, edges, boundary edges, non-manifold edges, misoriented edges"""
        return self._out(self._counts_tensor(), index=False)

    def euler_characteristic(self):
        """(K,) int64 = vertices - edges + faces of every facet component"""
        c = self._counts_tensor()
        return self._out(c[:, 1] - c[:, 2] + c[:, 0], index=False)

    def boundary_loops(self):
        """(loops (B,), ptr (L + 1,)): loop l is loops[ptr[l]:ptr[l + 1]]"""
        if not self._loops_defined:
            raise ValueError("boundary is not a set of oriented cycles")
        return self._out(self._loops[0]), self._out(self._loops[1])

    @_native.retry_on_oom
    def _measures(self, v):
        K, F = self.num_facet_components, self.num_faces
        out = torch.empty((K, 2), dtype=torch.float64, device=self.device)
        terms = torch.empty((F, 2), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().ls_topo_measures(_native.ptr(v), _native.ptr(self._tri), _native.ptr(self._forder), _native.ptr(self._fseg),
                                                         F, self.num_vertices, K, _native.ptr(terms), _native.ptr(out), self.device.index,
                                                         _native.stream_of(self.device)))
        return out

    def measures(self, V):
        """(K, 2) float64: the area and the signed volume of every facet component for the positions V (num_vertices, 3) float32. Not
        differentiable: a V that requires grad raises."""
        if isinstance(V, torch.Tensor) and V.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("MeshTopology.measures is not differentiable: pass V.detach()")
        v, v_np = _as_points(V, "V")
        if v.shape[0] != self.num_vertices:
            raise ValueError(f"V must have {self.num_vertices} rows, got {v.shape[0]}")
        out = self._measures(_on(v, self.device))
        return out.cpu().numpy() if v_np else out

    def _mask(self, mask):
        K = self.num_facet_components
        if isinstance(mask, torch.Tensor):
            _native.require_device(mask, "mask")
            if mask.dtype != torch.bool:
                raise TypeError(f"mask must be bool, got {mask.dtype}")
            m = _on(mask, self.device)
        else:
            m = np.asarray(mask)
            if m.dtype != np.bool_:
                raise TypeError(f"mask must be bool, got {m.dtype}")
        if m.ndim != 1 or m.shape[0] != K:
            raise ValueError(f"mask must be ({K},), one entry per facet component, got {tuple(m.shape)}")
        return _on(np.ascontiguousarray(m), self.device) if not isinstance(m, torch.Tensor) else m.contiguous()

    @_native.retry_on_oom
    def _keep(self, m, sizes):
        F, V, dev = self.num_faces, self.num_vertices, self.device
        capturing = torch.cuda.is_current_stream_capturing()
        if sizes is None and capturing:
            raise RuntimeError("MeshTopology.keep: the sizes of the result cannot be read back during stream capture; pass "
                               "sizes=(faces, vertices) of an earlier call with this mask")
        cap = (F, V) if sizes is None else (_int(sizes[0], "sizes[0]"), _int(sizes[1], "sizes[1]"))
        if not (0 <= cap[0] <= F and 0 <= cap[1] <= V):
            raise ValueError(f"sizes must be within ({F}, {V}), got {cap}")
        F2 = torch.empty((cap[0], 3), dtype=self.dtype, device=dev)
        I, J = torch.empty(V, dtype=self.dtype, device=dev), torch.empty(cap[1], dtype=self.dtype, device=dev)
        n = torch.empty(2, dtype=torch.int64, device=dev)
        ws = _native.workspace("ls_topo_keep_workspace_bytes", (F, V), dev)
        with torch.cuda.device(dev):
            _native.check(_native.lib().ls_topo_keep(_native.ptr(self._tri), _native.ptr(self._fcomp), _native.ptr(m.view(torch.uint8)), F, V,
                                                     self.num_facet_components, F2.element_size(), cap[0], cap[1], _native.ptr(F2),
                                                     _native.ptr(I), _native.ptr(J), _native.ptr(n), _native.ptr(ws), ws.numel(), dev.index,
                                                     _native.stream_of(dev)))
        if sizes is None:
            nf, nv = (int(x) for x in n.cpu())
            F2, J = F2[:nf], J[:nv]
        return F2, I, J

    def keep(self, mask, sizes=None):
        """mask (K,) bool over the facet components -> (F2, I, J): the kept faces in their order, renumbered; I (V,) the new id of an old
        vertex or -1; J (V2,) the old id of a new vertex. sizes = (F2.shape[0], J.shape[0]) of an earlier call with the same mask saves
        the read-back of the two sizes, the call's only synchronisation (and is needed under stream capture)."""
        F2, I, J = self._keep(self._mask(mask), sizes)
        return self._out(F2, False), self._out(I, False), self._out(J, False)


# ---- the one-shot forms -----------------------------------------------------------------------------------------------------------------
def _faces_only(F, num_vertices=None):
    f = _as_faces(F)
    if num_vertices is None:
        if f.shape[0] == 0:
            num_vertices = 0
        else:
            num_vertices = int(f.max()) + 1
            if int(f.min()) < 0:
                raise ValueError(f"a face index is outside [0, {num_vertices})")
    return MeshTopology(f, num_vertices)


def vertex_components(F, num_vertices=None):
    """igl.vertex_components: (V,) the component of every vertex, V = max(F) + 1 unless given"""
    return _faces_only(F, num_vertices).vertex_components


def facet_components(F):
    """igl.facet_components: (F,) the edge-connected component of every face"""
    return _faces_only(F).facet_components


def boundary_loops(F):
    """igl.boundary_loop (all loops): a list of 1-D index arrays, each from its lowest vertex, ordered by lowest vertex"""
    loops, ptr = _faces_only(F).boundary_loops()
    p = [int(x) for x in (ptr.cpu() if isinstance(ptr, torch.Tensor) else ptr)]
    return [loops[p[i]:p[i + 1]] for i in range(len(p) - 1)]


def boundary_loop(F):
    """igl.boundary_loop (one loop): the longest; ties go to the lower minimum vertex. An empty array for a closed mesh."""
    topo = _faces_only(F)
    loops, ptr = topo.boundary_loops()
    p = np.asarray(ptr.cpu() if isinstance(ptr, torch.Tensor) else ptr, dtype=np.int64)
    if len(p) < 2:
        return loops[:0]
    best = int(np.argmax(np.diff(p)))            # (the first of equal lengths: loops are in ascending lowest vertex)
    return loops[int(p[best]):int(p[best + 1])]


def is_edge_manifold(F):
    """igl.is_edge_manifold: no edge with more than two half-edges"""
    return _faces_only(F).is_edge_manifold


def _mesh(V, F):
    v, v_np = _as_points(V, "V")
    f = _as_faces(F)
    if not v_np and isinstance(f, torch.Tensor) and f.device != v.device:
        raise RuntimeError(f"all tensors must be on one device: got {v.device} and {f.device}")
    topo = MeshTopology(f, v.shape[0])
    return topo, _on(v, topo.device), v_np


def _kept(topo, v, v_np, mask, with_maps):
    F2, I, J = topo._keep(topo._mask(mask), None)
    V2 = v[J.long()]
    f_np = topo._numpy
    out = (V2.cpu().numpy() if v_np else V2, F2.cpu().numpy() if f_np else F2)
    if with_maps:
        out += (I.cpu().numpy() if f_np else I, J.cpu().numpy() if f_np else J)
    return out


def remove_unreferenced(V, F):
    """igl.remove_unreferenced: (NV, NF, I, J) with NV = V[J], NF = I[F]; I is -1 at a vertex no face names"""
    topo, v, v_np = _mesh(V, F)
    return _kept(topo, v, v_np, np.ones(topo.num_facet_components, dtype=bool), True)


def keep_components(V, F, mask):
    """(V2, F2): the facet components of the mesh whose mask entry is True, unreferenced vertices dropped"""
    topo, v, v_np = _mesh(V, F)
    return _kept(topo, v, v_np, mask, False)


def _largest(topo, v, by):
    if by not in ("faces", "area", "volume"):
        raise ValueError(f"by must be 'faces', 'area' or 'volume', got {by!r}")
    K = topo.num_facet_components
    mask = np.zeros(K, dtype=bool)
    if K:
        if by == "faces":
            key = topo._counts_tensor()[:, 0]
        else:
            m = topo._measures(v)
            key = m[:, 0] if by == "area" else m[:, 1].abs()
        key = key.cpu().numpy()
        mask[int(np.argmax(key))] = True          # (the first of equal keys: the lower component id)
    return mask


def keep_largest_component(V, F, by="faces"):
    """(V2, F2): the one facet component with the most faces, the largest area or the largest |signed volume|; ties go to the lower id"""
    topo, v, v_np = _mesh(V, F)
    return _kept(topo, v, v_np, _largest(topo, v, by), False)


def keep_outer_components(V, F):
    """(V2, F2): the facet components of positive signed volume -- of a level set (largesteps.levelset.remesh_level_set returns every
    closed sheet) the outward-facing skins, without the inward-facing shells around enclosed voids"""
    topo, v, v_np = _mesh(V, F)
    return _kept(topo, v, v_np, topo._measures(v)[:, 1] > 0, False)
