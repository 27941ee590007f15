"""
Differentiable rasterizer on the MI355X, in the shape of the nvdiffrast calls the reference's renderer makes
(rgl-epfl/large-steps-pytorch scripts/render.py): `import nvdiffrast.torch as dr` becomes `import largesteps.render as dr`.

Primitives (autograd Functions over hand-written HIP, csrc/raster.hip; the rules are DESIGN.md section 2.7, restated in numpy by
tests/render_statement.py):

    rast, rast_db = rasterize(ctx, pos, tri, resolution)       pos (B, V, 4) clip space, tri (F, 3) int32 / int64, resolution (H, W)
    rast, rast_db = rasterize(ctx, pos, tri, resolution, ranges=R)     range mode: pos (V, 4), R (B, 2) int32 CPU rows (start, count);
                                                               image b draws tri[start_b : start_b + count_b] (the slice law, below)
    with DepthPeeler(ctx, pos, tri, resolution) as peeler:     depth peeling, both modes (ranges=R): each call of
        rast, rast_db = peeler.rasterize_next_layer()          rasterize_next_layer() gives the surfaces behind the layer before (below)
    out, _ = interpolate(attr, rast, tri)                      attr (V, C), (1, V, C) or (B, V, C)
    color_aa = antialias(color, rast, pos, tri, pos_gradient_boost=1.0)
    texture(tex, uv, filter_mode='linear', boundary_mode='wrap')    tex (1 or B, Ht, Wt, C), uv (B, H, W, 2); nearest / linear, wrap / clamp /
                                                               zero (csrc/texture.hip, restated by tests/texture_statement.py)
    out, uv_da = interpolate(attr, rast, tri, rast_db=rast_db, diff_attrs='all')       the attribute's change per pixel step
    texture(tex, uv, uv_da, filter_mode='linear-mipmap-linear')     the mipmapped lookup (csrc/mip.hip, restated by tests/mip_statement.py);
                                                               texture_construct_mip(tex) builds a reusable pyramid, pixel_differentials(rast,
                                                               pos, tri) the differentials of the barycentrics themselves
    texture(cube, dirs, boundary_mode='cube')                  the cube-map lookup: cube (1 or B, 6, n, n, C), dirs (B, H, W, 3) directions;
                                                               nearest / linear, seamless across edges and corners (csrc/cube.hip, restated
                                                               by tests/cube_statement.py)

plus the renderer built on them: `persp_proj`, `SphericalHarmonics`, `NVDRenderer` (same constructor keys, same values as the
reference's). Conventions: rast = (u, v, z/w, id + 1), 0 for background; an attribute interpolates as u a0 + v a1 + (1 - u - v) a2;
row 0 of an image is NDC y = -1, pixel (x, y) has its centre at NDC ((2x + 1) / W - 1, (2y + 1) / H - 1). Gradients: rasterize passes
the gradients of u and v to pos (the z/w channel's gradient is dropped), interpolate to attr and to rast[..., :2], antialias to color
and (scaled by pos_gradient_boost) to pos, texture to tex and (linear filtering) to uv -- so interpolate(uv attribute) -> texture ->
antialias learns a texture and moves the geometry under it. No float atomics anywhere: images and gradients are bitwise reproducible, and no call
synchronises with the host once a face tensor has been seen (its edge adjacency and corner ranking are cached per tensor object), so
the whole render can sit inside `CapturedStep`. There is no CPU path (but a plain-torch `texture` forward, linear + wrap, for CPU tensors).

Range mode renders B different meshes (`MeshBatch.faces` with `MeshBatch.ranges()`) in one call. The slice law: image b of a range-mode
call is, bit for bit, what the instanced call on pos[None] and the slice tri[start_b : start_b + count_b] produces, with start_b added
to the id channel of covered pixels -- for `rasterize`, `interpolate` and `antialias` -- and every gradient (pos from rasterize and from
antialias, attr, color, rast[..., :2]) equals bit for bit the sum of the B slice calls' gradients, accumulated in ascending b starting
from image 0's. Ranges may overlap, be unsorted, be empty (an all-zero image) or leave faces out; silhouettes are those of each image's
own faces (a closed surface cut by a range has a boundary along the cut). The rast of a range-mode call carries its range table:
`interpolate` and `antialias` must be given that very tensor.

Depth peeling (`DepthPeeler`, nvdiffrast's class) shows what lies behind the nearest surface: nested shells, the far side of a closed
mesh, translucent targets, a thickness loss. Layer 0 is `rasterize` itself (the same native call, the same bits); layer l + 1 keeps, per
pixel, the nearest covering fragment strictly behind the one layer l shows, in the order the depth pass resolves a pixel by: (z/w as
fp32, face id). So layer l is the l-th covering fragment of the pixel in that order -- exact depth ties peel in face order, there is no
epsilon -- and a pixel that ran out of fragments is background from then on. Every layer is a rast like any other (it carries its
frame): `interpolate`, `antialias` and the pixel differentials take it unchanged, and the gradient of its u and v flows to pos through
the backward of `rasterize`; which fragment a layer shows is a discrete choice and carries no gradient. The slice law holds layer by
layer.

Above the kernels the two modes share one code path: `_Rasterize`, `_Interpolate` and `_Antialias` convert, allocate and save once, and ask
the frame that the rast carries (`rast._largesteps_frame`) for what a mode supplies -- the number of keys and images, the workspace size,
the shape rules of pos and tri, the edge adjacency and the native calls (`_InstancedFrame` knows F, `_RangeFrame` its range table). The
frame also holds the pixel order of the backward passes, made at most once per version of the rast. A rast that no `rasterize` made (a
clone, a fabricated tensor) gets a fresh instanced frame; a range frame is made by `rasterize` only.
"""
import collections
import ctypes
import functools

import numpy as np
import torch
from torch.autograd import Function

from . import _native
from .normals import _plan as _corner_plan

__all__ = ["RasterizeContext", "RasterizeGLContext", "RasterizeCudaContext", "rasterize", "DepthPeeler", "interpolate", "antialias", "texture",
           "texture_construct_mip", "pixel_differentials", "persp_proj", "SphericalHarmonics", "NVDRenderer"]


class RasterizeContext:
    """Accepted and ignored: the rasterizer keeps no per-context state (nvdiffrast's GL / CUDA contexts hold buffers)."""

    def __init__(self, *args, **kwargs):
        pass


RasterizeGLContext = RasterizeContext
RasterizeCudaContext = RasterizeContext


# ---- per face tensor: range check + corner ranking (normals.py's cache) and the edge adjacency ------------------------------------------
_adjacency = _native.IdentityCache()


def _faces(tri, V):
    _native.require_device(tri, "tri")
    if tri.dim() != 2 or tri.shape[1] != 3:
        raise ValueError(f"tri must be (F, 3), got {tuple(tri.shape)}")
    if tri.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"tri must be int32 or int64, got {tri.dtype}")
    f = tri if tri.is_contiguous() else tri.contiguous()
    vptr, _, narrow, order = _corner_plan(f, V)       # range check: an index outside [0, V) raises IndexError
    if narrow.dtype != torch.int32:
        raise OverflowError("tri needs indices below 2**31")
    return f, narrow, vptr, order


def _plain(t, align):
    """detached, contiguous and aligned for the kernels' vector loads (float2 / float4 rows: torch's allocations are 256-byte aligned, a
    view into one need not be); None stays None"""
    if t is None:
        return None
    d = t.detach()
    d = d if d.is_contiguous() else d.contiguous()
    return d if d.data_ptr() % align == 0 else d.clone()


def _adjacent(f, narrow):
    adj = _adjacency.get(f)
    if adj is None:
        F, dev = narrow.shape[0], f.device
        ws = _native.workspace("ls_raster_adjacency_workspace_bytes", (F,), dev)
        adj = torch.empty(max(3 * F, 1), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _native.check(_native.lib().ls_raster_adjacency(_native.ptr(narrow), F, _native.ptr(adj), _native.ptr(ws), ws.numel(), dev.index,
                                                            _native.stream_of(dev)))
        _adjacency.put(f, adj)
    return adj


def _pos(pos, shared=False):
    """the clip-space positions detached, fp32 and contiguous: (B, V, 4), or the one (V, 4) of range mode (`shared`)"""
    _native.require_device(pos, "pos")
    if pos.dim() != (2 if shared else 3) or pos.shape[-1] != 4:
        raise ValueError(f"pos must be (V, 4) clip-space positions in range mode, got {tuple(pos.shape)}" if shared else
                         f"pos must be (B, V, 4) clip-space positions (instanced mode), got {tuple(pos.shape)}")
    p = pos.detach()
    if p.dtype != torch.float32 or not p.is_contiguous():
        p = p.to(torch.float32).contiguous()
    return _plain(p, 16) if shared else p


def _rast(rast):
    _native.require_device(rast, "rast")
    if rast.dim() != 4 or rast.shape[3] != 4:
        raise ValueError(f"rast must be (B, H, W, 4), got {tuple(rast.shape)}")
    r = rast.detach()
    return r if (r.dtype == torch.float32 and r.is_contiguous()) else r.to(torch.float32).contiguous()


# ---- range mode: the table of a ranges tensor --------------------------------------------------------------------------------------------
_range_tables = _native.IdentityCache()


class _RangeTable:
    """The device table (B, 3) = (start, count, item_ptr) of one ranges tensor, and the item adjacency of every face tensor it was used with
    (cached per (face tensor, ranges tensor) in the style of `_adjacent`)."""
    __slots__ = ("B", "N", "F", "dev", "adj")

    def __init__(self, B, N, F, dev):
        self.B, self.N, self.F, self.dev, self.adj = B, N, F, dev, _native.IdentityCache()

    def adjacency(self, f, narrow):
        """(3 N) int32: the item across each edge of each item within its image, -1 for none"""
        adj = self.adj.get(f)
        if adj is None:
            dev = self.dev.device
            ws = _native.workspace("ls_range_adjacency_workspace_bytes", (self.N,), dev)
            adj = torch.empty(max(3 * self.N, 1), dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _native.check(_native.lib().ls_range_adjacency(_native.ptr(narrow), narrow.shape[0], _native.ptr(self.dev), self.B, self.N,
                                                               _native.ptr(adj), _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))
            self.adj.put(f, adj)
        return adj


def _check_ranges(ranges, F):
    """Host validation of a range-mode `ranges` against F faces (a CPU tensor: no synchronisation). Returns (B, N = the number of items)."""
    if not isinstance(ranges, torch.Tensor):
        raise TypeError(f"ranges must be a torch.Tensor, got {type(ranges).__name__}")
    if ranges.device.type != "cpu":
        raise ValueError(f"ranges must be a CPU tensor (its rows are read on the host), got device '{ranges.device}'")
    if ranges.dtype != torch.int32:
        raise TypeError(f"ranges must be int32, got {ranges.dtype}")
    if ranges.dim() != 2 or ranges.shape[1] != 2 or ranges.shape[0] < 1:
        raise ValueError(f"ranges must be (B, 2) rows of (start, count) with B >= 1, got {tuple(ranges.shape)}")
    r = ranges.to(torch.int64)
    start, count = r[:, 0], r[:, 1]
    bad = (start < 0) | (count < 0) | (start + count > F)
    if bool(bad.any()):
        b = int(torch.nonzero(bad)[0])
        raise ValueError(f"ranges[{b}] = (start {int(start[b])}, count {int(count[b])}) is outside the {F} faces of tri: "
                         "0 <= start, 0 <= count and start + count <= F are required")
    N = int(count.sum())
    if 3 * N >= 2 ** 31 - 1:
        raise OverflowError(f"ranges hold {N} faces in all: the kernels index their corners with int32")
    return ranges.shape[0], N


def _range_table(ranges, F, dev):
    """the device table of `ranges`, validated against F faces; cached per ranges tensor (identity, version, data pointer)"""
    tab = _range_tables.get(ranges, (F, dev))
    if tab is None:
        B, N = _check_ranges(ranges, F)
        host = torch.empty((B, 3), dtype=torch.int32)
        host[:, :2] = ranges
        count = ranges[:, 1].to(torch.int64)
        host[:, 2] = (torch.cumsum(count, 0) - count).to(torch.int32)
        tab = _range_tables.put(ranges, _RangeTable(B, N, F, host.to(dev)), (F, dev))
    return tab


# ---- the frame of a rast: what differs between the modes above the kernels ------------------------------------------------------------------
class _Frame:
    """What the rast of `rasterize` carries (`rast._largesteps_frame`), instanced or range mode. It owns the pixels of the frame sorted by
    key ((image, face), or item) -- the order every backward sums in, made at most once per version of the rast by the first backward that
    needs it -- and, in its two implementations, what a mode supplies: the number of keys and of images, the workspace, the shape rules
    of pos and tri, the edge adjacency and the native calls (`rasterize`, and `rasterize_layer` behind a previous layer: depth peeling).
    F: the faces of tri; tab: the `_RangeTable`, None when instanced. fresh(): another frame of the same mode, for another rast."""
    __slots__ = ("F", "tab", "version", "order", "seg")

    def __init__(self, F, tab=None):
        self.F, self.tab, self.version, self.order, self.seg = F, tab, None, None, None

    def pixel_order(self, r, version):
        if self.order is None or self.version != version:
            B, H, W, _ = r.shape
            dev = r.device
            order = torch.empty(B * H * W, dtype=torch.int32, device=dev)
            seg = torch.empty(self.keys(B) + 1, dtype=torch.int32, device=dev)
            ws = self.workspace(B, H, W, 0, dev)
            with torch.cuda.device(dev):
                self.sort_pixels(r, B, H, W, order, seg, ws, dev)
            self.order, self.seg, self.version = order, seg, version
        return self.order, self.seg


class _InstancedFrame(_Frame):
    """B views of one mesh: pos (B, V, 4), keys (image, face)"""
    __slots__ = ()
    pos = staticmethod(_pos)
    faces = staticmethod(_faces)
    adjacency = staticmethod(_adjacent)

    def fresh(self):
        return _InstancedFrame(self.F)

    def keys(self, B):
        return B * self.F

    def images(self, p):
        return p.shape[0]

    def workspace(self, B, H, W, C, dev):
        return _native.workspace("ls_raster_workspace_bytes", (B, self.F, H, W, C), dev)

    def sort_pixels(self, r, B, H, W, order, seg, ws, dev):
        _native.check(_native.lib().ls_raster_pixel_order(_native.ptr(r), B, self.F, H, W, _native.ptr(order), _native.ptr(seg), _native.ptr(ws),
                                                          ws.numel(), dev.index, _native.stream_of(dev)))

    def rasterize(self, p, narrow, B, H, W, rast, ws, dev):
        _native.check(_native.lib().ls_raster_forward(_native.ptr(p), B, p.shape[1], _native.ptr(narrow), narrow.shape[0], H, W, _native.ptr(rast),
                                                      _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))

    def rasterize_layer(self, p, narrow, B, H, W, prev, rast, ws, dev):
        _native.check(_native.lib().ls_peel_forward(_native.ptr(p), B, p.shape[1], _native.ptr(narrow), narrow.shape[0], H, W, _native.ptr(prev),
                                                    _native.ptr(rast), _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))

    def rasterize_backward(self, p, narrow, B, H, W, g, order, seg, vptr, corner_order, gp, ws, dev):
        _native.check(_native.lib().ls_raster_backward(_native.ptr(p), B, p.shape[1], _native.ptr(narrow), narrow.shape[0], H, W, _native.ptr(g),
                                                       _native.ptr(order), _native.ptr(seg), _native.ptr(vptr), _native.ptr(corner_order),
                                                       _native.ptr(gp), _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))

    def interpolate_backward(self, a, r, narrow, g, vptr, corner_order, ga, gr, version):
        (B, H, W, _), (Ba, V, C), dev = r.shape, a.shape, r.device
        order = seg = ws = None
        if ga is not None:
            order, seg = self.pixel_order(r, version)
            ws = self.workspace(B, H, W, C, dev)
        _native.check(_native.lib().ls_raster_interpolate_backward(
            _native.ptr(a), Ba, V, C, _native.ptr(r), B, H, W, _native.ptr(narrow), narrow.shape[0], _native.ptr(g), _native.ptr(order),
            _native.ptr(seg), _native.ptr(vptr), _native.ptr(corner_order), _native.ptr(ga), _native.ptr(gr), _native.ptr(ws),
            0 if ws is None else ws.numel(), dev.index, _native.stream_of(dev)))

    def antialias(self, c, r, p, narrow, adj, B, H, W, out, dev):
        C = c.shape[3]
        _native.check(_native.lib().ls_raster_antialias(_native.ptr(c), C, _native.ptr(r), _native.ptr(p), B, p.shape[1], H, W, _native.ptr(narrow),
                                                        narrow.shape[0], _native.ptr(adj), _native.ptr(out), dev.index, _native.stream_of(dev)))

    def antialias_backward(self, c, r, p, narrow, adj, B, H, W, C, g, boost, order, seg, vptr, corner_order, gc, gp, ws, dev):
        _native.check(_native.lib().ls_raster_antialias_backward(
            _native.ptr(c), C, _native.ptr(r), _native.ptr(p), B, p.shape[1], H, W, _native.ptr(narrow), narrow.shape[0], _native.ptr(adj),
            _native.ptr(g), boost, _native.ptr(order), _native.ptr(seg), _native.ptr(vptr), _native.ptr(corner_order), _native.ptr(gc),
            _native.ptr(gp), _native.ptr(ws), 0 if ws is None else ws.numel(), dev.index, _native.stream_of(dev)))


class _RangeFrame(_Frame):
    """B images of the N items of a range table: one shared pos (V, 4), keys = items. Made by `rasterize` and `DepthPeeler` only."""
    __slots__ = ()

    def __init__(self, tab):
        super().__init__(tab.F, tab)

    def fresh(self):
        return _RangeFrame(self.tab)

    def keys(self, B):
        return self.tab.N

    def images(self, p):
        return self.tab.B

    def pos(self, pos):
        return _pos(pos, shared=True)

    def faces(self, tri, V):
        f, narrow, vptr, order = _faces(tri, V)
        if narrow.shape[0] != self.F:
            raise ValueError(f"tri has {narrow.shape[0]} faces, the range-mode rast was rasterized from {self.F}")
        return f, narrow, vptr, order

    def adjacency(self, f, narrow):
        return self.tab.adjacency(f, narrow)

    def workspace(self, B, H, W, C, dev):
        return _native.workspace("ls_range_workspace_bytes", (B, self.tab.N, H, W, C), dev)

    def sort_pixels(self, r, B, H, W, order, seg, ws, dev):
        tab = self.tab
        _native.check(_native.lib().ls_range_pixel_order(_native.ptr(r), _native.ptr(tab.dev), B, tab.N, tab.F, H, W, _native.ptr(order),
                                                         _native.ptr(seg), _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))

    def rasterize(self, p, narrow, B, H, W, rast, ws, dev):
        tab = self.tab
        _native.check(_native.lib().ls_range_forward(_native.ptr(p), p.shape[0], _native.ptr(narrow), tab.F, _native.ptr(tab.dev), B, tab.N, H, W,
                                                     _native.ptr(rast), _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))

    def rasterize_layer(self, p, narrow, B, H, W, prev, rast, ws, dev):
        tab = self.tab
        _native.check(_native.lib().ls_peel_range_forward(_native.ptr(p), p.shape[0], _native.ptr(narrow), tab.F, _native.ptr(tab.dev), B, tab.N, H,
                                                          W, _native.ptr(prev), _native.ptr(rast), _native.ptr(ws), ws.numel(), dev.index,
                                                          _native.stream_of(dev)))

    def rasterize_backward(self, p, narrow, B, H, W, g, order, seg, vptr, corner_order, gp, ws, dev):
        tab = self.tab
        _native.check(_native.lib().ls_range_backward(_native.ptr(p), p.shape[0], _native.ptr(narrow), tab.F, _native.ptr(tab.dev), B, tab.N, H, W,
                                                      _native.ptr(g), _native.ptr(order), _native.ptr(seg), _native.ptr(vptr),
                                                      _native.ptr(corner_order), _native.ptr(gp), _native.ptr(ws), ws.numel(), dev.index,
                                                      _native.stream_of(dev)))

    def interpolate_backward(self, a, r, narrow, g, vptr, corner_order, ga, gr, version):
        (B, H, W, _), (_, V, C), dev, tab = r.shape, a.shape, r.device, self.tab
        st = _native.stream_of(dev)
        if gr is not None:          # ids are global and attr is shared: the instanced kernel as it is, as in the forward
            _native.check(_native.lib().ls_raster_interpolate_backward(
                _native.ptr(a), 1, V, C, _native.ptr(r), B, H, W, _native.ptr(narrow), narrow.shape[0], _native.ptr(g), None, None, None, None, None,
                _native.ptr(gr), None, 0, dev.index, st))
        if ga is not None:
            order, seg = self.pixel_order(r, version)
            ws = self.workspace(B, H, W, C, dev)
            _native.check(_native.lib().ls_range_interpolate_backward(
                _native.ptr(r), _native.ptr(tab.dev), B, tab.N, H, W, V, C, _native.ptr(g), _native.ptr(order), _native.ptr(seg), _native.ptr(vptr),
                _native.ptr(corner_order), _native.ptr(ga), _native.ptr(ws), ws.numel(), dev.index, st))

    def antialias(self, c, r, p, narrow, adj, B, H, W, out, dev):
        C, tab = c.shape[3], self.tab
        _native.check(_native.lib().ls_range_antialias(_native.ptr(c), C, _native.ptr(r), _native.ptr(p), p.shape[0], _native.ptr(narrow), tab.F,
                                                       _native.ptr(tab.dev), B, tab.N, H, W, _native.ptr(adj), _native.ptr(out), dev.index,
                                                       _native.stream_of(dev)))

    def antialias_backward(self, c, r, p, narrow, adj, B, H, W, C, g, boost, order, seg, vptr, corner_order, gc, gp, ws, dev):
        tab = self.tab
        _native.check(_native.lib().ls_range_antialias_backward(
            _native.ptr(c), C, _native.ptr(r), _native.ptr(p), p.shape[0], _native.ptr(narrow), tab.F, _native.ptr(tab.dev), B, tab.N, H, W,
            _native.ptr(adj), _native.ptr(g), boost, _native.ptr(order), _native.ptr(seg), _native.ptr(vptr), _native.ptr(corner_order),
            _native.ptr(gc), _native.ptr(gp), _native.ptr(ws), 0 if ws is None else ws.numel(), dev.index, _native.stream_of(dev)))


def _range_frame(rast):
    """the range frame of a rast that a range-mode `rasterize` returned, None for any other tensor"""
    frame = getattr(rast, "_largesteps_frame", None)
    if frame is None or frame.tab is None or not isinstance(rast, torch.Tensor) or rast.dim() != 4 or rast.shape[0] != frame.tab.B:
        return None
    return frame


def _instanced_frame(rast, tri):
    """the instanced frame that rast carries for the F faces of tri, or a fresh one (a rast that no `rasterize` of this package made, or
    one made from another F); the caller leaves it on rast once its call went through"""
    F = tri.shape[0] if isinstance(tri, torch.Tensor) and tri.dim() == 2 else 0
    frame = getattr(rast, "_largesteps_frame", None)
    return frame if frame is not None and frame.tab is None and frame.F == F else _InstancedFrame(F)


class _Rasterize(Function):
    @staticmethod
    def forward(ctx, pos, tri, H, W, frame, prev=None):
        p = frame.pos(pos)
        f, narrow, vptr, order = frame.faces(tri, p.shape[-2])
        B, dev = frame.images(p), p.device
        rast = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
        ws = frame.workspace(B, H, W, 0, dev)
        with torch.cuda.device(dev):
            if prev is None:
                frame.rasterize(p, narrow, B, H, W, rast, ws, dev)
            else:                         # depth peeling: the layer behind `prev`, the peeler's own copy of the layer before
                frame.rasterize_layer(p, narrow, B, H, W, prev, rast, ws, dev)
        rast_db = torch.zeros((B, H, W, 4), dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(rast_db)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p, narrow, vptr, order, rast)
        ctx.frame = frame
        return rast, rast_db

    @staticmethod
    def backward(ctx, g_rast, g_db):
        if g_rast is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        p, narrow, vptr, corner_order, rast = ctx.saved_tensors
        (B, H, W, _), dev, frame = rast.shape, p.device, ctx.frame
        g = g_rast.to(torch.float32).contiguous()
        order, seg = frame.pixel_order(rast, rast._version)
        ws = frame.workspace(B, H, W, 0, dev)
        gp = torch.empty_like(p)
        with torch.cuda.device(dev):
            frame.rasterize_backward(p, narrow, B, H, W, g, order, seg, vptr, corner_order, gp, ws, dev)
        return gp, None, None, None, None, None


def _range_frame_for(pos, tri, H, W, resolution, ranges):
    """the checks of a range-mode `rasterize`, and its frame"""
    for t, what in ((pos, "pos"), (tri, "tri")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor, got {type(t).__name__}")
    if pos.dim() == 3:
        raise ValueError(f"range mode (ranges=...) takes one shared pos (V, 4), got {tuple(pos.shape)}: a (B, V, 4) pos is instanced mode "
                         "(ranges=None)")
    if pos.dim() != 2 or pos.shape[1] != 4:
        raise ValueError(f"pos must be (V, 4) clip-space positions in range mode, got {tuple(pos.shape)}")
    if tri.dim() != 2 or tri.shape[1] != 3:
        raise ValueError(f"tri must be (F, 3), got {tuple(tri.shape)}")
    F = tri.shape[0]
    on_device = pos.is_cuda and tri.is_cuda
    tab = _range_table(ranges, F, pos.device) if on_device else None
    if tab is None:
        _check_ranges(ranges, F)
    if not (1 <= H <= 4096 and 1 <= W <= 4096):
        raise ValueError(f"resolution must be (H, W) with each in [1, 4096], got {tuple(resolution)}")
    if not on_device:
        raise NotImplementedError("largesteps.render.rasterize: range mode (ranges=...) needs a HIP device: pos and tri must live on 'cuda' "
                                  "(there is no CPU path in this package)")
    if tab.B * H * W >= 2 ** 31 - 1:
        raise OverflowError(f"{tab.B} images of {H} x {W} pixels: the kernels index pixels with int32")
    return _RangeFrame(tab)


def _frame_for(pos, tri, H, W, resolution, ranges):
    """the frame of a `rasterize` call or of a `DepthPeeler`, after the checks that come before the Function's own"""
    if ranges is not None:
        return _range_frame_for(pos, tri, H, W, resolution, ranges)
    if not (1 <= H <= 4096 and 1 <= W <= 4096):
        raise ValueError(f"resolution must be (H, W) with each in [1, 4096], got {tuple(resolution)}")
    return _InstancedFrame(tri.shape[0] if isinstance(tri, torch.Tensor) and tri.dim() == 2 else 0)


def _rasterize(pos, tri, H, W, frame, prev=None):
    """one frame through `_Rasterize`: the nearest surface, or (depth peeling) the one behind `prev`; the rast leaves with its frame"""
    rast, rast_db = _Rasterize.apply(pos, tri, H, W, frame, prev)
    rast._largesteps_frame = frame
    if frame.tab is None:
        rast_db._largesteps_db = _DbSource(pos, tri, rast_db._version)
    return rast, rast_db


@_native.retry_on_oom
def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """
    Rasterize triangles (nvdiffrast.torch.rasterize, instanced and range mode). Returns (rast, rast_db).

    glctx : RasterizeContext (ignored)
    pos : (B, V, 4) fp32 clip-space positions on a HIP device; (V, 4) in range mode
    tri : (F, 3) int32 or int64
    resolution : (H, W), each in [1, 4096]
    ranges : None (instanced mode), or range mode: a (B, 2) int32 CPU tensor of (start, count) rows with 0 <= start, 0 <= count and
             start + count <= F. pos is then (V, 4), shared by the B images, and image b holds the faces tri[start_b : start_b + count_b]
             with GLOBAL ids (face index in tri, plus one): bit for bit the instanced frame of pos[None] and that slice, start_b added to
             the ids (the slice law of the module's docstring). Ranges may overlap, be unsorted or empty. The device copy of the table is
             cached per ranges tensor (identity, version, data pointer): keep one tensor (`MeshBatch.ranges()`) and nothing is copied
             from the host after the first call. The returned rast carries the table for `interpolate` and `antialias`; rast_db is
             then a plain zero tensor (pixel differentials are not supported in range mode).
    grad_db : ignored. rast_db holds zeros (rasterize computes no image-space derivatives) and asking for its gradient raises; it carries
              the detached pos and tri, from which `interpolate(..., rast_db=rast_db, diff_attrs=...)` computes the differentials when
              they are wanted (`pixel_differentials`).

    rast (B, H, W, 4) = (u, v, z/w, triangle id + 1), 0 for background pixels. Coverage: a pixel is covered iff its centre lies in the
    projected triangle (top-left rule, watertight along shared edges) and z/w is in [-1, 1] (near and far clipping); the nearest
    covering triangle wins (ties: the lower id). The gradient of rast[..., 0:2] flows to pos; the gradient of the z/w channel is dropped.
    """
    H, W = (int(resolution[0]), int(resolution[1]))
    return _rasterize(pos, tri, H, W, _frame_for(pos, tri, H, W, resolution, ranges))


class DepthPeeler:
    """
    Depth peeling (nvdiffrast.torch.DepthPeeler, instanced and range mode): the surfaces behind the nearest one, a layer per call.

        with DepthPeeler(glctx, pos, tri, resolution) as peeler:
            for _ in range(layers):
                rast, rast_db = peeler.rasterize_next_layer()

    The arguments are those of `rasterize`, checked as `rasterize` checks them (range mode: pos (V, 4) and ranges). Layer 0 is what
    `rasterize` returns, bit for bit. Layer l + 1 holds, per pixel, the nearest covering fragment strictly behind the one in layer l, in
    the order the depth pass resolves a pixel by -- (z/w as fp32, face id) -- so layer l is the pixel's l-th covering fragment in that
    order: fragments at exactly the same depth peel one by one in face order, and nothing is skipped or repeated by an epsilon. A pixel
    whose fragments are used up is background (all zeros) in every later layer, and so is a whole layer past the deepest one.

    Each layer is computed from the peeler's own detached copy of the one before: editing a returned rast does not change later layers.
    Every returned rast carries its frame, so `interpolate`, `antialias` and (instanced mode) `rast_db` with diff_attrs take it as they
    take the rast of `rasterize`, and the gradient of rast[..., :2] of any layer flows to pos through the backward of `rasterize`;
    which fragment a layer shows is a discrete choice without a gradient. In range mode the slice law holds for every layer. pos must
    not be changed in place between layers (ValueError). No call synchronises with the host: a peeling render can be captured.
    """

    def __init__(self, glctx, pos, tri, resolution, ranges=None, grad_db=True):
        H, W = (int(resolution[0]), int(resolution[1]))
        frame = _frame_for(pos, tri, H, W, resolution, ranges)
        frame.faces(tri, frame.pos(pos).shape[-2])          # what `_Rasterize` checks, here rather than at the first layer
        self._args = (pos, tri, H, W)
        self._frame, self._pos_version, self._prev = frame, pos._version, None
        self._active = False                                # True inside the `with` block

    def __enter__(self):
        if self._args is None:
            raise RuntimeError("largesteps.render.DepthPeeler: a peeler is used in one `with` block only")
        self._active = True
        return self

    def __exit__(self, *exc):
        self._active, self._args, self._frame, self._prev = False, None, None, None
        return False

    @_native.retry_on_oom
    def rasterize_next_layer(self):
        """(rast, rast_db) of the next layer, as `rasterize` returns them: first the nearest surface, then what lies behind it"""
        if not self._active:
            raise RuntimeError("largesteps.render.DepthPeeler.rasterize_next_layer: call it inside the peeler's `with` block")
        pos, tri, H, W = self._args
        if pos._version != self._pos_version:
            raise ValueError("pos was changed in place after the DepthPeeler was made: the next layer would not lie behind the last one")
        rast, rast_db = _rasterize(pos, tri, H, W, self._frame.fresh(), self._prev)
        self._prev = rast.detach().clone()
        return rast, rast_db


class _DbSource:
    """What the zero placeholder `rast_db` of `rasterize` carries: the detached clip-space positions and the faces of its frame, and the
    differentials once an `interpolate` has asked for them (computed at most once per frame, never kept across a stream capture)."""
    __slots__ = ("pos", "tri", "pos_version", "version", "db")

    def __init__(self, pos, tri, version):
        self.pos, self.tri, self.pos_version, self.version, self.db = pos.detach(), tri, pos._version, version, None


@_native.retry_on_oom
def pixel_differentials(rast, pos, tri):
    """
    The change of the barycentrics per pixel step: (B, H, W, 4) fp32 = (du/dX, du/dY, dv/dX, dv/dY), X and Y in pixels (one pixel is
    2 / W in NDC x, 2 / H in NDC y), u and v the perspective-correct weights of corners 0 and 1 as `rasterize` writes them.

    rast : the first output of `rasterize`;  pos, tri : what `rasterize` was given.

    For a covered pixel whose face has clip-space corners p_k = (x_k, y_k, w_k): a_k(Xn, Yn) = A_k Xn + B_k Yn + C_k are the rows of the
    adjugate of [p_0; p_1; p_2], u = a_0 / s, v = a_1 / s, s = a_0 + a_1 + a_2, and du/dXn = (A_0 - u (A_0 + A_1 + A_2)) / s (likewise v
    and Yn), times 2 / W (2 / H). Background pixels and degenerate faces (s or the determinant zero or not finite) get 0.

    The result is not differentiable. nvdiffrast propagates a second-order term through its rast_db to pos; this package does not: the
    level of detail chosen from these differentials is treated as a constant of the geometry.
    """
    if isinstance(pos, torch.Tensor) and pos.dim() == 2:
        raise NotImplementedError("largesteps.render.pixel_differentials: a (V, 4) pos (range mode) is not supported; pixel differentials "
                                  "need instanced mode, pos (B, V, 4)")
    r, p = _rast(rast), _pos(pos)
    B, H, W, _ = r.shape
    if p.shape[0] != B:
        raise ValueError(f"pos has {p.shape[0]} batches for {B} images")
    V = p.shape[1]
    f, narrow, _, _ = _faces(tri, V)
    F, dev = narrow.shape[0], r.device
    out = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().ls_mip_pixel_differentials(_native.ptr(r), _native.ptr(_plain(p, 16)), B, V, _native.ptr(narrow), F, H, W,
                                                               _native.ptr(out), dev.index, _native.stream_of(dev)))
    return out


def _resolve_db(rast_db, rast):
    """the differentials behind a rast_db: an ordinary tensor as it is, the placeholder of `rasterize` through `pixel_differentials`"""
    if not isinstance(rast_db, torch.Tensor):
        raise TypeError(f"rast_db must be a torch.Tensor, got {type(rast_db).__name__}")
    src = getattr(rast_db, "_largesteps_db", None)
    if src is None or src.version != rast_db._version:
        if tuple(rast_db.shape) != tuple(rast.shape):
            raise ValueError(f"rast_db must have the shape of rast {tuple(rast.shape)}, got {tuple(rast_db.shape)}")
        return _plain(rast_db.detach().to(torch.float32), 16)
    if src.pos._version != src.pos_version:
        raise ValueError("pos was changed in place after rasterize: its rast_db can no longer give the pixel differentials")
    if torch.cuda.is_current_stream_capturing():
        return pixel_differentials(rast, src.pos, src.tri)
    if src.db is None:
        src.db = pixel_differentials(rast, src.pos, src.tri)
    return src.db


def _attr_da(attr, rast, tri, db, diff_attrs):
    r = _rast(rast)
    B, H, W, _ = r.shape
    a = (attr.unsqueeze(0) if attr.dim() == 2 else attr).detach()
    if a.dtype != torch.float32 or not a.is_contiguous():
        a = a.to(torch.float32).contiguous()
    Ba, V, C = a.shape
    if isinstance(diff_attrs, str):
        if diff_attrs != 'all':
            raise ValueError(f"diff_attrs must be 'all' or a list of channel indices, got {diff_attrs!r}")
        sel = None
    else:
        sel = [int(c) for c in diff_attrs]
        for c in sel:
            if not 0 <= c < C:
                raise IndexError(f"diff_attrs: channel {c} is outside [0, {C})")
    f, narrow, _, _ = _faces(tri, V)
    F, dev = narrow.shape[0], r.device
    out = torch.empty((B, H, W, 2 * C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().ls_mip_interpolate_da(_native.ptr(a), Ba, V, C, _native.ptr(r), _native.ptr(db), B, H, W, _native.ptr(narrow), F,
                                                          _native.ptr(out), dev.index, _native.stream_of(dev)))
    if sel is None or sel == list(range(C)):
        return out
    return torch.cat([out[..., 2 * c:2 * c + 2] for c in sel], dim=-1)


class _Interpolate(Function):
    @staticmethod
    def forward(ctx, attr, rast, tri, frame):
        _native.require_device(attr, "attr")
        r = _rast(rast)
        B, H, W, _ = r.shape
        if attr.dim() == 2:
            a3 = attr.unsqueeze(0)
        elif attr.dim() == 3:
            a3 = attr
        else:
            raise ValueError(f"attr must be (V, C), (1, V, C) or (B, V, C), got {tuple(attr.shape)}")
        if a3.shape[0] not in (1, B):
            raise ValueError(f"attr has {a3.shape[0]} batches for {B} images")
        a = a3.detach()
        if a.dtype != torch.float32 or not a.is_contiguous():
            a = a.to(torch.float32).contiguous()
        Ba, V, C = a.shape
        f, narrow, vptr, order = frame.faces(tri, V)
        F, dev = narrow.shape[0], r.device
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):          # in range mode too: ids are global and attr is shared (Ba = 1), the instanced kernel as it is
            _native.check(_native.lib().ls_raster_interpolate(_native.ptr(a), Ba, V, C, _native.ptr(r), B, H, W, _native.ptr(narrow), F,
                                                              _native.ptr(out), dev.index, _native.stream_of(dev)))
        ctx.save_for_backward(a, r, narrow, vptr, order)
        ctx.frame = frame
        ctx.rast_version = rast._version
        ctx.attr_shape = tuple(attr.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        need_attr, need_rast = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_attr or need_rast):
            return None, None, None, None
        a, r, narrow, vptr, corner_order = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        ga = torch.empty_like(a) if need_attr else None
        gr = torch.empty(r.shape, dtype=torch.float32, device=r.device) if need_rast else None
        with torch.cuda.device(r.device):
            ctx.frame.interpolate_backward(a, r, narrow, g, vptr, corner_order, ga, gr, ctx.rast_version)
        return (ga.view(ctx.attr_shape) if need_attr else None), gr, None, None


@_native.retry_on_oom
def interpolate(attr, rast, tri, rast_db=None, diff_attrs=None):
    """
    Interpolate vertex attributes over the rasterized images (nvdiffrast.torch.interpolate). Returns (out, attr_da); attr_da is None
    unless diff_attrs is given.

    attr : (V, C), (1, V, C) (shared by every image, as the reference passes it) or (B, V, C) fp32
    rast : the first output of `rasterize`. The rast of a range-mode call (it carries the range table; pass the very tensor `rasterize`
           returned) takes attr (V, C) or (1, V, C) only, indexed by the global vertex ids of tri; the slice law of the module's docstring
           holds for out and for both gradients. diff_attrs is not supported with it (NotImplementedError).
    tri : the faces given to `rasterize`
    rast_db : the second output of `rasterize` (the differentials are then computed from its frame, once, by `pixel_differentials`) or
              an ordinary (B, H, W, 4) tensor of (du/dX, du/dY, dv/dX, dv/dY), used as given. Needed only with diff_attrs.
    diff_attrs : None, 'all' or a list of K channel indices in [0, C)

    out (B, H, W, C) = u a0 + v a1 + (1 - u - v) a2 per covered pixel, 0 for background. Gradients flow to attr and to rast[..., :2].
    attr_da (B, H, W, 2 K) = [da_c/dX, da_c/dY] per selected channel, in order: da/dX = du/dX (a0 - a2) + dv/dX (a1 - a2), 0 for
    background. For a two-channel uv attribute it is the uv_da of `texture`. It is not differentiable (see `pixel_differentials`).
    """
    if diff_attrs is not None and rast_db is None:
        raise ValueError("largesteps.render.interpolate: diff_attrs needs rast_db (the second output of rasterize)")
    frame = _range_frame(rast)
    if frame is None:
        frame = _instanced_frame(rast, tri)
    elif diff_attrs is not None:
        raise NotImplementedError("largesteps.render.interpolate: diff_attrs is not supported for a rast of range mode (ranges=...)")
    elif not isinstance(attr, torch.Tensor) or attr.dim() not in (2, 3) or (attr.dim() == 3 and attr.shape[0] != 1):
        raise ValueError("attr must be (V, C) or (1, V, C) for a rast of range mode (the images share one vertex array), got "
                         f"{tuple(attr.shape) if isinstance(attr, torch.Tensor) else type(attr).__name__}")
    out = _Interpolate.apply(attr, rast, tri, frame)
    rast._largesteps_frame = frame
    if diff_attrs is None:
        return out, None
    with torch.no_grad():
        return out, _attr_da(attr, rast, tri, _resolve_db(rast_db, rast), diff_attrs)


class _Antialias(Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, boost, frame):
        _native.require_device(color, "color")
        r = _rast(rast)
        p = frame.pos(pos)
        B, H, W, _ = r.shape
        if color.dim() != 4 or tuple(color.shape[:3]) != (B, H, W):
            raise ValueError(f"color must be ({B}, {H}, {W}, C), got {tuple(color.shape)}")
        if frame.images(p) != B:
            raise ValueError(f"pos has {p.shape[0]} batches for {B} images")
        c = color.detach()
        if c.dtype != torch.float32 or not c.is_contiguous():
            c = c.to(torch.float32).contiguous()
        f, narrow, vptr, order = frame.faces(tri, p.shape[-2])
        adj = frame.adjacency(f, narrow)
        out, dev = torch.empty_like(c), r.device
        with torch.cuda.device(dev):
            frame.antialias(c, r, p, narrow, adj, B, H, W, out, dev)
        ctx.save_for_backward(c, r, p, narrow, adj, vptr, order)
        ctx.boost = float(boost)
        ctx.frame = frame
        ctx.rast_version = rast._version
        return out

    @staticmethod
    def backward(ctx, g):
        need_color, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if not (need_color or need_pos):
            return None, None, None, None, None, None
        c, r, p, narrow, adj, vptr, corner_order = ctx.saved_tensors
        (B, H, W, C), dev, frame = c.shape, c.device, ctx.frame
        g = g.to(torch.float32).contiguous()
        gc = torch.empty_like(c) if need_color else None
        gp = torch.empty_like(p) if need_pos else None
        order = seg = ws = None
        if need_pos:
            order, seg = frame.pixel_order(r, ctx.rast_version)
            ws = frame.workspace(B, H, W, 0, dev)
        with torch.cuda.device(dev):
            frame.antialias_backward(c, r, p, narrow, adj, B, H, W, C, g, ctx.boost, order, seg, vptr, corner_order, gc, gp, ws, dev)
        return gc, None, gp, None, None, None


@_native.retry_on_oom
def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
    """
    Analytic silhouette antialiasing (nvdiffrast.torch.antialias; Laine et al. 2020). Returns the blended (B, H, W, C) image.

    For every horizontally or vertically adjacent pixel pair with different triangle ids, the triangle t of the nearer pixel
    (background is infinitely far) is searched for a silhouette edge -- a mesh-boundary edge, or one whose neighbour triangle has the
    opposite screen-space winding in this view -- whose projection crosses the segment between the two pixel centres, at distance
    alpha (pixels) from the nearer centre. Then, with c_n / c_o the colours of the nearer / other pixel:
        alpha > 1/2: other += (alpha - 1/2) (c_n - c_o)        alpha < 1/2: nearer += (1/2 - alpha) (c_o - c_n)
    which makes the image continuous in the vertex positions. Gradients flow to color and to pos (the latter scaled by
    pos_gradient_boost). topology_hash is accepted and ignored (the edge adjacency is cached per face tensor).

    Range mode: pos (V, 4) and the rast that the range-mode `rasterize` returned (the tensor itself: it carries the range table). The
    silhouette test then uses each image's own faces -- the neighbour across an edge within tri[start_b : start_b + count_b], cached per
    (face tensor, ranges tensor) -- and the slice law of the module's docstring holds for the image and for both gradients.
    """
    frame = _range_frame(rast)
    if isinstance(pos, torch.Tensor) and pos.dim() == 2:
        if frame is None:
            raise ValueError("largesteps.render.antialias: a (V, 4) pos is range mode and needs the range table that its rast carries: pass "
                             "the tensor that rasterize(..., ranges=...) returned (not a copy of it)")
    elif frame is not None:
        raise ValueError(f"rast comes from a range-mode rasterize: pos must be the (V, 4) positions given to it, got "
                         f"{tuple(pos.shape) if isinstance(pos, torch.Tensor) else type(pos).__name__}")
    else:
        frame = _instanced_frame(rast, tri)
    out = _Antialias.apply(color, rast, pos, tri, float(pos_gradient_boost), frame)
    rast._largesteps_frame = frame
    return out


_FILTER_MODES = {'nearest': 0, 'linear': 1, 'auto': 1}                  # LS_TEXTURE_* of the header
_BOUNDARY_MODES = {'wrap': 0, 'clamp': 1, 'zero': 2}
_MIP_FILTER_MODES = {'linear-mipmap-nearest': 0, 'linear-mipmap-linear': 1}     # LS_MIP_* of the header
TEXTURE_MAX_SIZE = 8192                                                 # texels per side
TEXTURE_MAX_CHANNELS = 32


def _mip_keys(Bt, Ht, Wt, Lmax, mode, bnd):
    return Bt * sum((max(Ht >> l, 1) + 1) * (max(Wt >> l, 1) + 1) for l in range(Lmax + 1))


# What differs between the three lookups above the kernels. For the item order: the attribute it is cached under on the uv tensor (one
# each, so that a uv used by two kinds of lookup keeps both orders), how many leading arguments are the tensors whose versions form the
# key, the native workspace and order functions, the items per pixel and the number of keys (both from the integers that follow the
# tensors: the texture's sizes and the modes). For `_Texture`: the native lookup, (Bt, sizes) of a texture's shape, uv's alignment.
_Lookup = collections.namedtuple("_Lookup", "attr tensors workspace order items nkeys forward backward dims uv_align", defaults=(None,) * 4)
_TEXEL = _Lookup("_largesteps_texel_order", 1, "ls_texture_workspace_bytes", "ls_texture_order", lambda Bt, Ht, Wt, filt, bnd: 1,
                 lambda Bt, Ht, Wt, filt, bnd: Bt * (Ht + 1) * (Wt + 1), "ls_texture_forward", "ls_texture_backward", lambda shape: shape[:3], 16)
_MIP = _Lookup("_largesteps_mip_order", 3, "ls_mip_workspace_bytes", "ls_mip_order", lambda Bt, Ht, Wt, Lmax, mode, bnd: 2 if mode == 1 else 1, _mip_keys)
_CUBE = _Lookup("_largesteps_cube_order", 1, "ls_cube_workspace_bytes", "ls_cube_order", lambda Bt, n, filt: 4 if filt == 1 else 1,
                lambda Bt, n, filt: 6 * Bt * n * n, "ls_cube_forward", "ls_cube_backward", lambda shape: (shape[0], shape[2]), 4)


class _Order:
    """The items of one lookup in the order the gradient to the texels sums them in: the pixels of a uv image sorted by their base tap
    (`_TEXEL`), its (pixel, level) items sorted by (level, base tap) (`_MIP`: two items per pixel for 'linear-mipmap-linear'), its
    (pixel, tap) items sorted by their destination texel (`_CUBE`: four items per pixel for 'linear'). It depends on uv (and uv_da and the
    bias), the texture's shape and the modes, not on the texture's values: made at most once per uv tensor and version, by the first
    backward that needs it, and shared through the uv tensor (a fixed uv -- backgrounds, texture fitting on fixed geometry -- sorts
    once)."""
    __slots__ = ("kind", "key", "order", "seg")

    def __init__(self, kind, key):
        self.kind, self.key, self.order, self.seg = kind, key, None, None

    def get(self, *args):
        """args: the kind's tensors as the kernels get them (uv first), then the integers of its native order function"""
        if self.order is None:
            kind, lib = self.kind, _native.lib()
            tensors, conf = args[:kind.tensors], args[kind.tensors:]
            B, H, W, _ = tensors[0].shape
            dev = tensors[0].device
            ws = _native.workspace(kind.workspace, (B, H, W), dev)
            order = torch.empty(kind.items(*conf) * B * H * W, dtype=torch.int32, device=dev)
            seg = torch.empty(kind.nkeys(*conf) + 1, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _native.check(getattr(lib, kind.order)(*map(_native.ptr, tensors), B, H, W, *conf, _native.ptr(order), _native.ptr(seg),
                                                       _native.ptr(ws), ws.numel(), dev.index, _native.stream_of(dev)))
            self.order, self.seg = order, seg
        return self.order, self.seg


_TexelOrder, _CubeOrder = functools.partial(_Order, _TEXEL), functools.partial(_Order, _CUBE)


def _order_slot(kind, tensors, conf):
    # while a graph is being captured the order is neither taken from the tensor nor left on it: a replay must sort the uv it finds
    # (a captured body may read a uv that is updated in place between replays), and memory of the graph's pool must not outlive it
    if torch.cuda.is_current_stream_capturing():
        return _Order(kind, None)
    key = sum(((None,) if t is None else (t._version, t.data_ptr(), tuple(t.shape), tuple(t.stride())) for t in tensors), ()) + tuple(conf)
    slot = getattr(tensors[0], kind.attr, None)
    if slot is not None and slot.key == key:
        return slot
    return _Order(kind, key)


def _lookup(kind, fn, tensors, conf, *args):
    """fn.apply(*args, slot) with the order slot of (tensors, conf); the slot stays on uv = tensors[0] if it has a key"""
    slot = _order_slot(kind, tensors, conf)
    out = fn.apply(*args, slot)
    if slot.key is not None:
        setattr(tensors[0], kind.attr, slot)
    return out


def _grad_buffers(g, *wanted):
    """the upstream gradient made plain, then an empty gradient like t for every (t, needed) with needed set, else None"""
    return (_plain(g.to(torch.float32), 16),) + tuple(torch.empty_like(t) if needed else None for t, needed in wanted)


def _views(grads, shapes):
    """the gradients in the shapes the caller's tensors had"""
    return tuple(None if x is None else x.view(shape) for x, shape in zip(grads, shapes))


class _Texture(Function):
    """the plain 2D lookup (`_TEXEL`) and the cube-map lookup (`_CUBE`); modes = (filter, boundary) and (filter,)"""
    @staticmethod
    def forward(ctx, tex, uv, kind, modes, slot):
        t, u = _plain(tex, 16), _plain(uv, kind.uv_align)
        dims, C = kind.dims(t.shape), t.shape[-1]
        B, H, W, _ = u.shape
        dev = u.device
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check(getattr(_native.lib(), kind.forward)(_native.ptr(t), *dims, C, _native.ptr(u), B, H, W, *modes, _native.ptr(out),
                                                               dev.index, _native.stream_of(dev)))
        ctx.save_for_backward(t, u)
        ctx.conf = (kind, dims, modes)
        ctx.slot = slot
        ctx.shapes = (tuple(tex.shape), tuple(uv.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        need_tex, need_uv = ctx.needs_input_grad[:2]
        if not (need_tex or need_uv):
            return (None,) * 5
        t, u = ctx.saved_tensors
        kind, dims, modes = ctx.conf
        C = t.shape[-1]
        B, H, W, _ = u.shape
        dev = u.device
        g, gt, gu = _grad_buffers(g, (t, need_tex), (u, need_uv))
        order = seg = None
        if need_tex:
            order, seg = ctx.slot.get(u, *dims, *modes)
        with torch.cuda.device(dev):
            _native.check(getattr(_native.lib(), kind.backward)(_native.ptr(t), *dims, C, _native.ptr(u), B, H, W, *modes, _native.ptr(g),
                                                                _native.ptr(order), _native.ptr(seg), _native.ptr(gt), _native.ptr(gu),
                                                                dev.index, _native.stream_of(dev)))
        return _views((gt, gu), ctx.shapes) + (None, None, None)


def _mip_last_level(Ht, Wt, max_mip_level=None):
    """the last level of the pyramid of an Ht x Wt texture: 1 x 1, or max_mip_level if that comes first. Every level that is halved
    must have sides that are 1 or even."""
    if max_mip_level is not None and int(max_mip_level) < 0:
        raise ValueError(f"max_mip_level must not be negative, got {max_mip_level}")
    h, w, level = int(Ht), int(Wt), 0
    while (h > 1 or w > 1) and (max_mip_level is None or level < int(max_mip_level)):
        if (h > 1 and h % 2) or (w > 1 and w % 2):
            raise ValueError(f"mip level {level} is {h} x {w} texels: each side must be 1 or even to build level {level + 1} "
                             f"(pass max_mip_level={level} to stop here)")
        h, w, level = max(h // 2, 1), max(w // 2, 1), level + 1
    return level


def _mip_texels(Ht, Wt, first, last):
    """texels per batch entry of levels first .. last"""
    return sum(max(Ht >> l, 1) * max(Wt >> l, 1) for l in range(first, last + 1))


class _Mip:
    """The opaque result of `texture_construct_mip`: levels 1 .. Lmax of one texture in one packed device buffer, and the identity of the
    texture they were built from."""
    __slots__ = ("shape", "Lmax", "pyr", "version", "ptr")

    def __init__(self, tex, Lmax, pyr):
        self.shape, self.Lmax, self.pyr, self.version, self.ptr = tuple(tex.shape), Lmax, pyr, tex._version, tex.data_ptr()

    def check(self, tex):
        if tuple(tex.shape) != self.shape or tex.data_ptr() != self.ptr or tex._version != self.version:
            raise ValueError("the mip object is stale: it was built from another texture, or the texture was changed in place since; "
                             "call texture_construct_mip again (or pass mip=None)")


def _check_tex(tex):
    if not isinstance(tex, torch.Tensor):
        raise TypeError(f"tex must be a torch.Tensor, got {type(tex).__name__}")
    if tex.dtype != torch.float32:
        raise TypeError(f"tex must be float32, got {tex.dtype}")
    if tex.dim() != 4:
        raise ValueError(f"tex must be (1 or B, Ht, Wt, C), got {tuple(tex.shape)}")
    Bt, Ht, Wt, C = tex.shape
    if Bt < 1:
        raise ValueError(f"tex must not be empty, got {tuple(tex.shape)}")
    if not (1 <= Ht <= TEXTURE_MAX_SIZE and 1 <= Wt <= TEXTURE_MAX_SIZE):
        raise ValueError(f"the texture must be between 1 and {TEXTURE_MAX_SIZE} texels a side, got {Ht} x {Wt}")
    if not 1 <= C <= TEXTURE_MAX_CHANNELS:
        raise ValueError(f"the texture must have between 1 and {TEXTURE_MAX_CHANNELS} channels, got {C}")


def _build_pyramid(t, Lmax):
    """levels 1 .. Lmax of the contiguous texture t, packed"""
    Bt, Ht, Wt, C = t.shape
    dev = t.device
    pyr = torch.empty(max(Bt * _mip_texels(Ht, Wt, 1, Lmax) * C, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().ls_mip_build(_native.ptr(t), Bt, Ht, Wt, C, Lmax, _native.ptr(pyr), dev.index, _native.stream_of(dev)))
    return pyr


@_native.retry_on_oom
def texture_construct_mip(tex, max_mip_level=None, cube_mode=False):
    """
    The mipmap pyramid of a texture (nvdiffrast.torch.texture_construct_mip): an opaque object for `texture(..., mip=...)`, worth
    building when one texture is looked up several times unchanged.

    Level 0 is tex; level l + 1 has max(W_l / 2, 1) x max(H_l / 2, 1) texels, each the mean of its 2 x 2 children (2 x 1 or 1 x 2 when
    one side is already 1), fp32 as ((c00 + c10) + (c01 + c11)) * 0.25 and (a + b) * 0.5. The last level is 1 x 1, or max_mip_level if
    that comes first; a level that is halved must have sides that are 1 or even (ValueError). The object remembers the texture's
    version: after an in-place change of tex it is stale and `texture` raises ValueError. Gradients do not flow through the object
    itself -- `texture` sends the gradient of every level back to tex on its own.
    """
    if cube_mode:
        raise NotImplementedError("largesteps.render.texture_construct_mip: cube_mode=True (mipmapped cube maps) is not supported; "
                                  "texture(..., boundary_mode='cube') looks a cube map up without mipmaps")
    _check_tex(tex)
    Lmax = _mip_last_level(tex.shape[1], tex.shape[2], max_mip_level)
    if not tex.is_cuda:
        raise NotImplementedError("largesteps.render.texture_construct_mip: the mipmap pyramid needs a HIP device")
    return _Mip(tex, Lmax, _build_pyramid(_plain(tex, 16), Lmax))


class _TextureMip(Function):
    @staticmethod
    def forward(ctx, tex, uv, uv_da, bias, pyr, Lmax, mode, bnd, slot):
        t, u, da, b = _plain(tex, 16), _plain(uv, 16), _plain(uv_da, 16), _plain(bias, 4)
        Bt, Ht, Wt, C = t.shape
        B, H, W, _ = u.shape
        dev = u.device
        if pyr is None:
            pyr = _build_pyramid(t, Lmax)
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check(_native.lib().ls_mip_forward(_native.ptr(t), _native.ptr(pyr), Bt, Ht, Wt, C, Lmax, _native.ptr(u), _native.ptr(da),
                                                       _native.ptr(b), B, H, W, mode, bnd, _native.ptr(out), dev.index, _native.stream_of(dev)))
        ctx.save_for_backward(t, pyr, u, da, b)
        ctx.conf = (Lmax, mode, bnd)
        ctx.slot = slot
        ctx.shapes = (tuple(tex.shape), tuple(uv.shape), None if uv_da is None else tuple(uv_da.shape), None if bias is None else tuple(bias.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        need_tex, need_uv, need_da, need_bias = ctx.needs_input_grad[:4]
        if not (need_tex or need_uv or need_da or need_bias):
            return (None,) * 9
        t, pyr, u, da, b = ctx.saved_tensors
        Lmax, mode, bnd = ctx.conf
        Bt, Ht, Wt, C = t.shape
        B, H, W, _ = u.shape
        dev = u.device
        g, gt, gpyr, gu = _grad_buffers(g, (t, need_tex), (pyr, need_tex), (u, need_uv))
        glod = torch.empty((B, H, W), dtype=torch.float32, device=dev) if (need_da or need_bias) else None
        gda = torch.empty_like(da) if need_da else None
        order = seg = None
        if need_tex:
            order, seg = ctx.slot.get(u, da, b, Bt, Ht, Wt, Lmax, mode, bnd)
        lib = _native.lib()
        with torch.cuda.device(dev):
            st = _native.stream_of(dev)
            _native.check(lib.ls_mip_backward(_native.ptr(t), _native.ptr(pyr), Bt, Ht, Wt, C, Lmax, _native.ptr(u), _native.ptr(da), _native.ptr(b),
                                              B, H, W, mode, bnd, _native.ptr(g), _native.ptr(order), _native.ptr(seg), _native.ptr(gt),
                                              _native.ptr(gpyr), _native.ptr(gu), _native.ptr(glod), _native.ptr(gda), dev.index, st))
            if need_tex and Lmax > 0:
                _native.check(lib.ls_mip_fold(_native.ptr(gt), Bt, Ht, Wt, C, Lmax, _native.ptr(gpyr), dev.index, st))
        return _views((gt, gu, gda, glod if need_bias else None), ctx.shapes) + (None,) * 5


def _check_mip_inputs(uv, uv_da, mip_level_bias):
    """the level-of-detail inputs of a mipmapped lookup against uv (B, H, W, 2)"""
    if uv_da is None and mip_level_bias is None:
        raise ValueError("largesteps.render.texture: the mipmap filter modes need uv_da or mip_level_bias (or both) to choose a level")
    B, H, W, _ = uv.shape
    for t, what, shape in ((uv_da, "uv_da", (B, H, W, 4)), (mip_level_bias, "mip_level_bias", (B, H, W))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what} must be float32, got {t.dtype}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{what} must be {shape}, got {tuple(t.shape)}")
        if t.device != uv.device:
            raise ValueError(f"{what} is on {t.device}, uv on {uv.device}")


def _texture_mip(tex, uv, uv_da, mip_level_bias, mip, mode, bnd, max_mip_level):
    _check_mip_inputs(uv, uv_da, mip_level_bias)
    Bt, Ht, Wt, C = tex.shape
    if 2 * uv.shape[0] * uv.shape[1] * uv.shape[2] >= 2 ** 31 - 1:
        raise OverflowError(f"uv has {uv.numel() // 2} pixels: the mipmapped lookup indexes two items per pixel with int32")
    if mip is not None:
        if not isinstance(mip, _Mip):
            raise TypeError(f"mip must come from texture_construct_mip, got {type(mip).__name__}")
        mip.check(tex)
        Lmax = mip.Lmax if max_mip_level is None else min(mip.Lmax, _mip_last_level(Ht, Wt, max_mip_level))
        pyr = mip.pyr
    else:
        Lmax, pyr = _mip_last_level(Ht, Wt, max_mip_level), None
    return _lookup(_MIP, _TextureMip, (uv, uv_da, mip_level_bias), (Bt, Ht, Wt, Lmax, mode, bnd), tex, uv, uv_da, mip_level_bias, pyr, Lmax, mode, bnd)


def _check_lookup(tex, uv, cube):
    """what `texture` checks of tex and uv for the 2D lookups and for the cube lookup, in the order its docstring gives"""
    for t, what in ((tex, "tex"), (uv, "uv")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what} must be float32, got {t.dtype}")
    if cube:
        if tex.dim() != 5 or tex.shape[1] != 6 or tex.shape[2] != tex.shape[3]:
            raise ValueError(f"a cube map must be (1 or B, 6, n, n, C) with square faces, got {tuple(tex.shape)}")
        if uv.dim() != 4 or uv.shape[3] != 3:
            raise ValueError(f"uv must be (B, H, W, 3) directions for boundary_mode='cube', got {tuple(uv.shape)}")
    else:
        if tex.dim() != 4:
            raise ValueError(f"tex must be (1 or B, Ht, Wt, C), got {tuple(tex.shape)}")
        if uv.dim() != 4 or uv.shape[3] != 2:
            raise ValueError(f"uv must be (B, H, W, 2), got {tuple(uv.shape)}")
    Bt, (Ht, Wt, C) = tex.shape[0], tex.shape[-3:]
    B, H, W, _ = uv.shape
    if Bt not in (1, B):
        raise ValueError(f"tex has {Bt} batches for {B} images")
    if not (1 <= Ht <= TEXTURE_MAX_SIZE and 1 <= Wt <= TEXTURE_MAX_SIZE):
        raise ValueError(f"a cube face must be between 1 and {TEXTURE_MAX_SIZE} texels a side, got {Ht}" if cube else
                         f"the texture must be between 1 and {TEXTURE_MAX_SIZE} texels a side, got {Ht} x {Wt}")
    if not 1 <= C <= TEXTURE_MAX_CHANNELS:
        raise ValueError(f"the texture must have between 1 and {TEXTURE_MAX_CHANNELS} channels, got {C}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"uv must not be empty, got {tuple(uv.shape)}")
    if (4 if cube else 1) * B * H * W >= 2 ** 31 - 1:
        raise OverflowError(f"uv has {B * H * W} pixels: " + ("the cube lookup indexes four items per pixel with int32" if cube else
                                                              "the kernels index them with int32"))
    if cube and 6 * Bt * Ht * Ht >= 2 ** 31 - 2:
        raise OverflowError(f"the cube maps have {6 * Bt * Ht * Ht} texels: the kernels index them with int32")
    if tex.device != uv.device:
        raise ValueError(f"tex is on {tex.device}, uv on {uv.device}")


def _texture_cube(tex, uv, filter_mode):
    """texture(..., boundary_mode='cube'): the checks in the order the docstring of `texture` gives, then the native lookup"""
    if any(isinstance(t, torch.Tensor) and not t.is_cuda for t in (tex, uv)):
        raise NotImplementedError("largesteps.render.texture: boundary_mode='cube' (cube maps) needs a HIP device")
    if filter_mode in _MIP_FILTER_MODES:
        raise NotImplementedError(f"largesteps.render.texture: filter_mode={filter_mode!r} with boundary_mode='cube' (mipmapped cube maps) "
                                  "is not supported; use 'linear' or 'nearest'")
    if filter_mode not in _FILTER_MODES:
        raise ValueError(f"filter_mode must be one of {sorted(_FILTER_MODES)}, got {filter_mode!r}")
    _check_lookup(tex, uv, True)
    filt = _FILTER_MODES[filter_mode]
    return _lookup(_CUBE, _Texture, (uv,), (tex.shape[0], tex.shape[2], filt), tex, uv, _CUBE, (filt,))


def _texture_cpu(tex, uv):
    """the lookup in plain torch, linear + wrap, forward only: what a CPU tensor gets (the device kernel keeps this operation order)"""
    with torch.no_grad():
        Ht, Wt = tex.shape[1], tex.shape[2]
        x = uv[..., 0] * Wt - 0.5
        y = uv[..., 1] * Ht - 0.5
        x0, y0 = torch.floor(x), torch.floor(y)
        fx, fy = (x - x0)[..., None], (y - y0)[..., None]
        i0 = torch.remainder(x0.long(), Wt)
        j0 = torch.remainder(y0.long(), Ht)
        i1, j1 = torch.remainder(i0 + 1, Wt), torch.remainder(j0 + 1, Ht)
        B = uv.shape[0]
        t = tex if tex.shape[0] == B else tex.expand(B, *tex.shape[1:])
        bi = torch.arange(B, device=uv.device).view(B, *([1] * (uv.dim() - 2)))
        t00, t10 = t[bi, j0, i0], t[bi, j0, i1]
        t01, t11 = t[bi, j1, i0], t[bi, j1, i1]
        top = t00 + (t10 - t00) * fx
        bot = t01 + (t11 - t01) * fx
        return top + (bot - top) * fy


@_native.retry_on_oom
def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode='linear', boundary_mode='wrap', max_mip_level=None):
    """
    2D texture lookup (nvdiffrast.torch.texture): tex (1 or B, Ht, Wt, C), uv (B, H, W, 2) -> (B, H, W, C), all fp32.

    filter_mode : 'linear' (bilinear), 'nearest', 'auto' (= 'linear'), 'linear-mipmap-linear' (trilinear), 'linear-mipmap-nearest'.
    boundary_mode : 'wrap', 'clamp' or 'zero', applied to each tap index: modulo the size; clamped to [0, size - 1]; a tap outside
                    reads 0 and receives no gradient. 'cube': a cube-map lookup by direction (below).
    uv_da, mip_level_bias, mip, max_mip_level : the mipmap modes' inputs (below); accepted and ignored by the other modes.

    Cube maps (boundary_mode='cube', HIP device only; csrc/cube.hip, restated by tests/cube_statement.py). tex (1 or B, 6, n, n, C), faces
    in the order +x, -x, +y, -y, +z, -z (OpenGL's), uv (B, H, W, 3): a direction d = (x, y, z) that need not be normalised.
    filter_mode 'nearest', 'linear' or 'auto'; a mipmap filter mode raises NotImplementedError (mipmapped cube maps are not supported).
    The major axis is x if |x| >= |y| and |x| >= |z|, else y if |y| >= |z|, else z; its sign picks the face, and with (sc, tc, ma) =
    (-z, -y, x) (z, -y, x) (x, z, y) (x, -z, y) (x, -y, z) (-x, -y, z) for the six faces s = (sc / |ma| + 1) / 2, t = (tc / |ma| + 1) / 2
    are the face coordinates, looked up as a 2D texture of n x n texels: a pixel whose four taps lie inside the face is bit for bit
    texture(tex[:, f], (s, t), 'linear', 'clamp'). A linear tap one texel outside the face reads the texel of the neighbouring face
    that contains the centre of that outside texel (filtering is seamless across the 12 edges); a tap outside in both directions (at
    one of the 8 corners) has no texel, and its weight is shared evenly by the other three. A direction with a non-finite component, or
    (0, 0, 0), gives 0 and no gradient. Gradients flow to tex and (linear) to uv -- with the face choice held fixed, perpendicular to d
    -- without float atomics; the item order is cached per uv tensor and version. Checks, in this order: tensors that are not on a HIP
    device raise NotImplementedError; types and dtypes (TypeError); tex (1 or B, 6, n, n, C) with square faces and uv (B, H, W, 3)
    (ValueError); the batch, size and channel limits (ValueError) and 4 B H W, 6 Bt n^2 < 2^31 (OverflowError).

    Mipmap modes (HIP device only). uv_da (B, H, W, 4) = (du/dX, du/dY, dv/dX, dv/dY) in texture units per pixel (the second output of
    `interpolate(uv_attr, rast, tri, rast_db, diff_attrs='all')`), mip_level_bias (B, H, W); one may be None, not both. mip: a pyramid
    from `texture_construct_mip` (built here otherwise; see there for its rules), max_mip_level: the last level Lmax to use.
    With sx = du/dX Wt, sy = du/dY Wt, tx = dv/dX Ht, ty = dv/dY Ht, A = sx^2 + tx^2, B = sy^2 + ty^2, Cc = sx sy + tx ty:
    m = (A + B) / 2 + sqrt((A - B)^2 / 4 + Cc^2) is the squared major axis of the pixel's footprint in level-0 texels and
    lod = log2(m) / 2 + bias (the bias alone without uv_da), clamped to [0, Lmax]. 'linear-mipmap-linear': l0 = floor(lod),
    f = lod - l0, out = c0 + (c1 - c0) f with c_l the bilinear lookup of level l (when f = 0 or l0 = Lmax only l0 is read);
    'linear-mipmap-nearest': the level min(floor(lod + 1/2), Lmax). A non-finite uv, uv_da or bias gives 0 and no gradient. Gradients
    flow to tex through every level, to uv from both levels, and to mip_level_bias and uv_da through d out / d lod = c1 - c0 (zero where
    lod was clamped and in 'linear-mipmap-nearest').

    Texel (i, j) has its centre at ((i + 0.5) / Wt, (j + 0.5) / Ht). Linear: x = u Wt - 0.5, i0 = floor(x), fx = x - i0 (likewise y),
    out = top + (bot - top) fy with top = t00 + (t10 - t00) fx, bot = t01 + (t11 - t01) fx. Nearest: the texel (floor(u Wt), floor(v Ht)).
    A non-finite uv gives 0 and no gradient. Sizes: 1 <= Ht, Wt <= 8192, C <= 32, B H W < 2^31.

    Gradients flow to tex in every mode (summed over the images when tex has one batch entry) and to uv in linear mode (zero for
    'nearest'), without float atomics: bitwise reproducible. The pixel order the texture gradient sums in is cached per uv tensor
    and version. Tensors on a HIP device take the native path whether or not a gradient is wanted; CPU tensors get a plain-torch
    forward without gradient, for 'linear' + 'wrap' only.
    """
    mipmapped = filter_mode in _MIP_FILTER_MODES
    if mipmapped and not (isinstance(uv, torch.Tensor) and uv.is_cuda and isinstance(tex, torch.Tensor) and tex.is_cuda):
        raise NotImplementedError(f"largesteps.render.texture: filter_mode={filter_mode!r} (mipmaps) needs a HIP device")
    if boundary_mode == 'cube':
        return _texture_cube(tex, uv, filter_mode)
    if filter_mode not in _FILTER_MODES and not mipmapped:
        raise ValueError(f"filter_mode must be one of {sorted(_FILTER_MODES)}, got {filter_mode!r}")
    if boundary_mode not in _BOUNDARY_MODES:
        raise ValueError(f"boundary_mode must be one of {sorted(_BOUNDARY_MODES)}, got {boundary_mode!r}")
    _check_lookup(tex, uv, False)
    Bt, Ht, Wt, _ = tex.shape
    if mipmapped:
        return _texture_mip(tex, uv, uv_da, mip_level_bias, mip, _MIP_FILTER_MODES[filter_mode], _BOUNDARY_MODES[boundary_mode], max_mip_level)
    filt, bnd = _FILTER_MODES[filter_mode], _BOUNDARY_MODES[boundary_mode]
    if not uv.is_cuda:
        if (filt, bnd) != (1, 0):
            raise NotImplementedError("largesteps.render.texture: CPU tensors get filter_mode='linear' with boundary_mode='wrap' only; "
                                      "every other mode needs a HIP device")
        return _texture_cpu(tex, uv)
    return _lookup(_TEXEL, _Texture, (uv,), (Bt, Ht, Wt, filt, bnd), tex, uv, _TEXEL, (filt, bnd))


def persp_proj(fov_x=45, ar=1, near=0.1, far=100, device=None):
    """OpenGL-style perspective projection with the reference's sign conventions (x mirrored, w = view-space z): a (4, 4) fp32 tensor.
    fov_x: horizontal field of view in degrees, ar = width / height."""
    t = np.tan(np.deg2rad(fov_x) / 2.0)
    P = np.zeros((4, 4), dtype=np.float64)
    P[0, 0] = -1.0 / t
    P[1, 1] = float(np.float32(ar)) / t
    P[2, 2] = (far + near) / (far - near)
    P[2, 3] = 2.0 * far * near / (near - far)
    P[3, 2] = 1.0
    return torch.tensor(P, dtype=torch.float32, device=device)


class SphericalHarmonics:
    """
    Order-2 spherical-harmonic irradiance of an environment map (Ramamoorthi and Hanrahan 2001, "An efficient representation for
    irradiance environment maps"), with Y as the up axis. `M` is (3, 4, 4), one quadratic form per colour channel;
    `eval(n)` returns n_h^T M n_h for n_h = (n, 1).
    """

    # normalisation constants of the real spherical harmonics up to l = 2, and the irradiance-filter constants c1..c5 of the paper
    _K00, _K1, _K2a, _K2b, _K2c = 0.282095, 0.488603, 1.092548, 0.315392, 0.546274
    _C1, _C2, _C3, _C4, _C5 = 0.429043, 0.511664, 0.743125, 0.886227, 0.247708

    def __init__(self, envmap):
        h, w = envmap.shape[:2]
        dev = envmap.device
        theta = torch.linspace(0, np.pi, h, device=dev)[:, None].expand(h, w)            # polar angle per row
        phi = torch.linspace(3 * np.pi, np.pi, w, device=dev)[None, :].expand(h, w)      # azimuth per column
        st = torch.sin(theta)
        dx, dy, dz = st * torch.cos(phi), torch.cos(theta), -st * torch.sin(phi)
        # the nine basis functions: constant; z, x, y; 3 z^2 - 1, x z, x^2 - y^2, x y, y z
        basis = [None, self._K1 * dz, self._K1 * dx, self._K1 * dy,
                 self._K2b * (3 * dz.square() - 1), self._K2a * dx * dz, self._K2c * (dx.square() - dy.square()), self._K2a * dx * dy,
                 self._K2a * dy * dz]
        rad = envmap[..., :3]
        dw = 2.0 * np.pi ** 2 / (w * h)                        # solid-angle weight per texel (times sin theta)

        def coeff(y):
            if y is None:
                return (rad * self._K00 * st[..., None] * dw).sum(dim=(0, 1))
            return (rad * (y * st)[..., None] * dw).sum(dim=(0, 1))

        # projections of the radiance on the basis functions, named after their polynomial (zz: 3 z^2 - 1, xxyy: x^2 - y^2)
        Lc, Lz, Lx, Ly, Lzz, Lxz, Lxxyy, Lxy, Lyz = [coeff(y) for y in basis]
        # Ramamoorthi-Hanrahan eq. 12, with their z axis played by this frame's z and the (x, y, z, 1) ordering of n_h
        c1, c2, c3, c4, c5 = self._C1, self._C2, self._C3, self._C4, self._C5
        rows = [
            [c1 * Lxxyy, c1 * Lxy, c1 * Lxz, c2 * Lx],
            [c1 * Lxy, -c1 * Lxxyy, c1 * Lyz, c2 * Ly],
            [c1 * Lxz, c1 * Lyz, c3 * Lzz, c2 * Lz],
            [c2 * Lx, c2 * Ly, c2 * Lz, c4 * Lc - c5 * Lzz],
        ]
        self.M = torch.stack([torch.stack(r) for r in rows]).movedim(2, 0)

    def eval(self, n):
        nh = torch.nn.functional.pad(n.reshape(-1, 3), (0, 1), 'constant', 1.0).t()           # (4, N)
        return (nh * (self.M @ nh)).sum(dim=1).t().reshape(n.shape)


class NVDRenderer:
    """
    The reference's renderer (scripts/render.py) on this package's primitives: the same constructor keys (res_x, res_y, fov,
    near_clip, far_clip, view_mats, envmap, envmap_scale), the same images. Tensors stay on the device of the scene's tensors.

    shading : shade with the environment's SH irradiance over a background of the environment; otherwise white silhouettes
    boost : pos_gradient_boost of the antialiasing
    """

    def __init__(self, scene_params, shading=True, boost=1.0):
        near, far = scene_params["near_clip"], scene_params["far_clip"]
        self.fov_x = scene_params["fov"]
        w, h = scene_params["res_x"], scene_params["res_y"]
        self.res = (h, w)
        self.view_mats = torch.stack(list(scene_params["view_mats"]))
        dev = self.view_mats.device
        self.proj_mat = persp_proj(self.fov_x, w / h, near, far, device=dev)
        self.mvps = self.proj_mat @ self.view_mats
        self.boost = boost
        self.shading = shading
        self.glctx = RasterizeContext()
        envmap = scene_params['envmap_scale'] * scene_params['envmap']
        self.sh = SphericalHarmonics(envmap)
        self.render_backgrounds(envmap)

    def background_uvs(self):
        """the envmap coordinates of every pixel's view ray, (n_views, H, W, 2), before the vertical flip of the backgrounds"""
        h, w = self.res
        dev = self.view_mats.device
        idx = torch.arange(w * h, dtype=torch.int32, device=dev)
        pix = 0.5 - torch.stack((idx % w, idx // w), dim=1) / torch.tensor((w, h), device=dev)
        half = np.deg2rad(self.fov_x) / 2
        scale = torch.tensor((2 * np.tan(half), 2 * np.tan(half) / (w / h)), device=dev, dtype=torch.float32)
        rays = torch.cat((pix * scale, torch.ones((w * h, 1), device=dev), torch.zeros((w * h, 1), device=dev)), dim=1)
        rays = rays / torch.norm(rays, dim=1, keepdim=True)
        world = torch.matmul(rays, self.view_mats.inverse().transpose(1, 2)).reshape((self.view_mats.shape[0], h, w, -1))
        theta = torch.acos(world[..., 1])
        phi = torch.atan2(world[..., 0], world[..., 2])
        return torch.stack([0.75 - phi / (2 * np.pi), theta / np.pi], dim=-1)

    def render_backgrounds(self, envmap):
        self.bgs = texture(envmap[None, ...], self.background_uvs(), filter_mode='linear').flip(1)
        self.bgs[..., -1] = 0

    def render(self, v, n, f):
        """Images (n_views, H, W, 4) of the mesh (v, n, f) from every view, differentiable in v (and n when shading)."""
        v_ndc = torch.matmul(torch.nn.functional.pad(v, (0, 1), 'constant', 1.0), self.mvps.transpose(1, 2))
        rast = rasterize(self.glctx, v_ndc, f, self.res)[0]
        if self.shading:
            light = interpolate(self.sh.eval(n).contiguous()[None, ...], rast, f)[0]
            col = torch.cat((light / np.pi, torch.ones((*light.shape[:-1], 1), device=v.device)), dim=-1)
            return antialias(torch.where(rast[..., -1:] != 0, col, self.bgs), rast, v_ndc, f, pos_gradient_boost=self.boost)
        col = interpolate(torch.ones_like(v)[None, ...], rast, f)[0]
        return antialias(col, rast, v_ndc, f, pos_gradient_boost=self.boost)
