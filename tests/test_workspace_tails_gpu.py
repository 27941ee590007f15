"""No entry point writes past the workspace its size function asks for.

Python allocates exactly what a size function says, so a region that is carved but not counted would land in the allocator's padding and
no other test would see it. Here `_native.workspace` is replaced by one that hands out the first n bytes of a buffer 4096 bytes longer,
fills the tail with a fixed byte and remembers every buffer; a case runs one forward and backward through the public API at the smallest
shapes that still use every region, then every tail must still hold its byte. One case per family of csrc/ that carves a caller's
workspace through csrc/workspace.h. A write past the end lands in the test's own buffer. The library's own pool buffers (the mesh handle,
the bisection) are not seen here: the bitwise comparison of tools/dump_sort_users.py and the suite cover those."""
import math

import numpy as np
import pytest
import torch

import largesteps.render as dr
from largesteps import _native, distance, synthetic
from largesteps.geometry import compute_matrix
from largesteps.levelset import isosurface
from largesteps.meshops import average_edge_length, massmatrix_voronoi, remove_duplicates
from largesteps.normals import compute_face_normals, compute_vertex_normals
from largesteps.parameterize import to_differential
from largesteps.raycast import RayMesh
from largesteps.sampling import sample_surface

pytestmark = pytest.mark.gpu
TAIL, FILL = 4096, 0xA5


@pytest.fixture
def dev():
    return torch.device("cuda:0")


class Handed:
    """every workspace handed out: (size function, sizes, bytes asked, the whole buffer with its tail)"""

    def __init__(self):
        self.all = []

    def check(self, *expected):
        torch.cuda.synchronize()
        names = {h[0] for h in self.all}
        assert set(expected) <= names, f"the case did not allocate {sorted(set(expected) - names)} (it allocated {sorted(names)})"
        for name, sizes, n, buf in self.all:
            tail = buf[n:]
            assert tail.numel() == TAIL and bool((tail == FILL).all()), f"{name}{sizes}: a write past its {n} bytes"


@pytest.fixture
def handed(monkeypatch):
    h = Handed()

    def workspace(size_fn_name, sizes, device, nbytes=None):
        n = _native.workspace_bytes(size_fn_name, sizes) if nbytes is None else nbytes
        buf = torch.empty(n + TAIL, dtype=torch.uint8, device=device)
        buf[n:] = FILL
        h.all.append((size_fn_name, tuple(sizes), n, buf))
        return buf[:n]

    monkeypatch.setattr(_native, "workspace", workspace)
    return h


def sphere(dev, n=4, seed=0, grad=True):
    """a closed mesh of 20 n^2 faces (320), its vertices off the sphere so that no two faces are alike"""
    v, f = synthetic.icosphere(n)
    v = synthetic.perturb(v, radial=0.05, seed=seed).astype(np.float32)
    return torch.from_numpy(v).to(dev).requires_grad_(grad), torch.from_numpy(f).to(dev)


def weights(t, seed=1):
    g = torch.Generator(device=t.device)
    g.manual_seed(seed)
    return torch.randn(t.shape, generator=g, device=t.device, dtype=t.dtype)


def test_compute_matrix_and_the_transpose(dev, handed):
    v, f = sphere(dev, grad=False)
    for kw in (dict(lambda_=10.0), dict(lambda_=0.0, alpha=0.9, cotan=True)):
        M = compute_matrix(v, f, **kw).coalesce()
    scale = 1.0 + torch.rand(v.shape[0], device=dev)                 # rows scaled one by one: unsymmetric, the backward transposes
    L = torch.sparse_coo_tensor(M.indices(), M.values() * scale[M.indices()[0]], M.shape).coalesce()
    x = v.clone().requires_grad_(True)
    u = to_differential(L, x)
    (u * weights(u)).sum().backward()
    assert x.grad is not None
    handed.check("ls_assemble_workspace_bytes", "ls_csr_transpose_workspace_bytes")


def test_remove_duplicates_on_the_face_soup(dev, handed):
    v, f = sphere(dev, grad=False)
    soup = v[f.reshape(-1)].contiguous()
    vu, fu, _ = remove_duplicates(soup, torch.arange(soup.shape[0], device=dev).reshape(-1, 3))
    assert vu.shape[0] == v.shape[0] and fu.shape == f.shape
    handed.check("ls_remove_duplicates_workspace_bytes")


def test_both_normals_with_gradients(dev, handed):
    v, f = sphere(dev)
    fn = compute_face_normals(v, f)
    vn = compute_vertex_normals(v, f, fn)
    ((fn * weights(fn)).sum() + (vn * weights(vn, 2)).sum()).backward()
    assert v.grad is not None
    handed.check("ls_corner_ranks_workspace_bytes", "ls_normals_workspace_bytes")


def test_mass_matrix_and_edge_length_with_gradients(dev, handed):
    v, f = sphere(dev)
    mass, ael = massmatrix_voronoi(v, f), average_edge_length(v, f)
    ((mass * weights(mass)).sum() + ael.sum()).backward()
    assert v.grad is not None
    handed.check("ls_meshgeom_workspace_bytes")


def test_distance_and_rays_with_gradients(dev, handed):
    v, f = sphere(dev)
    p = (1.5 * weights(torch.empty((500, 3), device=dev), 3)).requires_grad_(True)
    d = (-p.detach() + 0.3 * weights(p, 4)).requires_grad_(True)
    with RayMesh(v, f) as m:
        sqr, _, _ = m.squared_distance(p)
        t, I, _ = m.intersect(p, d)
        hit = I >= 0
        assert int(hit.sum()) > 0
        ((sqr * weights(sqr)).sum() + (torch.where(hit, t, torch.zeros_like(t)) * weights(t, 5)).sum()).backward()
    assert v.grad is not None and p.grad is not None and d.grad is not None
    handed.check("ls_mesh_distance_backward_workspace_bytes", "ls_mesh_ray_backward_workspace_bytes")


def test_winding_number(dev, handed):
    v, f = sphere(dev, grad=False)
    p = 1.5 * weights(torch.empty((500, 3), device=dev), 3)
    w = distance.winding_number(v, f, p, 2.0)
    assert w.shape == (500,) and distance.winding_number(v, f, p, math.inf).shape == (500,)
    handed.check("ls_mesh_winding_bytes")


def test_self_intersections(dev, handed):
    v, f = sphere(dev, grad=False)
    v2 = torch.cat([v, v + torch.tensor([0.7, 0.1, 0.05], device=dev)])            # two spheres that cross
    pairs = distance.self_intersections(v2, torch.cat([f, f + v.shape[0]]))
    assert pairs.shape[0] > 0
    handed.check("ls_mesh_selfx_workspace_bytes")


def test_sample_surface_with_its_gradient(dev, handed):
    v, f = sphere(dev)
    P, _, _ = sample_surface(v, f, 3000, seed=1)
    (P * weights(P)).sum().backward()
    assert v.grad is not None
    handed.check("ls_sample_workspace_bytes")


def scene(dev):
    """a small sphere in front of two large triangles: clip-space pos (V, 4), tri int32 and the number of sphere faces"""
    vi, fi = synthetic.icosphere(2)
    nv = vi.shape[0]
    quad = np.array([[-0.9, -0.9, 0.5], [0.9, -0.9, 0.5], [0.9, 0.9, 0.5], [-0.9, 0.9, 0.5]])
    P = np.concatenate([0.6 * vi, quad])
    tri = np.concatenate([fi, np.array([[nv, nv + 1, nv + 2], [nv, nv + 2, nv + 3]])]).astype(np.int32)
    pos = np.concatenate([P, 1.0 + 0.2 * P[:, 2:3]], 1).astype(np.float32)
    return torch.from_numpy(pos).to(dev), torch.from_numpy(tri).to(dev), fi.shape[0]


def render(pos, tri, ranges):
    attr = weights(torch.empty((pos.shape[-2], 3), device=pos.device), 6).requires_grad_(True)
    rast, _ = dr.rasterize(None, pos, tri, (16, 16), ranges=ranges)
    assert int((rast[..., 3] > 0).sum()) > 0
    color, _ = dr.interpolate(attr, rast, tri)
    aa = dr.antialias(color, rast, pos, tri)
    ((aa * weights(aa, 7)).sum() + (rast[..., :2] * weights(rast[..., :2], 8)).sum()).backward()
    assert pos.grad is not None and attr.grad is not None


def test_render_instanced_with_gradients(dev, handed):
    pos, tri, _ = scene(dev)
    render(torch.stack([pos, pos * torch.tensor([-1.0, 1.0, 1.0, 1.0], device=dev)]).contiguous().requires_grad_(True), tri, None)
    handed.check("ls_raster_workspace_bytes", "ls_raster_adjacency_workspace_bytes", "ls_corner_ranks_workspace_bytes")


def test_render_range_mode_with_gradients(dev, handed):
    pos, tri, nf = scene(dev)
    ranges = torch.tensor([[0, nf + 2], [nf, 2], [0, nf]], dtype=torch.int32)
    render(pos.clone().requires_grad_(True), tri, ranges)
    handed.check("ls_range_workspace_bytes", "ls_range_adjacency_workspace_bytes", "ls_corner_ranks_workspace_bytes")


def test_texture_plain_mipmapped_and_cube_with_gradients(dev, handed):
    uv = (weights(torch.empty((2, 16, 16, 2), device=dev), 9) * 0.6 + 0.5).requires_grad_(True)
    da = (weights(torch.empty((2, 16, 16, 4), device=dev), 10) * 0.2).requires_grad_(True)
    tex = torch.rand((1, 16, 16, 3), device=dev).requires_grad_(True)
    plain = dr.texture(tex, uv, filter_mode="linear", boundary_mode="wrap")
    mipped = dr.texture(tex, uv, uv_da=da, filter_mode="linear-mipmap-linear", boundary_mode="clamp")
    dirs = weights(torch.empty((2, 16, 16, 3), device=dev), 11).requires_grad_(True)
    cube_tex = torch.rand((1, 6, 16, 16, 3), device=dev).requires_grad_(True)
    cube = dr.texture(cube_tex, dirs, filter_mode="linear", boundary_mode="cube")
    ((plain * weights(plain, 12)).sum() + (mipped * weights(mipped, 13)).sum() + (cube * weights(cube, 14)).sum()).backward()
    assert tex.grad is not None and cube_tex.grad is not None and uv.grad is not None
    handed.check("ls_texture_workspace_bytes", "ls_mip_workspace_bytes", "ls_cube_workspace_bytes")


def test_isosurface_with_its_gradient(dev, handed):
    ax = torch.linspace(-1.0, 1.0, 8, device=dev)
    ball = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt() - 0.6
    S = (ball + 0.02 * weights(ball, 15)).requires_grad_(True)
    V, F = isosurface(S, 0.0, (-1.0, -1.0, -1.0), 2.0 / 7.0)
    assert V.shape[0] > 0 and F.shape[0] > 0
    (V * weights(V)).sum().backward()
    assert S.grad is not None
    handed.check("ls_iso_workspace_bytes")
