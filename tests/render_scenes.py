"""
The scenes of the rasterizer tests (tests/test_render_gpu.py, tests/test_render_scale_gpu.py, tests/test_render_statement_cpu.py): views,
clip-space projection and the small named scenes, all built from largesteps.synthetic without a device.
"""
import numpy as np


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """world -> view (4, 4) with the camera looking along +z of the view (w = view z under persp_proj)"""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[0, :3], M[1, :3], M[2, :3] = x, y, z
    M[:3, 3] = -M[:3, :3] @ eye
    return M


def clip(v, views, fov=45.0, ar=1.0, near=0.1, far=100.0):
    from largesteps.render import persp_proj
    P = persp_proj(fov, ar, near, far).double().numpy()
    vh = np.concatenate([v.astype(np.float64), np.ones((v.shape[0], 1))], 1)
    return np.stack([(vh @ (P @ M).T) for M in views]).astype(np.float32)


def scene(name):
    """(pos (B, V, 4) fp32, tri (F, 3) int64, H, W)"""
    from largesteps import synthetic
    if name == "sphere":
        v, f = synthetic.icosphere(4)
        return clip(v, [look_at((0.3, 0.4, -3.0))], ar=32 / 24), f, 24, 32
    if name == "sphere_b3":
        v, f = synthetic.icosphere(3)
        v = synthetic.perturb(v, radial=0.05, seed=1)
        return clip(v, [look_at((0, 0, -3.0)), look_at((3.0, 0.5, 0)), look_at((-1.5, 2.0, 2.0))]), f, 20, 20
    if name == "folded":
        v, f = synthetic.folded_sheet(6, gap=0.05)
        v = v - np.array([0.25, 0.5, 0.0], np.float32)
        return clip(v, [look_at((0.6, 0.3, -1.5))], ar=2.0), f, 16, 32
    if name == "near_plane":                     # a floor through the eye's plane: crosses near and w = 0
        v = np.array([[-3, -0.5, -2], [3, -0.5, -2], [3, -0.5, 6], [-3, -0.5, 6]], np.float32)
        f = np.array([[0, 1, 2], [0, 2, 3]])
        return clip(v, [look_at((0, 0, -0.5), (0, -0.2, 1.0))], near=0.5, far=10.0, ar=24 / 16), f, 16, 24
    if name == "sheet":                          # a tilted plane facing the camera: its silhouette is its boundary
        v, f = synthetic.plane(6)
        v = v - np.array([0.5, 0.5, 0.0], np.float32)
        return clip(v, [look_at((0.3, 0.2, -1.6))], ar=32 / 24), f, 24, 32
    if name == "quad":                           # full-screen 2-triangle quad, w = 1: the cooperative path
        pos = np.array([[[-1, -1, 0.5, 1], [1, -1, 0.5, 1], [1, 1, 0.5, 1], [-1, 1, 0.5, 1]]], np.float32)
        return pos, np.array([[0, 1, 2], [0, 2, 3]]), 40, 48
    if name == "empty":                          # everything behind the camera
        v, f = synthetic.icosphere(2)
        return clip(v + np.array([0, 0, -5], np.float32), [look_at((0, 0, 0), (0, 0, 1))]), f, 12, 12
    raise KeyError(name)


SCENES = ["sphere", "sphere_b3", "folded", "near_plane", "quad", "empty"]


def bench_views(B):
    """the look-at views of tools/bench_render.py: B cameras at distance 3 around the origin"""
    return [look_at((3 * np.cos(2 * np.pi * k / B), 0.8 * np.sin(3.0 * k), 3 * np.sin(2 * np.pi * k / B))) for k in range(B)]


def sphere70k(B, res):
    """the bench's cfg2_bunny70k noisy sphere from B of its views at res x res: (pos (B, V, 4) fp32, tri (F, 3) int64, res, res)"""
    from largesteps import synthetic
    v, f, _ = synthetic.config_mesh("cfg2_bunny70k")
    return clip(v, bench_views(B)), np.asarray(f, np.int64), res, res


def random_soup(seed, n=40, B=2, H=20, W=24):
    """random triangles around the camera: many cross w = 0 and the near plane, some are duplicated (same corners, shuffled face
    order: exact depth ties), a few edges are shared by three faces (non-manifold) and a few vertices are unreferenced"""
    rng = np.random.default_rng(seed)
    V = 3 * n + 4
    v = np.concatenate([rng.uniform(-2, 2, (V, 2)), rng.uniform(-2.5, 2.5, (V, 1))], 1)
    f = rng.permutation(3 * n).reshape(n, 3)
    fan = np.stack([f[:3, 0], f[:3, 1], rng.integers(0, 3 * n, 3)], 1)            # third faces on the first edges
    f = np.concatenate([f, f[: n // 4], fan])
    f = f[rng.permutation(len(f))]
    views = [look_at(rng.uniform(-0.3, 0.3, 3) + np.array([0, 0, -1.0]), (0, 0, 1.0)) for _ in range(B)]
    return clip(v.astype(np.float32), views, ar=W / H, near=0.5, far=10.0), f.astype(np.int64), H, W


def grid_mesh(n, lo, hi, jitter=0.0, seed=0, wscale=False, coords=None):
    """an n x n vertex grid spanning [lo, hi]^2 in NDC (w = 1), two triangles per cell; optional dyadic jitter of interior vertices and
    a per-vertex power-of-two homogeneous scale (same projection)"""
    t = np.linspace(lo, hi, n) if coords is None else coords
    X, Y = np.meshgrid(t, t, indexing="xy")
    rng = np.random.default_rng(seed)
    if jitter:
        J = np.round(rng.uniform(-jitter, jitter, X.shape) * 1024) / 1024
        X[1:-1, 1:-1] += J[1:-1, 1:-1]
        J = np.round(rng.uniform(-jitter, jitter, X.shape) * 1024) / 1024
        Y[1:-1, 1:-1] += J[1:-1, 1:-1]
    v = np.stack([X.ravel(), Y.ravel(), np.zeros(n * n), np.ones(n * n)], 1)
    if wscale:
        v *= 2.0 ** rng.integers(-2, 3, (n * n, 1))
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i, i + n + 1, i + n], 1)])
    return v.astype(np.float32)[None], f


def near_plane_triangles(seed=3, n=40, near=0.5, far=10.0):
    """the random clip-space triangles of test_near_plane_matches_homogeneous_clipping: corners in front of, across and behind the
    near plane and w = 0 under an unscaled perspective projection"""
    rng = np.random.default_rng(seed)
    P = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, (far + near) / (far - near), -2 * far * near / (far - near)], [0, 0, 1, 0]])
    out = []
    for _ in range(n):
        q = np.concatenate([rng.uniform(-2, 2, (3, 2)), rng.uniform(-1.5, 2.5, (3, 1))], 1)      # (x, y, view depth)
        out.append((np.concatenate([q[:, :2], q[:, 2:], np.ones((3, 1))], 1) @ P.T).astype(np.float32))
    return out
