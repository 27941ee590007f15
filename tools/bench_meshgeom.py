"""time average_edge_length and massmatrix_voronoi, forward and forward + backward, against a stock-torch formulation of the same
math (written here: gathers, (F, 3) intermediates, torch.where, an atomic scatter_add_):     python tools/bench_meshgeom.py [configs...]

Algorithmic bytes (csrc/meshgeom.hip, 4-byte face indices): what each call must move at least once, reported next to its time as a
fraction of 8 TB/s (HBM peak of the MI355X).
  mass forward        vptr 4 V + order 12 F + faces 12 F + verts 12 V + mass 4 V
  mass backward       faces 12 F + verts 12 V + g 4 V + cpos 12 F + corner buffer 36 F (written) + vptr 4 V + corner 36 F (read)
                      + grad 12 V
  average forward     faces 12 F + verts 12 V
  average backward    faces 12 F + verts 12 V + cpos 12 F + corner 36 F + vptr 4 V + corner 36 F + grad 12 V"""
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import torch  # noqa: E402
from largesteps import synthetic  # noqa: E402
from largesteps.meshops import average_edge_length, massmatrix_voronoi  # noqa: E402

HBM = 8e12
dev = torch.device("cuda:0")


def torch_mass(v, f):
    p = v[f]                                                            # (F, 3 corners, 3)
    l = torch.stack([(p[:, (k + 1) % 3] - p[:, (k + 2) % 3]).norm(dim=1) for k in range(3)], 1)
    l1, l2 = l.roll(-1, 1), l.roll(-2, 1)                              # l_{k+1}, l_{k+2}
    cos = (l1 * l1 + l2 * l2 - l * l) / (2 * l1 * l2)
    b = cos * l
    b = b / b.sum(1, keepdim=True)
    s = l.sum(1)
    area = 0.25 * (s * (s - 2 * l[:, 0]) * (s - 2 * l[:, 1]) * (s - 2 * l[:, 2])).clamp_min(0).sqrt()
    t = area[:, None] * b
    cells = 0.5 * (t.roll(-1, 1) + t.roll(-2, 1))
    for k in range(3):
        rule = torch.full_like(cells, 0.25)
        rule[:, k] = 0.5
        cells = torch.where((cos[:, k] < 0)[:, None], rule * area[:, None], cells)
    return torch.zeros(v.shape[0], dtype=v.dtype, device=v.device).scatter_add_(0, f.reshape(-1), cells.reshape(-1))


def torch_avg(v, f):
    p = v[f]
    return (p - p.roll(1, 1)).norm(dim=2).sum() / f.shape[0] / 3


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main(configs):
    for name in configs:
        v, f, _ = synthetic.config_mesh(name)
        V, F = v.shape[0], f.shape[0]
        tv = torch.from_numpy(v).to(dev).requires_grad_(True)
        tf = torch.from_numpy(f).to(dev)
        tfl = tf.long()
        w = torch.randn(V, device=dev)
        reps = 50
        with torch.no_grad():
            t_mf = timed(lambda: massmatrix_voronoi(tv, tf), reps)
            t_af = timed(lambda: average_edge_length(tv, tf), reps)
            r_mf = timed(lambda: torch_mass(tv, tfl), reps)
            r_af = timed(lambda: torch_avg(tv, tfl), reps)
        t_mb = timed(lambda: torch.autograd.grad((massmatrix_voronoi(tv, tf) * w).sum(), tv), reps)
        t_ab = timed(lambda: torch.autograd.grad(average_edge_length(tv, tf), tv), reps)
        r_mb = timed(lambda: torch.autograd.grad((torch_mass(tv, tfl) * w).sum(), tv), reps)
        r_ab = timed(lambda: torch.autograd.grad(torch_avg(tv, tfl), tv), reps)
        b_mf = 20 * V + 24 * F
        b_mb = 32 * V + 96 * F
        b_af = 12 * F + 12 * V
        b_ab = 28 * V + 96 * F
        with torch.no_grad():
            dm = float(((massmatrix_voronoi(tv, tf) - torch_mass(tv, tfl)).abs() / torch_mass(tv, tfl).abs()).max())
            da = float((average_edge_length(tv, tf) / torch_avg(tv, tfl) - 1).abs())
        print(f"{name}: V={V} F={F}")
        for what, t, r, b in (("massmatrix_voronoi forward", t_mf, r_mf, b_mf), ("massmatrix_voronoi fwd+bwd", t_mb, r_mb, b_mf + b_mb),
                              ("average_edge_length forward", t_af, r_af, b_af), ("average_edge_length fwd+bwd", t_ab, r_ab, b_af + b_ab)):
            print(f"  {what:30s} hip {t * 1e6:8.1f} us  ({b / 1e6:6.1f} MB algorithmic, {b / t / HBM * 100:5.1f} % of 8 TB/s)   "
                  f"stock torch {r * 1e6:8.1f} us   x{r / t:.1f}")
        print(f"  max relative |hip - torch| mass {dm:.2e}, average edge length {da:.2e}")


if __name__ == "__main__":
    main(sys.argv[1:] or ["cfg2_bunny70k", "cfg3_dragon250k", "cfg4b_sphere1m"])
