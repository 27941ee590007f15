"""Device time of largesteps.topology (csrc/topology.hip) on the 70k sphere (cfg2_bunny70k), the 1M noisy sphere (cfg4b_sphere1m) and the
1M plane (cfg4_plane1m) of largesteps.synthetic: the constructor (wall clock, it synchronises once), measures, and keep dropping every
other of the 1 000 components of a mesh of 1 000 spheres. Two baselines for the labelling alone: (a) plain torch on the same device --
labels propagated over the edges with scatter_reduce(amin) and pointer jumping until nothing changes (a host read per round); (b)
scipy.sparse.csgraph.connected_components on the host, the transfer of the faces included. measures of a mesh that is ONE component is
the sum of its ~2M faces by a single wave (the fixed order of the segmented sum): it is reported on its own line, next to the same
call on the 1 000-component mesh, so that a later change can decide whether it needs a wider fixed order. Each device figure is the
median of `repeats` timed runs (device events around `inner` calls, after warm-up), all in one process. Writes one JSON document. No
speed threshold belongs to it: the feature is gated by its bitwise tests.
    python tools/bench_topology.py [out.json] [repeats]"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd")]
import numpy as np
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import connected_components
from largesteps import synthetic
from largesteps.topology import MeshTopology

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "topology_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")


def timed(fn, inner=5):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts))


def wall(fn, n=5):
    fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def torch_labels(tf, V):
    """the lowest vertex id of every vertex's component, in plain torch: amin over the edges, then pointer jumping, to a fixed point"""
    a = torch.cat([tf[:, 0], tf[:, 1], tf[:, 2]])
    b = torch.cat([tf[:, 1], tf[:, 2], tf[:, 0]])
    label = torch.arange(V, device=tf.device)
    rounds = 0
    while True:
        rounds += 1
        new = label.scatter_reduce(0, a, label[b], "amin").scatter_reduce(0, b, label[a], "amin")
        new = new[new]
        new = new[new]
        if torch.equal(new, label):
            return label, rounds
        label = new


def scipy_labels(tf, V):
    f = tf.cpu().numpy()
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    A = sp.coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(V, V))
    return connected_components(A, directed=False)


def spheres(k, n):
    v, f = synthetic.icosphere(n)
    rng = np.random.default_rng(0)
    c = rng.uniform(-50, 50, (k, 3)).astype(np.float32)
    V = (v[None] + c[:, None]).reshape(-1, 3)
    F = (f[None] + (np.arange(k) * v.shape[0])[:, None, None]).reshape(-1, 3)
    return V, F


def main():
    doc = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "meshes": {}}
    for name in ("cfg2_bunny70k", "cfg4b_sphere1m", "cfg4_plane1m"):
        v, f, _ = synthetic.config_mesh(name)
        V = v.shape[0]
        tf, tv = torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
        topo = MeshTopology(tf, V)
        label, rounds = torch_labels(tf, V)
        k_scipy, _ = scipy_labels(tf, V)
        assert topo.num_vertex_components == k_scipy == int((label == torch.arange(V, device=dev)).sum())
        ms = {"constructor_wall": wall(lambda: MeshTopology(tf, V)),
              "torch_label_propagation_wall": wall(lambda: torch_labels(tf, V), 3),
              "scipy_connected_components_wall": wall(lambda: scipy_labels(tf, V), 3),
              "measures_one_component": timed(lambda: topo.measures(tv))}
        doc["meshes"][name] = {"vertices": V, "faces": int(f.shape[0]), "edges": topo.num_edges, "facet_components": topo.num_facet_components,
                               "boundary_loops": int(topo.boundary_loops()[1].shape[0]) - 1, "torch_rounds": rounds, "ms": ms}
    v, f = spheres(1000, 10)
    V = v.shape[0]
    tf, tv = torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
    topo = MeshTopology(tf, V)
    assert topo.num_facet_components == 1000
    mask = torch.arange(1000, device=dev) % 2 == 0
    F2, I, J = topo.keep(mask)
    sizes = (F2.shape[0], J.shape[0])
    doc["meshes"]["spheres_1000x1002"] = {"vertices": V, "faces": int(f.shape[0]), "facet_components": 1000, "ms": {
        "constructor_wall": wall(lambda: MeshTopology(tf, V)), "measures": timed(lambda: topo.measures(tv)),
        "keep_half_wall": wall(lambda: topo.keep(mask)), "keep_half_sizes_known": timed(lambda: topo.keep(mask, sizes=sizes)),
        "counts": timed(lambda: (setattr(topo, "_counts", None), topo.counts()))}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
