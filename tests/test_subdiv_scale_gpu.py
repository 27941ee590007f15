"""
largesteps.subdivide past one sweep of each stage of csrc/subdiv.hip, bit for bit against tests/subdiv_statement.py:

  * icosphere(9): 3 F = 4860 half-edges, more than one workgroup of the radix sort (1024 rows) and more than two tiles of the scan
    (2048), by a count that no block size divides (4860 = 2^2 3^5 5); perturbed values, so no symmetry hides a swapped term;
  * vertex ids above 65 536, so that both words of the half-edge key and the corner key need a second (and third) byte: a small mesh
    whose indices are offset behind 65 760 unreferenced vertices;
  * a closed fan of 200 faces: the interior vertex has 200 corners and is summed by its whole wave, forward and backward.
"""
import numpy as np
import pytest
import torch

import subdiv_statement as st

pytestmark = pytest.mark.gpu
F32 = np.float32
SCHEMES = (st.LOOP, st.MIDPOINT)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def check(dev, F, V, x, T, idx=torch.int64):
    from largesteps.subdivide import Subdivision
    tf = torch.from_numpy(F).to(dev).to(idx)
    g = st.values(V + T.E, x.shape[1], 21)
    for scheme in SCHEMES:
        sub = Subdivision(tf, V, scheme=scheme)
        assert sub.num_vertices == V + T.E
        assert same(sub.faces.to(torch.int64), T.faces) and same(sub.edges[0].to(torch.int64), T.edges)
        X = torch.from_numpy(x).to(dev).requires_grad_()
        Y = sub.apply(X)
        assert same(Y, st.apply(T, x, scheme))
        gX, = torch.autograd.grad(Y, X, torch.from_numpy(g).to(dev))
        assert same(gX, st.apply_transposed(T, g, scheme))


def test_more_than_one_sort_workgroup_and_two_scan_tiles(dev):
    from largesteps import synthetic
    from largesteps.sampling import SCAN_TILE
    v, F = synthetic.icosphere(9)
    assert 3 * len(F) > 2 * SCAN_TILE and 3 * len(F) % 64 != 0 and 3 * 20 * 8 * 8 <= 2 * SCAN_TILE       # the first level past two tiles
    x = synthetic.perturb(v, radial=0.1, tangential=0.2, edge=0.1, seed=3).astype(F32)
    check(dev, F.astype(np.int64), v.shape[0], x, st.Topology(F, v.shape[0]))


def test_vertex_ids_that_need_a_second_key_byte(dev):
    from largesteps import synthetic
    off = 65760                                                                # ids in [65760, 65852): bytes 0, 1 and 2 of both words vary
    v, F = synthetic.icosphere(3)
    F = F.astype(np.int64) + off
    V = off + v.shape[0]
    assert F.min() > 65536 and (F.max() >> 16) >= 1 and len(np.unique(F >> 8)) > 1
    T = st.Topology(F, V)
    assert T.E == 30 * 9 and int(T.valence[:off].max()) == 0
    check(dev, F, V, st.values(V, 2, 5), T, idx=torch.int32)


def test_a_vertex_of_200_corners_takes_the_whole_wave(dev):
    F, V = st.fan(200)
    T = st.Topology(F, V)
    assert len(T.corners[0]) == 200 > 64 and T.valence[0] == 200 and not T.bflag[0] and T.bflag[1:].all()
    for C in (3, 4):
        check(dev, F, V, st.values(V, C, 30 + C), T)
