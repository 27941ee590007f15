"""
The self-intersection query of largesteps.distance past one sort chunk and two key bytes: 216 exact copies of one small self-intersecting
mesh, whose answer is the base mesh's answer repeated. The statement (tests/selfx_statement.py) runs once, on the 320 faces of the base.

The base is the jittered icosphere(4) with its coordinates rounded to multiples of 2^-12; the copies sit on a 6 x 6 x 6 grid of integer
offsets 4 apart (the sphere has radius 1: copies do not touch). Every coordinate is then a multiple of 2^-12 below 32, 17 significant
bits, exact in fp32, and every difference the rule forms is the same number in every copy: the rule decides bit for bit alike in each.
The e of the box clause is 2^-40 x the largest coordinate, about 1 for the base and 21 for the copies; the gap between two corner boxes
is a multiple of 2^-12 or not positive, and 2 e is below 10^-10 and above the rounding of a coordinate below 32 in fp64 for both, so the
clause decides alike as well.
F = 69 120 > 2^16 faces take three byte passes of the sort's second key word, and k = 216 k_base pairs span many sort chunks (rs_chunk
of csrc/radix.h is 1024 rows up to 2^21). The device must return exactly the base pairs shifted by 320 j for copy j, in order -- and
so no pair across copies.
"""
import numpy as np
import pytest
import torch

import selfx_statement as sx

pytestmark = pytest.mark.gpu
F32 = np.float32
RS_CHUNK = 1024                  # rs_chunk(n) of csrc/radix.h for n <= 2^21
GRID, STEP = 6, 4.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case():
    v, f = sx.jittered(4, 1.0)
    v = (np.round(v.astype(np.float64) * 4096.0) / 4096.0).astype(F32)
    base = sx.pairs(v, f)
    offsets = np.array([[x, y, z] for x in range(GRID) for y in range(GRID) for z in range(GRID)], dtype=np.float64) * STEP
    V = (v.astype(np.float64)[None, :, :] + offsets[:, None, :]).reshape(-1, 3)
    assert np.array_equal(V.astype(F32).astype(np.float64), V)                                 # exact in fp32
    copies = offsets.shape[0]
    F = (f[None, :, :] + v.shape[0] * np.arange(copies)[:, None, None]).reshape(-1, 3)
    IF = (base[None, :, :] + f.shape[0] * np.arange(copies)[:, None, None]).reshape(-1, 2)
    return V.astype(F32), F, IF, base, f


def test_the_case_is_past_one_chunk_and_two_key_bytes(case):
    V, F, IF, base, f = case
    shared = sx.shares_a_vertex(f, base)
    assert base.shape[0] > 0 and shared.sum() > 0 and (~shared).sum() > 0
    assert F.shape[0] == 69120 > 2 ** 16 and IF.shape[0] == 216 * base.shape[0] > RS_CHUNK
    assert (np.diff(IF[:, 0] * F.shape[0] + IF[:, 1]) > 0).all()                               # merged in order


def test_copies_of_a_mesh_repeat_its_pairs(dev, case):
    from largesteps.distance import MeshDistance
    V, F, IF, base, f = case
    with MeshDistance(torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)) as m:
        got = m.self_intersections()
        cnt = m.count_self_intersections()
        faces = m.self_intersecting_faces()
        again = m.self_intersections()
    assert int(cnt) == IF.shape[0] and tuple(got.shape) == IF.shape
    got = got.cpu().numpy()
    assert (got[:, 0] // f.shape[0] == got[:, 1] // f.shape[0]).all(), "a pair across two copies"
    assert np.array_equal(got, IF)
    assert np.array_equal(again.cpu().numpy(), got)
    mask = np.zeros(F.shape[0], dtype=bool)
    mask[IF.reshape(-1)] = True
    assert np.array_equal(faces.cpu().numpy(), mask)
