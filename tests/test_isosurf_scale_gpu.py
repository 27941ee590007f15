"""
largesteps.levelset at sizes past one chunk of every helper, against tests/isosurf_statement.py, bit for bit: a grid of more than
2048^2 nodes, whose scan needs more than one sweep of its second level, and a call whose faces pass 2^22 rows.
"""
import numpy as np
import pytest
import torch

import isosurf_statement as st

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def compare(dev, S, seed):
    """the device's V, E, F and gS against the statement's, compared on the device"""
    from largesteps.levelset import isosurface
    t = torch.from_numpy(S).to(dev).requires_grad_()
    V, F, E = isosurface(t, return_edges=True)
    Vs, Es, Fs = st.extract(S)
    assert tuple(V.shape) == Vs.shape and tuple(F.shape) == Fs.shape
    assert torch.equal(V.detach().view(torch.int32), torch.from_numpy(Vs).to(dev).view(torch.int32))
    assert torch.equal(E, torch.from_numpy(Es).to(dev)) and torch.equal(F, torch.from_numpy(Fs).to(dev))
    gV = np.random.default_rng(seed).standard_normal(Vs.shape).astype(F32)
    gS, = torch.autograd.grad((V * torch.from_numpy(gV).to(dev)).sum(), t)
    assert torch.equal(gS.view(torch.int32), torch.from_numpy(st.grad_S(S, 0.0, 1.0, gV)).to(dev).view(torch.int32))
    return Vs.shape[0], Fs.shape[0]


def test_a_grid_past_2048_squared_nodes(dev):
    shape = (162, 162, 161)
    assert np.prod(shape) > 2048 ** 2
    S = (st.sphere_sdf(shape, (80.3, 79.6, 81.1), 60.4) + 0.3 * np.random.default_rng(1).standard_normal(shape)).astype(F32)
    n, m = compare(dev, S, 2)
    print(f"{shape}: {n} vertices, {m} faces")
    assert n > 2048 * 64


def test_faces_past_2_to_the_22_rows(dev):
    shape = (96, 97, 95)
    S = np.random.default_rng(3).standard_normal(shape).astype(F32)
    n, m = compare(dev, S, 4)
    print(f"{shape}: {n} vertices, {m} faces")
    assert m > 2 ** 22 and n > 2 ** 21
