"""
The cube-map gradients past one workgroup of the sort and two key bytes, against tests/cube_statement.py with the bounds derived in
tests/test_cube_gpu.py (the same comparison: `check_against_statement`):

  three_pass_n128        Bt = 1, n = 128: 6 * 128^2 + 1 = 98 305 keys, three byte passes of the radix sort (256^2 <= 98 304 < 256^3)
  three_pass_own_b4_n64  Bt = B = 4, n = 64, C = 4: the same 98 305 keys with a cube per image, float4 rows
  ragged_703             703 pixels: 2812 items (linear) span three 1024-item sort workgroups and end 252 items into a 256-thread block;
                         703 items (nearest) end inside the first
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cube_statement as cs  # noqa: E402
from test_cube_gpu import check_against_statement  # noqa: E402  (puts the package on the path)

pytestmark = pytest.mark.gpu

CASES = {                                   # name: (tex shape, uv shape)
    "three_pass_n128": ((1, 6, 128, 128, 3), (2, 64, 64)),
    "three_pass_own_b4_n64": ((4, 6, 64, 64, 4), (4, 48, 48)),
    "ragged_703": ((1, 6, 7, 7, 2), (1, 19, 37)),
}


def test_the_cases_meet_their_conditions():
    for name, (ts_, us) in CASES.items():
        keys = 6 * ts_[0] * ts_[2] * ts_[3] + 1
        if name.startswith("three_pass"):
            assert keys == 98305 and 256 ** 2 <= keys - 1 < 256 ** 3
    N = int(np.prod(CASES["ragged_703"][1]))
    assert N == 703 and 4 * N > 2 * 1024 and (4 * N) % 256 == 252 and N < 1024 and N % 256 != 0


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("filt", cs.FILTERS)
def test_native_matches_statement_at_scale(filt, name):
    tex_shape, uv_shape = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    tex = rng.standard_normal(tex_shape).astype(np.float32)
    uv = rng.standard_normal(uv_shape + (3,)).astype(np.float32)
    g = rng.standard_normal(uv_shape + tex_shape[4:]).astype(np.float32)
    r = check_against_statement(name, tex, uv, g, filt)
    assert r.finite.all() and set(r.face.ravel()) == set(range(6))
    if filt == "linear":
        assert r.grad_tex_n.sum() == 4 * r.finite.sum() - (r.drop >= 0).sum()
        if name.startswith("three_pass"):
            assert (~r.inside).sum() > 50                   # seams are crossed at this size too
            assert (r.grad_tex_n.reshape(tex_shape[0], -1).sum(1) > 0).all()
