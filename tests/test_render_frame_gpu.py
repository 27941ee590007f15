"""
The frame that a rast of largesteps.render carries: the pixel order of its backward passes is made at most once
per version of the rast, a rast that no `rasterize` of the package made gets a frame of its own, a frame made for another face count is
not reused, the three backward passes that share one frame compute what each computes alone, and a rast of one mode is refused with the
arguments of the other. Every comparison is bitwise.

The scene is the smallest with more than one image and more than one key per image: an icosahedron (12 vertices, 20 faces) at 16 x 16,
from two views in instanced mode, cut into two ranges of ten faces in range mode.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from render_scenes import clip, look_at  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
H = W = 16
C = 3
BLOCK = (slice(None), slice(5, 11), slice(5, 11))        # the pixels whose id an in-place edit sets to 0
MODES = ("instanced", "range")


def _rand(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


class Scene:
    """pos, tri and the keyword arguments of `rasterize` for one mode; attr, and the weights g of the losses"""

    def __init__(self, mode):
        from largesteps import synthetic
        v, f = synthetic.icosphere(1)
        assert f.shape == (20, 3)
        views = [look_at((0.3, 0.4, -3.0)), look_at((2.5, 0.5, 1.5))]
        self.tri = torch.from_numpy(f).to(DEV)
        if mode == "instanced":
            self.pos, self.kw = torch.from_numpy(clip(v, views)).to(DEV), {}
        else:
            self.pos = torch.from_numpy(clip(v, views[:1])[0]).to(DEV)
            self.kw = {"ranges": torch.tensor([[0, 10], [10, 10]], dtype=torch.int32)}
        self.attr = _rand((v.shape[0], C), 1)
        self.g = _rand((2, H, W, C), 2)

    def rasterize(self, pos=None, tri=None):
        import largesteps.render as dr
        return dr.rasterize(None, self.pos if pos is None else pos, self.tri if tri is None else tri, (H, W), **self.kw)[0]


def _edit(rast):
    assert (rast[BLOCK][..., 3] > 0).any(), "the edited block must hold covered pixels"
    rast[BLOCK][..., 3] = 0


def _grads(s, rast, tri=None):
    """(gradient of interpolate to attr, of antialias to color, of antialias to pos), each from a backward of its own on `rast`"""
    import largesteps.render as dr
    tri = s.tri if tri is None else tri
    a = s.attr.clone().requires_grad_(True)
    (dr.interpolate(a, rast, tri)[0] * s.g).sum().backward()
    col, p = s.g.flip(0).clone().requires_grad_(True), s.pos.clone().requires_grad_(True)
    (dr.antialias(col, rast, p, tri, pos_gradient_boost=2.0) * s.g).sum().backward()
    return a.grad, col.grad, p.grad


def _assert_equal(got, ref, what):
    for name, x, y in zip(("attr.grad", "color.grad", "pos.grad of antialias"), got, ref):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} elements"


# ---- a. an order cached on the frame is not used for a later version of the rast ------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_an_in_place_edit_of_the_rast_invalidates_the_cached_order(mode):
    s = Scene(mode)
    rast = s.rasterize()
    assert not rast.requires_grad
    before = _grads(s, rast)                  # the order is now cached on the frame
    _edit(rast)
    got = _grads(s, rast)
    if mode == "instanced":
        fresh = s.rasterize().clone()
    else:                                     # only the tensor that rasterize returned carries the range table
        fresh = s.rasterize()
    _edit(fresh)                              # the same edit, before any backward
    assert torch.equal(fresh, rast)
    _assert_equal(got, _grads(s, fresh), mode)
    assert not torch.equal(got[0], before[0]), "the edit must change the gradient"


# ---- b. a rast that carries no frame (instanced mode) -------------------------------------------------------------------------------------
def test_a_cloned_rast_gives_what_the_original_gives():
    import largesteps.render as dr
    s = Scene("instanced")
    rast = s.rasterize()
    copy = rast.clone()
    col = s.g.flip(0)
    mine, its = [(dr.interpolate(s.attr, r, s.tri)[0], dr.antialias(col, r, s.pos, s.tri)) for r in (rast, copy)]
    assert torch.equal(its[0], mine[0]) and torch.equal(its[1], mine[1])
    assert float(mine[0].abs().sum()) > 0 and not torch.equal(mine[1], col)
    _assert_equal(_grads(s, copy), _grads(s, rast), "clone")


# ---- c. a frame made for another face count is not reused (instanced mode) -------------------------------------------------------------------
def test_an_order_cached_for_another_face_count_is_not_reused():
    s = Scene("instanced")
    tri2 = s.tri[:12].contiguous()
    rast = s.rasterize(tri=tri2).clone()      # fabricated: ids in [0, 12], valid for tri (20 faces) and for tri2 (12 faces)
    first = _grads(s, rast)                   # backward through tri: the order of 2 x 20 keys is cached
    got = _grads(s, rast, tri2)
    _assert_equal(got, _grads(s, rast.clone(), tri2), "tri2 after tri")
    _assert_equal(_grads(s, rast), first, "tri after tri2")


# ---- d. three backward passes on one frame -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_backward_passes_that_share_a_frame_match_each_on_its_own(mode):
    import largesteps.render as dr
    s = Scene(mode)

    def loss(p_rast, p_aa, a):
        rast = s.rasterize(p_rast)
        return (dr.antialias(dr.interpolate(a, rast, s.tri)[0], rast, p_aa, s.tri) * s.g).sum()

    def leaf(t, on=True):
        return t.clone().requires_grad_(on)

    p, a = leaf(s.pos), leaf(s.attr)
    loss(p, p, a).backward()                  # rasterize, interpolate and antialias take one order from one frame
    alone = []
    for k in range(3):                        # one leaf at a time: exactly one of the three backward passes asks its frame for the order
        leaves = [leaf(s.pos, k == 0), leaf(s.pos, k == 1), leaf(s.attr, k == 2)]
        loss(*leaves).backward()
        alone.append(leaves[k].grad)
    g_rast, g_aa, g_attr = alone
    assert float(g_rast.abs().sum()) > 0 and float(g_aa.abs().sum()) > 0
    assert torch.equal(a.grad, g_attr)
    assert torch.equal(p.grad, g_rast + g_aa)           # two terms: the sum does not depend on the order autograd adds them in


# ---- e. a rast of one mode with the arguments of the other -------------------------------------------------------------------------------
def test_mixed_modes_are_refused():
    import largesteps.render as dr
    s = Scene("range")
    rast = s.rasterize()
    col = s.g
    with pytest.raises(ValueError, match=re.escape("rast comes from a range-mode rasterize: pos must be the (V, 4) positions given to it")):
        dr.antialias(col, rast, s.pos[None].expand(2, -1, -1).contiguous(), s.tri)
    with pytest.raises(ValueError, match=re.escape("a (V, 4) pos is range mode and needs the range table that its rast carries")):
        dr.antialias(col, rast.clone(), s.pos, s.tri)
    with pytest.raises(ValueError, match=re.escape("attr must be (V, C) or (1, V, C) for a rast of range mode")):
        dr.interpolate(s.attr[None].expand(2, -1, -1).contiguous(), rast, s.tri)
    assert torch.equal(dr.antialias(col, rast, s.pos, s.tri), dr.antialias(col, rast, s.pos, s.tri))
