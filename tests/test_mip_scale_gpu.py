"""
The mipmapped largesteps.render.texture on the device at the shapes of tests/texture_cases.py -- pyramids whose levels start in the
middle of a wave, levels one texel high or wide over many levels, item orders of three byte passes, clusters at 64 and 65 items on
level 0 and hundreds on level 2 -- against tests/mip_statement.py, with the bounds and the flag rule of tests/test_mip_gpu.py unchanged
(U = 2^-24, dlod = 16 U (1 + |lod|)):
  forward    |err| <= 16 U max|tex| + |d out / d lod| dlod
  gradients  an entry that sums n terms of magnitude sum S: |err| <= (n + 16) U S + |d entry / d lod| dlod.
Flagged pixels (lod within 64 U (1 + |lod|) of a level switch; at most 2 % of a case, checked without a device by tests/test_mip_cpu.py)
get no upstream gradient and are left out of the nearest-mode forward comparison.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import mip_statement as ms  # noqa: E402
import texture_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
U = 2.0 ** -24


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(tex, uv, da, bias, g, mode, boundary, max_level, mip=False):
    import largesteps.render as dr
    t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)
    d = None if da is None else dev(da).requires_grad_(True)
    b = None if bias is None else dev(bias).requires_grad_(True)
    m = dr.texture_construct_mip(t, max_mip_level=max_level) if mip else None
    out = dr.texture(t, c, d, b, mip=m, filter_mode=mode, boundary_mode=boundary, max_mip_level=max_level)
    (out * dev(g)).sum().backward()
    z = lambda x: None if x is None else x.grad.cpu().numpy()  # noqa: E731
    return out.detach().cpu().numpy(), t.grad.cpu().numpy(), c.grad.cpu().numpy(), z(d), z(b)


def _rel(e, b):
    return float((e / np.maximum(b, 1e-300)).max())


@pytest.mark.parametrize("name", list(tc.MIP_CASES))
@pytest.mark.parametrize("mode,boundary", tc.MIP_COMBOS)
def test_native_matches_statement(mode, boundary, name):
    tex, uv, da, bias, max_level, g = tc.mip_case(name)
    linear = mode == "linear-mipmap-linear"
    flag = ms.texture(tex, uv, da, bias, None, mode, boundary, max_level).flag
    assert flag.mean() <= 0.02, (name, flag.mean())
    g = g * ~flag[..., None]
    r = ms.texture(tex, uv, da, bias, g, mode, boundary, max_level)
    nk = tc.mip_keys(tex.shape, r.Lmax)
    if name.startswith("three_pass"):
        assert tc.texture_keys(tex.shape) >= 65536 and tc.radix_passes(nk) == 3
    keep = np.ones_like(flag) if linear else ~flag
    b_out = 16 * U * np.abs(tex).max() + np.abs(r.dout_dlod) * r.dlod[..., None]
    b_t = (r.grad_tex_n[..., None] + 16) * U * r.grad_tex_abs + r.grad_tex_lod
    b_c = (r.grad_uv_n + 16) * U * r.grad_uv_abs + r.grad_uv_lod
    b_b = (r.grad_bias_n + 16) * U * r.grad_bias_abs
    b_d = (r.grad_uv_da_n + 16) * U * r.grad_uv_da_abs
    # levels_straddle: once with the pyramid built inside the lookup, once with a prebuilt one -- the same bits, both within the bounds
    runs = [_run(tex, uv, da, bias, g, mode, boundary, max_level, mip=m) for m in ((False, True) if name.startswith("levels_straddle") else (False,))]
    for x, y in zip(runs[0], runs[-1]):
        assert (x is None and y is None) or np.array_equal(x, y)
    for out, gt, gc, gd, gb in runs:
        e_out, e_t, e_c, e_b = np.abs(out - r.out), np.abs(gt - r.grad_tex), np.abs(gc - r.grad_uv), np.abs(gb - r.grad_bias)
        line = (f"{name} {mode} {boundary}: {nk} keys, Lmax {r.Lmax}, flagged {int(flag.sum())}; forward err/bound {_rel(e_out[keep], b_out[keep]):.3f}; "
                f"grad_tex {_rel(e_t, b_t):.3f} (max terms {r.grad_tex_n.max()}); grad_uv {_rel(e_c, b_c):.3f}; grad_bias {_rel(e_b, b_b):.3f}")
        if da is not None:
            e_d = np.abs(gd - r.grad_uv_da)
            line += f"; grad_uv_da {_rel(e_d, b_d):.3f}"
        print(line)
        for a in (out, gt, gc, gd, gb):
            assert a is None or np.all(np.isfinite(a))
        assert np.all(e_out[keep] <= b_out[keep])
        assert np.all(e_t <= b_t), np.argwhere(e_t > b_t)[:4].tolist()
        assert np.all(e_c <= b_c), np.argwhere(e_c > b_c)[:4].tolist()
        assert np.all(e_b <= b_b)
        assert gt.any() and gc.any() and linear == bool(gb.any())
        if da is not None:
            assert np.all(e_d <= b_d)
            assert linear == bool(gd.any())
    if name == "mip_threshold":
        n0 = r.level_n[0]
        assert (n0 == 64).any() and (n0 == 65).any() and r.level_n[2].max() > 64
        assert linear == bool((r.level_n[1] > 64).any())
    else:
        assert (r.lod < 0).any() and (r.lod > r.Lmax).any() and (not linear or r.two.any())
        assert boundary == "zero" or max(n.max() for n in r.level_n) > 64          # texels that the whole wave sums (zero drops most pixels)


@pytest.mark.parametrize("name", ["levels_straddle_40x72_c3_max3", "deep_64x512_c3", "deep_512x2_c2", "three_pass_own_b2_128x256_c1", "mip_threshold"])
def test_two_runs_cached_and_rebuilt_order_are_bitwise_identical(name):
    import largesteps.render as dr
    tex, uv, da, bias, max_level, g = tc.mip_case(name)
    for mode, boundary in tc.MIP_COMBOS:
        a = _run(tex, uv, da, bias, g, mode, boundary, max_level)
        again = _run(tex, uv, da, bias, g, mode, boundary, max_level)                   # the same call twice
        prebuilt = _run(tex, uv, da, bias, g, mode, boundary, max_level, mip=True)      # and with a pyramid from texture_construct_mip
        for other in (again, prebuilt):
            for x, y in zip(a, other):
                assert (x is None and y is None) or np.array_equal(x, y), (mode, boundary, other is prebuilt)
        # one uv tensor used twice: the second backward takes the cached order
        t, c, d, bb, gg = dev(tex).requires_grad_(True), dev(uv), dev(da), dev(bias), dev(g)
        kw = dict(filter_mode=mode, boundary_mode=boundary, max_mip_level=max_level)
        (dr.texture(t, c, d, bb, **kw) * gg).sum().backward()
        slot = c._largesteps_mip_order
        assert slot.order is not None
        first, t.grad = t.grad.clone(), None
        (dr.texture(t, c, d, bb, **kw) * gg).sum().backward()
        assert c._largesteps_mip_order is slot
        assert torch.equal(t.grad, first) and np.array_equal(first.cpu().numpy(), a[1]), (mode, boundary)
        # changed in place: the order is rebuilt and the result is a fresh run's
        c.add_(0.013)
        t.grad = None
        (dr.texture(t, c, d, bb, **kw) * gg).sum().backward()
        assert c._largesteps_mip_order is not slot
        assert np.array_equal(t.grad.cpu().numpy(), _run(tex, c.cpu().numpy(), da, bias, g, mode, boundary, max_level)[1]), (mode, boundary)
