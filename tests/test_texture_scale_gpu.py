"""
largesteps.render.texture on the device at the shapes of tests/texture_cases.py -- textures of more than one workgroup of texels, rows
wider than a key byte, pixel orders of three and four byte passes, clusters of pixels at 63 .. 66, 127 .. 129 and 700 items a texel,
32 and 4 + 1 channels -- against tests/texture_statement.py, with the bounds of tests/test_texture_gpu.py unchanged (U = 2^-24):
  forward    |err| <= 16 U max|tex|
  gradients  an entry that sums n terms of magnitude sum S: |err| <= (n + 16) U S, n and S from the statement.
And against itself: two runs, a cached and a rebuilt pixel order, and rows that are not 16-byte aligned through the C ABI.
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

import texture_cases as tc  # noqa: E402
import texture_statement as ts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
U = 2.0 ** -24
PARAMS = [(name, f, b) for name, (_, _, modes) in tc.TEXTURE_CASES.items() for f, b in modes]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(tex, uv, g, filt, boundary):
    import largesteps.render as dr
    t, c = dev(tex).requires_grad_(True), dev(uv).requires_grad_(True)
    out = dr.texture(t, c, filter_mode=filt, boundary_mode=boundary)
    (out * dev(g)).sum().backward()
    return out.detach().cpu().numpy(), t.grad.cpu().numpy(), c.grad.cpu().numpy()


def _rel(e, b):
    return float((e / np.maximum(b, 1e-300)).max())


@pytest.mark.parametrize("name,filt,boundary", PARAMS)
def test_native_matches_statement(name, filt, boundary):
    tex, uv, g = tc.texture_case(name, filt)
    nk = tc.texture_keys(tex.shape)
    if name.startswith("three_pass"):
        assert 65536 <= nk < 2 ** 24 and tc.radix_passes(nk) == 3
    if name.startswith("four_pass"):
        assert nk >= 2 ** 24 and tc.radix_passes(nk) == 4
    out, gt, gc = _run(tex, uv, g, filt, boundary)
    r = ts.texture(tex, uv, g, filt, boundary)
    e_out, b_out = np.abs(out - r.out).max(), 16 * U * np.abs(tex).max()
    e_t, b_t = np.abs(gt - r.grad_tex), (r.grad_tex_n[..., None] + 16) * U * r.grad_tex_abs
    e_c, b_c = np.abs(gc - r.grad_uv), (r.grad_uv_n + 16) * U * r.grad_uv_abs
    print(f"{name} {filt} {boundary}: {nk} keys; forward err/bound {e_out / b_out:.3f}; grad_tex {_rel(e_t, b_t):.3f} (max terms "
          f"{r.grad_tex_n.max()}, texels with more than 64: {(r.grad_tex_n > 64).sum()}); grad_uv {_rel(e_c, b_c):.3f}")
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(gt)) and np.all(np.isfinite(gc))
    assert e_out <= b_out
    assert np.all(e_t <= b_t), np.argwhere(e_t > b_t)[:4].tolist()
    assert np.all(e_c <= b_c), np.argwhere(e_c > b_c)[:4].tolist()
    assert np.abs(gt).max() > 0 and (filt == "nearest") == (not gc.any())
    if name == "threshold":
        n = r.grad_tex_n[0]
        for m in (64, 65, 128, 129, 700):
            assert (n == m).any(), m
        if filt == "linear":
            assert np.array_equal(n, tc.threshold_counts(tc.THRESHOLD_CLUSTERS, *tex.shape[1:3]))
            assert n[10, 21] == 65 and n[11, 21] == 65 and n[14, 31] == 64


@pytest.mark.parametrize("name", ["wide_300x5_c3", "three_pass_255x257_c3", "three_pass_own_b4_128x128_c4", "threshold", "c32"])
def test_two_runs_cached_and_rebuilt_order_are_bitwise_identical(name):
    import largesteps.render as dr
    for filt, boundary in tc.TEXTURE_CASES[name][2]:
        tex, uv, g = tc.texture_case(name, filt)
        a = _run(tex, uv, g, filt, boundary)
        b = _run(tex, uv, g, filt, boundary)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (filt, boundary)
        # one uv tensor used twice: the second backward takes the cached order
        kw = dict(filter_mode=filt, boundary_mode=boundary)
        t, c, gg = dev(tex).requires_grad_(True), dev(uv), dev(g)
        (dr.texture(t, c, **kw) * gg).sum().backward()
        slot = c._largesteps_texel_order
        assert slot.order is not None
        first, t.grad = t.grad.clone(), None
        (dr.texture(t, c, **kw) * gg).sum().backward()
        assert c._largesteps_texel_order is slot
        assert torch.equal(t.grad, first) and np.array_equal(first.cpu().numpy(), a[1]), (filt, boundary)
        # changed in place: the order is rebuilt and the result is a fresh run's
        c.add_(0.013)
        t.grad = None
        (dr.texture(t, c, **kw) * gg).sum().backward()
        assert c._largesteps_texel_order is not slot
        assert np.array_equal(t.grad.cpu().numpy(), _run(tex, c.cpu().numpy(), g, filt, boundary)[1]), (filt, boundary)


@pytest.mark.parametrize("filt,boundary", tc.ALL_MODES)
def test_c4_rows_off_alignment_give_the_aligned_bits(filt, boundary):
    """C = 4 through the C ABI with tex, out, grad_out and grad_tex starting 4 bytes into their storage: the rows move as four floats
    instead of one float4 (the Python wrapper clones such views, so only the C ABI reaches this path), same bits as the aligned call"""
    import largesteps.render as dr
    from largesteps import _native
    lib, p = _native.lib(), _native.ptr
    rng = np.random.default_rng(44)
    Bt, Ht, Wt, C, B, H, W = 2, 9, 21, 4, 2, 24, 24               # 378 texels: a second, partial workgroup
    tex, g = rng.standard_normal((Bt, Ht, Wt, C), dtype=np.float32), rng.standard_normal((B, H, W, C), dtype=np.float32)
    uv = dev(rng.uniform(-1.5, 2.5, (B, H, W, 2)).astype(np.float32))
    fi, bi = dr._FILTER_MODES[filt], dr._BOUNDARY_MODES[boundary]
    order, seg = dr._TexelOrder(None).get(uv, Bt, Ht, Wt, fi, bi)
    st = _native.stream_of(DEV)

    def shifted(a, shift):
        """a device copy of `a` (or room for one) that starts 4 * shift bytes into a fresh allocation"""
        n = int(np.prod(a.shape))
        buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
        v = buf[shift:shift + n].view(a.shape)
        v.copy_(dev(a))
        assert v.data_ptr() % 16 == 4 * shift
        return v

    results = []
    for shift in (0, 1):
        t, go = shifted(tex, shift), shifted(g, shift)
        out, gt = shifted(np.zeros_like(g), shift), shifted(np.zeros_like(tex), shift)
        gu = torch.zeros_like(uv)
        assert lib.ls_texture_forward(p(t), Bt, Ht, Wt, C, p(uv), B, H, W, fi, bi, p(out), DEV.index, st) == 0, _native.last_error()
        assert lib.ls_texture_backward(p(t), Bt, Ht, Wt, C, p(uv), B, H, W, fi, bi, p(go), p(order), p(seg), p(gt), p(gu), DEV.index,
                                       st) == 0, _native.last_error()
        torch.cuda.synchronize()
        results.append((out.clone(), gt.clone(), gu))
    for k, (x, y) in enumerate(zip(*results)):
        assert torch.equal(x, y), ("forward", "grad_tex", "grad_uv")[k]
    assert results[0][0].abs().max() > 0 and results[0][1].abs().max() > 0
    # and the aligned call is the wrapper's
    want = _run(tex, uv.cpu().numpy(), g, filt, boundary)
    for x, y in zip(results[0], want):
        assert np.array_equal(x.cpu().numpy(), y)
