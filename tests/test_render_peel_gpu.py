"""
Depth peeling of largesteps.render on the device (`DepthPeeler`) against its numpy statement
(tests/peel_statement.py: layer l of a pixel is its l-th covering fragment in (order bits of z/w, face id) order), past one sweep of
the cooperative tile walk, against the slice law layer by layer, through the backward passes against render_statement.py's, and inside
a captured step.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import peel_statement as ps  # noqa: E402
import render_statement as rs  # noqa: E402
from render_scenes import look_at, random_soup, scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
BOOST = 2.0


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _scene(name):
    return random_soup(int(name[4:])) if name.startswith("soup") else scene(name)


def _rand(shape, seed, lo=None, hi=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) if lo is None else rng.uniform(lo, hi, shape)
    return torch.from_numpy(x.astype(np.float32)).to(DEV)


def _ranges(rows):
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 2)


def peel_layers(pos, tri, H, W, n, ranges=None):
    """the first n layers of a peeler on device tensors (as the peeler returns them: each carries its frame)"""
    import largesteps.render as dr
    with dr.DepthPeeler(dr.RasterizeGLContext(), pos, tri, (H, W), ranges=ranges) as peeler:
        return [peeler.rasterize_next_layer()[0] for _ in range(n)]


# ---- 1. against the statement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_b3", "near_plane", "soup0", "soup1"])
def test_every_layer_matches_the_statement(name):
    import largesteps.render as dr
    pos, f, H, W = _scene(name)
    ref = ps.peel(pos, f, H, W)
    depth = ref.shape[0]
    assert depth == {"sphere_b3": 4, "near_plane": 1, "soup0": 14, "soup1": 12}[name]
    tp, tf = torch.from_numpy(pos).to(DEV), torch.from_numpy(f).to(DEV)
    got = peel_layers(tp, tf, H, W, depth + 2)
    assert torch.equal(got[0], dr.rasterize(None, tp, tf, (H, W))[0])
    for l in range(depth):
        g = got[l].cpu().numpy()
        assert np.array_equal(g[..., 3], ref[l][..., 3]), f"{name}, layer {l}: ids differ at {np.argwhere(g[..., 3] != ref[l][..., 3])[:5]}"
        assert ulps(g[..., :3], ref[l][..., :3]).max() <= 1, f"{name}, layer {l}: u, v, z/w beyond 1 ulp"
        assert (ref[l][..., 3] > 0).any()
    assert torch.count_nonzero(got[depth]) == 0 and torch.count_nonzero(got[depth + 1]) == 0


def test_layers_carry_their_frame_and_give_pixel_differentials():
    """a layer is a rast like any other: rast_db -> diff_attrs (instanced mode) works on it as on the rast of rasterize"""
    import largesteps.render as dr
    pos, f, H, W = scene("sphere")
    tp, tf = torch.from_numpy(pos).to(DEV), torch.from_numpy(f).to(DEV)
    attr = _rand((pos.shape[1], 2), 1, 0.0, 1.0)
    with dr.DepthPeeler(None, tp, tf, (H, W)) as peeler:
        for l in range(2):
            rast, db = peeler.rasterize_next_layer()
            assert isinstance(rast._largesteps_frame, dr._InstancedFrame) and torch.count_nonzero(db) == 0
            out, da = dr.interpolate(attr, rast, tf, rast_db=db, diff_attrs='all')
            ref_out, ref_da = dr.interpolate(attr, rast.clone(), tf, rast_db=dr.pixel_differentials(rast, tp, tf), diff_attrs='all')
            assert torch.equal(out, ref_out) and torch.equal(da, ref_da)
            assert float(da.abs().max()) > 0
            assert torch.count_nonzero(da[rast[..., 3] == 0]) == 0


# ---- 2. past one sweep of the tile walk ---------------------------------------------------------------------------------------------------
def _thirteen_quads():
    """13 full-screen quads (w = 1) at distinct dyadic depths -- but two at the same one --, the quads in shuffled order"""
    rng = np.random.default_rng(5)
    depths = np.arange(-6, 7) / 8.0                  # -0.75 .. 0.75, 0.0 among them
    depths[9] = depths[3]                            # coincident: they peel in face order
    depths = depths[rng.permutation(13)].astype(np.float32)
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float32)
    pos = np.concatenate([np.concatenate([corners, np.full((4, 1), z, np.float32), np.ones((4, 1), np.float32)], 1) for z in depths])
    tri = np.concatenate([np.array([[0, 1, 2], [0, 2, 3]]) + 4 * q for q in range(13)])
    return pos[None], tri, depths


def test_thirteen_full_screen_quads_peel_past_one_sweep_of_the_tile_walk():
    H = W = 160
    pos, tri, depths = _thirteen_quads()
    assert tri.shape == (26, 3) and 26 * (H // 16) * (W // 16) == 2600 > 2048          # RS_LARGE_GRID workgroups walk 2600 tiles
    order = sorted(range(13), key=lambda q: (depths[q], q))
    assert sum(depths[order[i]] == depths[order[i + 1]] for i in range(12)) == 1
    ref = ps.peel(pos, tri, H, W, 14)
    got = [g.cpu().numpy() for g in peel_layers(torch.from_numpy(pos).to(DEV), torch.from_numpy(tri).to(DEV), H, W, 14)]
    for l in range(13):
        quad = (got[l][..., 3].astype(np.int64) - 1) // 2
        assert np.all(got[l][..., 3] > 0) and np.all(quad == order[l]), l
        assert np.all(got[l][..., 2] == depths[order[l]]), l
        assert np.array_equal(got[l][..., 3], ref[l][..., 3]), l
        assert np.array_equal(got[l][..., 2].view(np.uint32), ref[l][..., 2].view(np.uint32)), l
        assert ulps(got[l][..., :2], ref[l][..., :2]).max() <= 1, l
    assert not got[13].any() and not ref[13].any()


# ---- 3. the slice law, layer by layer ------------------------------------------------------------------------------------------------------
def merge(parts):
    """[(pos (V_i, 4), tri (F_i, 3))] -> one pos, one tri with offset vertex ids, and the ranges [(first face, faces)] of the parts"""
    pos, tri, rows, v0, f0 = [], [], [], 0, 0
    for p, f in parts:
        pos.append(np.asarray(p, np.float32))
        tri.append(np.asarray(f, np.int64) + v0)
        rows.append((f0, len(f)))
        v0, f0 = v0 + len(p), f0 + len(f)
    return np.concatenate(pos), np.concatenate(tri), rows


def _two_meshes():
    """sphere (320 faces, depth complexity 2) and sheet (50 faces) in one vertex array at 24 x 32; ranges that overlap, are unsorted,
    cut both meshes, and one that is empty"""
    parts = [(scene(n)[0][0], scene(n)[1]) for n in ("sphere", "sheet")]
    pos, tri, rows = merge(parts)
    assert rows == [(0, 320), (320, 50)]
    rows = [(200, 170), (340, 0), (320, 50), (0, 320), (100, 250)]
    return torch.from_numpy(pos).to(DEV), torch.from_numpy(tri).to(DEV), _ranges(rows), 24, 32


def test_every_layer_of_range_mode_obeys_the_slice_law():
    import largesteps.render as dr
    pos, tri, ranges, H, W = _two_meshes()
    L = 5
    got = peel_layers(pos, tri, H, W, L, ranges=ranges)
    nonempty = [0] * L
    for b, (s, c) in enumerate(ranges.tolist()):
        if c == 0:
            ref = [torch.zeros((1, H, W, 4), device=DEV)] * L
        else:
            ref = peel_layers(pos[None], tri[s:s + c].contiguous(), H, W, L)
        for l in range(L):
            want = ref[l].clone()
            want[..., 3] += (want[..., 3] > 0) * float(s)
            assert torch.equal(got[l][b:b + 1], want), (l, b)
            nonempty[l] += int(torch.count_nonzero(want[..., 3]))
    assert got[0]._largesteps_frame.tab is not None and isinstance(got[2]._largesteps_frame, dr._RangeFrame)
    assert nonempty[0] > nonempty[1] > nonempty[2] > 0 and nonempty[4] == 0, nonempty
    assert torch.equal(got[0], dr.rasterize(None, pos, tri, (H, W), ranges=ranges)[0])


# ---- 4. gradients --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gradient_case(name):
    """layers 0-2 of a scene through interpolate -> antialias -> a weighted sum: per layer the device's (attr, colour, pos) gradients
    (taken twice) and the statement's, fed the layer's rast; and the pos gradient of the three losses summed in one graph"""
    import largesteps.render as dr
    pos, f, H, W = _scene(name)
    V = pos.shape[1]
    attr = np.random.default_rng(2).uniform(0, 1, (1, V, 3)).astype(np.float32)
    tp, tf = torch.from_numpy(pos).to(DEV).requires_grad_(True), torch.from_numpy(f).to(DEV)
    ta = torch.from_numpy(attr).to(DEV).requires_grad_(True)
    losses, device, statement = [], [], []
    with dr.DepthPeeler(None, tp, tf, (H, W)) as peeler:
        for l in range(3):
            rast = peeler.rasterize_next_layer()[0]
            col = dr.interpolate(ta, rast, tf)[0]
            out = dr.antialias(col, rast, tp, tf, pos_gradient_boost=BOOST)
            g = _rand(tuple(out.shape), 3 + l)
            loss = (out * g).sum()
            runs = [[t.cpu().numpy() for t in torch.autograd.grad(loss, [ta, col, tp], retain_graph=True)] for _ in range(2)]
            r, c, gn = rast.detach().cpu().numpy(), col.detach().cpu().numpy(), g.cpu().numpy()
            gc_ref, gp_aa = rs.antialias_backward(c, r, pos, f, gn, boost=BOOST)
            ga_ref, gr_ref = rs.interpolate_backward(attr, r, f, gc_ref)
            gp_ref = gp_aa + rs.rasterize_backward(pos, f, r, gr_ref)
            losses.append(loss)
            device.append(runs)
            statement.append((ga_ref, gc_ref, gp_ref, int((r[..., 3] > 0).sum())))
    total = torch.autograd.grad(losses[0] + losses[1] + losses[2], [tp])[0].cpu().numpy()
    return device, statement, total


@pytest.mark.parametrize("layer", [1, 2])
@pytest.mark.parametrize("name", ["sphere_b3", "soup0"])
def test_gradients_of_a_layer_match_the_statement(name, layer):
    device, statement, _ = _gradient_case(name)
    (ga, gc, gp), again = device[layer]
    ga_ref, gc_ref, gp_ref, covered = statement[layer]
    assert covered > 0 and np.abs(gp_ref).max() > 0 and np.abs(ga_ref).max() > 0
    np.testing.assert_allclose(gc, gc_ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ga, ga_ref, rtol=1e-4, atol=1e-4)
    scale = np.abs(gp_ref).max()
    print(f"{name}, layer {layer}: {covered} covered pixels, pos gradient error {np.abs(gp - gp_ref).max():.3e}, scale {scale:.3e}")
    assert np.abs(gp - gp_ref).max() <= 2e-4 * max(scale, 1.0)
    assert np.all(gp[..., 2] == 0)
    for x, y in zip((ga, gc, gp), again):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["sphere_b3", "soup0"])
def test_losses_of_three_layers_in_one_graph_sum_their_gradients(name):
    _, statement, total = _gradient_case(name)
    gp_ref = statement[0][2] + statement[1][2] + statement[2][2]
    scale = np.abs(gp_ref).max()
    print(f"{name}: pos gradient error of layers 0-2 {np.abs(total - gp_ref).max():.3e}, scale {scale:.3e}")
    assert np.abs(total - gp_ref).max() <= 2e-4 * max(scale, 1.0)
    assert np.all(total[..., 2] == 0)


def test_a_layer_past_the_deepest_gives_zero_gradients():
    import largesteps.render as dr
    pos, f, H, W = scene("near_plane")
    tp, tf = torch.from_numpy(pos).to(DEV).requires_grad_(True), torch.from_numpy(f).to(DEV)
    with dr.DepthPeeler(None, tp, tf, (H, W)) as peeler:
        rasts = [peeler.rasterize_next_layer()[0] for _ in range(3)]
    assert torch.count_nonzero(rasts[0]) > 0 and torch.count_nonzero(rasts[2]) == 0
    (rasts[2] * _rand(tuple(rasts[2].shape), 1)).sum().backward()
    assert tp.grad is not None and torch.count_nonzero(tp.grad) == 0


def _layer_chain(make_peeler, lift, pos, tri, attr, g, layer):
    """layer `layer` -> interpolate -> antialias -> sum(out g), backward; pos enters the peeler and antialias through two leaves"""
    import largesteps.render as dr
    p_rast, p_aa, a = pos.clone().requires_grad_(True), pos.clone().requires_grad_(True), attr.clone().requires_grad_(True)
    with make_peeler(lift(p_rast)) as peeler:
        for _ in range(layer + 1):
            rast = peeler.rasterize_next_layer()[0]
    out = dr.antialias(dr.interpolate(a, rast, tri)[0], rast, lift(p_aa), tri, pos_gradient_boost=BOOST)
    (out * g).sum().backward()
    return [t.detach() for t in (rast, out, p_rast.grad, p_aa.grad, a.grad)]


def test_range_mode_gradients_of_layer_one_obey_the_slice_law():
    import largesteps.render as dr
    pos, tri, ranges, H, W = _two_meshes()
    attr, g = _rand((pos.shape[0], 3), 2, 0.0, 1.0), _rand((ranges.shape[0], H, W, 3), 3)
    got = _layer_chain(lambda p: dr.DepthPeeler(None, p, tri, (H, W), ranges=ranges), lambda p: p, pos, tri, attr, g, 1)
    per = []
    for b, (s, c) in enumerate(ranges.tolist()):
        if c == 0:          # by definition an all-zero image that no gradient of pos or attr passes through
            per.append([torch.zeros((1, H, W, 4), device=DEV), torch.zeros((1, H, W, 3), device=DEV), torch.zeros_like(pos),
                        torch.zeros_like(pos), torch.zeros_like(attr)])
            continue
        tri_b = tri[s:s + c].contiguous()
        one = _layer_chain(lambda p: dr.DepthPeeler(None, p, tri_b, (H, W)), lambda p: p[None], pos, tri_b, attr, g[b:b + 1], 1)
        one[0] = one[0].clone()
        one[0][..., 3] += (one[0][..., 3] > 0) * float(s)
        per.append(one)
    assert torch.equal(got[0], torch.cat([x[0] for x in per], 0)) and torch.equal(got[1], torch.cat([x[1] for x in per], 0))
    for i, what in ((2, "pos through rasterize"), (3, "pos through antialias"), (4, "attr")):
        acc = per[0][i].clone()
        for b in range(1, len(per)):
            acc = acc + per[b][i]
        assert float(acc.abs().max()) > 0, what
        assert torch.equal(got[i], acc), what


# ---- 5. isolation and misuse ---------------------------------------------------------------------------------------------------------------
def test_layers_come_from_the_peelers_own_copy_and_misuse_raises():
    import largesteps.render as dr
    pos, f, H, W = scene("sphere_b3")
    tp, tf = torch.from_numpy(pos).to(DEV), torch.from_numpy(f).to(DEV)
    want = peel_layers(tp, tf, H, W, 3)
    peeler = dr.DepthPeeler(None, tp, tf, (H, W))
    with pytest.raises(RuntimeError, match="`with` block"):
        peeler.rasterize_next_layer()
    with peeler:
        first = peeler.rasterize_next_layer()[0]
        first.zero_()
        second = peeler.rasterize_next_layer()[0]
        assert torch.equal(second, want[1]) and torch.count_nonzero(want[1]) > 0
        second[..., 2:] += 1.0
        assert torch.equal(peeler.rasterize_next_layer()[0], want[2]) and torch.count_nonzero(want[2]) > 0
        tp[0, 0, 0] += 0.0                                         # in place: the version counter moves
        with pytest.raises(ValueError, match="in place"):
            peeler.rasterize_next_layer()
    with pytest.raises(RuntimeError, match="`with` block"):
        peeler.rasterize_next_layer()
    assert peeler._prev is None and peeler._args is None


# ---- 6. captured ---------------------------------------------------------------------------------------------------------------------------
def test_three_captured_layers_match_eager():
    import largesteps.render as dr
    from largesteps import synthetic
    from largesteps.capture import CapturedStep
    H = W = 48
    v, f = synthetic.icosphere(5)
    tf = torch.from_numpy(f).to(DEV)
    mvp = (dr.persp_proj(45.0, 1.0, 0.1, 100.0).double() @ torch.from_numpy(look_at((0.8, 0.6, -3.0)))).float().to(DEV)
    attr = _rand((v.shape[0], 3), 4, 0.0, 1.0)

    def render(x):
        pos = torch.matmul(torch.nn.functional.pad(x, (0, 1), 'constant', 1.0), mvp.t()).contiguous()[None]
        outs = []
        with dr.DepthPeeler(None, pos, tf, (H, W)) as peeler:
            for _ in range(3):
                rast = peeler.rasterize_next_layer()[0]
                outs.append(dr.antialias(dr.interpolate(attr, rast, tf)[0], rast, pos, tf))
        return outs

    with torch.no_grad():
        ref = render(torch.from_numpy(v).to(DEV))
    assert float(ref[0].abs().sum()) > 0 and float(ref[1].abs().sum()) > 0 and float(ref[2].abs().sum()) == 0       # a sphere: two layers

    def make():
        x = torch.from_numpy(np.ascontiguousarray(0.8 * v, np.float32)).to(DEV).requires_grad_(True)

        def body():
            loss = sum((o - r).abs().mean() for o, r in zip(render(x), ref))
            x.grad = None
            loss.backward()
            with torch.no_grad():
                x.add_(x.grad, alpha=-0.5)
            return loss
        return x, body

    x1, body1 = make()
    eager = [float(body1().detach()) for _ in range(4)]
    x2, body2 = make()
    step = CapturedStep(body2, warmup=2)
    captured = [float(step().detach()) for _ in range(2)]
    torch.cuda.synchronize()
    np.testing.assert_allclose(captured, eager[2:], rtol=1e-5)
    np.testing.assert_allclose(x2.detach().cpu().numpy(), x1.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert len(set(eager)) == 4 and eager[0] > 0
