"""
largesteps.distance's winding number and signed distance on the device (csrc/winding.hip) against tests/winding_statement.py: the exact
kernel against the exact sum at every LDS tile and workgroup boundary, the node moments against their definitions on the hierarchy the
device exports, the walk against the statement's walk fed the device's own arrays and moments (so every open / accept decision compares
the same numbers), the handle's behaviour (update, reproducibility, a captured graph, a mesh far from the origin) and signed_distance.

Tolerance of a winding number of T faces against the statement: T 2^-50 max(1, sum |terms|), the sum taken from the statement.
Everything but atan2 is + - x / sqrt and can match bit for bit; atan2 is within a few ulp on both sides; T additions round once each;
2^-50 leaves a factor 8 over that.
"""
import numpy as np
import pytest
import torch

import winding_statement as ws
from test_winding_cpu import queries, sphere, tol
from largesteps import synthetic

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def to(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def handle(v, f, dev, cls=None):
    from largesteps.distance import MeshDistance
    return (cls or MeshDistance)(*to(dev, v, f))


def export(m):
    """the hierarchy and the moments of a handle, as the statement takes them"""
    from largesteps import _native
    T = m._f.shape[0]
    N = 2 * T - 1
    i32 = dict(dtype=torch.int32, device=m.device)
    left, right, esc, tri = torch.zeros(max(T - 1, 1), **i32), torch.zeros(max(T - 1, 1), **i32), torch.zeros(N, **i32), torch.zeros(T, **i32)
    box = torch.zeros((N, 6), dtype=torch.float32, device=m.device)
    mom = torch.zeros((N, ws.STRIDE), dtype=torch.float64, device=m.device)
    buf = m._moments()
    with torch.cuda.device(m.device):
        _native.check(_native.lib().ls_mesh_winding_arrays(m._h, _native.ptr(buf), _native.ptr(left), _native.ptr(right), _native.ptr(esc),
                                                           _native.ptr(tri), _native.ptr(box), _native.ptr(mom), _native.stream_of(m.device)))
    arrays = dict(left=left.cpu().numpy()[:T - 1], right=right.cpu().numpy()[:T - 1], esc=esc.cpu().numpy(), tri=tri.cpu().numpy(),
                  box=box.cpu().numpy(), V=m.V.cpu().numpy(), F=m._f.cpu().numpy())
    return arrays, mom.cpu().numpy()


def degenerate():
    """the sphere plus repeated-index faces, a collinear one and one that is a single point"""
    v, f = sphere()
    v = np.concatenate([v, F32([[0.5, 0.5, 0.5], [0.75, 0.75, 0.75], [1.0, 1.0, 1.0]])])
    k = v.shape[0] - 3
    extra = np.array([[0, 1, 1], [5, 5, 5], [k, k + 1, k + 2], [7, 7, 9]])
    return v, np.concatenate([f[:300], extra, f[300:]])


def mesh(name):
    if name == "single":
        return np.array([[0, 0, 0], [1, 0, 0], [0.25, 1, 0.5]], dtype=F32), np.array([[0, 1, 2]])
    if name == "pair":
        return np.array([[0, 0, 0], [1, 0, 0], [0.25, 1, 0.5], [1, 1, -0.25]], dtype=F32), np.array([[0, 1, 2], [1, 3, 2]])
    if name == "degenerate":
        return degenerate()
    if name == "ico32":
        v, f = synthetic.icosphere(32)
        return synthetic.perturb(v, radial=0.01, seed=4).astype(F32), np.asarray(f, dtype=np.int64)
    v, f = sphere()
    return (v, f) if name == "ico6" else (v, f[:int(name[3:])])           # "cut256": the first 256 faces, an open mesh


# ---- the exact kernel ------------------------------------------------------------------------------------------------------------------
CUTS = [1, 256, 257, 720]                   # a single face; a full, a just-over and a partial last LDS tile
COUNTS = [1, 255, 256, 257, 70000]
_exact = {}


def exact_reference():
    """70 000 queries against the sphere's first 1, 256, 257 and 720 faces: one pass over the terms, the running sum read at each cut"""
    if not _exact:
        v, f = sphere()
        rng = np.random.default_rng(11)
        P, _ = queries(v, f, seed=5, per=200, box=800)
        P = np.concatenate([P, rng.normal(scale=0.8, size=(COUNTS[-1] - P.shape[0] - 4, 3)).astype(F32),
                            F32([[np.nan, 0, 0], [0, -np.inf, 0], v[f[0, 0]], v[f[700]].astype(np.float64).mean(0)])])
        w, s = np.empty((len(CUTS), P.shape[0])), np.empty((len(CUTS), P.shape[0]))
        for i in range(0, P.shape[0], 4096):
            t = ws.solid_angles(P[i:i + 4096], v, f)
            run, mag = np.cumsum(t, axis=1), np.cumsum(np.abs(t), axis=1)
            for k, c in enumerate(CUTS):
                w[k, i:i + 4096], s[k, i:i + 4096] = run[:, c - 1], mag[:, c - 1]
        w[:, ~np.isfinite(P.astype(np.float64)).all(1)] = np.nan
        _exact.update(v=v, f=f, P=P, w=w, s=s)
    return _exact


@pytest.mark.parametrize("T", CUTS)
def test_the_exact_kernel_adds_every_face_in_order(T, dev):
    ref = exact_reference()
    k = CUTS.index(T)
    P = ref["P"]
    with handle(ref["v"], ref["f"][:T], dev) as m:
        for n in COUNTS:
            # the last n rows for the small counts, so that the non-finite queries and the ones on the surface are in every run
            sel = slice(P.shape[0] - n, P.shape[0])
            got = m.winding_number(to(dev, P[sel])[0], beta=np.inf).cpu().numpy()
            want, s = ref["w"][k, sel], ref["s"][k, sel]
            nan = np.isnan(want)
            assert nan.sum() == (2 if n > 4 else 0) and np.array_equal(np.isnan(got), nan)
            err = np.abs(got - want)[~nan]
            print(f"T = {T}, n = {n}: largest deviation {err.max():.2e} (allowed from {tol(T, s[~nan]).min():.2e})")
            assert (err <= tol(T, s[~nan])).all()


# ---- the moments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single", "pair", "ico6", "ico32", "degenerate"])
def test_the_moments_are_their_definitions(name, dev):
    """tolerance 2^-40 Ar R^k for the moment of order k of a node of area Ar, R the diagonal of the mesh's box; p and r to 2^-40 R. The
    re-centring of csrc/winding.hip cancels to about Ar R^k 2^-50; 2^-40 is headroom"""
    v, f = mesh(name)
    with handle(v, f, dev) as m:
        arrays, got = export(m)
    T = f.shape[0]
    assert T == {"single": 1, "pair": 2, "ico6": 720, "ico32": 20480, "degenerate": 724}[name]
    want = ws.moments(arrays)
    v64 = v.astype(np.float64)
    R = float(np.linalg.norm(v64.max(0) - v64.min(0)))
    e = 2.0 ** -40
    Ar = want[:, ws.AR_]
    dev_p = np.abs(got[:, :4] - want[:, :4]).max()
    print(f"{name}: p, r deviate by {dev_p / R:.2e} R")
    assert dev_p <= e * R
    for lo, hi, k in ((ws.N_, ws.AR_ + 1, 0), (ws.C_, ws.T_, 1), (ws.T_, ws.T_ + 18, 2)):
        d = np.abs(got[:, lo:hi] - want[:, lo:hi]).max(1)
        scale = Ar * R ** k
        print(f"{name}: order {k} deviates by {(d[scale > 0] / scale[scale > 0]).max():.2e} Ar R^{k}")
        assert (d <= e * scale).all()
    assert not got[:, 35].any()
    if name == "degenerate":
        assert (Ar[T - 1:] <= 1e-15).sum() == 4 and (Ar[:T - 1] > 0).all()


# ---- the walk --------------------------------------------------------------------------------------------------------------------------
_walks = {}


def walk_case(name, dev):
    """(v, f, P, side, arrays, moments, device exact w, statement exact (w, s)), once per mesh"""
    if name not in _walks:
        v, f = mesh(name)
        if name in ("single", "pair"):
            rng = np.random.default_rng(3)
            P, side = (rng.normal(scale=1.5, size=(300, 3)) + [0.5, 0.5, 0]).astype(F32), np.full(300, -1)
        else:
            P, side = queries(v, f, seed=7)
        P = np.concatenate([P, F32([[np.nan, 0, 0], [0, np.inf, 0]]), v[:3]])
        side = np.concatenate([side, np.full(5, -1)])
        with handle(v, f, dev) as m:
            arrays, mom = export(m)
            we = m.winding_number(to(dev, P)[0], beta=np.inf).cpu().numpy()
        _walks[name] = (v, f, P, side, arrays, mom, we, ws.exact(P, v, f))
    return _walks[name]


@pytest.mark.parametrize("beta", [1.0, 2.0, 1e30])
@pytest.mark.parametrize("name", ["single", "pair", "ico6", "degenerate"])
def test_the_walk_is_the_statements_walk_over_the_devices_arrays(name, beta, dev):
    v, f, P, side, arrays, mom, we, (se_w, se_s) = walk_case(name, dev)
    T = f.shape[0]
    with handle(v, f, dev) as m:
        got = m.winding_number(to(dev, P)[0], beta=beta).cpu().numpy()
        again = m.winding_number(P, beta=beta)                          # numpy in, numpy out, the same bits
    assert again.dtype == np.float64 and np.array_equal(got, again, equal_nan=True)
    want, s, acc, leaves = ws.walk(P, arrays, mom, beta)
    nan = np.isnan(want)
    assert nan.sum() == 2 and np.array_equal(np.isnan(got), nan)
    err = np.abs(got - want)[~nan]
    print(f"{name}, beta {beta:g}: largest deviation {err.max():.2e}; {acc.mean():.0f} nodes accepted, {leaves.mean():.0f} leaves per query")
    assert (err <= tol(T, s[~nan])).all()
    if beta == 1e30:
        # nothing is far -- but a leaf that is a single point has r = 0 and answers with its far field, which is 0
        assert ((acc + leaves)[~nan] == T).all() and (acc <= (1 if name == "degenerate" else 0)).all()
        assert (np.abs(got - we)[~nan] <= tol(T, se_s[~nan])).all()        # the device's own exact kernel
        assert (np.abs(we - se_w)[~nan] <= tol(T, se_s[~nan])).all()
    if beta == 2.0:
        e = np.abs(got - we)[~nan]
        print(f"{name}: |w_2 - w_exact| max {e.max():.2e} mean {e.mean():.2e}")
        assert e.max() < 0.25                                              # the sign is right iff below 0.5: a condition, not an accuracy claim
        if name == "ico6":
            known = side >= 0
            assert np.array_equal(got[known] >= 0.5, side[known] == 1)


# ---- the handle ------------------------------------------------------------------------------------------------------------------------
def test_update_answers_like_a_fresh_handle_and_two_calls_agree(dev):
    from largesteps.distance import MeshDistance
    v, f = sphere()
    v2 = (v.astype(np.float64) * [1.25, 0.75, 1.0] + [0.125, 0, -0.25]).astype(F32)
    P, _ = queries(v2, f, seed=9)
    tP, = to(dev, P)
    with handle(v, f, dev) as m, handle(v2, f, dev) as fresh:
        assert m._wn is None                                  # a handle that never asks pays nothing
        before = m.winding_number(tP)
        m.update(to(dev, v2)[0])
        after, want = m.winding_number(tP), fresh.winding_number(tP)
        assert torch.equal(bits(after), bits(want)) and not torch.equal(bits(after), bits(before))
        assert torch.equal(bits(m.winding_number(tP)), bits(want))
        for x, y in zip(m.signed_distance(tP), fresh.signed_distance(tP)):
            assert torch.equal(bits(x), bits(y))
        a, b = export(m), export(fresh)
        assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1])
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            other = m.winding_number(tP, beta=3.0)
        torch.cuda.current_stream(dev).wait_stream(s)
        assert torch.equal(bits(other), bits(fresh.winding_number(tP, beta=3.0)))


def test_a_captured_graph_replays_the_eager_bits(dev):
    from largesteps.raycast import RayMesh
    v, f = sphere()
    P, _ = queries(v, f, seed=10)
    tP, = to(dev, P)
    with handle(v, f, dev, RayMesh) as m:
        def step():
            return (m.winding_number(tP),) + tuple(m.signed_distance(tP)) + (m.winding_number(tP, beta=np.inf),)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            eager = [x.clone() for x in step()]                  # prepares the moments
        torch.cuda.current_stream(dev).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        for a, b in zip(eager, out):
            assert torch.equal(bits(a), bits(b))
        assert bool((eager[1] < 0).any()) and bool((eager[1] > 0).any())


def test_a_mesh_a_thousand_diagonals_from_the_origin_still_classifies(dev):
    v, f = sphere()
    v64 = v.astype(np.float64)
    far = (v64 + 1000.0 * np.linalg.norm(v64.max(0) - v64.min(0)) * np.array([0.6, 0.0, 0.8])).astype(F32)
    P, side = queries(far, f, seed=12)
    known = side >= 0
    with handle(far, f, dev) as m:
        w2, we = m.winding_number(P), m.winding_number(P, beta=np.inf)
    want, s = ws.exact(P, far, f)
    assert (np.abs(we - want) <= tol(f.shape[0], s)).all()
    assert np.array_equal(w2[known] >= 0.5, side[known] == 1) and np.abs(w2 - we).max() < 0.25
    assert np.abs(we[known] - side[known]).max() <= 1e-9


# ---- the signed distance -----------------------------------------------------------------------------------------------------------------
def test_signed_distance_is_the_distance_with_the_sign_of_the_winding_number(dev):
    """I and C are squared_distance's bits and |S| is the bits of sqrt(sqrD) (|S|^2 returns to sqrD within the two roundings of a root and
    a square, not bit for bit: fl(fl(sqrt(x))^2) != x for about half of all x)"""
    v, f, P, side, arrays, mom, we, (se_w, _) = walk_case("ico6", dev)
    tP, = to(dev, P)
    with handle(v, f, dev) as m:
        S, I, C = m.signed_distance(tP)
        sqrD, I0, C0 = m.squared_distance(tP)
        Sn, In, Cn = m.signed_distance(P)
    assert torch.equal(I, I0) and torch.equal(bits(C), bits(C0))
    fin = ~torch.isnan(S)
    assert int((~fin).sum()) == 2 and torch.equal(bits(S.abs()[fin]), bits(torch.sqrt(sqrD)[fin]))
    assert bool(((S * S - sqrD).abs()[fin] <= 2.0 ** -51 * sqrD[fin]).all())
    assert np.array_equal(Sn, S.cpu().numpy(), equal_nan=True) and np.array_equal(In, I.cpu().numpy()) and np.array_equal(Cn, C.cpu().numpy(), equal_nan=True)
    S = S.cpu().numpy()
    ok = ~np.isnan(se_w)
    assert np.array_equal(np.isnan(S), ~ok)
    on_vertex = np.arange(P.shape[0]) >= P.shape[0] - 3
    assert (S[on_vertex] == 0).all()
    inside = se_w >= 0.5
    assert np.array_equal(S[ok & ~on_vertex] < 0, inside[ok & ~on_vertex]) and inside[side == 1].all() and not inside[side == 0].any()
    from largesteps.distance import signed_distance
    S2, I2, C2 = signed_distance(P, v, f)
    assert np.array_equal(S2, S, equal_nan=True) and np.array_equal(I2, In)


def test_signed_distance_gradients_are_the_squared_distances_scaled(dev):
    v, f, P, *_ = walk_case("ico6", dev)
    P = P[np.isfinite(P).all(1)]                                            # the last three rows lie on vertices
    n = P.shape[0]
    from largesteps.distance import MeshDistance
    G, = to(dev, np.linspace(0.5, 2.0, n) * np.where(np.arange(n) % 2, -1.0, 1.0))
    outs = []
    for signed in (True, False):
        V, tP = (x.requires_grad_() for x in to(dev, v, P))
        with MeshDistance(V, to(dev, f)[0]) as m:
            if signed:
                S, I, C = m.signed_distance(tP)
                assert S.requires_grad and not I.requires_grad and not C.requires_grad
                gP, gV = torch.autograd.grad((S * G).sum(), (tP, V))
                keep = S.detach()
            else:
                sqrD, _, _ = m.squared_distance(tP)
                d = torch.sqrt(sqrD.detach())
                s = torch.where(keep < 0, -1.0, 1.0).to(torch.float64)
                coef = torch.where(d > 0, s / (2.0 * d), torch.zeros_like(d))
                gP, gV = torch.autograd.grad((sqrD * (G * coef)).sum(), (tP, V))
        outs.append((gP, gV))
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b)) and bool(torch.isfinite(a).all())
    gP = outs[0][0]
    assert not gP[-3:].any() and bool(gP[:-3].any(1).all()) and bool(outs[0][1].any())


def test_open_doubled_flipped_and_degenerate_meshes_follow_the_rule(dev):
    from largesteps.distance import signed_distance, winding_number
    v, f = sphere()
    P, side = queries(v, f, seed=13)
    known = side >= 0
    tv, tf, tP = to(dev, v, f, P)
    w = winding_number(tv, tf, tP)
    assert isinstance(w, torch.Tensor) and w.dtype == torch.float64 and w.device == tP.device
    w = w.cpu().numpy()
    # flipped: -1 inside, so nothing is "inside" for the sign
    wf = winding_number(v, f[:, ::-1].copy(), P)
    assert np.abs(wf + w).max() < 0.01 and (signed_distance(P, v, f[:, ::-1].copy())[0] > 0).all()
    # doubled: 2 inside, still negative there
    f2 = np.concatenate([f, f])
    w2 = winding_number(v, f2, P)
    assert np.abs(w2 - 2 * w).max() < 0.01
    S2 = signed_distance(P, v, f2)[0]
    assert np.array_equal(S2[known] < 0, side[known] == 1)
    # degenerate faces add nothing
    vd, fd = degenerate()
    wd = winding_number(vd, fd, P, beta=np.inf)
    want, s = ws.exact(P, v, f)
    assert (np.abs(wd - want) <= tol(fd.shape[0], s)).all()
    assert np.abs(winding_number(vd, fd, P) - want).max() < 0.25
    # open: the upper hemisphere; the sign is that of the statement's classification
    cap = f[v.astype(np.float64)[f].mean(1)[:, 2] > 0]
    wo, _ = ws.exact(P, v, cap)
    clear = np.abs(wo - 0.5) > 0.05
    So = signed_distance(P, v, cap)[0]
    assert clear.sum() > 0.8 * P.shape[0] and np.array_equal(So[clear] < 0, wo[clear] >= 0.5)
    assert ((wo > 0.05) & (wo < 0.95)).any()
    # a non-finite query is NaN in both
    bad = F32([[np.nan, 0, 0], [0, 0, np.inf]])
    assert np.isnan(winding_number(v, f, bad)).all() and np.isnan(signed_distance(bad, v, f)[0]).all()
    with pytest.raises(ValueError, match="beta"):
        winding_number(tv, tf, tP, beta=0.999)
