"""
csrc/adam.hip through largesteps.optimize.AdamUniform against tests/adam_statement.py (numpy; itself held to the reference's recorded
trajectory and to fp64 by tests/test_adam_statement_cpu.py): the parameters and both saved moments BIT FOR BIT after every step.

The launch is capped at 1024 workgroups of 256 threads, so past 262144 items (of 16 or of 4 bytes) the element loops take further
sweeps and the second kernel reduces 1024 partial maxima in four strides; the one number that scales every parameter is the global
maximum, and a sweep, a tail thread or a slot that loses it makes every step orders of magnitude too large without any other sign.
Hence: every size at which the launch changes shape (adam_statement.SIZES, printed with its layout), the one outstanding gradient
at every position where a loop or a reduction could lose it (adam_statement.spikes), the 4-byte path reached from either side
(parameter or gradient misaligned), NaN / infinity / subnormals / zero betas / zero step size, a far step number, the device-side
step counter (capturable=True) eagerly and replayed from a captured graph, several parameters and groups on the one scratch buffer
of the device, and the argument checks of the Python layer.

The device computes pow() itself in capturable mode and may round a bias correction one fp32 ulp away from the host's; there the
parameters must equal the statement bit for bit for ONE pair of corrections among host value / next below / next above, the same
pair for all elements (which pair is printed); the moments do not depend on the corrections and are always the statement's bits.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import adam_statement as st  # noqa: E402
from adam_statement import LR, BETAS, SIZES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
F32 = np.float32
SHIFT = {"16B": 0, "4B": 1}                      # floats between the start of the storage and the parameter / gradient
ALL_SIZES = [(path, n) for path in SIZES for n in SIZES[path]]
WRAPPED = {"16B": 4 * 262144 + 7, "4B": 262145}  # the smallest size per path with a second sweep (and, 16B, a full tail)
BIG = 1e3                                        # the outstanding gradient element, a million times the others


@functools.lru_cache(maxsize=None)
def case(n, steps=3):
    """p0 and the gradients of a size: computed once, shared by the tests, never written to (the tests copy before they place a value)"""
    p0, grads = st.inputs(n, steps, seed=n % 9973)
    p0.setflags(write=False)
    for g in grads:
        g.setflags(write=False)
    return p0, grads


def shifted(a, shift):
    """a copy of `a` on the device that starts `shift` floats into its storage"""
    a = np.array(a, F32)                         # a writable copy: the shared inputs are read-only
    store = torch.zeros(a.size + shift, device=DEV)
    view = store[shift:].view(a.shape) if shift else store.view(a.shape)
    view.copy_(torch.from_numpy(a).to(DEV))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * shift) % 16
    return view


class Run:
    """one parameter under an AdamUniform of its own; step(g) returns (p, g1, g2) as numpy"""

    def __init__(self, p0, p_shift=0, g_shift=0, lr=LR, betas=BETAS, capturable=False):
        from largesteps.optimize import AdamUniform
        self.p = torch.nn.Parameter(shifted(p0, p_shift))
        self.g_shift = g_shift
        self.opt = AdamUniform([self.p], lr=lr, betas=betas, capturable=capturable)

    @property
    def state(self):
        return self.opt.state[self.p]

    def read(self):
        torch.cuda.synchronize(DEV)
        return tuple(t.detach().cpu().numpy().copy() for t in (self.p, self.state["g1"], self.state["g2"]))

    def step(self, g):
        self.p.grad = shifted(g, self.g_shift)
        self.opt.step()
        return self.read()

    def layout(self):
        """the launch as the native code sees it: from the four pointers it gets"""
        s = self.state
        aligned = all(t.data_ptr() % 16 == 0 for t in (self.p, self.p.grad, s["g1"], s["g2"]))
        return st.layout(self.p.numel(), aligned)


def assert_bits(got, want, what):
    ok = st.same_bits(got, want)
    if not ok.all():
        j = int(np.flatnonzero(~ok.ravel())[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} values differ from the statement, first at element {j}: "
                             f"device {got.ravel()[j]!r}, statement {want.ravel()[j]!r}")


def assert_step(got, want, what):
    for g, w, name in zip(got, want, ("p", "g1", "g2")):
        assert g.dtype == F32 and g.shape == w.shape
        assert_bits(g, w, f"{what}, {name}")


def describe(path, n, L):
    return f"adam {path} n = {n}: vec {L['vec']}, G {L['G']}, sweeps {L['sweeps']}, pmax_strides {L['pmax_strides']}, tail {L['tail']}"


def with_spike(g, j, value=BIG):
    g = g.copy()
    g[j] = value
    return g


# ---- every size, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,n", ALL_SIZES, ids=[f"{p}-{n}" for p, n in ALL_SIZES])
def test_three_steps_are_the_statement_bit_for_bit(path, n):
    """gradients U(-1, 1) 1e-3 and, in step k, one element of 10^k at a seeded position of `spikes`: the maximum moves every step"""
    p0, grads = case(n)
    rng = np.random.default_rng(n)
    at = st.spikes(n, path == "16B")
    grads = [with_spike(g, int(rng.choice(at)), 10.0 ** k) for k, g in enumerate(grads, 1)]
    want = st.run32(p0, grads, LR, *BETAS)
    run = Run(p0, SHIFT[path], SHIFT[path])
    for k, g in enumerate(grads):
        got = run.step(g)
        if k == 0:
            L = run.layout()
            print(describe(path, n, L))
            assert L == st.layout(n, path == "16B")
        assert np.isfinite(want[k][0]).all()
        assert_step(got, want[k], f"{path} n = {n} step {k + 1}")
        assert run.state["step"] == k + 1 and type(run.state["step"]) is int
    assert set(run.state.keys()) == {"step", "g1", "g2"}


# ---- where the maximum sits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,n", [(path, n) for path in SIZES for n in SIZES[path][-2:]])
def test_the_largest_gradient_is_found_wherever_it_sits(path, n):
    """|g| <= 1e-3 but g[j] = 1e3, for every j of `spikes`. Bitwise the statement; and in plain words: no parameter moves further than
    lr (1 + 2^-20) -- without the element in the maximum, its parameter would move a million times further. (The parameter under
    the spike starts at 0, so that the bound holds the step and not the rounding of p - step, half an ulp of p.)"""
    p0, grads = case(n)
    L = st.layout(n, path == "16B")
    print(describe(path, n, L), "spikes", st.spikes(n, path == "16B"))
    assert L["sweeps"] >= 2 and L["pmax_strides"] == 4
    for j in st.spikes(n, path == "16B"):
        p, g = with_spike(p0, j, 0.0), with_spike(grads[0], j)
        want = st.run32(p, [g], LR, *BETAS)[0]
        run = Run(p, SHIFT[path], SHIFT[path])
        got = run.step(g)
        assert run.layout() == L
        moved = float(np.abs(got[0].astype(np.float64) - p).max())
        assert moved <= LR * (1 + 2.0 ** -20), f"{path} n = {n}, spike at {j}: a parameter moved by {moved:.3g}, lr is {LR}"
        assert moved >= LR * (1 - 2.0 ** -20)
        assert_step(got, want, f"{path} n = {n}, spike at {j}")


# ---- mixed alignment ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_shift,g_shift", [(0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)])
def test_one_misaligned_array_takes_the_4_byte_path(p_shift, g_shift):
    n = 4 * 262144 + 7
    p0, grads = case(n)
    grads = [with_spike(g, j) for g, j in zip(grads, (n - 1, 4 * 262144, 4 * 1023 * 256))]
    want = st.run32(p0, grads, LR, *BETAS)
    run = Run(p0, p_shift, g_shift)
    for k, g in enumerate(grads):
        got = run.step(g)
        L = run.layout()
        assert L["vec"] == 0 and L["sweeps"] == 5 and L == st.layout(n, False)
        assert_step(got, want[k], f"parameter + {p_shift}, gradient + {g_shift} floats, step {k + 1}")


# ---- special values -------------------------------------------------------------------------------------------------------------------
def special(kind, n, j):
    """(p0, three gradients, lr, betas) of a special case with its value at element j"""
    p0, grads = case(n)
    grads, lr, betas = [g.copy() for g in grads], LR, BETAS
    if kind == "nan":
        grads[1][j] = np.nan
    elif kind == "inf":
        grads[1][j] = np.inf                      # step 2 of 3: after a finite step, and a finite gradient follows
    elif kind == "zero":
        grads = [np.zeros(n, F32) for _ in grads]
    elif kind == "tiny":                          # squares are subnormal: g2 shows whether they are kept
        grads = [with_spike(g * F32(1e-17), j, 1e-19) for g in grads]
    elif kind == "zero_betas":
        grads, betas = [with_spike(g, j) for g in grads], (0.0, 0.0)
    elif kind == "zero_lr":
        grads, lr = [with_spike(g, j) for g in grads], 0.0
    return p0, grads, lr, betas


@pytest.mark.parametrize("kind", ["nan", "inf", "zero", "tiny", "zero_betas", "zero_lr"])
@pytest.mark.parametrize("path", list(SIZES))
def test_special_values_are_the_statement(path, kind):
    n = WRAPPED[path]
    assert st.layout(n, path == "16B")["sweeps"] == 2
    for j in st.spikes(n, path == "16B") if kind != "zero" else [0]:
        p0, grads, lr, betas = special(kind, n, j)
        want = st.run32(p0, grads, lr, *betas)
        run = Run(p0, SHIFT[path], SHIFT[path], lr=lr, betas=betas)
        got = [run.step(g) for g in grads]
        assert run.layout() == st.layout(n, path == "16B")
        for k in range(3):
            assert_step(got[k], want[k], f"{kind} at {j}, {path} n = {n}, step {k + 1}")
        # what the statement itself says in each case (tests/test_adam_statement_cpu.py has the reference's rule agree)
        others = np.arange(n) != j
        if kind == "nan":
            assert np.isfinite(got[0][0]).all() and np.isnan(got[1][0]).all() and np.isnan(got[2][0]).all()
        elif kind == "inf":
            assert np.isnan(got[1][0][j]) and np.isnan(got[2][0][j])
            assert np.array_equal(got[1][0][others], got[0][0][others]) and np.array_equal(got[2][0][others], got[0][0][others])
        elif kind in ("zero", "zero_lr"):
            assert np.array_equal(got[2][0].view(np.uint32), p0.view(np.uint32))
        elif kind == "tiny":
            g2 = got[0][2]
            assert 0 < g2[j] == g2.max() < np.finfo(F32).tiny, "the second moments are subnormal, and kept"


# ---- a far step number ----------------------------------------------------------------------------------------------------------------
def test_the_bias_corrections_at_a_far_step():
    assert st.inv_bias(BETAS[0], 10000) == F32(1) and F32(1) < st.inv_bias(BETAS[1], 10000) < F32(1.0001)


@pytest.mark.parametrize("path", list(SIZES))
def test_step_ten_thousand(path):
    """one ordinary step, the counter set to 9999, one more step: t = 10000, where b1^t has underflowed out of 1 - b1^t"""
    n = WRAPPED[path]
    p0, grads = case(n)
    run = Run(p0, SHIFT[path], SHIFT[path])
    p, a, v = st.step32(p0, np.zeros(n, F32), np.zeros(n, F32), grads[0], LR, *BETAS, 1)
    assert_step(run.step(grads[0]), (p, a, v), f"{path} step 1")
    run.state["step"] = 9999
    want = st.step32(p, a, v, grads[1], LR, *BETAS, 10000)
    assert_step(run.step(grads[1]), want, f"{path} step 10000")
    assert run.state["step"] == 10000


# ---- the step counter on the device ---------------------------------------------------------------------------------------------------
def assert_capturable_step(before, got, g, lr, betas, t, what):
    """`got` = the device's (p, g1, g2) after step t from ITS OWN (p, g1, g2) `before`: the moments are the statement's bits, and so
    are the parameters for one pair of bias corrections within an fp32 ulp of the host's. Returns that pair as offsets in ulps."""
    a, v = st.moments32(before[1], before[2], g, *betas)
    assert_bits(got[1], a, f"{what}, g1")
    assert_bits(got[2], v, f"{what}, g2")
    c1, c2 = st.inv_c_pair(*betas, t)
    near = lambda c, d: c if d == 0 else np.nextafter(c, F32(d * np.inf))      # noqa: E731
    for d1, d2 in sorted(((d1, d2) for d1 in (0, -1, 1) for d2 in (0, -1, 1)), key=lambda d: abs(d[0]) + abs(d[1])):
        p = st.apply32(before[0], a, lr, near(c1, d1), st.scale32(v, near(c2, d2)))
        if st.same_bits(got[0], p).all():
            return d1, d2
    p = st.apply32(before[0], a, lr, c1, st.scale32(v, c2))
    assert_bits(got[0], p, f"{what}: no pair of bias corrections within an ulp of the host's gives the device's parameters; with the host's, p")
    raise AssertionError(what)


@pytest.mark.parametrize("path,n", ALL_SIZES, ids=[f"{p}-{n}" for p, n in ALL_SIZES])
def test_the_device_side_counter_gives_the_same_steps(path, n):
    p0, grads = case(n)
    grads = [with_spike(g, j) for g, j in zip(grads, (0, n - 1, n // 2))]
    run = Run(p0, SHIFT[path], SHIFT[path], capturable=True)
    before, pairs = (p0, np.zeros(n, F32), np.zeros(n, F32)), []
    for k, g in enumerate(grads, 1):
        got = run.step(g)
        pairs.append(assert_capturable_step(before, got, g, LR, BETAS, k, f"{path} n = {n} step {k}"))
        counter = run.state["step"]
        assert counter.dtype == torch.int32 and int(counter[0]) == k
        before = got
    assert run.layout() == st.layout(n, path == "16B")
    print(f"adam {path} n = {n}, device-side counter: bias corrections (inv_c1, inv_c2) in ulps from the host's, per step: {pairs}")


@pytest.mark.parametrize("path", list(SIZES))
def test_step_ten_thousand_on_the_device_side_counter(path):
    n = WRAPPED[path]
    p0, grads = case(n)
    run = Run(p0, SHIFT[path], SHIFT[path], capturable=True)
    before = run.step(grads[0])
    run.state["step"].copy_(torch.tensor([9999, 0], dtype=torch.int32))
    got = run.step(grads[1])
    pair = assert_capturable_step(before, got, grads[1], LR, BETAS, 10000, f"{path} step 10000")
    assert run.state["step"].tolist()[0] == 10000
    print(f"adam {path} n = {n}, device-side counter at t = 10000: bias corrections in ulps from the host's: {pair}")


def test_a_captured_step_past_one_sweep():
    """two warm-up steps on a side stream, opt.step() captured with a static gradient buffer, three replays with new gradients"""
    n = WRAPPED["16B"]
    p0, grads = case(n, steps=5)
    grads = [with_spike(g, j) for g, j in zip(grads, st.spikes(n, True)[-5:])]
    run = Run(p0, capturable=True)
    static = shifted(grads[0], 0)
    run.p.grad = static
    before, pairs = (p0, np.zeros(n, F32), np.zeros(n, F32)), []

    def check(k):
        nonlocal before
        got = run.read()
        pairs.append(assert_capturable_step(before, got, grads[k], LR, BETAS, k + 1, f"step {k + 1}"))
        before = got

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for k in range(2):
            static.copy_(torch.from_numpy(grads[k]).to(DEV))
            run.opt.step()
            side.synchronize()
            check(k)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.opt.step()
    assert run.p.grad is static and int(run.state["step"][0]) == 2, "capturing runs nothing"
    for k in range(2, 5):
        static.copy_(torch.from_numpy(grads[k]).to(DEV))
        graph.replay()
        check(k)
    assert int(run.state["step"][0]) == 5
    assert run.layout() == st.layout(n, True) and run.layout()["sweeps"] == 2
    print(f"adam captured step n = {n}: bias corrections in ulps from the host's, per step: {pairs}")


# ---- several parameters and groups on the one scratch buffer --------------------------------------------------------------------------
def several(sizes_spikes, settings, order):
    """one optimizer over the parameters (n, spike or None) with one group per entry of `settings`; three steps. Every parameter
    against the statement run on it alone."""
    from largesteps.optimize import AdamUniform
    params, inputs = [], []
    for n, j in sizes_spikes:
        p0, grads = case(n)
        grads = [g if j is None else with_spike(g, j) for g in grads]
        params.append(torch.nn.Parameter(shifted(p0, 0)))
        inputs.append((p0, grads))
    if len(set(settings)) == 1:
        opt = AdamUniform([params[i] for i in order], lr=settings[0][0], betas=settings[0][1])
    else:
        opt = AdamUniform([dict(params=[params[i]], lr=settings[i][0], betas=settings[i][1]) for i in order])
    want = [st.run32(p0, grads, lr, *betas) for (p0, grads), (lr, betas) in zip(inputs, settings)]
    for k in range(3):
        for p, (_, grads) in zip(params, inputs):
            p.grad = shifted(grads[k], 0)
        opt.step()
        torch.cuda.synchronize(DEV)
        for i, p in enumerate(params):
            got = tuple(t.detach().cpu().numpy() for t in (p, opt.state[p]["g1"], opt.state[p]["g2"]))
            assert_step(got, want[i][k], f"parameter {i} of {len(params)} (n = {p.numel()}), order {order}, step {k + 1}")


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["large_first", "small_first"])
def test_two_parameters_share_the_scratch_without_sharing_a_maximum(order):
    """A: 3 2^20 + 3 floats with one gradient of 1e3 in the last slot of the partial maxima; B: 5 floats with gradients of 1e-3.
    A partial maximum of A left in the scratch would scale B's step down a million times"""
    n = 3 * 2 ** 20 + 3
    several([(n, 4 * 1023 * 256), (5, None)], [(LR, BETAS), (LR, BETAS)], order)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["large_first", "small_first"])
def test_two_groups_follow_their_own_settings(order):
    several([(WRAPPED["16B"], WRAPPED["16B"] - 1), (4 * 256 + 1, None)], [(0.05, (0.9, 0.999)), (0.5, (0.5, 0.9))], order)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------
def test_a_transposed_gradient_gives_the_bits_of_the_contiguous_one():
    from largesteps.optimize import AdamUniform
    V = 1025
    p0, grads = case(3 * V)
    out = []
    for transposed in (False, True):
        p = torch.nn.Parameter(shifted(p0.reshape(V, 3), 0))
        opt = AdamUniform([p], lr=LR, betas=BETAS)
        for g in grads:
            g = shifted(g.reshape(V, 3), 0)
            p.grad = g.t().contiguous().t() if transposed else g
            assert p.grad.is_contiguous() != transposed and p.grad.shape == (V, 3)
            opt.step()
        out.append(tuple(t.detach().cpu().numpy().reshape(-1) for t in (p, opt.state[p]["g1"], opt.state[p]["g2"])))
    want = st.run32(p0, grads, LR, *BETAS)[-1]
    assert_step(out[0], want, "contiguous gradient")
    assert_step(out[1], want, "transposed gradient")


def test_what_the_python_layer_refuses_and_what_it_lets_pass():
    from largesteps.optimize import AdamUniform

    def step(p):
        p = torch.nn.Parameter(p)
        p.grad = torch.zeros_like(p)
        AdamUniform([p], lr=LR).step()
        return p

    with pytest.raises(TypeError, match="float32"):
        step(torch.zeros(8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        step(torch.zeros(4, 6, device=DEV)[:, ::2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        step(torch.zeros(8))
    for capturable in (False, True):
        p = torch.nn.Parameter(torch.zeros(0, 3, device=DEV))
        p.grad = torch.zeros_like(p)
        opt = AdamUniform([p], lr=LR, capturable=capturable)
        opt.step()
        opt.step()
        torch.cuda.synchronize(DEV)
        assert p.shape == (0, 3) and opt.state[p]["g1"].shape == (0, 3)
        assert capturable or opt.state[p]["step"] == 2
