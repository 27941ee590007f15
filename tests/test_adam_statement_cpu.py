"""
tests/adam_statement.py held to account without a device (tests/test_adam_gpu.py then holds csrc/adam.hip to step32 bit for bit):

- step32, run on the fixture's quadratic, gives the reference's recorded trajectory at the tolerance of test_adam_uniform, and so
  does reference32 (our wording of the reference's rule, against what the reference's code recorded);
- step32 is a legitimate fp32 evaluation of the operation: its distance from the all-fp64 rule is at most twice the distance of the
  reference's own fp32 rule. Both are fp32 evaluations of the same two recurrences and differ in three roundings (betas held in
  fp32, a reciprocal bias correction that multiplies, one root of the maximum instead of a root per element), so neither can be
  expected to beat the other by more than a small factor; 2 leaves room for that and none for a wrong rule (a dropped bias
  correction at t = 1 is a factor 10 in the step). Measured (docs/measurements.md 25): 1.00, 0.95 and 1.00;
- special values: which elements are NaN, infinite or finite, as the reference's rule has it;
- the size table of the GPU test reaches every cell of `layout`;
- the argument checks of the two C entry points that return before any device work.
The measured figures are printed (-s).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "large-steps-pytorch_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import adam_statement as st  # noqa: E402
from adam_statement import LR, BETAS, SIZES  # noqa: E402

F32 = np.float32
GOLDEN = os.path.join(HERE, "golden", "reference_golden.npz")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- against the reference's recorded trajectory --------------------------------------------------------------------------------------
def fixture_trajectory(step):
    """five steps on the fixture's quadratic sum (p - target)^2, the gradient 2 (p - target) taken in fp32 at the rule's OWN parameters"""
    g = np.load(GOLDEN)
    p, tgt, traj = g["adam/p0"].copy(), g["adam/target"], g["adam/traj"]
    a, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for t in range(1, len(traj) + 1):
        grad = F32(2) * (p - tgt)
        assert grad.dtype == F32
        p, a, v = step(p, a, v, grad, 0.05, 0.9, 0.999, t)
        out.append(p)
    return np.stack(out), traj


@pytest.mark.parametrize("rule", ["step32", "reference32"])
def test_the_fixture_trajectory(rule):
    got, traj = fixture_trajectory(getattr(st, rule))
    assert got.shape == traj.shape == (5, 7, 3) and got.dtype == traj.dtype == F32
    print(f"{rule} against adam/traj: max |difference| = {np.abs(got.astype(np.float64) - traj).max():.3g}, "
          f"{int((bits(got) != bits(traj)).sum())} of {got.size} values differ in a bit")
    np.testing.assert_allclose(got, traj, rtol=2e-6, atol=2e-7)


# ---- against fp64, by the yardstick of the reference's own fp32 rule ------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(1000, 5), (1000, 200), (100000, 50)])
def test_step32_is_as_close_to_fp64_as_the_reference_fp32_rule(n, T):
    rng = np.random.default_rng(n + T)
    p0 = rng.standard_normal(n).astype(F32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(F32) for _ in range(T)]
    lr, (b1, b2) = LR, BETAS
    exact = st.run_reference(st.reference64, p0.astype(np.float64), grads, lr, b1, b2)
    ref32 = st.run_reference(st.reference32, p0, grads, lr, b1, b2)
    ours = [p for p, _, _ in st.run32(p0, grads, lr, b1, b2)]
    e_ours = max(float(np.abs(o.astype(np.float64) - e).max()) for o, e in zip(ours, exact))
    e_ref = max(float(np.abs(r.astype(np.float64) - e).max()) for r, e in zip(ref32, exact))
    print(f"n = {n}, T = {T}: max |step32 - fp64| = {e_ours:.3g}, max |reference32 - fp64| = {e_ref:.3g}, ratio {e_ours / e_ref:.2f}")
    assert e_ref > 0 and e_ours <= 2 * e_ref


# ---- special values -------------------------------------------------------------------------------------------------------------------
def kinds(x):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    return np.isnan(x) * 1 + np.isposinf(x) * 2 + np.isneginf(x) * 3


def both_rules(p0, grads, lr=LR, betas=BETAS):
    ours = [p for p, _, _ in st.run32(p0, grads, lr, *betas)]
    ref = st.run_reference(st.reference32, p0, grads, lr, *betas)
    for o, r in zip(ours, ref):
        assert np.array_equal(kinds(o), kinds(r))
    return ours, ref


def test_one_nan_gradient_makes_every_parameter_nan():
    p0, grads = st.inputs(1000, 3, seed=1)
    grads[1][617] = np.nan
    ours, ref = both_rules(p0, grads)
    for out in (ref, ours):
        assert np.isfinite(out[0]).all() and np.isnan(out[1]).all() and np.isnan(out[2]).all()


def test_one_infinite_gradient_after_a_finite_step_stops_every_other_parameter():
    """the largest root is infinite, so every finite first moment is divided down to an exact 0 and its parameter stays; the element
    itself is inf / inf. The infinite gradient comes in step 2, after a finite step has moved every parameter."""
    p0, grads = st.inputs(1000, 3, seed=2)
    grads[1][3] = np.inf
    ours, ref = both_rules(p0, grads)
    for out in (ref, ours):                                    # the reference's rule alone shows the pattern; then ours
        assert np.isfinite(out[0]).all() and (out[0] != p0).all()
        for k in (1, 2):
            assert np.isnan(out[k][3]) and np.isfinite(np.delete(out[k], 3)).all()
            assert np.array_equal(bits(np.delete(out[k], 3)), bits(np.delete(out[0], 3)))


def test_zero_gradient_leaves_the_parameters_bitwise():
    p0, _ = st.inputs(1000, 1, seed=3)
    p0[:2] = [-0.0, 1e-40]
    ours, ref = both_rules(p0, [np.zeros(1000, F32)] * 2)
    for out in (ref, ours):
        assert np.array_equal(bits(out[0]), bits(p0)) and np.array_equal(bits(out[1]), bits(p0))


def test_zero_betas_give_the_closed_form():
    """a = g, v = g^2, both corrections 1, and sqrt(fl(g g)) = |g| exactly in binary floating point"""
    p0, grads = st.inputs(1000, 3, seed=4, scale=1.0)
    ours, _ = both_rules(p0, grads, betas=(0.0, 0.0))
    p = p0
    for g, got in zip(grads, ours):
        p = p - F32(LR) * (g / (F32(1e-8) + np.abs(g).max()))
        assert p.dtype == F32 and np.array_equal(bits(got), bits(p))


def test_the_bias_corrections():
    assert st.inv_bias(0.9, 10000) == F32(1) and st.inv_bias(0.0, 1) == F32(1)
    assert st.inv_bias(0.5, 1) == F32(2) and st.inv_bias(0.5, 2) == F32(4) / F32(3)
    assert abs(float(st.inv_bias(0.999, 1)) - 1000.0) < 0.02            # fl32(0.999) is not 0.999: 1000.0129


# ---- the launch shapes ----------------------------------------------------------------------------------------------------------------
def test_layout_and_spikes_by_hand():
    assert st.layout(1, True) == dict(vec=1, items=0, G=1, sweeps=1, pmax_strides=1, tail=1)
    assert st.layout(4 * 262144, True) == dict(vec=1, items=262144, G=1024, sweeps=1, pmax_strides=4, tail=0)
    assert st.layout(4 * 262144 + 3, True) == dict(vec=1, items=262144, G=1024, sweeps=1, pmax_strides=4, tail=3)
    assert st.layout(4 * 262144 + 4, True) == dict(vec=1, items=262145, G=1024, sweeps=2, pmax_strides=4, tail=0)
    assert st.layout(3000000, True) == dict(vec=1, items=750000, G=1024, sweeps=3, pmax_strides=4, tail=0)
    assert st.layout(262145, False) == dict(vec=0, items=262145, G=1024, sweeps=2, pmax_strides=4, tail=0)
    assert st.layout(257, False) == dict(vec=0, items=257, G=2, sweeps=1, pmax_strides=1, tail=0)
    assert st.spikes(7, True) == [0, 3, 6]
    assert st.spikes(4 * 262144 + 7, True) == [0, 4 * 255 * 256, 4 * 256 * 256, 4 * 1023 * 256, 4 * 262144, 4 * 262144 + 3, 4 * 262144 + 6]
    assert st.spikes(3 * 262144 + 5, False) == [0, 255 * 256, 256 * 256, 1023 * 256, 262144, 2 * 262144, 3 * 262144, 3 * 262144 + 3,
                                                3 * 262144 + 4]


def test_the_size_table_reaches_every_cell_of_the_layout():
    for vec, sizes in ((1, SIZES["16B"]), (0, SIZES["4B"])):
        cells = [st.layout(n, bool(vec)) for n in sizes]
        assert all(c["vec"] == vec for c in cells)
        assert {min(c["sweeps"], 3) for c in cells} == {1, 2, 3}
        assert {c["pmax_strides"] for c in cells} >= {1, 2, 4}
        assert {c["tail"] for c in cells} == ({0, 1, 2, 3} if vec else {0})
        # a full grid without a second sweep, and the first item past it
        assert any(c["items"] == 262144 and c["sweeps"] == 1 for c in cells) and any(c["items"] == 262145 for c in cells)
    assert st.layout(SIZES["16B"][0], True)["items"] == 0                 # nothing but a tail
    assert max(SIZES["16B"]) == 3 * 2 ** 20 + 3


# ---- the C entry points' argument checks ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from largesteps import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native


def test_the_entry_points_refuse_bad_arguments_before_any_device_work(native):
    lib = native.lib()
    host = (ctypes.c_float * 4)()                   # never dereferenced: every call below returns at its argument check
    some = ctypes.c_void_p(ctypes.addressof(host))
    none = ctypes.c_void_p(0)

    def host_step(param=some, n=4, step=1, scratch=some):
        return lib.ls_adam_uniform_step(param, some, some, some, n, 0.05, 0.9, 0.999, step, scratch, 0, none)

    def device_step(d_step=some, n=4):
        return lib.ls_adam_uniform_step_device(some, some, some, some, n, 0.05, 0.9, 0.999, d_step, some, 0, none)

    size = "null pointer or negative size"
    for what, call, text in (("step = 0", lambda: host_step(step=0), "ls_adam_uniform_step: step must be >= 1"),
                             ("n < 0", lambda: host_step(n=-1), "ls_adam_uniform_step: " + size),
                             ("no scratch", lambda: host_step(scratch=none), "ls_adam_uniform_step: " + size),
                             ("no parameter", lambda: host_step(param=none), "ls_adam_uniform_step: " + size),
                             ("no step counter", lambda: device_step(d_step=none), "ls_adam_uniform_step_device: " + size)):
        rc = call()
        assert rc == native.LS_E_INVALID, what
        assert text in native.last_error(), f"{what}: {native.last_error()!r}"
        with pytest.raises(ValueError):
            native.check(rc)
    assert lib.ls_adam_uniform_step(none, none, none, none, 0, 0.05, 0.9, 0.999, 1, some, 0, none) == 0
    assert lib.ls_adam_uniform_step_device(none, none, none, none, 0, 0.05, 0.9, 0.999, some, some, 0, none) == 0
