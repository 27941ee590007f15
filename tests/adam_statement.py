"""
AdamUniform in plain numpy: the rule of csrc/adam.hip operation for operation (step32), the reference's update in fp32 and in
fp64 (reference32, reference64), and the launch shape of the two kernels (layout, spikes).

step32 is what tests/test_adam_gpu.py holds the device to BIT FOR BIT; tests/test_adam_statement_cpu.py holds step32 itself to the
reference's recorded trajectory and, against reference64, to the error of the reference's own fp32 rule.

The kernel's rule (header of csrc/adam.hip), every operation rounded to fp32 and none contracted (the library is
built with -ffp-contract=off):

    b1, b2, lr            rounded to fp32 once (the C ABI takes floats)
    a   = a*b1 + (1 - b1)*g
    v   = v*b2 + (1 - b2)*(g*g)
    inv_c(beta, t)        = fl32(1 / (1 - float64(beta32)**t))          -- inv_bias: a reciprocal, computed in double, rounded once
    m   = max over all elements of sqrt(v * inv_c2), starting from 0; a NaN is kept
    den = fl32(1e-8) + m
    p   = p - lr * ((a * inv_c1) / den)

The maximum of fp32 numbers is exact whatever the order, so the two-kernel reduction (per-lane, per-wave, per-workgroup, 1024
partial maxima) has exactly one right answer; the root is monotone, so it does not matter that the device takes a root per element.
Subnormals are kept (gfx950 does not flush fp32 subnormals and neither does numpy); infinities and NaNs follow IEEE 754.
"""
import numpy as np

F32 = np.float32
BLOCK = 256            # threads of a workgroup (csrc/common.h)
MAX_GROUPS = 1024      # adam_grid's cap = the partial maxima k_adam_apply reduces
EPS32 = F32(1e-8)


# ---- the kernel's rule ----------------------------------------------------------------------------------------------------------------
def inv_bias(beta, t):
    """fl32(1 / (1 - float64(fl32(beta))**t)): the bias correction as the reciprocal both entry points multiply by"""
    with np.errstate(divide="ignore"):
        return F32(np.float64(1.0) / np.float64(1.0 - float(F32(beta)) ** float(int(t))))


def inv_c_pair(b1, b2, t):
    return inv_bias(b1, t), inv_bias(b2, t)


def moments32(a, v, g, b1, b2):
    """the two running averages after one more gradient (they do not depend on the step number)"""
    b1, b2 = F32(b1), F32(b2)
    a, v, g = (np.asarray(x, F32) for x in (a, v, g))
    with np.errstate(all="ignore"):
        a = a * b1 + (F32(1) - b1) * g
        v = v * b2 + (F32(1) - b2) * (g * g)
    assert a.dtype == F32 and v.dtype == F32
    return a, v


def scale32(v, inv_c2):
    """the NaN-keeping maximum of sqrt(v * inv_c2) over all elements, starting from 0"""
    with np.errstate(all="ignore"):
        r = np.sqrt(np.asarray(v, F32) * F32(inv_c2))
    assert r.dtype == F32
    if r.size == 0:
        return F32(0)
    if np.isnan(r).any():
        return F32(np.nan)
    return np.maximum(F32(0), r.max())


def apply32(p, a, lr, inv_c1, m):
    with np.errstate(all="ignore"):
        den = EPS32 + F32(m)
        out = np.asarray(p, F32) - F32(lr) * ((np.asarray(a, F32) * F32(inv_c1)) / den)
    assert out.dtype == F32
    return out


def step32(p, a, v, g, lr, b1, b2, t, inv_c=None):
    """one step of the kernel's rule from parameters p and moments a, v with gradient g at step number t (>= 1). `inv_c`, when
    given, is the pair (inv_c1, inv_c2) to use instead of the host's. Returns the new (p, a, v), fp32."""
    c1, c2 = inv_c_pair(b1, b2, t) if inv_c is None else inv_c
    a, v = moments32(a, v, g, b1, b2)
    return apply32(p, a, lr, c1, scale32(v, c2)), a, v


def run32(p0, grads, lr, b1, b2, t0=0):
    """step32 from zero moments, one step per gradient, the first with step number t0 + 1: [(p, a, v) after every step]"""
    p = np.asarray(p0, F32).copy()
    a, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for k, g in enumerate(grads, 1):
        p, a, v = step32(p, a, v, g, lr, b1, b2, t0 + k)
        out.append((p, a, v))
    return out


# ---- the reference's update -----------------------------------------------------------------------------------------------------------
def reference64(p, g1, g2, g, lr, b1, b2, t):
    """the reference's step with every array and every scalar in float64: both moments are exponential averages, both are divided by
    1 - beta**t, and the first is divided by 1e-8 + the largest root of the second."""
    p, g1, g2, g = (np.asarray(x, np.float64) for x in (p, g1, g2, g))
    with np.errstate(all="ignore"):
        g1 = g1 * b1 + (1.0 - b1) * g
        g2 = g2 * b2 + (1.0 - b2) * (g * g)
        m1 = g1 / (1.0 - b1 ** t)
        m2 = g2 / (1.0 - b2 ** t)
        top = np.sqrt(m2).max() if m2.size else 0.0
        p = p - lr * (m1 / (1e-8 + top))
    return p, g1, g2


def reference32(p, g1, g2, g, lr, b1, b2, t):
    """the same with fp32 arrays, as the reference runs it: the scalars b1, 1 - b1, 1 - b1**t, ... are computed as Python doubles
    and rounded to fp32 where they meet a tensor; the moments are DIVIDED by the bias terms and the root is taken of every element."""
    p, g1, g2, g = (np.asarray(x, F32) for x in (p, g1, g2, g))
    with np.errstate(all="ignore"):
        g1 = g1 * F32(b1) + F32(1.0 - b1) * g
        g2 = g2 * F32(b2) + F32(1.0 - b2) * (g * g)
        m1 = g1 / F32(1.0 - b1 ** t)
        m2 = g2 / F32(1.0 - b2 ** t)
        top = np.sqrt(m2).max() if m2.size else F32(0)
        p = p - F32(lr) * (m1 / (EPS32 + top))
    assert p.dtype == F32 and g1.dtype == F32 and g2.dtype == F32
    return p, g1, g2


def run_reference(rule, p0, grads, lr, b1, b2):
    """`rule` (reference32 or reference64) from zero moments: the parameters after every step"""
    p = np.asarray(p0).copy()
    g1, g2 = np.zeros_like(p), np.zeros_like(p)
    out = []
    for t, g in enumerate(grads, 1):
        p, g1, g2 = rule(p, g1, g2, g, lr, b1, b2, t)
        out.append(p)
    return out


# ---- the launch -----------------------------------------------------------------------------------------------------------------------
def layout(n, aligned):
    """adam_vec / adam_grid of csrc/adam.hip for n >= 1 floats. aligned: parameter, gradient and both moments start on 16 bytes.
    vec          1: 16-byte items (4 floats) and a tail of n & 3 floats for the first threads of workgroup 0; 0: one float per item
    items        what the grid-stride loops walk: n >> 2 or n
    G            workgroups: one thread per item (the tail counted as an item), at most 1024
    sweeps       turns of the grid-stride loop of the busiest thread (1 also when there is no item at all)
    pmax_strides turns of k_adam_apply's loop over the G partial maxima (256 threads)
    tail         floats after the last 16-byte item (0 on the 4-byte path)"""
    assert n >= 1
    vec = 1 if aligned else 0
    items = n >> 2 if vec else n
    G = min(-(-max((n + 3) // 4 if vec else n, 1) // BLOCK), MAX_GROUPS)
    sweeps = max(-(-items // (G * BLOCK)), 1)
    return dict(vec=vec, items=items, G=G, sweeps=sweeps, pmax_strides=-(-G // BLOCK), tail=n & 3 if vec else 0)


def spikes(n, aligned):
    """the elements at which a reduction or a loop of the launch `layout(n, aligned)` could lose the largest value: sorted, unique.
    - element 0 and element n - 1 (on the 16-byte path the tail thread's, when there is a tail)
    - the last element of the 16-byte body, 4 (n >> 2) - 1
    - the first element of every sweep after the first
    - the first element of workgroups 255, 256 and 1023 in the first sweep: the last slot of the first stride over the partial
      maxima, the first slot of the second, the last slot of all
    - the last element of the last full workgroup of the last sweep"""
    L = layout(n, aligned)
    w = 4 if L["vec"] else 1
    items, per_sweep = L["items"], L["G"] * BLOCK
    at = {0, n - 1}
    if (n >> 2) > 0:
        at.add(4 * (n >> 2) - 1)
    for s in range(1, L["sweeps"]):
        at.add(s * per_sweep * w)
    for group in (255, 256, 1023):
        if group < L["G"] and group * BLOCK < items:
            at.add(group * BLOCK * w)
    first = (L["sweeps"] - 1) * per_sweep
    full = (items - first) // BLOCK
    if full > 0:
        at.add((first + full * BLOCK) * w - 1)
    assert all(0 <= j < n for j in at)
    return sorted(at)


# ---- cases and inputs -----------------------------------------------------------------------------------------------------------------
LR, BETAS = 0.05, (0.9, 0.999)
# the smallest sizes at which each path of the launch can go wrong (tests/test_adam_gpu.py; test_adam_statement_cpu.py holds the
# table to `layout`). 16B: everything aligned; 4B: parameter and gradient start one float into their storage.
SIZES = {"16B": [1, 3, 4, 7, 4 * 256 + 1, 4 * 65536 + 2, 4 * 262144, 4 * 262144 + 4, 4 * 262144 + 7, 3 * 2 ** 20 + 3],
         "4B": [1, 255, 256, 257, 65537, 262144, 262145, 3 * 262144 + 5]}


def inputs(n, steps, seed, scale=1e-3):
    """p0 standard normal and `steps` gradients uniform in (-scale, scale), fp32"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(F32), [(rng.uniform(-1.0, 1.0, n) * scale).astype(F32) for _ in range(steps)]


def same_bits(x, y):
    """elementwise: the same fp32 bit pattern, or a NaN on both sides (the payload of a NaN is nobody's contract)"""
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    return (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
