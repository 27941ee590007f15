"""
Cases of tests/test_direct_launches_gpu.py (TEST helper; also run by tools/record_direct_launch_bits.py, which writes the record the test
compares against): the smallest planes on which every kind of launch of the nested-dissection solve runs (csrc/direct.hip, LaunchKind),
chosen by running plan_level's selection rule over the host planner's trees (tests/native_plan.py).

    A   plane(120), 14 400 vertices, arity 4, leaf 24, no tier: 6 levels. The root's up step rides in its lanes-along down launch;
        level 1 up lanes-along, level 2 up staged, levels 3-5 packed in both sweeps, levels 0-2 down lanes-along.
    B   A with LS_ND_NO_PACK and LS_ND_NO_SMALL: level 1 up lanes-along, levels 2-5 up row-per-lane; levels 0-3 down lanes-along,
        levels 4-5 down row-per-lane.
    C   plane(30), 900 vertices, arity 2, leaf 24, no tier: 7 levels. The root's down sweep is packed (s = 30): the root is not fused
        and has a (staged) up launch of its own.
    D   A with the library's tier: the tier's two launches and the levels above it, whose kernels read the gathered right-hand side.
    E   A and D split over two ranks (shard = (r, 2)), both handles in one process: part 0 on each, the exchange buffers summed, part 1
        on each -- once through a caller's exchange buffer, once through each handle's own region (ls_direct_exchange_region: no
        staging copies). Both are cut at level 1 and their root is fused: part 1 is the down sweep alone. C split the same way
        (E-root) has the root's own up launch in part 1.

Every solver is built with ordering = 'longest-axis' and explicit leaf_size and arity: the plan, and with it every bit of x, is then a
function of the mesh and the case's environment alone. The environment is set BEFORE construction (the library reads it per create).
"""
import ctypes
import hashlib

import numpy as np

from largesteps import synthetic

LAMBDA = 25.0
KS = (1, 2, 3, 4)
GOLDEN = "direct_launch_bits.npz"
# every switch a case sets; a case clears the ones it does not name
SWITCHES = ("LS_ND_TIER_H", "LS_ND_NO_PACK", "LS_ND_NO_SMALL")
# case -> (plane n, arity, leaf_size, environment)
CASES = {
    "A": (120, 4, 24, {"LS_ND_TIER_H": "0"}),
    "B": (120, 4, 24, {"LS_ND_TIER_H": "0", "LS_ND_NO_PACK": "1", "LS_ND_NO_SMALL": "1"}),
    "C": (30, 2, 24, {"LS_ND_TIER_H": "0"}),
    "D": (120, 4, 24, {}),
}
# sharded case -> the unsharded case it splits over WORLD ranks; how the exchange travels
SHARDED = {"E-levels": "A", "E-tier": "D", "E-root": "C"}
WORLD = 2
EXCHANGE = ("caller", "region")
TIERED = ("D", "E-tier")          # cases in which the library must have run a tier


def base(case):
    return SHARDED.get(case, case)


def set_env(case, setenv, delenv):
    """the case's environment through setenv(name, value) / delenv(name) (monkeypatch's, or os.environ's in the recording tool)"""
    env = CASES[base(case)][3]
    for name in SWITCHES:
        if name in env:
            setenv(name, env[name])
        else:
            delenv(name)


def rhs(V):
    """(V, 4) white right-hand side; the k-column case solves its first k columns"""
    return np.random.default_rng(24).standard_normal((V, 4)).astype(np.float32)


def digest(x):
    """sha256 of the fp32 bits of x (a contiguous array) as 32 bytes"""
    a = np.ascontiguousarray(x, dtype=np.float32)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def system(case, dev):
    """(M, B): the case's matrix and its (V, 4) right-hand side on the device"""
    import torch
    from largesteps.geometry import compute_matrix
    v, f = synthetic.plane(CASES[base(case)][0])
    M = compute_matrix(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), LAMBDA)
    return M, torch.from_numpy(rhs(v.shape[0])).to(dev)


def solver(case, M, shard=(0, 1)):
    """the case's solver; the environment must be the case's (set_env) when this runs"""
    from largesteps.solvers import NestedDissectionSolver
    _, arity, leaf, _ = CASES[base(case)]
    return NestedDissectionSolver(M, leaf_size=leaf, arity=arity, shard=shard, ordering="longest-axis")


def shape_of(inf):
    return [inf["launches"], inf["tier_levels"], inf["tier_workgroups"], inf["levels"]]


def profile_rows(prof):
    """launch_profile() as an (n, 3) array of (lo, hi, sweep), sweep 0 up / 1 down"""
    return np.array([[r["levels"][0], r["levels"][1], ("up", "down").index(r["sweep"])] for r in prof], dtype=np.int64).reshape(-1, 3)


def run_unsharded(case, M, B):
    """dict(inf, x[k], x_profiled[k], prof) of one handle: info(), unprofiled solves for every k, the same solves under "profile" = 3
    and launch_profile() of the last of them"""
    s = solver(case, M)
    out = dict(inf=s.info(), x={}, x_profiled={})
    for k in KS:
        out["x"][k] = s.solve(B[:, :k].contiguous()).cpu().numpy()
    s.set_option("profile", 3)
    for k in KS:
        out["x_profiled"][k] = s.solve(B[:, :k].contiguous()).cpu().numpy()
    out["prof"] = s.launch_profile()
    s.set_option("profile", 0)
    s.close()
    return out


class _Region:
    """a handle's exchange region (device pointer, n floats) as something torch.as_tensor takes without a copy"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<f4", data=(ptr, False), version=2)


def run_sharded(case, M, B, exchange):
    """Both ranks' handles in this process. Returns dict(shape[r], cut[r], profile[r] (of part 1 under "profile" = 3), exch[k] (the summed
    exchange), x[k] (stitched by row ownership), x_profiled[k])."""
    import torch
    from largesteps import _native
    lib, dev = _native.lib(), B.device
    st = _native.stream_of(dev)
    ranks = [solver(case, M, shard=(r, WORLD)) for r in range(WORLD)]
    hs = [s._direct._h for s in ranks]
    out = dict(shape=[shape_of(s.info()) for s in ranks], cut=[], profile=[], exch={}, x={}, x_profiled={})
    owned, per_col = [], 0
    for h in hs:
        cut, pc = ctypes.c_int(0), ctypes.c_int64(0)
        mask = np.zeros(B.shape[0], dtype=np.uint8)
        _native.check(lib.ls_direct_shard_info(h, None, None, ctypes.byref(cut), ctypes.byref(pc), mask.ctypes.data_as(ctypes.c_void_p)))
        out["cut"].append(cut.value)
        owned.append(torch.from_numpy(mask.astype(bool)).to(dev))
        per_col = pc.value
    for profile, key in ((0, "x"), (3, "x_profiled")):
        for s in ranks:
            s.set_option("profile", profile)
        for k in KS:
            b = B[:, :k].contiguous()
            if exchange == "region":
                ex = []
                for h in hs:
                    region, n = ctypes.c_void_p(None), ctypes.c_int64(0)
                    _native.check(lib.ls_direct_exchange_region(h, k, ctypes.byref(region), ctypes.byref(n)))
                    assert n.value == per_col * k
                    ex.append(torch.as_tensor(_Region(region.value, n.value), device=dev))
            else:
                ex = [torch.zeros(per_col * k, dtype=torch.float32, device=dev) for _ in hs]
            xs = [torch.zeros_like(b) for _ in hs]
            for h, e, x in zip(hs, ex, xs):
                _native.check(lib.ls_direct_solve_part(h, _native.ptr(b), _native.ptr(x), k, 0, _native.ptr(e), st))
            total = torch.stack(ex).sum(0)          # (what the all-reduce does)
            for h, e, x in zip(hs, ex, xs):
                e.copy_(total)
                _native.check(lib.ls_direct_solve_part(h, _native.ptr(b), _native.ptr(x), k, 1, _native.ptr(e), st))
            x = torch.zeros_like(b)
            for o, xr in zip(owned, xs):
                x[o] = xr[o]
            out[key][k] = x.cpu().numpy()
            if not profile:
                out["exch"][k] = total.cpu().numpy()
    out["profile"] = [profile_rows(s.launch_profile()) for s in ranks]
    out["owned_once"] = bool((torch.stack(owned).sum(0) == 1).all())
    for s in ranks:
        s.set_option("profile", 0)
        s.close()
    return out
