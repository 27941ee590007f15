"""
tests/primitives_statement.py is what tests/test_primitives_gpu.py holds the device's sort, scan and reduction entry points to, so the
statements are themselves checked here, at small sizes, against something that shares no code with them: np.unique and the
reference's recorded remove_duplicates outputs, scipy's CSR transpose, a brute-force loop, and the reference's recorded AdamUniform
trajectory.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import primitives_statement as ps  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")

DEDUP_INPUTS = {
    "pool_1": lambda: ps.pool_rows(1, 1),
    "pool_2": lambda: ps.pool_rows(2, 2),
    "pool_65": lambda: ps.pool_rows(65, 3),
    "pool_1583": lambda: ps.pool_rows(1583, 4),
    "identical": lambda: ps.identical_rows(300),
    "ascending": lambda: ps.distinct_rows(500, "ascending"),
    "descending": lambda: ps.distinct_rows(500, "descending"),
    "shuffled": lambda: ps.distinct_rows(500, "shuffled"),
    "low_bit": lambda: ps.low_bit_rows(256),
    "sign": lambda: ps.sign_rows(256),
    "bits": lambda: ps.bit_pattern_rows(3000, 5, masked=False),
    "bits_masked": lambda: ps.bit_pattern_rows(3000, 6, masked=True),
}


@pytest.mark.parametrize("name", list(DEDUP_INPUTS))
def test_dedup_equals_np_unique(name):
    """values only: numpy keeps the zero's sign of whichever row its unstable sort puts first, the statement that of the lowest index"""
    v = DEDUP_INPUTS[name]()
    V = len(v)
    f = ps.faces_for(V, V // 2, seed=V)
    uv, inv, nf, first = ps.dedup(v, f)
    ruv, rinv = np.unique(v, axis=0, return_inverse=True)
    rinv = np.asarray(rinv).ravel()
    assert np.array_equal(uv, ruv) and np.array_equal(inv, rinv) and np.array_equal(nf, rinv[f])
    assert inv.dtype == np.int64 and nf.dtype == np.int64 and nf.shape == f.shape
    assert np.array_equal(uv[inv], v)
    brute = np.array([np.flatnonzero(inv == u)[0] for u in range(len(uv))])
    assert np.array_equal(first, brute)
    assert np.array_equal(uv.view(np.uint32), v[first].view(np.uint32))          # the statement's rows are bitwise those of `first`
    if name in ("ascending", "descending", "shuffled"):
        assert len(uv) == V
    if name in ("low_bit", "sign"):
        assert len(uv) == 2
    if name == "identical":
        assert len(uv) == 1 and not inv.any()


def test_dedup_generators_hold_what_they_promise():
    assert not any(np.isnan(make()).any() for make in DEDUP_INPUTS.values())
    lb = ps.low_bit_rows(256).view(np.uint32)
    assert len(np.unique(lb[:, 2])) == 2 and np.ptp(lb[:, 2]) == 1 and len(np.unique(lb[:, :2], axis=0)) == 1
    sg = ps.sign_rows(256).view(np.uint32)
    assert set(np.unique(sg[:, 0] ^ sg[0, 0]).tolist()) == {0, 0x80000000} and len(np.unique(sg[:, 1:], axis=0)) == 1
    pool = ps.pool_rows(4000, 9)
    assert set(pool.view(np.uint32).ravel().tolist()) == set(ps.POOL.view(np.uint32).tolist())
    assert np.signbit(pool[pool == 0]).any() and not np.signbit(pool[pool == 0]).all()
    raw = ps.bit_pattern_rows(200000, 7, masked=False)
    assert np.isinf(raw).sum() > 1000                                            # the NaN patterns became +inf
    digits = raw.view(np.uint8).reshape(-1, 12)
    assert all(len(np.unique(digits[:, b])) == 256 for b in range(12))
    # every row of the masked patterns is one of 31 * 7 * 511 values
    m = ps.bit_pattern_rows(200000, 8, masked=True)
    assert all(len(np.unique(m[:, c])) == k for c, k in enumerate((31, 7, 511)))


def test_dedup_equals_the_reference_fixture():
    d = np.load(os.path.join(GOLDEN, "reference_dedup.npz"))
    names = sorted({k.split("/")[0] for k in d.files})
    assert len(names) >= 6
    for n in names:
        uv, inv, nf, first = ps.dedup(d[f"{n}/v"], d[f"{n}/f"])
        assert np.array_equal(uv, d[f"{n}/unique"]) and np.array_equal(inv, d[f"{n}/inverse"]) and np.array_equal(nf, d[f"{n}/new_faces"]), n


def _scipy_case(V, nnz, seed):
    """unique, column-sorted entries (scipy's transpose is canonical for those)"""
    rng = np.random.default_rng(seed)
    flat = np.sort(rng.choice(V * V, size=min(nnz, V * V), replace=False))
    rows, cols = flat // V, flat % V
    rowptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=V))].astype(np.int32)
    return rowptr, cols.astype(np.int32), rng.standard_normal(len(flat)).astype(np.float32)


@pytest.mark.parametrize("V,nnz", [(1, 1), (2, 3), (7, 0), (50, 300), (257, 2000), (1000, 900)])
def test_transpose_equals_scipy(V, nnz):
    import scipy.sparse as sp
    rowptr, col, val = _scipy_case(V, nnz, seed=V)
    t_rowptr, t_col, t_val = ps.transpose(V, rowptr, col, val)
    T = sp.csr_matrix((val, col, rowptr), shape=(V, V)).T.tocsr()
    T.sort_indices()
    assert np.array_equal(t_rowptr, T.indptr) and np.array_equal(t_col, T.indices) and np.array_equal(t_val, T.data)
    assert t_val.dtype == np.float32


def test_transpose_keeps_the_input_order_inside_a_column():
    """rows whose columns are not sorted, and repeated (row, column) pairs: the entries of a column stay in their input order"""
    V = 40
    rowptr, col, val = ps.csr_random(V, 400, seed=3)
    t_rowptr, t_col, t_val = ps.transpose(V, rowptr, col, val)
    rows = ps.row_of_entry(V, rowptr)
    for c in range(V):
        e = np.flatnonzero(col == c)                                            # ascending entry id
        assert np.array_equal(t_col[t_rowptr[c]:t_rowptr[c + 1]], rows[e]) and np.array_equal(t_val[t_rowptr[c]:t_rowptr[c + 1]], val[e])
    assert t_rowptr[-1] == 400 and (col == 0).any() and (col == V - 1).any()
    for rp, cl, _ in (ps.csr_odd_rows_cols_1_mod_3(4000, 6000), ps.csr_one_column(4000, 10000, 1234), ps.csr_full_row(1000, 500, 2000)):
        assert rp[0] == 0 and rp[-1] == len(cl) and np.all(np.diff(rp) >= 0)
    rp, cl, _ = ps.csr_odd_rows_cols_1_mod_3(4000, 6000)
    assert not np.diff(rp)[0::2].any() and np.diff(rp)[-1] == 0 and np.all(cl % 3 == 1) and cl.max() < 3999
    rp, cl, _ = ps.csr_full_row(1000, 500, 2000)
    assert set(cl[rp[500]:rp[501]].tolist()) == set(range(1000))


def test_corner_ranks_equals_a_brute_force_loop():
    V, F = 23, 50
    f = ps.faces_with_hub(V, F, hub=7, seed=1)
    f[f == 0] = 1                                                               # vertex 0 unreferenced
    vptr, cpos = ps.corner_ranks(f, V)
    c = f.ravel()
    rank = 0
    for vtx in range(V):
        assert vptr[vtx] == rank
        for corner in range(3 * F):                                             # ascending corner id
            if c[corner] == vtx:
                assert cpos[corner] == rank
                rank += 1
    assert vptr[V] == rank == 3 * F and vptr[0] == vptr[1] == 0 and vptr[8] - vptr[7] >= F
    vptr, cpos = ps.corner_ranks(np.zeros((0, 3), np.int64), 5)
    assert np.array_equal(vptr, np.zeros(6)) and len(cpos) == 0
    vptr, cpos = ps.corner_ranks(np.zeros((0, 3), np.int64), 0)
    assert np.array_equal(vptr, [0]) and len(cpos) == 0


def test_adam_uniform_equals_the_reference_trajectory():
    """the gradients of the fixture's quadratic, taken at the reference's own recorded parameters; tolerance of test_adam_uniform"""
    g = np.load(os.path.join(GOLDEN, "reference_golden.npz"))
    p0, tgt, traj = g["adam/p0"], g["adam/target"], g["adam/traj"]
    before = [p0] + list(traj[:-1])
    grads = [np.float32(2) * (p - tgt) for p in before]
    assert all(gr.dtype == np.float32 for gr in grads)
    got = ps.adam_uniform(p0, grads, 0.05, 0.9, 0.999)
    assert len(got) == len(traj) == 5
    for step in range(5):
        np.testing.assert_allclose(got[step], traj[step], rtol=2e-6, atol=2e-7)


def test_adam_uniform_keeps_a_nan_and_a_zero_gradient():
    p0, grads = ps.adam_inputs(100, 3, seed=0)
    grads[1][37] = np.nan
    out = ps.adam_uniform(p0, grads, 0.05, 0.9, 0.999)
    assert not np.isnan(out[0]).any() and np.isnan(out[1]).all() and np.isnan(out[2]).all()
    assert np.array_equal(ps.adam_uniform(p0, [np.zeros(100, np.float32)], 0.05, 0.9, 0.999)[0], p0.astype(np.float64))
    assert ps.adam_uniform(np.zeros(0, np.float32), [np.zeros(0, np.float32)], 0.05, 0.9, 0.999)[0].shape == (0,)
    assert ps.adam_placements(2097155, 1048576) == {"first": 0, "end_of_sweep_1": 1048575, "start_of_sweep_2": 1048576,
                                                    "last_full_vector": 2097151, "last": 2097154}
