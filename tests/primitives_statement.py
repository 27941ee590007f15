"""
Plain numpy statements of what the library's sort, scan and reduction entry points compute, and the inputs the tests feed them.

  dedup          ls_remove_duplicates   three-word carried radix sort (csrc/radix.h: radix_argsort_words over KeyVerts), k_dedup_flags,
                                        exclusive_scan, k_dedup_emit
  transpose      ls_csr_transpose       k_count_keys, exclusive_scan, byte-wise radix_argsort over KeyInt, k_transpose_emit
  corner_ranks   ls_corner_ranks        k_faces_to_i32, k_count_keys, exclusive_scan, radix_argsort, k_invert_order
  adam_uniform   ls_adam_uniform_step   the NaN-keeping max reduction of csrc/adam.hip (and ls_adam_uniform_step_device)

Each statement is a few numpy library calls (lexsort, a stable argsort, bincount, cumsum) with no knowledge of digits, chunks or tiles;
tests/test_primitives_statement_cpu.py checks them against np.unique, scipy, a brute-force loop and the reference's recorded outputs.
numpy only: no torch, no project import.

NaN rows are out of scope for `dedup`, and no generator here produces one: the reference's own result for rows that hold a NaN
(torch.unique(dim=0)) depends on the comparator of its sort, so there is nothing to state. "Random bit patterns" below are uint32
words reinterpreted as float32 with every NaN pattern replaced by +inf.
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FLT_MIN = np.finfo(F32).tiny                                  # the smallest normal
SUBNORMAL = np.array([1], np.uint32).view(F32)[0]             # the smallest subnormal
# the keys key_of (csrc/radix.h) exists for: both zeros, both infinities, both ends of the subnormal and of the normal range
POOL = np.array([0.0, -0.0, np.inf, -np.inf, SUBNORMAL, -SUBNORMAL, FLT_MIN, -FLT_MIN, 1.0, -1.0, FLT_MAX, -FLT_MAX, 1.0 + 2.0 ** -23], F32)
assert len(POOL) == 13 and not np.isnan(POOL).any()


# ---- statements ----------------------------------------------------------------------------------------------------------------------
def dedup(v, f):
    """unique rows of v (V, 3) in lexicographic order of their VALUES (x first; -0.0 == 0.0), `inverse` (V,) int64 with
    unique[inverse] == v by value, new_faces = inverse[f], and first[u] = the lowest input index among the rows mapped to unique
    row u. Returns (unique, inverse, new_faces, first)."""
    v = np.asarray(v, F32).reshape(-1, 3)
    f = np.asarray(f).astype(np.int64).reshape(-1, 3)
    V = len(v)
    if V == 0:
        return v.copy(), np.zeros(0, np.int64), f.copy(), np.zeros(0, np.int64)
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    s = v[order]
    new = np.ones(V, bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)
    inverse = np.empty(V, np.int64)
    inverse[order] = np.cumsum(new) - 1
    first = np.minimum.reduceat(order, np.flatnonzero(new)).astype(np.int64)
    return s[new], inverse, inverse[f], first


def row_of_entry(V, rowptr):
    return np.repeat(np.arange(V, dtype=np.int64), np.diff(np.asarray(rowptr, np.int64)))


def transpose(V, rowptr, col, val):
    """CSR of the transpose: the entries ordered by column, entries of one column in their input order (ascending row when the rows
    are stored in order, whatever the order inside a row). Returns (t_rowptr (V + 1,), t_col, t_val)."""
    col = np.asarray(col, np.int64)
    order = np.argsort(col, kind="stable")
    t_rowptr = np.r_[0, np.cumsum(np.bincount(col, minlength=V))]
    return t_rowptr, row_of_entry(V, rowptr)[order], np.asarray(val)[order]


def corner_ranks(f, V):
    """the 3 F face corners grouped by vertex, in ascending corner id: vptr (V + 1,) = the ranks each vertex owns, cpos (3 F,) = the
    rank of every corner (the inverse permutation of the stable argsort of the corners' vertices)."""
    c = np.asarray(f, np.int64).ravel()
    vptr = np.r_[0, np.cumsum(np.bincount(c, minlength=V))]
    order = np.argsort(c, kind="stable")
    cpos = np.empty(len(c), np.int64)
    cpos[order] = np.arange(len(c))
    return vptr, cpos


def adam_uniform(p, grads, lr, b1, b2):
    """AdamUniform from zero moments, one step per gradient, all arithmetic in fp64 on the fp32 inputs: exponential averages of the
    gradient and of its square, both divided by 1 - beta^t, and the first one divided by the LARGEST root of the second (plus 1e-8)
    instead of element by element. The maximum is numpy's: NaN as soon as one element is. Returns the parameters after every step."""
    p = np.asarray(p, np.float64).copy()
    g1, g2 = np.zeros_like(p), np.zeros_like(p)
    out = []
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, np.float64)
        g1 = b1 * g1 + (1.0 - b1) * g
        g2 = b2 * g2 + (1.0 - b2) * g * g
        m1 = g1 / (1.0 - b1 ** t)
        m2 = g2 / (1.0 - b2 ** t)
        scale = np.sqrt(m2).max() if m2.size else 0.0
        p = p - lr * (m1 / (1e-8 + scale))
        out.append(p.copy())
    return out


# ---- inputs: vertex rows --------------------------------------------------------------------------------------------------------------
def faces_for(V, F, seed):
    """F random valid faces over V vertices"""
    return np.random.default_rng(seed).integers(0, max(V, 1), (F, 3)).astype(np.int64)


def pool_rows(V, seed):
    """every coordinate drawn from the 13 special values"""
    return POOL[np.random.default_rng(seed).integers(0, len(POOL), (V, 3))]


def identical_rows(V, seed=0):
    """one row V times: every tile of every pass falls into one digit"""
    row = np.random.default_rng(seed).standard_normal(3).astype(F32)
    return np.repeat(row[None], V, axis=0)


def distinct_rows(V, how, seed=0):
    """V distinct rows of a 3-D grid with negative, zero and positive coordinates, `how` in ascending, descending, shuffled"""
    nx = int(np.ceil(V ** (1 / 3))) + 1
    ax = np.linspace(-2.0, 2.0, nx).astype(F32)
    assert len(np.unique(ax)) == nx and nx ** 3 >= V
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    rows = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)[:V]                  # ascending in (x, y, z)
    if how == "descending":
        rows = rows[::-1]
    elif how == "shuffled":
        rows = rows[np.random.default_rng(seed).permutation(V)]
    else:
        assert how == "ascending"
    return np.ascontiguousarray(rows)


def low_bit_rows(V, seed=0):
    """rows that differ only in the lowest mantissa bit of z: the first byte pass alone orders them"""
    w = np.empty((V, 3), np.uint32)
    w[:, 0], w[:, 1] = F32(-0.75).view(np.uint32), F32(3.0).view(np.uint32)
    w[:, 2] = F32(1.5).view(np.uint32) | np.random.default_rng(seed).integers(0, 2, V).astype(np.uint32)
    return w.view(F32)


def sign_rows(V, seed=0):
    """rows that differ only in the sign of x (x != 0): the last byte pass alone orders them"""
    v = np.empty((V, 3), F32)
    v[:, 0] = np.where(np.random.default_rng(seed).integers(0, 2, V) == 1, F32(0.3), F32(-0.3))
    v[:, 1], v[:, 2] = -1.25, 7.0
    return v


MASKS = np.array([0x80C00003, 0x80800001, 0xFF800000], np.uint32)       # x, y, z: 31 * 7 * 511 = 110 887 distinct rows by value


def bit_pattern_rows(V, seed, masked):
    """random bit patterns. masked: the words are cut down to a few bits each (no mask leaves a NaN: x and y keep one exponent bit,
    z keeps the exponent and no mantissa), which makes the duplicate load heavy; unmasked: almost no duplicates"""
    w = np.random.default_rng(seed).integers(0, 1 << 32, (V, 3), dtype=np.uint64).astype(np.uint32)
    if masked:
        w &= MASKS[None, :]
    v = w.view(F32)
    v[np.isnan(v)] = np.inf
    assert not np.isnan(v).any()
    return v


# ---- inputs: CSR matrices (rowptr int32 (V + 1,), col int32, val fp32; rows in order, columns inside a row in any order) ---------------
def _csr(V, rows, cols, seed):
    rows = np.sort(np.asarray(rows, np.int64), kind="stable")
    rowptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=V))].astype(np.int32)
    val = np.random.default_rng(seed + 1000).standard_normal(len(rows)).astype(F32)
    return rowptr, np.asarray(cols).astype(np.int32), val


def csr_random(V, nnz, seed, must_have=None):
    """nnz random entries; the columns always include 0 and V - 1 (and `must_have`)"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, V, nnz)
    need = [0, V - 1] + list(must_have or [])
    cols[rng.permutation(nnz)[: len(need)]] = need
    return _csr(V, rng.integers(0, V, nnz), cols, seed)


def csr_odd_rows_cols_1_mod_3(V, nnz, seed=0):
    """only odd rows and only columns 1 mod 3, neither the first nor the last of either: runs of equal entries in both rowptrs"""
    rng = np.random.default_rng(seed)
    rows = 1 + 2 * rng.integers(0, (V - 2) // 2, nnz)
    cols = 1 + 3 * rng.integers(0, (V - 2) // 3, nnz)
    assert rows.max() < V - 1 and cols.max() < V - 1
    return _csr(V, rows, cols, seed)


def csr_one_column(V, nnz, column, seed=0):
    return _csr(V, np.random.default_rng(seed).integers(0, V, nnz), np.full(nnz, column), seed)


def csr_full_row(V, row, extra, seed=0):
    """row `row` holds an entry in every column (shuffled), `extra` random entries elsewhere"""
    rng = np.random.default_rng(seed)
    rows = np.r_[np.full(V, row), rng.integers(0, V, extra)]
    cols = np.r_[rng.permutation(V), rng.integers(0, V, extra)]
    o = np.argsort(rows, kind="stable")
    return _csr(V, rows[o], cols[o], seed)


def csr_empty(V):
    return np.zeros(V + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, F32)


# ---- inputs: faces for the corner ranking ---------------------------------------------------------------------------------------------
def faces_without_ends(V, F, seed=0):
    """vertices 0 and V - 1 unreferenced"""
    return np.random.default_rng(seed).integers(1, V - 1, (F, 3)).astype(np.int64)


def faces_with_hub(V, F, hub, seed=0):
    """vertex `hub` in every face, at a random corner"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, V, (F, 3)).astype(np.int64)
    f[np.arange(F), rng.integers(0, 3, F)] = hub
    return f


# ---- inputs: gradients for AdamUniform ------------------------------------------------------------------------------------------------
def adam_inputs(n, steps, seed):
    """p0 and `steps` gradients, all standard normal fp32"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(F32), [rng.standard_normal(n).astype(F32) for _ in range(steps)]


def adam_placements(n, sweep):
    """where the one outstanding gradient element sits in turn. sweep = the floats one pass of the capped grid covers
    (1024 workgroups x 256 threads x 4 floats on the 16-byte path, x 1 on the 4-byte path)"""
    return {"first": 0, "end_of_sweep_1": sweep - 1, "start_of_sweep_2": sweep, "last_full_vector": 4 * (n // 4) - 1, "last": n - 1}
