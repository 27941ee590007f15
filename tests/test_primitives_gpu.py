"""
The stable radix sort (csrc/radix.h: byte-wise and with carried keys), the three-kernel exclusive scan (csrc/assemble.hip) and the
NaN-keeping max reduction (csrc/adam.hip), through the entry points the product calls, against tests/primitives_statement.py (plain
numpy, itself checked by tests/test_primitives_statement_cpu.py).

- remove_duplicates: special values (both zeros, infinities, subnormals, +-FLT_MAX), rows that only the first or only the last of the
  twelve byte passes tells apart, one row V times, random bit patterns, and the carried sort on both sides of rs_chunk's switches
  (2^21, 2^22). Unique rows by value, inverse and faces exact, and STABILITY: a unique row is the bitwise copy of the lowest input
  row that maps to it (the sign of a kept zero shows a rank error among equal keys).
- ls_csr_transpose: t_rowptr, t_col, t_val exact, with V on both sides of every switch of radix_passes, empty rows and columns, one
  column or one row with everything, nnz = 0, nnz past rs_chunk's first switch, and out-of-range columns.
- ls_corner_ranks: vptr, cpos exact, with V at SCAN_CHUNK's boundary and past 256 scan workgroups, F = 0, a vertex that owns a corner of
  every face, and face indices that must not wrap into range.
- AdamUniform past the 1024-workgroup cap of its grid (two sweeps and a tail, 16-byte and 4-byte path), with one gradient element 1000
  times the others at every position where a reduction could lose it: against the fp64 statement at the tolerance of
  test_adam_uniform (rtol 2e-6, atol 2e-7); the worst |dev - ref| / (atol + rtol |ref|) of every case is printed (-s).
Every integer and copied value is compared exactly.
"""
import ctypes
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

import primitives_statement as ps  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
RATIOS = {}          # AdamUniform: largest |dev - ref| / (atol + rtol |ref|) per case (printed with -s)


def dev_of(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- remove_duplicates ----------------------------------------------------------------------------------------------------------------
def check_dedup(v, f, face_dtype):
    from largesteps.meshops import remove_duplicates
    uv, nf, inv = remove_duplicates(dev_of(v), dev_of(f, face_dtype))
    assert uv.dtype == torch.float32 and nf.dtype == torch.int64 and inv.dtype == torch.int64
    uv, nf, inv = uv.cpu().numpy(), nf.cpu().numpy(), inv.cpu().numpy()
    ruv, rinv, rnf, first = ps.dedup(v, f)
    assert uv.shape == ruv.shape, f"{len(uv)} unique rows, the statement has {len(ruv)}"
    assert np.array_equal(uv, ruv), f"unique rows differ at {np.argwhere(uv != ruv)[:3].tolist()}"
    assert np.array_equal(inv, rinv), f"inverse differs at {np.nonzero(inv != rinv)[0][:5].tolist()}"
    assert nf.shape == rnf.shape and np.array_equal(nf, rnf)
    assert np.array_equal(uv[inv], v)
    same = bits(uv) == bits(v[first])
    assert same.all(), f"unique rows {np.nonzero(~same.all(1))[0][:5].tolist()} are not the bitwise copies of their lowest input rows"
    return len(uv), inv


@pytest.mark.parametrize("face_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_remove_duplicates_special_values(V, face_dtype):
    v = ps.pool_rows(V, seed=V)
    U, _ = check_dedup(v, ps.faces_for(V, V // 2, seed=V + 1), face_dtype)
    if V >= 1023:
        assert U < V and np.signbit(v[v == 0]).any()


def test_remove_duplicates_without_faces():
    v = ps.pool_rows(257, seed=11)
    check_dedup(v, np.zeros((0, 3), np.int64), torch.int64)


@pytest.mark.parametrize("face_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_remove_duplicates_all_rows_identical(face_dtype):
    U, inv = check_dedup(ps.identical_rows(5000), ps.faces_for(5000, 2500, seed=1), face_dtype)
    assert U == 1 and not inv.any()


@pytest.mark.parametrize("face_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("how", ["ascending", "descending", "shuffled"])
def test_remove_duplicates_all_rows_distinct(how, face_dtype):
    assert check_dedup(ps.distinct_rows(5000, how), ps.faces_for(5000, 2500, seed=3), face_dtype)[0] == 5000


@pytest.mark.parametrize("face_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("rows", [ps.low_bit_rows, ps.sign_rows], ids=["z_lowest_mantissa_bit", "sign_of_x"])
def test_remove_duplicates_rows_one_byte_pass_tells_apart(rows, face_dtype):
    assert check_dedup(rows(4096), ps.faces_for(4096, 2048, seed=4), face_dtype)[0] == 2


def test_remove_duplicates_random_bit_patterns():
    """all 256 digits in all 12 passes, almost no duplicates"""
    V = 300000
    U, _ = check_dedup(ps.bit_pattern_rows(V, seed=5, masked=False), ps.faces_for(V, V // 2, seed=6), torch.int64)
    assert U > V - 100


@pytest.mark.parametrize("V", [1 << 21, (1 << 21) + 1, (1 << 22) + 1])
def test_remove_duplicates_carried_sort_at_the_chunk_switches(V):
    """masked bit patterns (at most 110 887 distinct rows): rs_chunk is 1024, 2048, 4096 at these sizes"""
    U, _ = check_dedup(ps.bit_pattern_rows(V, seed=V % 1000, masked=True), ps.faces_for(V, V // 2, seed=7), torch.int64)
    assert 100000 < U <= 110887


# ---- ls_csr_transpose -----------------------------------------------------------------------------------------------------------------
def device_transpose(V, rowptr, col, val):
    from largesteps import _native
    csr = _native.CsrMatrix(V, dev_of(rowptr, torch.int32), dev_of(col, torch.int32), dev_of(val, torch.float32), symmetric=None)
    t = _native.csr_transposed(csr)
    assert t.rowptr.dtype == torch.int32 and t.col.dtype == torch.int32 and t.val.dtype == torch.float32
    return t.rowptr.cpu().numpy(), t.col.cpu().numpy(), t.val.cpu().numpy()


def check_transpose(V, rowptr, col, val):
    t_rowptr, t_col, t_val = device_transpose(V, rowptr, col, val)
    r_rowptr, r_col, r_val = ps.transpose(V, rowptr, col, val)
    assert t_rowptr.shape == r_rowptr.shape and np.array_equal(t_rowptr, r_rowptr), \
        f"t_rowptr differs at {np.nonzero(t_rowptr != r_rowptr)[0][:5].tolist()}"
    assert t_col.shape == r_col.shape and np.array_equal(t_col, r_col), f"t_col differs at {np.nonzero(t_col != r_col)[0][:5].tolist()}"
    assert np.array_equal(bits(t_val), bits(r_val))


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 65536, 65537])
def test_transpose_at_the_switches_of_the_pass_count(V):
    rowptr, col, val = ps.csr_random(V, max(5 * V, 64), seed=V)
    assert col.min() == 0 and col.max() == V - 1
    check_transpose(V, rowptr, col, val)


def test_transpose_fourth_byte_pass():
    V = (1 << 24) + 1
    rowptr, col, val = ps.csr_random(V, 5000, seed=8, must_have=[(1 << 24) - 1])
    assert {0, (1 << 24) - 1, 1 << 24} <= set(col.tolist())
    check_transpose(V, rowptr, col, val)


def test_transpose_with_empty_rows_and_columns():
    check_transpose(4000, *ps.csr_odd_rows_cols_1_mod_3(4000, 6000))


def test_transpose_one_column_holds_everything():
    check_transpose(4000, *ps.csr_one_column(4000, 10000, 1234))


def test_transpose_one_row_holds_every_column():
    check_transpose(1000, *ps.csr_full_row(1000, 500, 2000))


def test_transpose_of_no_entries():
    t_rowptr, t_col, t_val = device_transpose(7, *ps.csr_empty(7))
    assert np.array_equal(t_rowptr, np.zeros(8, np.int32)) and len(t_col) == 0 and len(t_val) == 0


def test_transpose_past_the_first_chunk_switch():
    check_transpose(70000, *ps.csr_random(70000, (1 << 21) + 1, seed=9))


@pytest.mark.parametrize("bad", ["V", "-1"])
def test_transpose_rejects_an_out_of_range_column(bad):
    V = 300
    rowptr, col, val = ps.csr_random(V, 2000, seed=10)
    wrong = col.copy()
    wrong[1234] = V if bad == "V" else -1
    with pytest.raises(IndexError):
        device_transpose(V, rowptr, wrong, val)
    check_transpose(V, rowptr, col, val)                                        # the stream is still good


# ---- ls_corner_ranks ------------------------------------------------------------------------------------------------------------------
def device_corner_ranks(f, V, face_dtype):
    """the calls of largesteps.normals._plan"""
    from largesteps import _native
    tf = dev_of(np.asarray(f).reshape(-1, 3), face_dtype)
    F = tf.shape[0]
    n = ctypes.c_size_t(0)
    _native.check(_native.lib().ls_corner_ranks_workspace_bytes(F, V, ctypes.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    vcorner = torch.empty(max(3 * F, 1), dtype=torch.int32, device=DEV)[: 3 * F]
    vptr = torch.empty(V + 1, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _native.check(_native.lib().ls_corner_ranks(_native.ptr(tf), tf.element_size(), F, V, _native.ptr(vptr), _native.ptr(vcorner), _native.ptr(ws),
                                                    ws.numel(), DEV.index, _native.stream_of(DEV)))
    return vptr.cpu().numpy(), vcorner.cpu().numpy()


def check_corner_ranks(f, V):
    r_vptr, r_cpos = ps.corner_ranks(f, V)
    for face_dtype in (torch.int32, torch.int64):
        vptr, cpos = device_corner_ranks(f, V, face_dtype)
        assert vptr.shape == r_vptr.shape and np.array_equal(vptr, r_vptr), f"{face_dtype}: vptr differs at {np.nonzero(vptr != r_vptr)[0][:5].tolist()}"
        assert cpos.shape == r_cpos.shape and np.array_equal(cpos, r_cpos), f"{face_dtype}: cpos differs at {np.nonzero(cpos != r_cpos)[0][:5].tolist()}"


@pytest.mark.parametrize("V", [5, 0])
def test_corner_ranks_without_faces(V):
    check_corner_ranks(np.zeros((0, 3), np.int64), V)


def test_corner_ranks_unreferenced_first_and_last_vertex():
    check_corner_ranks(ps.faces_without_ends(1000, 2000), 1000)


def test_corner_ranks_one_vertex_in_every_face():
    check_corner_ranks(ps.faces_with_hub(3000, 20000, hub=7), 3000)


@pytest.mark.parametrize("V", [2047, 2048, 2049, 524288, 524289])
def test_corner_ranks_at_the_scan_boundaries(V):
    """SCAN_CHUNK = 2048 vertices a scan workgroup; past 256 workgroups k_scan_bsums takes a second trip"""
    check_corner_ranks(ps.faces_for(V, 2 * V, seed=V % 1000), V)


def test_corner_ranks_past_the_first_chunk_switch():
    F = 699051
    assert 3 * F > (1 << 21) >= 3 * (F - 1)
    check_corner_ranks(ps.faces_for(349527, F, seed=12), 349527)


@pytest.mark.parametrize("face_dtype,bad", [(torch.int64, (1 << 32) + 3), (torch.int64, -1), (torch.int64, 100), (torch.int32, -1), (torch.int32, 100)])
def test_corner_ranks_rejects_an_out_of_range_index(face_dtype, bad):
    """2^32 + 3 must not wrap into vertex 3"""
    f = ps.faces_for(100, 300, seed=13)
    f[123, 1] = bad
    with pytest.raises(IndexError):
        device_corner_ranks(f, 100, face_dtype)
    f[123, 1] = 3
    check_corner_ranks(f, 100)


# ---- AdamUniform ----------------------------------------------------------------------------------------------------------------------
LR, BETAS, RTOL, ATOL = 0.05, (0.9, 0.999), 2e-6, 2e-7
# (n, offset of the parameter in its storage in floats, floats per sweep of the capped 1024 x 256 grid)
ADAM_SIZES = {"16B": (2097155, 0, 1024 * 256 * 4), "4B": (524289, 1, 1024 * 256)}
PLACES = ["first", "end_of_sweep_1", "start_of_sweep_2", "last_full_vector", "last"]
_adam_inputs = {}


def adam_case(path, place):
    n, shift, sweep = ADAM_SIZES[path]
    if path not in _adam_inputs:
        _adam_inputs[path] = ps.adam_inputs(n, 3, seed=n % 1000)
    p0, grads = _adam_inputs[path]
    return n, shift, p0, [g.copy() for g in grads], ps.adam_placements(n, sweep)[place]


def device_adam(p0, grads, shift, capturable):
    """the parameters after every step; shift = 1: a view one float into its storage (4-byte accesses)"""
    from largesteps.optimize import AdamUniform
    n = len(p0)
    p = torch.nn.Parameter(torch.zeros(n + shift, device=DEV)[shift:])
    assert p.data_ptr() % 16 == (4 * shift) % 16 and p.is_contiguous()
    with torch.no_grad():
        p.copy_(dev_of(p0))
    opt = AdamUniform([p], lr=LR, betas=BETAS, capturable=capturable)
    out = []
    for g in grads:
        gs = torch.zeros(n + shift, device=DEV)
        gs[shift:] = dev_of(g)
        p.grad = gs[shift:]
        opt.step()
        out.append(p.detach().cpu().numpy().copy())
    return out


@pytest.mark.parametrize("capturable", [False, True], ids=["host_step", "device_step"])
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("path", list(ADAM_SIZES))
def test_adam_uniform_finds_the_largest_gradient_wherever_it_sits(path, place, capturable):
    """a reduction that loses the element's workgroup or sweep makes every step about 1000 / 5 times too large"""
    n, shift, p0, grads, at = adam_case(path, place)
    for g in grads:
        g[at] = 1000.0
    ref = ps.adam_uniform(p0, grads, LR, *BETAS)
    got = device_adam(p0, grads, shift, capturable)
    name = f"adam {path} {place} {'device' if capturable else 'host'} step"
    worst = 0.0
    for r, d in zip(ref, got):
        worst = max(worst, float((np.abs(d.astype(np.float64) - r) / (ATOL + RTOL * np.abs(r))).max()))
    RATIOS[name] = worst
    print(f"{name}: max |dev - ref| / (atol + rtol |ref|) = {worst:.3g}")
    for r, d in zip(ref, got):
        np.testing.assert_allclose(d, r, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("capturable", [False, True], ids=["host_step", "device_step"])
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("path", list(ADAM_SIZES))
def test_adam_uniform_one_nan_gradient_poisons_every_parameter(path, place, capturable):
    n, shift, p0, grads, at = adam_case(path, place)
    grads[1][at] = np.nan
    ref = ps.adam_uniform(p0, grads, LR, *BETAS)
    got = device_adam(p0, grads, shift, capturable)
    np.testing.assert_allclose(got[0], ref[0], rtol=RTOL, atol=ATOL)
    assert np.isnan(ref[1]).all() and np.isnan(ref[2]).all()
    assert np.isnan(got[1]).all(), f"{int((~np.isnan(got[1])).sum())} of {n} parameters are not NaN after the step with the NaN gradient"
    assert np.isnan(got[2]).all()


@pytest.mark.parametrize("capturable", [False, True], ids=["host_step", "device_step"])
@pytest.mark.parametrize("path", list(ADAM_SIZES))
def test_adam_uniform_zero_gradient_changes_nothing(path, capturable):
    n, shift, p0, _, _ = adam_case(path, "first")
    got = device_adam(p0, [np.zeros(n, np.float32)], shift, capturable)
    assert np.array_equal(bits(got[0]), bits(p0))


@pytest.mark.parametrize("capturable", [False, True], ids=["host_step", "device_step"])
def test_adam_uniform_parameter_of_no_elements(capturable):
    from largesteps.optimize import AdamUniform
    p = torch.nn.Parameter(torch.zeros(0, device=DEV))
    q = torch.nn.Parameter(torch.ones(5, device=DEV))
    opt = AdamUniform([p, q], lr=LR, betas=BETAS, capturable=capturable)
    p.grad, q.grad = torch.zeros(0, device=DEV), torch.zeros(5, device=DEV)
    opt.step()
    torch.cuda.synchronize()
    assert p.shape == (0,) and torch.equal(q.detach(), torch.ones(5, device=DEV))
