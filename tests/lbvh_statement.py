"""
Statement of the build of csrc/lbvh.h in numpy: what the arrays of the hierarchy over the T faces of a mesh (fp32 V, faces F) must be,
written top-down from the sorted codes, not as Karras' per-node searches (tests/test_lbvh_statement_cpu.py holds those against it).
No device.

1. Vertex box. lo, hi are the fp32 min / max per axis over all rows of V, referenced by a face or not; a NaN coordinate is passed over,
   as fmin / fmax pass it over in the boxes of rule 6 (an axis that holds nothing but NaN has a NaN box, and rule 2 gives it ext = 1).
2. Codes, in fp32 in the kernel's order of operations (the library is built with -ffp-contract=off, so numpy fp32 gives the same bits):
   cen = ((a + b) + c) / 3 per axis for the corners a, b, c of a face; ext = hi - lo if hi - lo > 0 else 1;
   q = trunc(min(max((cen - lo) / ext * 1024, 0), 1023)), the clamp taken as a float with fmax / fmin, so that a NaN becomes 0 and
   the truncation is always defined; code = the bits of qx, qy, qz interleaved, x the most significant of each triple: 30 bits.
3. Order. tri is the stable argsort of the codes: equal codes keep the order of their face ids. Leaf i holds face tri[i].
4. Tree. N = 2 T - 1 nodes: internal node i of T - 1, leaf i at T - 1 + i. The key of leaf i is code[tri[i]] << 32 | i: the keys
   increase strictly. The root is node 0 over the leaves [0, T - 1]. A node over [i, j] splits after the last leaf g in [i, j) that
   agrees with leaf i on the highest bit in which the keys of i and j differ; its left child is leaf g (node T - 1 + g) when g == i,
   otherwise internal node g, over [i, g]; its right child is leaf g + 1 when g + 1 == j, otherwise internal node g + 1, over [g + 1, j].
5. Escape links. esc[x] is the node that follows the subtree of x in the pre-order (left first), -1 past the end: -1 for the root,
   the right sibling for a left child, the parent's link for a right child.
6. Boxes. Leaf i: the fp32 fmin / fmax of the three corners of face tri[i] (min xyz, max xyz; the margin of a mesh handle is 0). An
   internal node: the fmin / fmax of the boxes of its leaves. (fmin / fmax of +0 and -0 is the one thing numpy and the device may
   order differently; `has_negative_zero` lets a test state that its mesh has none.)

`build` returns the dict format of tests/winding_statement.py (left, right, esc, tri, box, V, F) plus `code` (T, per face) and `parent`
(N, -1 for the root). `check_invariants` checks what any valid hierarchy in that format satisfies, without this statement. The meshes
of the tests are at the end.
"""
import numpy as np

F32 = np.float32


# ---- rules 1 to 3 ------------------------------------------------------------------------------------------------------------------
def vertex_box(V):
    """rule 1: (lo (3,), hi (3,)) fp32"""
    V = np.asarray(V, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.fmin.reduce(V, axis=0), np.fmax.reduce(V, axis=0)


def expand(x):
    """the 10 bits of x spread to every third bit"""
    x = np.asarray(x, dtype=np.uint32)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def codes(V, F):
    """rule 2: (T,) int64, the 30-bit code of every face"""
    V, F = np.asarray(V, dtype=F32), np.asarray(F, dtype=np.int64)
    lo, hi = vertex_box(V)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        cen = ((a + b) + c) / F32(3.0)
        d = hi - lo
        ext = np.where(d > 0, d, F32(1.0)).astype(F32)
        x = (cen - lo) / ext * F32(1024.0)
        assert x.dtype == F32
        q = np.fmin(np.fmax(x, F32(0.0)), F32(1023.0)).astype(np.int64)           # astype truncates; the values are in [0, 1023]
    return ((expand(q[:, 0]) << np.uint32(2)) | (expand(q[:, 1]) << np.uint32(1)) | expand(q[:, 2])).astype(np.int64)


def order(code):
    """rule 3"""
    return np.argsort(code, kind="stable").astype(np.int32)


# ---- rules 4 to 6 ------------------------------------------------------------------------------------------------------------------
def tree(scode):
    """rules 4 and 5 from the sorted codes (T,): (left, right (T - 1,), parent, esc (2 T - 1,), pre-order of the internal nodes)"""
    T = len(scode)
    N = 2 * T - 1
    left, right = np.zeros(max(T - 1, 0), np.int32), np.zeros(max(T - 1, 0), np.int32)
    parent, esc = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    keys = (np.asarray(scode, dtype=np.uint64) << np.uint64(32)) | np.arange(T, dtype=np.uint64)
    klist = [int(k) for k in keys]
    pre = []
    stack = [(0, 0, T - 1)] if T > 1 else []
    while stack:
        node, i, j = stack.pop()
        pre.append(node)
        bit = (klist[i] ^ klist[j]).bit_length() - 1
        # the keys of [i, j] agree above `bit` and increase: those with the bit clear come first
        g = int(np.searchsorted(keys, np.uint64(((klist[i] >> bit) + 1) << bit), side="left")) - 1
        assert i <= g < j
        lc = T - 1 + g if g == i else g
        rc = T - 1 + g + 1 if g + 1 == j else g + 1
        left[node], right[node] = lc, rc
        parent[lc] = parent[rc] = node
        esc[lc], esc[rc] = rc, esc[node]
        if rc < T - 1:
            stack.append((rc, g + 1, j))
        if lc < T - 1:
            stack.append((lc, i, g))
    return left, right, parent, esc, pre


def leaf_boxes(V, F, tri):
    """rule 6 for the leaves: (T, 6) fp32"""
    c = np.asarray(V, dtype=F32)[np.asarray(F, dtype=np.int64)[tri]]
    with np.errstate(invalid="ignore"):
        return np.concatenate([np.fmin(np.fmin(c[:, 0], c[:, 1]), c[:, 2]), np.fmax(np.fmax(c[:, 0], c[:, 1]), c[:, 2])], axis=1)


def build(V, F):
    """the arrays of the hierarchy over (V, F)"""
    V, F = np.asarray(V, dtype=F32), np.asarray(F)
    T = F.shape[0]
    code = codes(V, F)
    tri = order(code)
    left, right, parent, esc, pre = tree(code[tri])
    box = np.zeros((2 * T - 1, 6), F32)
    box[T - 1:] = leaf_boxes(V, F, tri)
    with np.errstate(invalid="ignore"):
        for x in reversed(pre):                             # children before parents; fmin / fmax do not depend on the grouping
            box[x, :3] = np.fmin(box[left[x], :3], box[right[x], :3])
            box[x, 3:] = np.fmax(box[left[x], 3:], box[right[x], 3:])
    return dict(left=left, right=right, esc=esc, tri=tri, box=box, V=V, F=F, code=code, parent=parent)


def runs(code):
    """the lengths of the runs of equal codes, in code order"""
    return np.unique(np.asarray(code), return_counts=True)[1]


def depth(arrays):
    """the number of nodes on the longest path from the root to a leaf, both counted"""
    left, right = arrays["left"], arrays["right"]
    T = len(arrays["tri"])
    d = np.zeros(2 * T - 1, np.int64)
    best = 0
    stack = [0] if T > 1 else []
    while stack:
        x = stack.pop()
        for c in (int(left[x]), int(right[x])):
            d[c] = d[x] + 1
            if c < T - 1:
                stack.append(c)
            else:
                best = max(best, int(d[c]))
    return best + 1


def has_negative_zero(V):
    V = np.asarray(V, dtype=F32)
    return bool(((V == 0) & np.signbit(V)).any())


def bits(box):
    return np.ascontiguousarray(box, dtype=F32).view(np.int32)


def differing(a, b, names=("left", "right", "esc", "tri", "box")):
    """the names of the arrays that differ between two hierarchies, the boxes compared as bits"""
    return [k for k in names if not np.array_equal(*(bits(x[k]) if k == "box" else np.asarray(x[k]) for x in (a, b)))]


# ---- what every valid hierarchy satisfies ------------------------------------------------------------------------------------------
def check_invariants(arrays):
    """raises AssertionError naming the property that broke: 'parent' (every node but the root is the child of exactly one node),
    'contiguous' (a node's leaves are a range, the left child's first), 'pre-order' (left / esc from the root visit the leaves
    0 .. T - 1 once each in order and end at -1), 'box' (an internal box is the fmin / fmax of its children's, bit for bit), 'tri' (a
    permutation). Reads left, right, esc, tri, box only."""
    left, right, esc, tri = (np.asarray(arrays[k]).astype(np.int64) for k in ("left", "right", "esc", "tri"))
    T = tri.shape[0]
    N = 2 * T - 1
    box = np.asarray(arrays["box"], dtype=F32).reshape(N, 6)
    assert left.shape == right.shape == (T - 1,) and esc.shape == (N,), "shape"
    assert np.array_equal(np.sort(tri), np.arange(T)), "tri: not a permutation of the faces"
    kids = np.concatenate([left, right])
    assert ((kids >= 1) & (kids < N)).all(), "parent: a child outside [1, N)"
    times = np.bincount(kids, minlength=N)
    assert times[0] == 0 and (times[1:] == 1).all(), "parent: a node that is not the child of exactly one node"
    # with one parent each and N - 1 edges the nodes reached from the root form a tree; every node must be reached
    lo, hi = np.full(N, -1), np.full(N, -1)
    lo[T - 1:] = hi[T - 1:] = np.arange(T)
    pre, stack = [], [0] if T > 1 else []
    while stack:
        x = stack.pop()
        pre.append(x)
        assert len(pre) <= T - 1, "parent: a cycle among the internal nodes"
        stack.extend(int(c) for c in (right[x], left[x]) if c < T - 1)
    assert len(pre) == T - 1, "parent: an internal node is not reached from the root"
    for x in reversed(pre):
        l, r = left[x], right[x]
        assert lo[l] >= 0 and lo[r] >= 0 and lo[r] == hi[l] + 1, f"contiguous: node {x} has leaves {lo[l]}..{hi[l]} left and {lo[r]}..{hi[r]} right"
        lo[x], hi[x] = lo[l], hi[r]
    assert T == 1 or (lo[0] == 0 and hi[0] == T - 1), "contiguous: the root does not hold every leaf"
    node, seen, steps = 0, [], 0
    while node >= 0:
        steps += 1
        assert steps <= N and node < N, "pre-order: the walk does not end"
        if node >= T - 1:
            seen.append(node - (T - 1))
            node = esc[node]
        else:
            node = left[node]
    assert node == -1 and seen == list(range(T)), "pre-order: the walk does not visit the leaves 0 .. T - 1 in order"
    # every link, not only those the full walk follows: the node after the subtree of x is the first leaf past it, or its ancestor
    want = np.full(N, -1)
    for x in pre:
        want[left[x]], want[right[x]] = right[x], want[x]
    assert np.array_equal(esc, want), f"pre-order: the escape link of node {int(np.nonzero(esc != want)[0][0])} skips or repeats leaves"
    with np.errstate(invalid="ignore"):
        for x in pre:
            want_box = np.concatenate([np.fmin(box[left[x], :3], box[right[x], :3]), np.fmax(box[left[x], 3:], box[right[x], 3:])])
            assert np.array_equal(bits(want_box), bits(box[x])), f"box: node {x} is not the fmin / fmax of its children"


# ---- the meshes of the tests ---------------------------------------------------------------------------------------------------------
SMALL_T = [1, 2, 3, 4, 5, 255, 256, 257]          # one either side of a workgroup of the Karras, refit and escape kernels
ICO32_FACTOR = 64.0             # chosen on the CPU so that icosphere(32) has runs of 1 and runs of >= 8 (test_lbvh_statement_cpu)


def sphere():
    from largesteps import synthetic
    v, f = synthetic.icosphere(6)
    return v.astype(F32), np.asarray(f, dtype=np.int64)


def with_far_vertex(v, s):
    """v and one more row (s, s, s)"""
    return np.concatenate([v, F32([[s, s, s]])])


def powers_of_two(n=40):
    """n faces that are single points (three vertex rows each) at (2^-k, 2^-k, 2^-k), k < n, in a random face order, plus a vertex at
    the origin: the box is [0, 1]^3, the cells of the centroids halve down to 0, and the faces with k >= 11 share cell 0"""
    k = np.random.default_rng(40).permutation(n)
    p = (2.0 ** -k.astype(np.float64)).astype(F32)
    v = np.concatenate([np.repeat(p, 3)[:, None].repeat(3, 1), F32([[0, 0, 0]])])
    return v, np.arange(3 * n).reshape(n, 3)


def case(name):
    """(V fp32, F int64) of a row of the case table"""
    from largesteps import synthetic
    v, f = sphere()
    if name == "far4096":                       # every face in one Morton cell
        return with_far_vertex(v, 4096.0), f
    if name == "far320":                        # runs of equal codes of many lengths
        return with_far_vertex(v, 320.0), f
    if name == "far_face":                      # the far vertex referenced: one face alone in the last cell
        return with_far_vertex(v, 4096.0), np.concatenate([f, [[0, 1, v.shape[0]]]])
    if name == "repeated":
        return v, np.tile(f[:1], (300, 1))
    if name.startswith("first"):
        return v, f[:int(name[5:])]
    if name == "plane":                         # an axis of zero extent would need a flat mesh: plane(24) on its side
        pv, pf = synthetic.plane(24)
        pv = pv.astype(F32)
        pv[:, 2] = F32(0.25)
        return pv, np.asarray(pf, dtype=np.int64)
    if name == "powers":
        return powers_of_two()
    if name == "ico32_far":
        bv, bf = synthetic.icosphere(32)
        return with_far_vertex(bv.astype(F32), ICO32_FACTOR), np.asarray(bf, dtype=np.int64)
    if name == "nan":                           # a referenced vertex with a NaN x
        v = v.copy()
        v[f[100, 1], 0] = np.nan
        return v, f
    raise KeyError(name)


CASES = ["far4096", "far320", "far_face", "repeated"] + [f"first{t}" for t in SMALL_T] + ["plane", "powers", "ico32_far"]
