"""
Statement of the surface sampler of csrc/sample.hip (largesteps.sampling): the rule of DESIGN.md section 2.9 in numpy, vectorised over
the samples. The device answers with the same bits.

  1. Weights. The fp32 corners a, b, c of a face widened to fp64; u = b - a, v = c - a, x = u x v (each component one product minus
     the other), area = 0.5 sqrt((x0 x0 + x1 x1) + x2 x2), no contraction. A face whose area is not finite or not positive, or which
     names a vertex outside [0, V), has weight 0. amax = the largest area. q_f = (uint64) floor((area_f / amax) * 2^32), cumq = the
     inclusive uint64 prefix sum, Q = cumq[F - 1]. A face smaller than amax 2^-32 is never drawn.
  2. Random numbers. Philox4x32-10, stateless: sample i uses the counter (i_lo, i_hi, stream, 0) and the key (seed_lo, seed_hi); the
     output words are x0 .. x3. i counts from `offset`.
  3. Face. r = x0 2^32 + x1, T = (r Q) >> 64, I_i = the first f with cumq[f] > T.
  4. Point. u1 = (x2 + 0.5) 2^-32, u2 = (x3 + 0.5) 2^-32 (exact), s = sqrt(u1), w = (1 - s, s (1 - u2), s u2) in fp64, W_i = fp32(w),
     P_i = fp32((W0 a + W1 b) + W2 c) per coordinate in fp64 from the rounded weights.
  5. Q == 0 (no face can be drawn, or F == 0): every P is NaN, every I is -1, every W is 0.
"""
import numpy as np

U32, U64, F64 = np.uint32, np.uint64, np.float64
_M0, _M1, _W0, _W1 = U64(0xD2511F53), U64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
_LOW = U64(0xFFFFFFFF)
_S32 = U64(32)


def philox4x32_10(counter, key):
    """counter (..., 4) and key (2,) or (..., 2) of 32-bit words -> the output words (..., 4) uint32"""
    c = [np.asarray(counter)[..., j].astype(U64) & _LOW for j in range(4)]
    key = np.asarray(key)
    k0, k1 = int(key[..., 0].reshape(-1)[0]), int(key[..., 1].reshape(-1)[0])
    assert (key[..., 0] == k0).all() and (key[..., 1] == k1).all(), "one key per call"
    for r in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                 # 32 x 32 -> 64 bits: exact in uint64
        kk0, kk1 = U64((k0 + r * _W0) & 0xFFFFFFFF), U64((k1 + r * _W1) & 0xFFFFFFFF)
        c = [(p1 >> _S32) ^ c[1] ^ kk0, p1 & _LOW, (p0 >> _S32) ^ c[3] ^ kk1, p0 & _LOW]
    return np.stack(c, -1).astype(U32)


def mulhi64(a, b):
    """(a * b) >> 64 of uint64 arrays, by 32-bit limbs"""
    a, b = np.asarray(a, dtype=U64), np.asarray(b, dtype=U64)
    a0, a1, b0, b1 = a & _LOW, a >> _S32, b & _LOW, b >> _S32
    ll, lh, hl, hh = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (ll >> _S32) + (lh & _LOW) + (hl & _LOW)      # < 3 * 2^32
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def areas(V, F):
    """rule 1's area per face, fp64; 0 for a face of weight 0"""
    V = np.asarray(V, dtype=np.float32).astype(F64)
    F = np.asarray(F).astype(np.int64).reshape(-1, 3)
    ok = ((F >= 0) & (F < V.shape[0])).all(1)
    Fs = np.where(ok[:, None], F, 0) if V.shape[0] else F
    if V.shape[0] == 0:
        return np.zeros(F.shape[0], F64)
    a, b, c = V[Fs[:, 0]], V[Fs[:, 1]], V[Fs[:, 2]]
    u, v = b - a, c - a
    with np.errstate(all="ignore"):
        x0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        x1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        x2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        ar = 0.5 * np.sqrt((x0 * x0 + x1 * x1) + x2 * x2)
        return np.where(ok & np.isfinite(ar) & (ar > 0), ar, 0.0)


def weights(V, F):
    """(q (F,), cumq (F,), Q) as uint64 / int"""
    ar = areas(V, F)
    if ar.size == 0 or not (ar > 0).any():
        return np.zeros(ar.size, U64), np.zeros(ar.size, U64), 0
    q = np.floor((ar / ar.max()) * 4294967296.0).astype(U64)
    cumq = np.cumsum(q, dtype=U64)
    return q, cumq, int(cumq[-1])


def words(n, seed=0, stream=0, offset=0):
    """x (n, 4) uint32 of the samples offset .. offset + n - 1"""
    i = np.arange(n, dtype=U64) + U64(offset)
    counter = np.stack([i & _LOW, i >> _S32, np.full(n, stream, U64), np.zeros(n, U64)], -1)
    return philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=U64))


def sample_surface(V, F, n, seed=0, stream=0, offset=0):
    """(P (n, 3) float32, I (n,) int64, W (n, 3) float32)"""
    V32 = np.asarray(V, dtype=np.float32)
    F = np.asarray(F).astype(np.int64).reshape(-1, 3)
    _, cumq, Q = weights(V32, F)
    if Q == 0:
        return np.full((n, 3), np.nan, np.float32), np.full(n, -1, np.int64), np.zeros((n, 3), np.float32)
    x = words(n, seed, stream, offset).astype(U64)
    T = mulhi64((x[:, 0] << _S32) | x[:, 1], np.full(n, Q, U64))
    I = np.searchsorted(cumq, T, side="right").astype(np.int64)          # the first f with cumq[f] > T
    u1, u2 = (x[:, 2].astype(F64) + 0.5) * 2.0 ** -32, (x[:, 3].astype(F64) + 0.5) * 2.0 ** -32
    s = np.sqrt(u1)
    W = np.stack([1.0 - s, s * (1.0 - u2), s * u2], -1).astype(np.float32)
    Vd, Wd = V32.astype(F64), W.astype(F64)
    a, b, c = Vd[F[I, 0]], Vd[F[I, 1]], Vd[F[I, 2]]
    P = ((Wd[:, 0:1] * a + Wd[:, 1:2] * b) + Wd[:, 2:3] * c).astype(np.float32)
    return P, I, W


def grad_vertices(V, F, I, W, gP):
    """the fp64 value of gV = sum_i W_ik gP_i and the sum of the terms' magnitudes, (V, 3) each: what the device's fp32 result is
    measured against (autograd of sum_k W[:, k, None] * V[F[I, k]] gives the same sums in another order)"""
    F = np.asarray(F).astype(np.int64)
    I = np.asarray(I)
    nv = np.asarray(V).shape[0]
    g, mag = np.zeros((nv, 3), F64), np.zeros((nv, 3), F64)
    keep = I >= 0
    Wd, gd = np.asarray(W, dtype=F64)[keep], np.asarray(gP, dtype=F64)[keep]
    for k in range(3):
        t = Wd[:, k:k + 1] * gd
        np.add.at(g, F[I[keep], k], t)
        np.add.at(mag, F[I[keep], k], np.abs(t))
    return g, mag


def triangles_with_bases(bases=range(1, 9)):
    """coplanar triangles of height 1 over the given bases, side by side on z = 0: the areas base / 2 are exact"""
    v, f, x = [], [], 0.0
    for b in bases:
        v += [[x, 0.0, 0.0], [x + b, 0.0, 0.0], [x, 1.0, 0.0]]
        f.append([len(v) - 3, len(v) - 2, len(v) - 1])
        x += b
    return np.array(v, np.float32), np.array(f, np.int64)
