"""NumPy restatement of the FPFH / feature-matching contract of include/o3dslam_reg.h: fp64, one rounding
per operation, the operation order of the header.  Neighbourhoods by brute force in fp32 with np.lexsort on (d2, index);
feature distances accumulated one dimension at a time, so that the bits are those of the contract."""
import math

import numpy as np

PI = math.pi
DIM = 33


def neighbourhoods(xyz, max_nn, radius, block=512):
    """ids (n x max_nn int32, ascending (d2, index), -1 padded) of the up to max_nn nearest points within radius, the point
    itself included -- the order reg_estimate_normals reports."""
    x = np.ascontiguousarray(np.asarray(xyz)[:, :3], np.float32)
    n = x.shape[0]
    r2 = np.float32(radius) * np.float32(radius)
    ids = np.full((n, max_nn), -1, np.int32)
    idx = np.arange(n)
    for s in range(0, n, block):
        q = x[s:s + block]
        dx = q[:, None, 0] - x[None, :, 0]
        dy = q[:, None, 1] - x[None, :, 1]
        dz = q[:, None, 2] - x[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        for r in range(q.shape[0]):
            inside = np.nonzero(d2[r] <= r2)[0]
            order = inside[np.lexsort((idx[inside], d2[r][inside]))][:max_nn]
            ids[s + r, :order.size] = order
    return ids


def drop_self(ids):
    """Point i dropped by index from row i; returns (ids n x max_nn, m n)."""
    n, k = ids.shape
    out = np.full((n, k), -1, np.int32)
    m = np.zeros(n, np.int32)
    for i in range(n):
        row = ids[i][(ids[i] >= 0) & (ids[i] != i)]
        out[i, :row.size] = row
        m[i] = row.size
    return out, m


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(pi, ni, pj, nj):
    """(f0, f1, f2) of the pairs (i, j), vectorised over the leading axis; fp64 on the promoted fp32 values."""
    pi, ni, pj, nj = (np.asarray(a, np.float32).astype(np.float64).reshape(-1, 3) for a in (pi, ni, pj, nj))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = pj - pi
        L = np.sqrt(_dot(d, d))
        a1 = _dot(ni, d) / L
        a2 = _dot(nj, d) / L
        swap = np.abs(a1) < np.abs(a2)
        n1 = np.where(swap[:, None], nj, ni)
        n2 = np.where(swap[:, None], ni, nj)
        d = np.where(swap[:, None], -d, d)
        f2 = np.where(swap, -a2, a1)
        v = _cross(d, n1)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[:, None]
        w = _cross(n1, v)
        f1 = _dot(v, n2)
        f0 = np.arctan2(_dot(w, n2), _dot(n1, n2))
    zero = (L == 0) | (vn == 0)
    return np.where(zero, 0.0, f0), np.where(zero, 0.0, f1), np.where(zero, 0.0, f2)


def bin_coords(f0, f1, f2):
    """The three bin coordinates before floor()."""
    return (11.0 * (f0 + PI)) / (2.0 * PI), (11.0 * (f1 + 1.0)) * 0.5, (11.0 * (f2 + 1.0)) * 0.5


def _clamp_bin(t):
    t = np.floor(t)
    t = np.where(t >= 0.0, t, 0.0)     # NaN lands in bin 0, as on the device
    return np.where(t > 10.0, 10.0, t).astype(np.int64)


def pair_bins(pi, ni, pj, nj):
    return tuple(_clamp_bin(t) for t in bin_coords(*pair_features(pi, ni, pj, nj)))


def _pairs(ids, m):
    i = np.repeat(np.arange(ids.shape[0]), m)
    j = ids[ids >= 0]
    return i, j.astype(np.int64)


def f0_border_margin(xyz, normals, ids, m):
    """Smallest distance of the f0 bin coordinate of any pair from an interior bin border 1..10 (the precondition of the GPU
    tests: atan2 is the only operation whose last bit may differ between the device and libm)."""
    x, nr = np.asarray(xyz, np.float32)[:, :3], np.asarray(normals, np.float32)[:, :3]
    i, j = _pairs(ids, m)
    if i.size == 0:
        return math.inf
    t0 = bin_coords(*pair_features(x[i], nr[i], x[j], nr[j]))[0]
    return float(np.min(np.abs(t0[:, None] - np.arange(1.0, 11.0)[None, :])))


def compute_fpfh(xyz, normals, max_nn, radius, ids_with_self=None):
    """Returns dict(fpfh n x 33, spfh n x 33, m n int32, counts n x 33 int64, ids n x max_nn)."""
    x = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    nr = np.ascontiguousarray(np.asarray(normals, np.float32)[:, :3])
    n = x.shape[0]
    if ids_with_self is None:
        ids_with_self = neighbourhoods(x, max_nn, radius)
    ids, m = drop_self(ids_with_self)
    i, j = _pairs(ids, m)
    counts = np.zeros((n, DIM), np.int64)
    if i.size:
        b0, b1, b2 = pair_bins(x[i], nr[i], x[j], nr[j])
        np.add.at(counts, (i, b0), 1)
        np.add.at(counts, (i, 11 + b1), 1)
        np.add.at(counts, (i, 22 + b2), 1)
    spfh = np.zeros((n, DIM))
    has = m > 0
    spfh[has] = counts[has].astype(np.float64) * (100.0 / m[has].astype(np.float64))[:, None]
    xd = x.astype(np.float64)
    # serial over the neighbour rank, vectorised over the points: every point adds its neighbours in their stored order
    acc = np.zeros((n, DIM))
    for r in range(ids.shape[1]):
        p = np.nonzero(m > r)[0]
        if p.size == 0:
            break
        q = ids[p, r]
        d = xd[q] - xd[p]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = d2 != 0.0
        p, q, d2 = p[ok], q[ok], d2[ok]
        acc[p] = acc[p] + spfh[q] / d2[:, None]
    fpfh = np.zeros((n, DIM))
    for t in range(3):
        s = np.zeros(n)
        for b in range(11):
            s = s + acc[:, 11 * t + b]
        with np.errstate(divide="ignore"):
            scale = np.where(s != 0.0, 100.0 / s, 0.0)
        fpfh[:, 11 * t:11 * t + 11] = acc[:, 11 * t:11 * t + 11] * scale[:, None] + spfh[:, 11 * t:11 * t + 11]
    return {"fpfh": fpfh, "spfh": spfh, "m": m, "counts": counts, "ids": ids}


def nearest(fa, fb, block=256):
    """nn[a] = argmin_b D(a, b), D accumulated one dimension at a time in fp64; ties to the lowest b."""
    fa, fb = np.ascontiguousarray(fa, np.float64), np.ascontiguousarray(fb, np.float64)
    nn = np.empty(fa.shape[0], np.int32)
    for s in range(0, fa.shape[0], block):
        a = fa[s:s + block]
        D = np.zeros((a.shape[0], fb.shape[0]))
        for j in range(fa.shape[1]):
            d = a[:, j][:, None] - fb[:, j][None, :]
            D = D + d * d
        nn[s:s + block] = np.argmin(D, axis=1)     # the first occurrence of the minimum
    return nn


def nearest_both(fa, fb, block=256):
    """(nearest(fa, fb), nearest(fb, fa)) from one pass over D: (x - y)^2 and (y - x)^2 have the same bits, so D(b, a) is
    D(a, b); the column minima are merged block by block with a strict <, which keeps the lowest a of a tie."""
    fa, fb = np.ascontiguousarray(fa, np.float64), np.ascontiguousarray(fb, np.float64)
    na, nb = fa.shape[0], fb.shape[0]
    nn_ab, nn_ba = np.empty(na, np.int32), np.zeros(nb, np.int32)
    best = np.full(nb, np.inf)
    fbt = np.ascontiguousarray(fb.T)
    for s in range(0, na, block):
        a = fa[s:s + block]
        D = np.zeros((a.shape[0], nb))
        d = np.empty_like(D)
        for j in range(fa.shape[1]):
            np.subtract(a[:, j][:, None], fbt[j][None, :], out=d)
            np.multiply(d, d, out=d)
            np.add(D, d, out=D)
        nn_ab[s:s + block] = np.argmin(D, axis=1)
        col = np.argmin(D, axis=0)
        val = D[col, np.arange(nb)]
        better = val < best if s else np.ones(nb, bool)
        nn_ba[better] = col[better] + s
        best[better] = val[better]
    return nn_ab, nn_ba


def match_features(fa, fb):
    """(nn_ab, nn_ba, mutual k x 2): mutual holds (a, nn_ab[a]) with nn_ba[nn_ab[a]] == a, ascending in a."""
    nn_ab, nn_ba = nearest_both(fa, fb)
    a = np.nonzero(nn_ba[nn_ab] == np.arange(nn_ab.size))[0]
    return nn_ab, nn_ba, np.stack([a, nn_ab[a]], axis=1).astype(np.int32)


def correspondences(fa, fb, mutual_filter=True, ransac_n=3):
    nn_ab, _, mutual = match_features(fa, fb)
    if mutual_filter and mutual.shape[0] >= ransac_n:
        return mutual
    return np.stack([np.arange(nn_ab.size), nn_ab], axis=1).astype(np.int32)
