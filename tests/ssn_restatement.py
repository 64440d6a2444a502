"""Independent numpy restatement of the device data-point filters (include/o3dslam_reg.h).

SamplingSurfaceNormalDataPointsFilter (libpointmatcher DataPointsFilters/SamplingSurfaceNormal.cpp buildNew / fuseRange)
under the determinism contract of reg_sampling_surface_normal:
  - a segment is ordered by (coordinate on the cut axis with -0 == +0, original index); the left child gets
    count - count/2 points; the cut value (first point of the right half) bounds both children on that axis;
  - the cut axis is the first strict argmax of the PROPAGATED box extents (utils.h argMax: starts from 0);
  - a leaf (count <= knn) keeps the order the last split left; mean = sequential fp32 sum / float(count);
    C = sum (q - mean)(q - mean)^T sequentially in fp32; the eigen-decomposition follows k_pca_finish (rank rule,
    ascending eigenvalues, sign: largest component positive);
  - the kept index of a leaf is its smallest original index; output ascending by it.
The reading-side filters follow each inPlaceFilter with the norm evaluated as sqrtf((x*x + y*y) + z*z) in fp32.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
EPS_RANK = 3.0 * 1.1920929e-07


def tree_segments(n: int, knn: int):
    """Leaves (begin, count) in depth-first order and, per level, the open segments (begin, count).  The shape depends
    only on (n, knn)."""
    levels, leaves = [], []
    cur = [(0, n)] if n > knn else []
    if n <= knn:
        leaves.append((0, n))
    while cur:
        levels.append(cur)
        nxt = []
        for b, c in cur:
            left = c - c // 2
            for cb, cc in ((b, left), (b + left, c - left)):
                if cc > knn:
                    nxt.append((cb, cc))
                else:
                    leaves.append((cb, cc))
        cur = nxt
    leaves.sort()
    return levels, leaves


def _axis(lo, hi):
    ext = (hi - lo).astype(F32)
    best, arg = F32(0), 0
    for a in range(3):
        if ext[a] > best:
            best, arg = ext[a], a
    return arg


def ssn_order(xyz: np.ndarray, knn: int):
    """The permutation the splits leave (leaf order), level by level."""
    xyz = np.asarray(xyz, F32)
    n = xyz.shape[0]
    if not np.all(np.isfinite(xyz)):
        raise ValueError("non-finite input")
    perm = np.arange(n, dtype=np.int64)
    levels, leaves = tree_segments(n, knn)
    boxes = {(0, n): (xyz.min(axis=0).astype(F32), xyz.max(axis=0).astype(F32))} if n else {}
    canon = xyz + F32(0.0)   # -0 -> +0
    for segs in levels:
        for b, c in segs:
            lo, hi = boxes.pop((b, c))
            ax = _axis(lo, hi)
            ids = perm[b:b + c]
            o = np.lexsort((ids, canon[ids, ax]))
            perm[b:b + c] = ids[o]
            left = c - c // 2
            cut = xyz[perm[b + left], ax]
            lhi = hi.copy()
            lhi[ax] = cut
            rlo = lo.copy()
            rlo[ax] = cut
            boxes[(b, left)] = (lo, lhi)
            boxes[(b + left, c - left)] = (rlo, hi)
    return perm, leaves


def leaf_moments(P: np.ndarray):
    """mean, C (xx xy xz yy yz zz), max squared distance from the mean: sequential fp32 sums in the given order."""
    P = np.asarray(P, F32)
    m = P.shape[0]
    mean = np.cumsum(P, axis=0, dtype=F32)[-1] / F32(m)
    d = (P - mean).astype(F32)
    prods = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                      d[:, 2] * d[:, 2]], axis=1).astype(F32)
    C = np.cumsum(prods, axis=0, dtype=F32)[-1]
    s2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32) + d[:, 2] * d[:, 2]).astype(F32)
    return mean.astype(F32), C.astype(F32), F32(s2.max())


def pca(C: np.ndarray):
    """(rank, eigenvalues ascending fp64, eigenvectors as columns, normal with k_pca_finish's sign rule)."""
    M = np.array([[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]], np.float64)
    lam, V = np.linalg.eigh(M)
    lmax = abs(lam[2])
    rank = int(np.sum(np.abs(lam) > lmax * EPS_RANK)) if lmax > 0 else 0
    v = V[:, 0].copy()
    big = 0
    if abs(v[1]) > abs(v[big]):
        big = 1
    if abs(v[2]) > abs(v[big]):
        big = 2
    if v[big] < 0:
        v = -v
    return rank, lam, V, np.clip(v.astype(F32), -1, 1)


def density(m: int, mx) -> np.float32:
    c0 = F32(4.0 / 3.0) * F32(np.pi)
    vol = F32(c0 * F32(F32(mx) * np.sqrt(F32(mx))))
    return F32(F32(m) / vol) if vol > 0 else F32(0)


def sampling_surface_normal(xyz, knn=7, samplingMethod=1, ratio=0.5, maxBoxDim=np.inf, keepNormals=True,
                            keepDensities=False, keepEigenValues=False, keepEigenVectors=False):
    xyz = np.asarray(xyz, F32)
    n = xyz.shape[0]
    if samplingMethod == 0 and ratio < 1:
        raise NotImplementedError("random subsampling")
    perm, leaves = ssn_order(xyz, knn)
    need_eig = keepNormals or keepEigenValues or keepEigenVectors
    leaf_id = np.full(n, -1, np.int32)
    recs = []
    n_unfit = 0
    for li, (b, c) in enumerate(leaves):
        ids = perm[b:b + c]
        P = xyz[ids]
        box = (P.max(axis=0) - P.min(axis=0)).astype(F32)
        if box.max() > F32(maxBoxDim):
            n_unfit += c
            continue
        mean, C, mx = leaf_moments(P)
        rank, lam, V, nrm = pca(C)
        if need_eig and rank + 1 < 3:
            n_unfit += c
            continue
        leaf_id[ids] = li
        recs.append((li, int(ids.min()), ids, mean, nrm, density(c, mx), lam, V))
    rows = []   # (kept index, xyz, record)
    for r in recs:
        if samplingMethod == 1:
            rows.append((r[1], r[3], r))
        else:
            for i in r[2]:
                rows.append((int(i), xyz[i], r))
    rows.sort(key=lambda t: t[0])
    m = len(rows)
    out = {"src_idx": np.array([t[0] for t in rows], np.int32).reshape(m),
           "xyz": np.array([t[1] for t in rows], F32).reshape(m, 3),
           "normals": np.array([t[2][4] for t in rows], F32).reshape(m, 3),
           "densities": np.array([t[2][5] for t in rows], F32).reshape(m),
           "eigvals": np.array([t[2][6] for t in rows], F32).reshape(m, 3),
           "eigvecs": np.array([t[2][7].T.reshape(9) for t in rows], F32).reshape(m, 9),
           "leaf_id": leaf_id, "n_unfit": n_unfit, "n_out": m}
    return out


# ---- reading-side filters -------------------------------------------------------------------------------------------
def _norm(P):
    P = np.asarray(P, F32)
    s = (P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]).astype(F32)
    s = (s + P[:, 2] * P[:, 2]).astype(F32)
    return np.sqrt(s).astype(F32)


def point_filter_keep(P: np.ndarray, f: dict) -> np.ndarray:
    """Boolean mask of one filter over the current cloud P (n x 3 fp32).  f: {"type": name, ...reference params}."""
    t = f["type"]
    n = P.shape[0]
    if t == "Identity":
        return np.ones(n, bool)
    if t in ("MaxDist", "MinDist", "DistanceLimit"):
        dim = int(f.get("dim", -1))
        key = {"MaxDist": "maxDist", "MinDist": "minDist", "DistanceLimit": "dist"}[t]
        v = F32(f.get(key, 1.0))
        x = _norm(P) if dim == -1 else P[:, dim]
        if dim == -1:
            v = abs(v)
        if t == "MaxDist":
            return x < v
        if t == "MinDist":
            return x > v
        return x > v if int(f.get("removeInside", 1)) else x < v
    if t == "BoundingBox":
        b = [F32(f.get(k, d)) for k, d in (("xMin", -1), ("xMax", 1), ("yMin", -1), ("yMax", 1), ("zMin", -1),
                                           ("zMax", 1))]
        inside = ((P[:, 0] > b[0]) & (P[:, 0] < b[1]) & (P[:, 1] > b[2]) & (P[:, 1] < b[3]) & (P[:, 2] > b[4]) &
                  (P[:, 2] < b[5]))
        return ~inside if int(f.get("removeInside", 1)) else inside
    if t == "RemoveNaN":
        return ~np.isnan(P).any(axis=1)
    if t == "MaxQuantileOnAxis":
        dim = int(f.get("dim", 0))
        k = int(F32(n) * F32(f.get("ratio", 0.5)))
        v = P[:, dim]
        if np.isnan(v).any() or k >= n:
            raise ValueError("MaxQuantileOnAxis: NaN on the axis or empty quantile")
        limit = np.sort(v)[k]
        return v < limit
    if t == "FixStepSampling":
        step = int(f.get("startStep", 10))
        phase = int(f.get("phase", 0))
        keep = np.zeros(n, bool)
        keep[phase::step] = True
        return keep
    raise NotImplementedError(t)


def filter_points(xyz, filters):
    """Runs the chain; returns (kept xyz, source indices)."""
    P = np.asarray(xyz, F32)
    idx = np.arange(P.shape[0], dtype=np.int64)
    for f in filters:
        k = point_filter_keep(P[idx], f)
        idx = idx[k]
    return P[idx], idx.astype(np.int32)
