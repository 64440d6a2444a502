"""Independent numpy restatement of the device OctreeGridDataPointsFilter (reg_octree_grid, include/o3dslam_reg.h,
DESIGN.md 5h).

libpointmatcher DataPointsFilters/OctreeGrid.cpp with utils/octree/Octree.tpp (build, idx, visit) and
OctreeSamplers.tpp, everything in T = float:
  - root box: min / max per axis; radii = max - min; centre 0 (centerAtOrigin) or min + radii * 0.5f;
    radius = float(pow(2, ceil(log(x) / log(2)))) with x = double(max(radii)) * 0.5 in double with libm (x == 0 gives
    radius 0);
  - a node is a leaf when double(radius) * 2.0 <= maxSizeByNode or count <= maxPointByNode; otherwise a point goes to
    child (x > cx) | (y > cy) << 1 | (z > cz) << 2, the child centre is c + (+-0.5f * r) and the child radius r * 0.5f;
    members keep their input order; empty children are skipped;
  - leaves are visited depth-first (children 0..7); each non-empty leaf emits one row (the contract's deviation from
    the samplers' swapCols bookkeeping: row k is the sample of the k-th non-empty leaf):
      FIRST (0) the first member; RAND (1) member size_t(float(size - 1) * (float(rand()) / float(RAND_MAX))) with one
      glibc draw per non-empty leaf after srand(1); CENTROID (2) a sequential fp32 sum in member order starting from
      the first member, / float(count), normals and covariances averaged the same way (src_idx: the first member);
      MEDOID (3) the first member (in member order) of smallest sqrtf(dx*dx + (dy*dy + dz*dz)) to the leaf mean
      (sequential fp32 sum from 0 / float(count)), strict < starting from FLT_MAX.

The tree is restated level by level (every open node splits at once); `transcription` is the recursive build + visit
of Octree.tpp and `reference_samplers` replays the samplers' swapCols / indexVector bookkeeping.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
RAND_MAX = 2147483647


def glibc_rand(count: int, seed: int = 1) -> np.ndarray:
    """The first `count` values of glibc's rand() after srand(seed) (TYPE_3 additive generator, 310 discarded)."""
    r = [0] * (344 + count)
    r[0] = seed & 0xffffffff
    for i in range(1, 31):
        w = r[i - 1] if r[i - 1] < 2**31 else r[i - 1] - 2**32
        hi, lo = int(w / 127773), w - int(w / 127773) * 127773
        w = 16807 * lo - 2836 * hi
        if w < 0:
            w += 2147483647
        r[i] = w
    for i in range(31, 34):
        r[i] = r[i - 31]
    for i in range(34, 344 + count):
        r[i] = (r[i - 31] + r[i - 3]) & 0xffffffff
    return np.array([v >> 1 for v in r[344:]], np.int64)


def random_picks(sizes, rands=None) -> np.ndarray:
    """RandomPtsSampler's member position per non-empty leaf: size_t(float(size - 1) * (float(rand()) /
    float(RAND_MAX))), clamped to size - 1 (only reachable for leaves above 2^24 points)."""
    sizes = np.asarray(sizes, np.int64)
    rands = glibc_rand(len(sizes)) if rands is None else np.asarray(rands, np.int64)
    ratio = (rands.astype(F32) / F32(RAND_MAX)).astype(F32)
    picks = ((sizes - 1).astype(F32) * ratio).astype(F32).astype(np.int64)
    return np.minimum(picks, sizes - 1)


def octree_root(xyz, center_at_origin=True):
    """(centre float32[3], radius float32) of Octree_::build."""
    xyz = np.asarray(xyz, F32)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    return root_from_bounds(lo, hi, center_at_origin)


def root_from_bounds(lo, hi, center_at_origin=True):
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    radii = (hi - lo).astype(F32)
    centre = np.zeros(3, F32) if center_at_origin else (lo + (radii * F32(0.5)).astype(F32)).astype(F32)
    x = float(radii.max()) * 0.5
    radius = F32(0.0) if x == 0.0 else F32(math.pow(2.0, math.ceil(math.log(x) / math.log(2.0))))
    return centre, radius


def _radii_until_size_stop(r0, max_size):
    """Radius of every depth up to (and including) the first depth whose nodes are leaves by size."""
    radii = [F32(r0)]
    while not (float(radii[-1]) * 2.0 <= max_size):
        radii.append(F32(radii[-1] * F32(0.5)))
    return radii


def octree_leaves(xyz, maxPointByNode=1, maxSizeByNode=0.0, centerAtOrigin=True):
    """Level-by-level restatement of the tree.  Returns (leaf_id per input point, leaf depth per input point,
    n_leaves); leaf ids are the depth-first index of the non-empty leaves."""
    xyz = np.asarray(xyz, F32)
    n = xyz.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    if not np.all(np.isfinite(xyz)):
        raise ValueError("non-finite input")
    centre, r0 = octree_root(xyz, centerAtOrigin)
    radii = _radii_until_size_stop(r0, float(F32(maxSizeByNode)))
    M = int(maxPointByNode)
    rank = np.zeros(n, np.int64)          # dense depth-first rank of each point's current node
    depth = np.full(n, -1, np.int64)      # leaf depth (-1: still open)
    c = np.tile(centre, (n, 1)).astype(F32)
    d = 0
    while True:
        open_ = depth < 0
        if not open_.any():
            break
        counts = np.bincount(rank, minlength=int(rank.max()) + 1)
        stop = open_ & ((counts[rank] <= M) | (float(radii[d]) * 2.0 <= float(F32(maxSizeByNode))))
        depth[stop] = d
        split = depth < 0
        bit = np.zeros(n, np.int64)
        if split.any():
            p, cs = xyz[split], c[split]
            b = ((p[:, 0] > cs[:, 0]).astype(np.int64) | ((p[:, 1] > cs[:, 1]).astype(np.int64) << 1) |
                 ((p[:, 2] > cs[:, 2]).astype(np.int64) << 2))
            bit[split] = b + 1
            off = np.where(((b[:, None] >> np.arange(3)) & 1).astype(bool), F32(0.5), F32(-0.5)).astype(F32)
            c[split] = (cs + (off * radii[d]).astype(F32)).astype(F32)
        # children of a split node follow it in depth-first order; settled nodes keep their place (bit 0)
        _, rank = np.unique(rank * 9 + bit, return_inverse=True)
        rank = rank.reshape(-1)
        d += 1
    return rank.astype(np.int32), depth.astype(np.int32), int(rank.max()) + 1


def _seq_sum_rows(vals, members, starts, sizes, first_from_zero):
    """Sequential fp32 sum of vals[members] per leaf (member order); starts from the first member's value, or from
    0.0f + first member when first_from_zero (which maps -0.0 to +0.0)."""
    L = len(sizes)
    acc = vals[members[starts]].astype(F32).copy()
    if first_from_zero:
        acc = (F32(0.0) + acc).astype(F32)
    small = sizes <= 64
    for j in range(1, int(min(sizes.max(), 64))):
        sel = small & (sizes > j)
        if not sel.any():
            break
        acc[sel] = (acc[sel] + vals[members[starts[sel] + j]]).astype(F32)
    for L_ in np.nonzero(~small)[0]:
        seg = vals[members[starts[L_]:starts[L_] + sizes[L_]]].astype(F32)
        if first_from_zero:
            seg = np.concatenate([np.zeros((1,) + seg.shape[1:], F32), seg])
        acc[L_] = np.add.accumulate(seg, axis=0, dtype=F32)[-1]
    return acc


def medoid_dist(p, m):
    d = (p - m).astype(F32)
    sq = (d * d).astype(F32)
    return np.sqrt((sq[..., 0] + (sq[..., 1] + sq[..., 2]).astype(F32)).astype(F32)).astype(F32)


def octree_grid(xyz, normals=None, covs=None, maxPointByNode=1, maxSizeByNode=0.0, samplingMethod=0,
                centerAtOrigin=True):
    """The filter under the contract: dict with xyz (m,3), src_idx (m,), normals / covs (when given), leaf_id (n,),
    leaf_depth (n,), n_out."""
    xyz = np.asarray(xyz, F32)
    if xyz.ndim == 2 and xyz.shape[1] > 3:
        xyz = np.ascontiguousarray(xyz[:, :3])
    leaf, depth, L = octree_leaves(xyz, maxPointByNode, maxSizeByNode, centerAtOrigin)
    out = {"leaf_id": leaf, "leaf_depth": depth, "n_out": L}
    members = np.argsort(leaf, kind="stable")           # by leaf, ascending input index inside
    sizes = np.bincount(leaf, minlength=L).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    nr = None if normals is None else np.asarray(normals, F32)
    cv = None if covs is None else np.asarray(covs, F32)
    if L == 0:
        src = np.zeros(0, np.int64)
    elif samplingMethod == 0:
        src = members[starts]
    elif samplingMethod == 1:
        src = members[starts + random_picks(sizes)]
    elif samplingMethod == 2:
        src = members[starts]
        div = sizes.astype(F32)
        out["xyz"] = (_seq_sum_rows(xyz, members, starts, sizes, False) / div[:, None]).astype(F32)
        if nr is not None:
            out["normals"] = (_seq_sum_rows(nr, members, starts, sizes, False) / div[:, None]).astype(F32)
        if cv is not None:
            out["covs"] = (_seq_sum_rows(cv, members, starts, sizes, False) / div[:, None]).astype(F32)
    elif samplingMethod == 3:
        mean = (_seq_sum_rows(xyz, members, starts, sizes, True) / sizes.astype(F32)[:, None]).astype(F32)
        dist = medoid_dist(xyz[members], mean[leaf[members]])   # in member order
        dist = np.where(dist < FLT_MAX, dist, np.inf)
        best = np.full(L, np.inf, F32)
        np.minimum.at(best, leaf[members], dist)
        hit = dist == best[leaf[members]]
        pos = np.arange(len(members))
        first = np.full(L, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(first, leaf[members][hit], pos[hit])
        first = np.where(first == np.iinfo(np.int64).max, starts, first)   # no distance below FLT_MAX: first member
        src = members[first]
    else:
        raise ValueError("samplingMethod must lie in 0..3")
    out["src_idx"] = src.astype(np.int32)
    if "xyz" not in out:
        out["xyz"] = xyz[src].astype(F32).reshape(-1, 3)
        if nr is not None:
            out["normals"] = nr[src].astype(F32).reshape(-1, 3)
        if cv is not None:
            out["covs"] = cv[src].astype(F32).reshape(-1, 6)
    return out


# ---- the reference, transcribed -------------------------------------------------------------------------------------
def transcription(xyz, maxPointByNode=1, maxSizeByNode=0.0, centerAtOrigin=True):
    """Octree_::build (recursive, stable partition) + visit: the non-empty leaves' member lists in depth-first order
    and their depths."""
    import sys
    xyz = np.asarray(xyz, F32)
    centre, radius = octree_root(xyz, centerAtOrigin)
    table = [np.array([(-0.5, 0.5)[(i >> a) & 1] for a in range(3)], F32) for i in range(8)]
    leaves = []
    max_size = F32(maxSizeByNode)

    def build(data, c, r, d):
        if float(r) * 2.0 <= float(max_size) or len(data) <= maxPointByNode:
            if data:
                leaves.append((data, d))
            return
        cells = [[] for _ in range(8)]
        for i in data:
            p = xyz[i]
            cells[int(p[0] > c[0]) | (int(p[1] > c[1]) << 1) | (int(p[2] > c[2]) << 2)].append(i)
        half = F32(r * F32(0.5))
        for k in range(8):
            build(cells[k], (c + (table[k] * r).astype(F32)).astype(F32), half, d + 1)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 4000))
    try:
        build(list(range(xyz.shape[0])), centre, radius, 0)
    finally:
        sys.setrecursionlimit(old)
    return leaves


def reference_samplers(xyz, leaves, samplingMethod=0, normals=None):
    """The samplers of OctreeSamplers.tpp on a copy of the cloud, swapCols / indexVector bookkeeping included.
    Returns (rows xyz (m,3), rows normals or None, stale (m,) bool: a lookup of that step missed
    the point it meant, or a later step swapped the row out)."""
    feat = np.asarray(xyz, F32).copy()
    nrm = None if normals is None else np.asarray(normals, F32).copy()
    n = feat.shape[0]
    content = np.arange(n)            # which input point each column holds
    index_vector = np.zeros(n, np.int64)
    rands = glibc_rand(len(leaves)) if samplingMethod == 1 else None
    stale = np.zeros(len(leaves), bool)
    for idx, (data, _) in enumerate(leaves):
        def look(dd):
            j = index_vector[dd] if dd < idx else dd
            if content[j] != dd:
                stale[idx] = True
            return j
        if samplingMethod in (0, 1):
            pick = 0 if samplingMethod == 0 else int(random_picks([len(data)], rands[idx:idx + 1])[0])
            j = look(data[pick])
        elif samplingMethod == 2:
            j = look(data[0])
            for dd in data[1:]:
                i = look(dd)
                feat[j] = (feat[j] + feat[i]).astype(F32)
                if nrm is not None:
                    nrm[j] = (nrm[j] + nrm[i]).astype(F32)
            feat[j] = (feat[j] / F32(len(data))).astype(F32)
            if nrm is not None:
                nrm[j] = (nrm[j] / F32(len(data))).astype(F32)
        else:
            cols = [look(dd) for dd in data]
            centre = np.zeros(3, F32)
            for i in cols:
                centre = (centre + feat[i]).astype(F32)
            centre = (centre / F32(len(data))).astype(F32)
            best, j = FLT_MAX, 0
            for i in cols:
                dist = medoid_dist(feat[i], centre)
                if dist < best:
                    best, j = dist, i
        if j < idx:
            stale[j] = True           # an emitted row is swapped back out
        for arr in (feat, nrm, content):
            if arr is not None:
                arr[[idx, j]] = arr[[j, idx]]
        index_vector[idx] = j
    m = len(leaves)
    return feat[:m], (None if nrm is None else nrm[:m]), stale
