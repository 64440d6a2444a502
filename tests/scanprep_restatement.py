"""numpy restatement of the scan front end's contracts (include/o3dslam_reg.h); no device.

voxel_down_sample   PointCloud::VoxelDownSample: origin = min_bound - voxel / 2, index = floor((p - origin) / voxel), one
                    point per occupied voxel from sequential sums in input order; NaN normals skipped, the averaged normal
                    not re-normalised; voxels in ascending (z, y, x) index.
random_down_sample  the count = (int64)(ratio n) smallest (key, index) pairs, key = splitmix64 of (seed, index) in Python
                    integers; ascending indices.
process_scan        wide crop, voxel grid, normals (a callback), random selection, narrow crop, composed from the two and
                    the crop predicate of the map rows (tests/map_rows_cases.py: the oracle's crop_mask)."""
import numpy as np

from tests import map_rows_cases as M

_G, _A, _B, _M64 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, (1 << 64) - 1
KEY_BITS = 21


def scan_key(seed, i):
    """The sampler of reg_ransac_correspondences for ctr = i, before its range reduction."""
    z = (seed + (i + 1) * _G) & _M64
    z = ((z ^ (z >> 30)) * _A) & _M64
    z = ((z ^ (z >> 27)) * _B) & _M64
    return z ^ (z >> 31)


def origin_of(xyz, voxel):
    return np.asarray(xyz, np.float64).reshape(-1, 3).min(axis=0) - 0.5 * voxel


def voxel_indices(xyz, voxel):
    """floor((p - origin) / voxel) per axis as float64 (a true division)."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.floor((x - origin_of(x, voxel)) / voxel)


def integer_margin(xyz, voxel):
    """Smallest distance of any (p - origin) / voxel to an integer (inf for an empty cloud): the inputs of the GPU tests keep
    it above 1e-9, so that no rounding of the division can move a point across a voxel face."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    if not x.size:
        return float("inf")
    a = (x - origin_of(x, voxel)) / voxel
    return float(np.min(np.abs(a - np.rint(a))))


def voxel_down_sample(xyz, voxel, normals=None, covs=None):
    """Returns (xyz, normals, covs).  A sequential per-voxel loop in input order."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel_size")
    n = x.shape[0]
    nr = None if normals is None else np.asarray(normals, np.float64).reshape(n, 3)
    cv = None if covs is None else np.asarray(covs, np.float64).reshape(n, 9)
    if n == 0:
        return x.copy(), nr, cv
    if not np.isfinite(x).all():
        raise ValueError("non-finite coordinate")
    v = voxel_indices(x, voxel)
    if v.min() < 0 or v.max() >= (1 << KEY_BITS):
        raise ValueError("voxel index out of range")
    v = v.astype(np.int64)
    key = (v[:, 2] << (2 * KEY_BITS)) | (v[:, 1] << KEY_BITS) | v[:, 0]
    order = np.argsort(key, kind="stable")                 # ascending key, input order inside a voxel
    starts = np.nonzero(np.r_[True, key[order][1:] != key[order][:-1]])[0]
    ends = np.r_[starts[1:], n]
    ox = np.empty((starts.size, 3))
    on = None if nr is None else np.empty((starts.size, 3))
    oc = None if cv is None else np.empty((starts.size, 9))
    for o, (a, b) in enumerate(zip(starts, ends)):
        p, s, c = np.zeros(3), np.zeros(3), np.zeros(9)
        for i in order[a:b]:
            p = p + x[i]
            if nr is not None and not np.isnan(nr[i]).any():
                s = s + nr[i]
            if cv is not None:
                c = c + cv[i]
        cnt = float(b - a)
        ox[o] = p / cnt
        if on is not None:
            on[o] = s / cnt
        if oc is not None:
            oc[o] = c / cnt
    return ox, on, oc


def sample_count(n, ratio):
    return int(np.float64(ratio) * np.float64(n))


def random_down_sample(n, ratio, seed):
    """Ascending int32 indices of the kept points."""
    if not (0.0 <= ratio <= 1.0):
        raise ValueError("ratio")
    count = sample_count(n, ratio)
    pairs = sorted((scan_key(seed, i), i) for i in range(n))
    return np.array(sorted(i for _, i in pairs[:count]), np.int32)


def process_scan(xyz, wide, narrow, voxel, ratio, seed, normals_fn=None, normals=None, covs=None):
    """normals_fn(xyz32) -> (normals32, covs6_32 or None) stands for the estimation stage (None: no estimation); it runs
    only on a cloud without normals.  Returns a dict: the counts, the merge cloud (xyz, normals, covs) and the rows of
    the merge cloud that form the reading (match_idx)."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    nr = None if normals is None else np.asarray(normals, np.float64).reshape(-1, 3)
    cv = None if covs is None else np.asarray(covs, np.float64).reshape(-1, 9)
    keep = M.mask_of(x, wide)
    x, nr, cv = x[keep], (None if nr is None else nr[keep]), (None if cv is None else cv[keep])
    out = {"n_wide": x.shape[0]}
    if voxel > 0 and x.shape[0]:
        x, nr, cv = voxel_down_sample(x, voxel, nr, cv)
    out["n_voxels"] = x.shape[0]
    if nr is None and normals_fn is not None and x.shape[0]:
        n32, c32 = normals_fn(x.astype(np.float32))
        nr = n32.astype(np.float64)
        if c32 is not None and cv is None:
            cv = c32.astype(np.float64)[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
    if ratio < 1.0:
        idx = random_down_sample(x.shape[0], ratio, seed)
        x, nr, cv = x[idx], (None if nr is None else nr[idx]), (None if cv is None else cv[idx])
    out["n_merge"] = x.shape[0]
    out["merge"] = (x, nr, cv)
    out["match_idx"] = np.nonzero(M.mask_of(x, narrow))[0].astype(np.int32)
    out["n_match"] = out["match_idx"].size
    return out
