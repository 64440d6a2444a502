"""A literal numpy / Python restatement of the dense map's numeric contract (include/o3dslam_reg.h): a dict keyed
by integer triples, float64 scalars, sequential sums with the contract's associations.  Written from the contract, one
rounding per operation (numpy's elementwise operators and Python floats are IEEE doubles without contraction).  Also the
driver of icp.DenseMapBuilder's sequence (Submap.cpp:98-113,146-157)."""
import math

import numpy as np

LIMIT = 1 << 20        # voxel indices lie within +-(2^20 - 1)
MAX_OFFSETS = 16
MAX_STEPS = 65536.0


def _f(v):
    return np.float64(v)


def map_key(p, voxel):
    """floor(p * (1.0 / voxel)) per axis -> (x, y, z); ValueError for a non-finite coordinate or an index outside +-2^20.
    On the device: vox_index / vox_fits / vox_pack of csrc/kernels_cloud64.hpp, called from k_dm_keys."""
    inv = _f(1.0) / _f(voxel)
    out = []
    for c in p:
        c = _f(c)
        if not np.isfinite(c):
            raise ValueError("non-finite coordinate")
        k = np.floor(c * inv)
        if not abs(k) < LIMIT:
            raise ValueError("voxel index outside +-2^20")
        out.append(int(k))
    return tuple(out)


def transform_point(T, p):
    """w = ((T30 x + T31 y) + T32 z) + T33; x' = (((T00 x + T01 y) + T02 z) + T03) / w"""
    T = np.asarray(T, np.float64)
    x, y, z = (_f(v) for v in p)
    w = ((T[3, 0] * x + T[3, 1] * y) + T[3, 2] * z) + T[3, 3]
    return np.array([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]) / w for r in range(3)], np.float64)


def transform_normal(T, n):
    """(T (n, 0)).head<3>(): (T00 nx + T01 ny) + T02 nz"""
    T = np.asarray(T, np.float64)
    x, y, z = (_f(v) for v in n)
    return np.array([(T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z for r in range(3)], np.float64)


def transform_cloud(T, xyz, normals=None):
    x = np.array([transform_point(T, p) for p in xyz], np.float64).reshape(-1, 3)
    n = np.array([transform_normal(T, v) for v in normals], np.float64).reshape(-1, 3) if normals is not None else None
    return x, n


def offsets(r, v):
    """The running sum -r, +v, +v ... while <= r (VoxelHashMap.cpp:25-27)."""
    r, v = _f(r), _f(v)
    out = []
    d = -r
    while d <= r:
        if len(out) == MAX_OFFSETS:
            raise ValueError("more than 16 offsets per axis")
        out.append(d)
        d = d + v
    return np.array(out, np.float64)


def check_carve_args(r, max_ray, truncation, voxel):
    if not (math.isfinite(r) and r > 0 and math.isfinite(max_ray) and max_ray > 0 and math.isfinite(truncation)):
        raise ValueError("carve: radius and max_ray finite and > 0, truncation finite")
    off = offsets(r, voxel)
    if _f(max_ray) / (_f(2.0) * _f(r)) > MAX_STEPS:
        raise ValueError("carve: too many steps")
    return off


def dedup(xyz, voxel):
    """removeDuplicatePointsWithinSameVoxels: the lowest-index point of every voxel, ascending indices."""
    seen, kept = set(), []
    for i, p in enumerate(np.asarray(xyz, np.float64).reshape(-1, 3)):
        k = map_key(p, voxel)
        if k not in seen:
            seen.add(k)
            kept.append(i)
    return np.array(kept, np.int32)


def color_mask(colors, rgb_min, rgb_max):
    c = np.asarray(colors, np.float64)
    return np.all((np.asarray(rgb_min, np.float64) <= c) & (c <= np.asarray(rgb_max, np.float64)), axis=1)


def crop_mask(xyz, crop):
    """The volumes of croppers.cpp:118-170 (crop: the dict of capi.Registration.set_target_f64; None: everything)."""
    x = np.asarray(xyz, np.float64)
    if crop is None or crop.get("type", 0) == 0:
        return np.ones(x.shape[0], bool)
    d = x - np.asarray(crop.get("center", (0.0, 0.0, 0.0)), np.float64)
    t = crop["type"]
    if t == 4:
        rad = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        return (x[:, 2] >= crop["min_z"]) & (x[:, 2] <= crop["max_z"]) & (rad <= crop["radius_max"])
    rad = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    if t == 1:
        return rad <= crop["radius_max"]
    if t == 2:
        return rad >= crop["radius_min"]
    return (rad <= crop["radius_max"]) & (rad >= crop["radius_min"])


class DenseMap:
    """o3d_slam::VoxelizedPointCloud: voxels[(x, y, z)] = [count, position sum, normal sum, colour sum]."""

    def __init__(self, voxel):
        self.voxel = _f(voxel)
        self.voxels = {}
        self.has_normals = self.has_colors = False

    def size(self):
        return len(self.voxels)

    def clear(self):
        self.voxels = {}

    def insert(self, xyz, normals=None, colors=None, T=None):
        """Returns (n_voxels, n_new).  A refused point (ValueError) leaves the map unchanged."""
        x = np.asarray(xyz, np.float64).reshape(-1, 3)
        nr = np.asarray(normals, np.float64).reshape(-1, 3) if normals is not None else None
        cl = np.asarray(colors, np.float64).reshape(-1, 3) if colors is not None else None
        if T is not None:
            x, nr = transform_cloud(T, x, nr)
        keys = [map_key(p, self.voxel) for p in x]       # every point is checked before the first one is added
        before = len(self.voxels)
        for i, k in enumerate(keys):
            a = self.voxels.get(k)
            if a is None:
                a = self.voxels[k] = [0, np.zeros(3), np.zeros(3), np.zeros(3)]
            a[0] += 1
            a[1] = a[1] + x[i]
            if nr is not None:
                a[2] = a[2] + nr[i]
            if cl is not None:
                a[3] = a[3] + cl[i]
        if x.shape[0]:
            self.has_normals = self.has_normals or nr is not None
            self.has_colors = self.has_colors or cl is not None
        return len(self.voxels), len(self.voxels) - before

    def insert_scan(self, xyz, normals=None, colors=None, crop=None, rgb_min=(0, 0, 0), rgb_max=(1, 1, 1), T=None):
        """Submap.cpp:99-106.  Returns (n_inserted, n_voxels)."""
        x = np.asarray(xyz, np.float64).reshape(-1, 3)
        keep = crop_mask(x, crop)
        if colors is not None:
            keep = keep & color_mask(colors, rgb_min, rgb_max)
        pick = lambda a: np.asarray(a, np.float64).reshape(-1, 3)[keep] if a is not None else None
        if keep.sum() > 0:
            self.insert(x[keep], pick(normals), pick(colors), T)
        return int(keep.sum()), len(self.voxels)

    def sorted_keys(self):
        return sorted(self.voxels, key=lambda k: (k[2], k[1], k[0]))

    def export(self):
        """dict(xyz, normals, colors, keys, counts) in ascending (z, y, x) key order; sum / count, nothing re-normalised."""
        ks = self.sorted_keys()
        col = lambda j: np.array([self.voxels[k][j] / _f(self.voxels[k][0]) for k in ks], np.float64).reshape(-1, 3)
        return dict(xyz=col(1), normals=col(2) if self.has_normals else None, colors=col(3) if self.has_colors else None,
                    keys=np.array(ks, np.int32).reshape(-1, 3), counts=np.array([self.voxels[k][0] for k in ks], np.int32))

    def sums(self):
        ks = self.sorted_keys()
        return tuple(np.array([self.voxels[k][j] for k in ks], np.float64).reshape(-1, 3) for j in (1, 2, 3))

    def neighborhood_keys(self, sample, r, off):
        """getVoxelsWithinPointNeighborhood: the lookup keys of one sample, as a set (marks are idempotent)."""
        v = self.voxel
        g = np.array([(dx, dy, dz) for dx in off for dy in off for dz in off], np.float64).reshape(-1, 3)
        t = sample[None, :] + g
        k = np.floor(t / v)
        c = k * v + v * _f(0.5)
        d = t - c
        ok = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= _f(r)
        cand = [k[i] for i in np.nonzero(ok)[0]] + [np.floor(sample / v)]
        return {tuple(int(a) for a in c3) for c3 in cand if np.all(np.abs(c3) < LIMIT)}, int(ok.sum()), int((~ok).sum())

    def carve(self, scan, sensor, r=0.1, max_ray=20.0, truncation=0.1, stats=None):
        """getKeysOfCarvedPoints + removeKey.  Returns the erased keys, k x 3 int32, ascending (z, y, x)."""
        off = check_carve_args(r, max_ray, truncation, self.voxel)
        s = np.asarray(sensor, np.float64)
        step = _f(2.0) * _f(r)
        hit = set()
        if not self.voxels:
            return np.zeros((0, 3), np.int32)
        for p in np.asarray(scan, np.float64).reshape(-1, 3):
            d = p - s
            length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if not (length > 0.0) or not (length < np.inf):
                continue
            u = d / length
            reach = max(step, min(length - _f(truncation), _f(max_ray)))
            distance = _f(0.0)
            while distance < reach:
                sample = distance * u + s
                keys, n_ok, n_rej = self.neighborhood_keys(sample, r, off)
                if stats is not None:
                    stats["accepted"] = stats.get("accepted", 0) + n_ok
                    stats["rejected"] = stats.get("rejected", 0) + n_rej
                    stats["fallback"] = stats.get("fallback", 0) + (n_ok == 0)
                hit |= {k for k in keys if k in self.voxels}
                distance = distance + step
        for k in hit:
            del self.voxels[k]
        ks = sorted(hit, key=lambda k: (k[2], k[1], k[0]))
        return np.array(ks, np.int32).reshape(-1, 3)

    def transform(self, T):
        """VoxelizedPointCloud::transform, literally: position and normal sums become ((R0 x + R1 y) + R2 z) + t."""
        T = np.asarray(T, np.float64)
        move = lambda s: np.array([((T[r, 0] * s[0] + T[r, 1] * s[1]) + T[r, 2] * s[2]) + T[r, 3] for r in range(3)], np.float64)
        for a in self.voxels.values():
            a[1] = move(a[1])
            if self.has_normals:
                a[2] = move(a[2])

    def center(self):
        c = np.zeros(3)
        for k in self.sorted_keys():
            a = self.voxels[k]
            c = c + a[1] / _f(a[0])
        return c / (_f(len(self.voxels)) + _f(1e-6))


def drive_builder(scans, poses, voxel, carve_every, carve_in_map_frame=False, crop=None, rgb_min=(0, 0, 0), rgb_max=(1, 1, 1),
                  r=0.1, max_ray=20.0, truncation=0.1):
    """Submap::insertScanDenseMap over a sequence: scans = [(xyz, normals, colors)], poses = 4x4 map-to-sensor.  Carving runs
    when nScansInsertedDenseMap_ % carve_every == 1 (the counter is incremented after the call), on the de-duplicated RAW scan
    against the map-frame sensor position -- the reference's choice -- or, carve_in_map_frame, on the transformed one.
    Returns (map, [erased keys per scan or None])."""
    m = DenseMap(voxel)
    erased = []
    n_inserted = 0
    for (xyz, nr, cl), T in zip(scans, poses):
        T = np.asarray(T, np.float64)
        m.insert_scan(xyz, nr, cl, crop, rgb_min, rgb_max, T)
        out = None
        if m.size() > 0 and n_inserted % carve_every == 1:
            x = np.asarray(xyz, np.float64).reshape(-1, 3)
            if carve_in_map_frame:
                x, _ = transform_cloud(T, x)
            x = x[dedup(x, voxel)]
            out = m.carve(x, T[:3, 3], r, max_ray, truncation)
        erased.append(out)
        n_inserted += 1
    return m, erased
