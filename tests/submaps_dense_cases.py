"""Inputs of the tests of the fused carve and of the collection's dense maps (tests/test_submaps_dense_host.py on the CPU,
tests/test_gpu_submaps_dense.py on the GPU), built once and shared, with the counts the GPU tests pin as
literals.  Every literal was taken from tests/dense_map_restatement.py and is re-derived from it by the CPU tests."""
import functools

import numpy as np

from tests import dense_map_cases as DK
from tests import dense_map_restatement as R
from tests import submaps_cases as SK


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def centres(keys, v):
    """One point in the middle of every voxel of `keys` (k x 3 integers)."""
    return (np.asarray(keys, np.float64) + 0.5) * np.float64(v)


# ---- carve_scan on the wall-and-floor map of tests/dense_map_cases.py ---------------------------------------------------------
CARVE = dict(max_ray=DK.CARVE_MAX_RAY, truncation=DK.CARVE_TRUNC)
SCAN_SIZES = (1, 63, 64, 65, 257)
MAP_SIZES = (1, 1023, 1025)
SIZES_RV = (0.1, 0.05)          # the (r, v) of the scan-size and map-size cases


@functools.lru_cache(None)
def all_rays():
    """The "all" rays of tests/dense_map_cases.py (map frame) without the two rows that hold a NaN or an infinity: those are
    refused by the de-duplication (all_rays_with_non_finite keeps them for the refusal test).  The zero-length ray and the
    five duplicates stay."""
    x = DK.carve_scan("all")
    return _ro(np.ascontiguousarray(x[np.all(np.isfinite(x), axis=1)]))


def all_rays_with_non_finite():
    return DK.carve_scan("all")


@functools.lru_cache(None)
def rays_in_sensor_frame():
    """(scan in the sensor frame, T map-to-sensor): T applied to the scan gives the "all" rays up to rounding."""
    T = DK.T_RPY
    x = (all_rays() - T[:3, 3]) @ T[:3, :3]
    return _ro(np.ascontiguousarray(x)), T


def repeated_rays(n):
    """n rays: the finite "all" rays, repeated in order."""
    return np.ascontiguousarray(np.resize(all_rays(), (n, 3)))


def carve_reference(r, v, points, colors, scan, sensor, T=None, max_ray=DK.CARVE_MAX_RAY, truncation=DK.CARVE_TRUNC):
    """Submap::carve on the restatement: (erased keys, export after) of transform, dedup, carve on a map of `points`."""
    m = R.DenseMap(v)
    m.insert(points, None, colors)
    x = np.asarray(scan, np.float64).reshape(-1, 3)
    if T is not None:
        x, _ = R.transform_cloud(T, x)
    x = x[R.dedup(x, v)] if len(x) else x
    erased = m.carve(x, sensor, r, max_ray, truncation)
    return erased, m.export()


@functools.lru_cache(None)
def wall_reference(r, v, in_map_frame):
    """The four (r, v) with the "all" rays: raw (the scan is the map-frame rays) or transformed from the sensor frame."""
    x, cl = DK.carve_map(v)
    if in_map_frame:
        scan, T = rays_in_sensor_frame()
        return carve_reference(r, v, x, cl, scan, DK.CARVE_SENSOR, T)
    return carve_reference(r, v, x, cl, all_rays(), DK.CARVE_SENSOR)


@functools.lru_cache(None)
def sized_map(n):
    """n voxel centres of the wall-and-floor map at SIZES_RV: min(60, (n + 1) // 2) voxels the "all" rays erase, the rest
    voxels they keep."""
    r, v = SIZES_RV
    before = DK.carve_reference(r, v, "all")[0]["keys"]
    erased, after = wall_reference(r, v, False)
    k = min(60, (n + 1) // 2)
    keys = np.concatenate([erased[:: max(len(erased) // k, 1)][:k], after["keys"][: n - k]])
    assert len(keys) == n and len(before) == len(erased) + len(after["keys"])
    return _ro(centres(keys, v)), k


@functools.lru_cache(None)
def sized_map_reference(n):
    r, v = SIZES_RV
    return carve_reference(r, v, sized_map(n)[0], None, all_rays(), DK.CARVE_SENSOR)


@functools.lru_cache(None)
def sized_scan_reference(n):
    r, v = SIZES_RV
    x, cl = DK.carve_map(v)
    return carve_reference(r, v, x, cl, repeated_rays(n), DK.CARVE_SENSOR)


# ---- brick edges: a lattice on z-layers either side of brick boundaries, rays that cross them ------------------------------------
BRICK_LAYERS = (-9, -8, -1, 0, 7, 8)
BRICK_VOXELS = 9600
BRICK_ERASED = {(0.1, 0.05): 636, (0.1, 0.03): 1114, (0.15, 0.05): 840, (0.05, 0.1): 66}


@functools.lru_cache(None)
def brick_case(v):
    """(points, sensor, ray ends, max_ray): a 40 x 40 lattice of voxel indices -20 .. 19 in x and y on BRICK_LAYERS, one point
    per voxel within +-0.2 v of its centre; everything scales with v."""
    rng = np.random.default_rng(21)
    ix, iy, iz = np.meshgrid(np.arange(-20, 20), np.arange(-20, 20), np.array(BRICK_LAYERS), indexing="ij")
    keys = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1)
    x = centres(keys, v) + rng.uniform(-0.2, 0.2, size=(len(keys), 3)) * v
    sensor = np.array([0.4, -0.3, 30.3]) * v
    ends = np.array([[3.2, 2.1, -14.0], [-7.9, 8.1, -14.0], [15.0, -15.0, -14.0], [-8.5, -0.5, -30.0]]) * v
    return _ro(x, sensor, ends) + (100.0 * v,)


@functools.lru_cache(None)
def brick_reference(r, v):
    x, sensor, ends, max_ray = brick_case(v)
    return carve_reference(r, v, x, None, ends, sensor, None, max_ray, 0.0)


# ---- key extremes: voxels at +-(2^20 - 1), rays whose neighbourhoods reach past the packable range ---------------------------------
EXT_V, EXT_R, EXT_K = 0.05, 0.1, (1 << 20) - 1
_K = EXT_K
EXT_KEYS = ((_K, 0, 0), (_K - 1, 0, 0), (_K - 2, 1, 0), (_K - 9, 0, 0), (_K - 3, 3, 0), (-_K, 0, 0), (-_K + 1, 0, 1),
            (-_K + 9, 0, 0), (-_K + 3, 0, -3), (0, _K, 0), (0, 0, -_K))
EXT_MAX_RAY = 3.0
EXT_ERASED = {"positive": ((_K - 9, 0, 0), (_K - 1, 0, 0), (_K, 0, 0), (_K - 2, 1, 0)),      # ascending (z, y, x)
              "negative": ((-_K, 0, 0), (-_K + 9, 0, 0), (-_K + 1, 0, 1))}


def ext_points():
    return centres(np.array(EXT_KEYS, np.int64), EXT_V)


def ext_ray(kind):
    """(sensor, scan of one point) along x at y = z = v / 2."""
    v, h = np.float64(EXT_V), np.float64(EXT_V) / 2
    if kind == "positive":
        return np.array([(_K - 19.5) * v, h, h]), np.array([[(_K + 0.9) * v, h, h]])
    return np.array([(-_K + 20.9) * v, h, h]), np.array([[(-_K + 0.1) * v, h, h]])


@functools.lru_cache(None)
def ext_reference(kind):
    sensor, scan = ext_ray(kind)
    return carve_reference(EXT_R, EXT_V, ext_points(), None, scan, sensor, None, EXT_MAX_RAY, 0.0)


# ---- the collection: one dense insert per step of the walk of tests/submaps_cases.py ---------------------------------------------------
DENSE = dict(every=2, voxel=0.1, crop=dict(type=DK.MAX_RADIUS, center=(0.0, 0.0, 0.0), radius_max=3.5),
             rgb=((0.05, 0.05, 0.05), (0.95, 0.95, 0.95)), carve=dict(r=0.1, max_ray=1.0, truncation=0.3))
DENSE_N = 700
# the submap that receives step k of the walk (the active one BEFORE the mapper's insert), from tests/submaps_cases.host_walk
WALK_RECEIVERS = (0, 0, 1, 1, 2, 2, 2, 3, 2, 2, 4, 4, 5, 6)


@functools.lru_cache(None)
def dense_scan_at(k):
    """700 raw points of step k in the sensor frame with normals and colours."""
    xs, ns = SK.scan_at(k, DENSE_N, seed=57)
    cl = np.random.default_rng(2000 + k).uniform(0.0, 1.0, size=(DENSE_N, 3))
    return _ro(np.array(xs), np.array(ns), cl)


class DenseBuilder:
    """Submap::insertScanDenseMap on the restatement, one step at a time (the loop body of R.drive_builder)."""

    def __init__(self, p=None, in_map_frame=False):
        self.p = dict(DENSE if p is None else p)
        self.map = R.DenseMap(self.p["voxel"])
        self.in_map_frame = in_map_frame
        self.scans_inserted = 0
        self.erased = []                       # per insert: None (no carve) or the erased keys

    def insert(self, xyz, normals, colors, T, perform_carving=True):
        p, T = self.p, np.asarray(T, np.float64)
        n_inserted, _ = self.map.insert_scan(xyz, normals, colors, p["crop"], p["rgb"][0], p["rgb"][1], T)
        out = None
        if perform_carving and self.map.size() > 0 and self.scans_inserted % p["every"] == 1:
            x = np.asarray(xyz, np.float64).reshape(-1, 3)
            if self.in_map_frame:
                x, _ = R.transform_cloud(T, x)
            x = x[R.dedup(x, p["voxel"])]
            out = self.map.carve(x, T[:3, 3], **p["carve"])
        self.erased.append(out)
        self.scans_inserted += 1
        return n_inserted, out


def walk_receivers():
    """The active submap before every insert of the walk, from the CPU restatement of the collection."""
    col = SK.R.SubmapCollection(SK.PARAMS, SK.HostMap)
    out = []
    steps = SK.walk()
    gen = SK.drive(col)
    for k in range(len(steps)):
        out.append(col.activeSubmapIdx_)
        next(gen)
    return tuple(out)


@functools.lru_cache(None)
def dense_walk(in_map_frame):
    """[per step: {submap: (export, scans_inserted)} after the step], [builders]: the restatement's dense maps along the walk."""
    steps = SK.walk()
    builders, states = {}, []
    for k, rec in enumerate(WALK_RECEIVERS):
        b = builders.setdefault(rec, DenseBuilder(in_map_frame=in_map_frame))
        xs, ns, cl = dense_scan_at(k)
        b.insert(xs, ns, cl, steps[k][2])
        states.append({i: (bb.map.export(), bb.scans_inserted) for i, bb in builders.items()})
    return states, builders


# ---- reg_submaps_transform with dense maps ---------------------------------------------------------------------------------------------
TRANSFORM_IDS = (0, 1)             # the others follow their parents by POSITION (reg_host_submaps_transform_plan)


def transform_increments():
    out = []
    for k in range(len(TRANSFORM_IDS)):
        out.append(DK.rpy_T(0.01 * (k + 1), -0.02, 0.03 * (k + 1), (0.1 * k + 0.05, -0.05, 0.02)))
    return out
