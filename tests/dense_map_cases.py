"""Inputs of the dense-map tests (tests/test_dense_map_host.py on the CPU, tests/test_gpu_dense_map.py on the GPU), built once
and shared, with the counts the GPU tests pin as literals; every literal was taken from tests/dense_map_restatement.py and
is re-derived from it by the CPU tests."""
import functools

import numpy as np

from tests import dense_map_restatement as R

MAX_RADIUS = 1           # reg_crop_type


def rpy_T(roll, pitch, yaw, t):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


T_RPY = rpy_T(0.1, -0.2, 0.7, (0.4, -1.3, 0.25))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ---- one insert: 4096 points in [-3, 3]^3 at voxel 0.5 with normals and colours ----
ONE_VOXEL = 0.5
ONE_COUNT = 1558


@functools.lru_cache(None)
def one_insert():
    rng = np.random.default_rng(11)
    return rng.uniform(-3.0, 3.0, size=(4096, 3)), _unit(rng, 4096), rng.uniform(0.0, 1.0, size=(4096, 3))


# ---- successive inserts: sizes 1, 63, 64, 65, 5000; one wholly inside existing voxels; one below, one above every key ----
SEQ_VOXEL = 0.25
SEQ_NEW = (1, 62, 63, 63, 2757, 0, 39, 39)
SEQ_TOTAL = (1, 63, 126, 189, 2946, 2946, 2985, 3024)


@functools.lru_cache(None)
def successive():
    rng = np.random.default_rng(12)
    clouds = []
    for n in (1, 63, 64, 65, 5000):
        clouds.append((rng.uniform(-2.0, 2.0, size=(n, 3)), _unit(rng, n), rng.uniform(0.0, 1.0, size=(n, 3))))
    inside = clouds[4][0][rng.permutation(5000)[:700]].copy()          # the same points again: no new voxel
    clouds.append((inside, _unit(rng, 700), rng.uniform(0.0, 1.0, size=(700, 3))))
    for z in (-9.9, 9.9):                                             # z is the most significant part of the key
        x = rng.uniform(-2.0, 2.0, size=(40, 3))
        x[:, 2] = z + rng.uniform(-0.05, 0.05, size=40)
        clouds.append((x, _unit(rng, 40), rng.uniform(0.0, 1.0, size=(40, 3))))
    return tuple(clouds)


# ---- 3000 points of mixed magnitude in one voxel: the sequential sum differs from a tree sum ----
MIXED_VOXEL = 128.0


@functools.lru_cache(None)
def mixed_magnitude():
    rng = np.random.default_rng(13)
    x = 10.0 ** rng.uniform(-8.0, 2.0, size=(3000, 3))
    return x, rng.normal(size=(3000, 3)) * 10.0 ** rng.uniform(-6.0, 3.0, size=(3000, 1)), 10.0 ** rng.uniform(-9.0, 0.0, size=(3000, 3))


# ---- lattice points k * v: floor(p * (1 / v)) and floor(p / v) disagree on some ----
LATTICE_VOXELS = (0.05, 0.03, 0.1)


@functools.lru_cache(None)
def lattice(v):
    k = np.random.default_rng(17).integers(-100, 100, size=(4000, 3))
    return k.astype(np.float64) * np.float64(v)


def lattice_disagreements(v):
    x = lattice(v)
    return np.any(np.floor(x * (np.float64(1.0) / np.float64(v))) != np.floor(x / np.float64(v)), axis=1)


LATTICE_CARVE = dict(r=0.1, max_ray=1.0, truncation=0.0)


@functools.lru_cache(None)
def lattice_carve_scan(v):
    """(sensor, scan): sensors are lattice points on which the two key formulas disagree; each ray is shorter than a step,
    so its only sample is the sensor itself."""
    x = lattice(v)
    bad = x[lattice_disagreements(v)]
    sensor = bad[len(bad) // 2]
    return sensor, sensor[None, :] + np.array([[0.01, 0.0, 0.0], [0.0, 0.02, 0.01]])


# ---- key extremes at voxel 1 ----
EXT_VOXEL = 1.0
EXT_OK = np.array([[(1 << 20) - 0.5, 0.25, -((1 << 20) - 1.0)], [-((1 << 20) - 1.0), (1 << 20) - 1.0, 0.5], [0.5, 0.5, 0.5]])
EXT_BAD = {"beyond+": [float(1 << 20), 0.0, 0.0], "beyond-": [0.0, -((1 << 20) - 1.0) - 0.5, 0.0], "nan": [0.0, np.nan, 0.0],
           "inf": [0.0, 0.0, np.inf], "-inf": [-np.inf, 0.0, 0.0]}


# ---- insert_scan: MaxRadius crop at the origin, a colour range that rejects some points, a transform ----
SCAN_VOXEL = 0.2
SCAN_CROP = dict(type=MAX_RADIUS, center=(0.0, 0.0, 0.0), radius_max=3.0)
SCAN_RGB = ((0.1, 0.0, 0.2), (0.9, 0.8, 1.0))
SCAN_INSERTED = 346            # of 3000: both croppers
SCAN_INSERTED_NO_COLORS = 639   # the crop alone


@functools.lru_cache(None)
def scan_cloud():
    rng = np.random.default_rng(14)
    return rng.uniform(-4.0, 4.0, size=(3000, 3)), _unit(rng, 3000), rng.uniform(0.0, 1.0, size=(3000, 3))


# ---- carve: a wall-and-floor map, a blob around the sensor; (r, v) of the issue's list ----
CARVE_RV = ((0.1, 0.05), (0.1, 0.03), (0.15, 0.05), (0.05, 0.1))
CARVE_OFFSETS = {(0.1, 0.05): 5, (0.1, 0.03): 7, (0.15, 0.05): 6, (0.05, 0.1): 2}
CARVE_SENSOR = np.array([0.013, -0.021, 1.007])
CARVE_TRUNC, CARVE_MAX_RAY = 0.5, 2.5
CARVE_ERASED = {(0.1, 0.05): (119, 2452), (0.1, 0.03): (164, 7089), (0.15, 0.05): (145, 2426), (0.05, 0.1): (18, 628)}   # (erased, kept) voxels of "all"


@functools.lru_cache(None)
def carve_map(v):
    """Floor z ~ 0 over x in [0.6, 3], y in [-0.8, 0.8]; wall x ~ 3 over z in [0, 1.6]; a blob within 0.04 of the sensor."""
    rng = np.random.default_rng(15)
    s = 0.7 * v
    gx, gy = np.meshgrid(np.arange(0.6, 3.0, s), np.arange(-0.8, 0.8, s), indexing="ij")
    floor = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1)
    gy, gz = np.meshgrid(np.arange(-0.8, 0.8, s), np.arange(0.0, 1.6, s), indexing="ij")
    wall = np.stack([np.full(gy.size, 3.0), gy.ravel(), gz.ravel()], axis=1)
    blob = CARVE_SENSOR + rng.uniform(-0.04, 0.04, size=(30, 3))
    x = np.concatenate([floor, wall, blob]) + rng.uniform(0.0, 0.2 * v, size=(floor.shape[0] + wall.shape[0] + 30, 3))
    return x, rng.uniform(0.0, 1.0, size=x.shape)


CARVE_RAYS = ("through-floor", "short", "truncated", "max-ray", "duplicates", "degenerate", "all")


@functools.lru_cache(None)
def carve_scan(kind):
    """Scan points (map frame) of one kind of ray from CARVE_SENSOR."""
    s = CARVE_SENSOR
    floor = np.array([[1.9, 0.3, -0.5], [1.5, -0.4, -0.6], [1.2, 0.1, -0.45]])       # cross z = 0 within max_ray
    short = s + np.array([[0.03, 0.01, -0.02], [-0.02, 0.03, 0.01]])                 # shorter than one step: one sample
    trunc = np.array([[3.0, 0.2, 0.9], [3.0, -0.5, 1.2]])                            # end 0.5 before the wall
    far = np.array([[5.0, 0.1, -0.7], [6.0, -0.3, 1.1]])                             # cut by max_ray: floor crossing at > 2.5 m
    degenerate = np.array([s, [np.nan, 0.0, 0.0], [1.0, np.inf, 0.0]])               # zero length, NaN, infinite
    table = {"through-floor": floor, "short": short, "truncated": trunc, "max-ray": far,
             "duplicates": np.concatenate([floor[:1]] * 5), "degenerate": degenerate}
    if kind == "all":
        return np.concatenate([table[k] for k in CARVE_RAYS[:-1]])
    return table[kind]


@functools.lru_cache(None)
def carve_reference(r, v, kind):
    """(map before, erased keys, map after) of the restatement."""
    x, cl = carve_map(v)
    m = R.DenseMap(v)
    m.insert(x, None, cl)
    before = m.export()
    stats = {}
    erased = m.carve(carve_scan(kind), CARVE_SENSOR, r, CARVE_MAX_RAY, CARVE_TRUNC, stats)
    return before, erased, m.export(), stats


# ---- DenseMapBuilder: five scans along a short trajectory, carving every second scan ----
BUILD_VOXEL, BUILD_EVERY = 0.1, 2
BUILD_CARVE = dict(r=0.1, max_ray=3.0, truncation=0.3)
BUILD_CROP = dict(type=MAX_RADIUS, center=(0.0, 0.0, 0.0), radius_max=3.2)
BUILD_RGB = ((0.05, 0.05, 0.05), (0.95, 0.95, 0.95))
BUILD_RESULT = {False: (696, (None, 96, None, 87, None)), True: (476, (None, 162, None, 247, None))}   # voxels, erased per scan


@functools.lru_cache(None)
def build_sequence():
    """[(xyz, normals, colors)] in the sensor frame, [map-to-sensor pose]: a wall 2.5 m ahead and the floor 0.5 m below."""
    rng = np.random.default_rng(16)
    scans, poses = [], []
    for i in range(5):
        wall = np.stack([np.full(150, 2.5), rng.uniform(-1.0, 1.0, 150), rng.uniform(-0.5, 1.0, 150)], axis=1)
        floor = np.stack([rng.uniform(0.5, 3.4, 150), rng.uniform(-1.0, 1.0, 150), np.full(150, -0.5)], axis=1)
        x = np.concatenate([wall, floor]) + rng.normal(size=(300, 3)) * 0.004
        nr = np.concatenate([np.tile([-1.0, 0.0, 0.0], (150, 1)), np.tile([0.0, 0.0, 1.0], (150, 1))])
        scans.append((x, nr, rng.uniform(0.0, 1.0, size=(300, 3))))
        poses.append(rpy_T(0.0, 0.01 * i, 0.05 * i, (0.12 * i, 0.03 * i, 0.5)))
    return scans, poses


@functools.lru_cache(None)
def build_reference(in_map_frame):
    scans, poses = build_sequence()
    return R.drive_builder(scans, poses, BUILD_VOXEL, BUILD_EVERY, in_map_frame, BUILD_CROP, BUILD_RGB[0], BUILD_RGB[1],
                           **BUILD_CARVE)


def same_bits(a, b):
    """Bit-exact equality of two float64 (or integer) arrays of the same shape."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a, b)


def same_export(got, want):
    """The export dicts of capi.DenseMap and of the restatement agree bit for bit, field by field."""
    for k in ("xyz", "normals", "colors", "keys", "counts"):
        g, w = got[k], want[k]
        if (g is None) != (w is None):
            return False
        if g is not None and not same_bits(g, w):
            return False
    return True
