"""Inputs shared by tests/test_map_rows_host.py (CPU: the restatements pinned by hand, the inputs' preconditions) and
tests/test_gpu_map_rows.py (device against the restatements): cropping volumes on exact boundaries, voxelization clouds
and space-carving scenes.  Every builder is deterministic, cached and returns read-only arrays.

Volumes are dicts as `capi.Registration._crop_struct` takes them; `mask_of` evaluates `oracle.crop_mask` on one.
Voxel sizes are 1.0, 0.5 or 0.25 wherever a point is meant to lie on a face: their reciprocal is exact, so is
`p * (1 / voxel)` for the lattice points used, and `floor` alone decides."""
import functools

import numpy as np

from oracle import oracle as orc

NONE, MAX_RADIUS, MIN_RADIUS, MIN_MAX_RADIUS, CYLINDER = 0, 1, 2, 3, 4
KEY_LIMIT = 1 << 20          # 21 bits per axis, offset binary: indices -(2^20 - 1) .. 2^20 - 1 are accepted
BLOCK_EDGES = (1, 255, 256, 257, 513)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def mask_of(xyz, vol):
    if vol is None:
        return np.ones(np.asarray(xyz).shape[0], bool)
    kw = {k: v for k, v in vol.items() if k != "type"}
    return orc.crop_mask(xyz, vol["type"], **kw)


def c9(c6):
    """Symmetric 3x3 (9 doubles a row) from xx xy xz yy yz zz."""
    return np.ascontiguousarray(np.asarray(c6, np.float64)[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]])


# ---- cropping ------------------------------------------------------------------------------------------------------------------
CENTER = (1.0, -2.0, 0.5)     # off-origin; every offset below is exact in fp64


@functools.lru_cache(maxsize=None)
def boundary_cloud():
    """Ten points around CENTER; |(3, 4, 0)| = |(0, 0, 5)| = |(-3, 0, -4)| = 5 and |(6, 8, 0)| = 10 exactly.  Points 2 / 3
    are one ulp of z beyond / before the sphere of radius 5 on the z axis, where d = sqrt(dz^2) has no other term."""
    cx, cy, cz = CENTER
    return _ro(np.array([
        [cx + 3.0, cy + 4.0, cz],                              # 0  on the sphere r = 5, on the cylinder wall
        [cx, cy, cz + 5.0],                                    # 1  on the sphere, z = 5.5 = max_z
        [cx, cy, np.nextafter(cz + 5.0, np.inf)],              # 2  one ulp outside, one ulp above max_z
        [cx, cy, np.nextafter(cz + 5.0, -np.inf)],             # 3  one ulp inside
        [cx, cy, cz],                                          # 4  the centre, d = 0
        [cx - 3.0, cy, cz - 4.0],                              # 5  on the sphere, z = -3.5 = min_z
        [cx + 6.0, cy + 8.0, cz],                              # 6  d = 10
        [np.nan, cy, cz],                                      # 7  NaN x
        [cx, cy, np.nan],                                      # 8  NaN z
        [cx + 3.0, cy + 4.0, np.nextafter(cz - 4.0, -np.inf)],  # 9  on the cylinder wall, one ulp below min_z; d > 5
    ], np.float64))


# volume -> the mask written out by hand (1: inside)
BOUNDARY_VOLUMES = {
    "max5": (dict(type=MAX_RADIUS, center=CENTER, radius_max=5.0), [1, 1, 0, 1, 1, 1, 0, 0, 0, 0]),
    "min5": (dict(type=MIN_RADIUS, center=CENTER, radius_min=5.0), [1, 1, 1, 0, 0, 1, 1, 0, 0, 1]),
    "minmax5_5": (dict(type=MIN_MAX_RADIUS, center=CENTER, radius_min=5.0, radius_max=5.0), [1, 1, 0, 0, 0, 1, 0, 0, 0, 0]),
    "minmax5_10": (dict(type=MIN_MAX_RADIUS, center=CENTER, radius_min=5.0, radius_max=10.0), [1, 1, 1, 0, 0, 1, 1, 0, 0, 1]),
    "cyl": (dict(type=CYLINDER, center=CENTER, radius_max=5.0, min_z=-3.5, max_z=5.5), [1, 1, 0, 1, 1, 1, 0, 0, 0, 0]),
}

PATTERN_VOLUME = dict(type=MAX_RADIUS, center=CENTER, radius_max=5.0)


@functools.lru_cache(maxsize=None)
def crop_pattern(m, pattern):
    """m points with unit normals: `alt` alternates inside / outside PATTERN_VOLUME starting inside, `one` keeps only
    index m // 2, `all` keeps everything.  Returns (xyz, normals, inside)."""
    rng = np.random.default_rng(1000 + m)
    inside = {"alt": np.arange(m) % 2 == 0, "one": np.arange(m) == m // 2, "all": np.ones(m, bool)}[pattern]
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = np.where(inside, rng.uniform(0.5, 4.0, size=m), rng.uniform(6.0, 9.0, size=m))
    xyz = np.asarray(CENTER) + d * r[:, None]
    nrm = rng.normal(size=(m, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return _ro(xyz, nrm, inside)


def half_ulp_up(a32):
    """fp64 values exactly half way between each fp32 value and its neighbour away from zero: round-to-nearest-even ties."""
    a32 = np.asarray(a32, np.float32)
    nxt = np.nextafter(a32, np.where(a32 >= 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    return (a32.astype(np.float64) + nxt.astype(np.float64)) * 0.5


# fp64 values in or next to the fp32 subnormal range and what round-to-nearest-even makes of them
SUBNORMALS = np.array([2.0 ** -130, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149, 2.0 ** -150 * (1 + 2.0 ** -30), 3e-42,
                       -(2.0 ** -150), 2.0 ** -126 * (1 - 2.0 ** -25)], np.float64)


# ---- voxelization --------------------------------------------------------------------------------------------------------------
def _attrs(rng, m):
    nrm = rng.normal(size=(m, 3))
    cov = c9(rng.uniform(-1.0, 1.0, size=(m, 6)))
    cov[:, 1] += 0.25          # a non-symmetric input: every one of the nine entries travels on its own
    return nrm, cov


@functools.lru_cache(maxsize=None)
def vox_half(m):
    """m points, every other one inside the ball (the first inside), several points per voxel at 0.5."""
    rng = np.random.default_rng(2000 + m)
    inside = np.arange(m) % 2 == 0
    xyz = np.where(inside[:, None], rng.uniform(-1.5, 1.5, size=(m, 3)), rng.uniform(6.0, 8.0, size=(m, 3)))
    nrm, cov = _attrs(rng, m)
    vol = dict(type=MAX_RADIUS, center=(0.0, 0.0, 0.0), radius_max=4.0)
    assert np.array_equal(mask_of(xyz, vol), inside)
    return _ro(xyz, nrm, cov) + (0.5, vol)


@functools.lru_cache(maxsize=None)
def vox_all_inside():
    rng = np.random.default_rng(2100)
    xyz = rng.uniform(-2.0, 2.0, size=(257, 3))
    nrm, cov = _attrs(rng, 257)
    return _ro(xyz, nrm, cov) + (0.5, dict(type=MAX_RADIUS, center=(0.0, 0.0, 0.0), radius_max=100.0))


@functools.lru_cache(maxsize=None)
def vox_all_outside():
    xyz, nrm, cov, voxel, _ = vox_all_inside()
    return xyz, nrm, cov, voxel, dict(type=MAX_RADIUS, center=(100.0, 0.0, 0.0), radius_max=1.0)


VOX_VOLUMES = {
    "none": None,
    "max": dict(type=MAX_RADIUS, center=(0.5, -0.5, 0.25), radius_max=4.5),
    "min": dict(type=MIN_RADIUS, center=(0.5, -0.5, 0.25), radius_min=5.5),
    "minmax": dict(type=MIN_MAX_RADIUS, center=(0.5, -0.5, 0.25), radius_min=3.0, radius_max=5.5),
    "cyl": dict(type=CYLINDER, center=(0.5, -0.5, 100.0), radius_max=5.0, min_z=-4.0, max_z=3.0),
}


@functools.lru_cache(maxsize=None)
def vox_volume_cloud():
    rng = np.random.default_rng(2200)
    xyz = rng.uniform(-6.0, 6.0, size=(513, 3))
    nrm, cov = _attrs(rng, 513)
    return _ro(xyz, nrm, cov) + (0.5,)


@functools.lru_cache(maxsize=None)
def vox_long_run():
    """100 points of voxel (0, 0, 0), then 1000 points of voxel (1, 0, 0) interleaved with 1000 of voxel (2, 0, 0), at
    voxel size 0.5: after the sort the run of (1, 0, 0) covers positions 100..1099 and that of (2, 0, 0) 1100..2099, each
    across several 256-thread blocks, and only a stable sort restores index order inside them.  Coordinates, normals and
    covariances spread over many orders of magnitude, so that the order of the fp64 additions shows in the bits."""
    rng = np.random.default_rng(2300)

    def inside_voxel(n):
        return 0.5 * 10.0 ** (-rng.uniform(0.0, 12.0, size=(n, 3))) * rng.uniform(0.5, 0.999, size=(n, 3))

    a, b, c = inside_voxel(100), inside_voxel(1000), inside_voxel(1000)
    b[:, 0] += 0.5
    c[:, 0] += 1.0
    inter = np.empty((2000, 3))
    inter[0::2], inter[1::2] = b, c
    xyz = np.concatenate([a, inter])
    m = xyz.shape[0]
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    nrm = sign((m, 3)) * 10.0 ** rng.uniform(-8.0, 8.0, size=(m, 3))
    cov = sign((m, 9)) * 10.0 ** rng.uniform(-8.0, 8.0, size=(m, 9))
    return _ro(xyz, nrm, cov) + (0.5, None)


@functools.lru_cache(maxsize=None)
def vox_face_lattice(voxel):
    """Every multiple of `voxel` in [-1, 1)^3 (exactly on three faces each, -0.0 included) and the same lattice moved by
    voxel / 2 along x, in that order: two points per voxel, every sum and mean exact."""
    g = np.arange(-1.0, 1.0, voxel)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    lat[lat == 0.0] = -0.0
    assert np.signbit(lat).any() and (lat < 0).any()
    xyz = np.concatenate([lat, lat + np.array([voxel / 2, 0.0, 0.0])])
    return _ro(xyz), voxel


@functools.lru_cache(maxsize=None)
def vox_key_extremes():
    """Voxel indices +-(2^20 - 1) on all three axes at once (voxel 1.0), the eight sign combinations in a scrambled
    order, two points in each, plus the voxels around the origin."""
    e = float(KEY_LIMIT - 1)
    signs = np.array([[1, -1, 1], [-1, -1, -1], [1, 1, 1], [-1, 1, -1], [1, 1, -1], [-1, -1, 1], [1, -1, -1], [-1, 1, 1]], np.float64)
    corners = signs * e + 0.25
    near = np.array([[0.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.5, 0.5, -0.5], [-0.5, -0.5, -0.5]])
    xyz = np.concatenate([corners, near, corners + 0.5])
    idx = np.floor(xyz)
    assert np.abs(idx).max() == e and np.all(np.abs(idx[:8]) == e)
    return _ro(xyz), 1.0


def vox_out_of_range_point(axis):
    """A point whose voxel index on `axis` is 2^20 (voxel 1.0): one past the accepted range."""
    p = np.array([0.5, 0.5, 0.5])
    p[axis] = KEY_LIMIT + 0.5
    return p


@functools.lru_cache(maxsize=None)
def vox_normal_cases():
    """Voxel size 1.0, one voxel per case along x, two rows of y (means of normals are not exact: three points each):
       x = 0: every normal NaN                      -> the zero vector
       x = 1: normals that cancel exactly           -> the zero vector stays zero (no 0 / 0)
       x = 2: one normal with a single NaN component -> that whole normal is skipped, the divisor stays 3
       x = 3: plain"""
    nan = np.nan
    xyz = np.array([[0.2, 0.5, 0.5], [0.4, 0.5, 0.5], [0.6, 0.5, 0.5],
                    [1.2, 0.5, 0.5], [1.4, 0.5, 0.5], [1.6, 0.5, 0.5],
                    [2.2, 0.5, 0.5], [2.4, 0.5, 0.5], [2.6, 0.5, 0.5],
                    [3.2, 0.5, 0.5], [3.4, 0.5, 0.5], [3.6, 0.5, 0.5]])
    nrm = np.array([[nan, nan, nan], [nan, nan, nan], [nan, nan, nan],
                    [1.0, 2.0, 3.0], [-0.25, -0.5, -0.75], [-0.75, -1.5, -2.25],
                    [0.3, 0.1, 0.7], [5.0, nan, 5.0], [0.1, 0.9, 0.2],
                    [0.3, 0.1, 0.7], [0.2, 0.2, 0.2], [0.1, 0.9, 0.2]])
    return _ro(xyz, nrm) + (1.0,)


# ---- space carving -------------------------------------------------------------------------------------------------------------
def carve_want(case):
    mask = None if case.get("subset") is None else mask_of(case["map"], case["subset"])
    return orc.carve_indices(case["map"], case["scan"], case["sensor"], case["voxel"], case["max_ray"], case["trunc"],
                             case["min_dot"], case.get("nrm"), mask)


def _case(map_xyz, scan, sensor, voxel, max_ray=20.0, trunc=0.1, min_dot=0.5, nrm=None, subset=None):
    map_xyz, scan = np.asarray(map_xyz, np.float64).reshape(-1, 3), np.asarray(scan, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3) if nrm is not None else None
    _ro(map_xyz, scan, nrm)
    return dict(map=map_xyz, scan=scan, sensor=tuple(float(v) for v in sensor), voxel=voxel, max_ray=max_ray, trunc=trunc,
                min_dot=min_dot, nrm=nrm, subset=subset)


@functools.lru_cache(maxsize=None)
def carve_block_edge(n):
    """n rays of length 4 (16 steps of 0.25) through n map points; normals on every point, a subset volume."""
    rng = np.random.default_rng(3000 + n)
    sensor = (0.1, 0.2, 0.3)
    mp = rng.uniform(-3.0, 3.0, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    scan = np.asarray(sensor) + 4.0 * d
    return _case(mp, scan, sensor, 0.25, nrm=rng.normal(size=(n, 3)), min_dot=0.3,
                 subset=dict(type=MAX_RADIUS, center=sensor, radius_max=3.5))


def carve_short_ray():
    """length 0.05 < truncation 0.1: length - truncation < 0, so reach = step and the only sample is the sensor itself.
    Map: 0 in the sensor's voxel, 1 in the next voxel along the ray, 2 in the voxel of the scan point's far side."""
    return _case([[0.6, 0.6, 0.6], [1.1, 0.6, 0.6], [0.1, 0.6, 0.6]], [[0.65, 0.6, 0.6]], (0.6, 0.6, 0.6), 0.5)


def carve_max_ray():
    """A ray of length 10 along x, max_ray 3, step 0.5: samples at 0, 0.5 .. 2.5.  Map points at x = 1.2, 2.7 (voxel of the
    last sample), 3.2 and 8.0 (beyond max_ray, before the scan point)."""
    return _case([[1.2, 0.1, 0.1], [2.7, 0.1, 0.1], [3.2, 0.1, 0.1], [8.0, 0.1, 0.1]], [[10.25, 0.25, 0.25]],
                 (0.25, 0.25, 0.25), 0.5, max_ray=3.0)


@functools.lru_cache(maxsize=None)
def carve_axis_rays():
    """Sensor (1.0, 0.5, -0.5) exactly on three voxel faces of a 0.25 grid; six rays of length 4 along +-x, +-y, +-z: every
    sample is sensor + k * 0.25 exactly, on a face.  The map holds the centre and the lower corner of every voxel within 5
    voxels around every sample line, so a sample that floor() puts one voxel off marks other points."""
    sensor = np.array([1.0, 0.5, -0.5])
    scan = np.concatenate([sensor + 4.0 * np.eye(3), sensor - 4.0 * np.eye(3)])
    pts = []
    for axis in range(3):
        for k in range(-18, 19):
            for off in (-1, 0):
                for o2 in (-1, 0):
                    v = sensor / 0.25
                    v[axis] += k
                    v[(axis + 1) % 3] += off
                    v[(axis + 2) % 3] += o2
                    pts.append(v * 0.25)                  # lower corner: on the faces
                    pts.append(v * 0.25 + 0.125)          # centre
    return _case(np.array(pts), scan, sensor, 0.25, trunc=0.25)


def carve_subset_split():
    """Four map points in voxel (2, 0, 0) at voxel 1.0, two of them inside the subset ball; the ray passes through."""
    mp = [[2.1, 0.1, 0.1], [2.9, 0.9, 0.9], [2.2, 0.1, 0.2], [2.8, 0.9, 0.8], [4.5, 0.5, 0.5]]
    return _case(mp, [[6.5, 0.5, 0.5]], (0.5, 0.5, 0.5), 1.0, subset=dict(type=MAX_RADIUS, center=(2.0, 0.0, 0.0), radius_max=0.4))


def carve_min_dot(min_dot):
    """Ray along +x (u = (1, 0, 0) exactly: 4 / 4), one map point with the normal (3, 4, 0): |u . n / |n|| = 3.0 / 5.0."""
    return _case([[2.1, 0.1, 0.1]], [[4.5, 0.5, 0.5]], (0.5, 0.5, 0.5), 1.0, nrm=[[3.0, 4.0, 0.0]], min_dot=min_dot)


MIN_DOT_TIE = 3.0 / 5.0        # what the restatement computes for that pair: sqrt(25) = 5, 3 / 5, 1 * 0.6 + 0 + 0


def carve_degenerate_normals():
    """Map points on the ray with a zero normal, a NaN normal, a normal along the ray (removed) and one across it (kept)."""
    mp = [[1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5], [4.5, 0.5, 0.5]]
    nrm = [[0.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 3.0]]
    return _case(mp, [[8.5, 0.5, 0.5]], (0.5, 0.5, 0.5), 1.0, nrm=nrm)


def carve_key_edge():
    """Two cases on one map (voxel 1.0): a sensor 3.5 voxels inside index 2^20 with a ray of length 10 pointing outwards
    along +x, and one 3.5 voxels inside -(2^20) with a ray along -y.  The samples past index +-(2^20 - 1) have no key and
    are skipped.  A key computed without the range check would carry into the next field: index 2^20 + 1 on x lands on
    (-(2^20 - 1), y + 1, z), where map point 2 waits."""
    L = float(KEY_LIMIT)
    mp = [[L - 0.75, 0.5, 0.5],           # 0  index 2^20 - 1 on x, on the first ray: removed by it
          [L - 2.25, 0.5, 0.5],           # 1  on the first ray: removed by it
          [-L + 1.5, 1.5, 0.5],           # 2  where x index 2^20 + 1 would wrap to: kept
          [0.5, -L + 1.25, 0.5],          # 3  index -(2^20 - 1) on y, on the second ray: removed by it
          [0.5, -L + 2.25, 0.5],          # 4  on the second ray: removed by it
          [0.5, 0.5, 0.5]]                # 5  far from both rays
    return (_case(mp, [[L - 3.5 + 10.0, 0.5, 0.5]], (L - 3.5, 0.5, 0.5), 1.0),
            _case(mp, [[0.5, -L + 3.5 - 10.0, 0.5]], (0.5, -L + 3.5, 0.5), 1.0))


def carve_bad_scan_points():
    """NaN, +-inf and a zero-length ray are skipped; the one valid ray removes point 0 only."""
    sensor = (0.5, 0.5, 0.5)
    mp = [[2.5, 0.5, 0.5], [0.6, 1.6, 0.6], [0.5, 2.5, 0.5]]
    scan = [[np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], list(sensor), [4.5, 0.5, 0.5],
            [0.5, 0.5, np.nan]]
    return _case(mp, scan, sensor, 1.0, trunc=1.0)


@functools.lru_cache(maxsize=None)
def carve_duplicate_rays():
    """300 identical rays through a voxel that holds three map points (indices 1, 3, 4)."""
    mp = [[9.0, 9.0, 9.0], [2.2, 0.5, 0.5], [9.5, 9.0, 9.0], [2.5, 0.4, 0.6], [2.7, 0.5, 0.5]]
    return _case(mp, np.tile([[4.5, 0.5, 0.5]], (300, 1)), (0.5, 0.5, 0.5), 1.0)
