"""Inputs shared by tests/test_constraints_host.py (CPU: the restatement alone) and tests/test_gpu_constraints.py (device): the
walk of tests/submaps_cases.py with a wider view.  The flat maps of that walk (z spans 0.18 m) are fine for selection and
bookkeeping and degenerate for ICP and FPFH; here every scan reaches 11 m and the maps keep 14 m, so the submaps hold walls
(z from -1.7 to 6.6).  Every builder is deterministic, cached and returns read-only arrays."""
import functools

import numpy as np

from tests import map_cloud_cases as K
from tests import map_cloud_restatement as MR
from tests import submaps_cases as S
from tests import submaps_restatement as R

WALK_X, WALK_N, RAW_N = S.WALK_X, S.WALK_N, S.RAW_N
REACH = 11.0
MAP = dict(S.MAP, crop=dict(type=K.MAX_RADIUS, center=(0.0, 0.0, 0.0), radius_max=14.0))
PARAMS = dict(S.PARAMS, max_num_points=100000)
pose_at = S.pose_at

# what the restatement gives on this walk (tests/test_constraints_host.py asserts it)
N_SUBMAPS = 7
PARENTS = (0, 0, 1, 2, 3, 4, 5)
ODOMETRY_PAIRS = tuple((k, k + 1) for k in range(6))             # with every finished submap as candidate
ODOMETRY_PAIRS_NO_ARGUMENT = ODOMETRY_PAIRS[:5]                  # the overload without candidates skips the active submap
LOOP_CANDIDATES = {5: [0], 6: [0, 1]}
LOOP_PAIRS = ((5, 0), (6, 0), (6, 1))
LOOP_RPY, LOOP_T = (0.01, -0.02, 0.05), (0.2, -0.15, 0.05)        # the initial transform of the loop pairs
OVERLAP_VOXELS = (10.0, 1.0)                                     # everything selected / proper subsets
OVERLAP_01_AT_1M = (1552, 1855, 1552, 1867)                      # selected source / target of source / target rows
LOOP_OVERLAP_AT_1M = {(5, 0): (1818, 1502), (6, 0): (1574, 1493), (6, 1): (1581, 1788)}
FEATURE_VOXEL = 1.0
ICP_DISTANCE = 0.75                                              # 1.5 x the map voxel size


def loop_transform():
    from open3d_slam_private_amd import synth
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_R(*LOOP_RPY)
    T[:3, 3] = LOOP_T
    return T


def scan_at(k, n, seed=11, reach=REACH):
    return S.scan_at(k, n, seed, reach)


@functools.lru_cache(maxsize=None)
def walk():
    """[(raw, (xyz, normals, None), T, stamp_ns)] of the wide walk."""
    out = []
    for k, (x, n) in enumerate(zip(WALK_X, WALK_N)):
        xs, ns = scan_at(k, n)
        raw = scan_at(k, RAW_N, seed=61)[0]
        out.append((raw, (xs, ns, None), pose_at(x), 1_000_000_000 + 100_000_000 * k))
    return out


class HostMap(MR.MapCloud):
    def __init__(self):
        super().__init__(**MAP)

    def n_rows(self):
        return len(self.xyz)

    def points(self):
        return self.xyz


@functools.lru_cache(maxsize=None)
def host_walk():
    """The wide walk on the CPU restatement: the collection after the last scan."""
    col = R.SubmapCollection(PARAMS, HostMap)
    for _ in S.drive(col, steps=walk()):
        pass
    return col


def host_clouds():
    """[(xyz, normals)] of the restatement's submaps."""
    return [(np.asarray(s.map.xyz), np.asarray(s.map.nrm)) for s in host_walk().submaps_]
