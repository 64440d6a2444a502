"""numpy / dict restatement of o3d_slam::computeIndicesOfOverlappingPoints (helpers.cpp:320-345) and of the point
transform in front of it (helpers.cpp:302-303), written from their described behaviour:

  transformed source, T with rows r0..r3:  w = ((T30 x + T31 y) + T32 z) + T33,  x' = (((T00 x + T01 y) + T02 z) + T03) / w
  voxel key per axis:                      floor(p * (1.0 / voxel_size))                    (VoxelHashMap.hpp:43-51)
  selected voxel:                          >= k points of the target and >= k points of the transformed source
  result:                                  every point of either cloud in a selected voxel, ascending index

All in fp64, one rounding per operation (numpy's element-wise ufuncs do not contract).  Shared by test_overlap_host.py
(CPU) and test_gpu_overlap.py (device parity)."""
import numpy as np

KEY_LIMIT = 1 << 20   # 21 bits per axis, offset binary


def rpy_transform(roll_deg, pitch_deg, yaw_deg, t):
    r, p, y = np.deg2rad([roll_deg, pitch_deg, yaw_deg])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def transform_points(xyz, T):
    """T * (x, y, z, 1), divided by w; None: the points themselves."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    if T is None:
        return xyz
    T = np.asarray(T, np.float64).reshape(4, 4)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]

    def row(r):
        return ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]

    w = row(3)
    return np.stack([row(0) / w, row(1) / w, row(2) / w], axis=1)


def voxel_indices(xyz, voxel_size):
    """N x 3 int64 voxel indices; ValueError for what the device refuses (non-finite, outside +-2^20)."""
    inv = 1.0 / voxel_size
    v = np.floor(np.asarray(xyz, np.float64).reshape(-1, 3) * inv)
    if not np.all(np.abs(v) < KEY_LIMIT):   # NaN compares false
        raise ValueError("non-finite coordinate or voxel index outside +-2^20")
    return v.astype(np.int64)


def integer_margin(xyz, voxel_size):
    """Smallest distance of any coordinate * (1 / voxel_size) to an integer (inf for an empty cloud)."""
    a = np.asarray(xyz, np.float64).reshape(-1, 3) * (1.0 / voxel_size)
    return float(np.min(np.abs(a - np.rint(a)))) if a.size else float("inf")


def face_lattice(voxel):
    """Points exactly on voxel faces, negative coordinates included: multiples of `voxel` in [-2, 2)^3 for the target, the
    same lattice shifted by one voxel along x for the source."""
    g = np.arange(-2.0, 2.0, voxel)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    src = tgt + np.array([voxel, 0.0, 0.0])
    return src, tgt


def _packed(v):
    o = v + KEY_LIMIT
    return (o[:, 2] << 42) | (o[:, 1] << 21) | o[:, 0]


def overlap_indices(src_xyz, tgt_xyz, T, voxel_size, min_points=1):
    """(src_idx, tgt_idx), int32, ascending."""
    if not (voxel_size > 0 and np.isfinite(voxel_size)) or min_points < 1:
        raise ValueError("voxel_size > 0, min_points >= 1")
    src = np.asarray(src_xyz, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt_xyz, np.float64).reshape(-1, 3)
    if src.shape[0] == 0 or tgt.shape[0] == 0:
        return np.empty(0, np.int32), np.empty(0, np.int32)
    ks = _packed(voxel_indices(transform_points(src, T), voxel_size))
    kt = _packed(voxel_indices(tgt, voxel_size))
    us, cs = np.unique(ks, return_counts=True)
    ut, ct = np.unique(kt, return_counts=True)
    both = np.intersect1d(us[cs >= min_points], ut[ct >= min_points], assume_unique=True)
    return (np.nonzero(np.isin(ks, both))[0].astype(np.int32), np.nonzero(np.isin(kt, both))[0].astype(np.int32))
