"""Inputs shared by tests/test_cloud64_cases_host.py (CPU: the inputs reach the boundaries they claim) and
tests/test_gpu_cloud64_shared.py (device: the operators on the fp64 clouds agree on the voxel key and on the transform).
Every builder is deterministic, cached and returns read-only arrays."""
import functools

import numpy as np

VOXEL = 0.25          # exact reciprocal
N_LONE, N_X, N_Y = 300, 300, 260
N_EXACT = 40          # rows of lone_cloud() that sit exactly on voxel boundaries in every coordinate
SPACING = 1.5         # lattice of lone_cloud(): six voxels, so that no two rows share a voxel under either transform
JITTER = 0.2


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


@functools.lru_cache(maxsize=None)
def transforms():
    """(T_rigid, T_w2): a rigid transform with a rotation about all three axes, and the same with T[3][3] = 2 (w != 1)."""
    T = np.eye(4)
    T[:3, :3] = _rot(0.3, -0.2, 0.7)
    T[:3, 3] = (0.37, -1.21, 0.58)
    T2 = T.copy()
    T2[3, 3] = 2.0
    return _ro(T, T2)


def apply(T, xyz):
    """T * (x, y, z, 1) divided by w, in numpy (its rounding is not the device's: for properties with a margin only)."""
    h = np.concatenate([xyz, np.ones((len(xyz), 1))], axis=1) @ T.T
    return h[:, :3] / h[:, 3:4]


def keys_of(xyz, voxel=VOXEL):
    """The map voxel key per row: floor(p * (1 / voxel)), int64 triples."""
    return np.floor(np.asarray(xyz, np.float64) * (1.0 / voxel)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def lone_cloud():
    """(xyz, normals): 300 rows (more than one 256-thread block), every row in a voxel of its own -- also after either
    transform (the second halves all distances), since any two rows stay further apart than a voxel diagonal.  The first N_EXACT rows lie exactly on
    k * voxel in every coordinate, negative k included, and carry -0.0 where an even row has a zero coordinate."""
    rng = np.random.default_rng(64)
    g = np.arange(-3, 4)
    nodes = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    exact = rng.permutation(np.nonzero((nodes == 0).any(axis=1))[0])[:N_EXACT]      # nodes with a zero coordinate
    rest = rng.permutation(np.setdiff1d(np.arange(len(nodes)), exact))
    order = np.concatenate([exact, rest])[:N_LONE]
    xyz = nodes[order].astype(np.float64) * SPACING
    xyz[N_EXACT:] += rng.uniform(-JITTER, JITTER, size=(N_LONE - N_EXACT, 3))
    even = np.arange(N_EXACT) % 2 == 0
    head = xyz[:N_EXACT]
    head[even[:, None] & (head == 0.0)] = -0.0
    nrm = rng.normal(size=(N_LONE, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return _ro(np.ascontiguousarray(xyz), np.ascontiguousarray(nrm))


@functools.lru_cache(maxsize=None)
def pair():
    """(X, Y): 300 and 260 rows.  T_rigid * X and Y fall into voxels of a shared set, near the voxel centres (at least
    0.075 from every face, so that no rounding decides a key).  Shared voxel j holds 1 + j % 3 rows of X and
    1 + (j // 3) % 3 rows of Y: every combination of 1, 2 and 3.  Further voxels hold rows of one cloud only (4 or 3 of X,
    2 of Y).  The rows are shuffled."""
    rng = np.random.default_rng(65)
    T = transforms()[0]
    g = np.arange(-4, 4)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = cells[rng.permutation(len(cells))] * 2          # every second voxel per axis
    n_shared, only_x, only_y = 117, [4] * 12 + [3] * 6, [2] * 13
    cx = [1 + j % 3 for j in range(n_shared)] + only_x + [0] * len(only_y)
    cy = [1 + (j // 3) % 3 for j in range(n_shared)] + [0] * len(only_x) + only_y
    assert sum(cx) == N_X and sum(cy) == N_Y

    def rows(counts):
        c = np.repeat(cells[:len(counts)], counts, axis=0)
        p = (c + 0.5) * VOXEL + rng.uniform(-0.05, 0.05, size=(len(c), 3))
        return p[rng.permutation(len(p))]

    in_target_frame, Y = rows(cx), rows(cy)
    X = (in_target_frame - T[:3, 3]) @ T[:3, :3]             # T^-1 of a rigid T
    return _ro(np.ascontiguousarray(X), np.ascontiguousarray(Y))
