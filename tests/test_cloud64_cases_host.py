"""The inputs of tests/test_gpu_cloud64_shared.py (tests/cloud64_cases.py) reach the boundaries they claim: numpy only."""
import numpy as np

from tests import cloud64_cases as K


def _counts(keys):
    _, c = np.unique(keys, axis=0, return_counts=True)
    return c


def test_the_lone_cloud_crosses_a_block_and_sits_on_voxel_boundaries():
    xyz, nrm = K.lone_cloud()
    assert xyz.shape == nrm.shape == (K.N_LONE, 3) and K.N_LONE > 256
    scaled = xyz * (1.0 / K.VOXEL)
    on_boundary = scaled == np.floor(scaled)                    # exactly k * voxel
    assert on_boundary[:K.N_EXACT].all() and int(on_boundary.sum()) >= 10
    assert int((on_boundary & (xyz < 0.0)).sum()) >= 10          # negative boundaries: floor, not truncation
    minus_zero = (xyz == 0.0) & np.signbit(xyz)
    assert int(minus_zero.sum()) >= 3 and int(((xyz == 0.0) & ~np.signbit(xyz)).sum()) >= 3
    assert np.array_equal(K.keys_of(xyz)[minus_zero], np.zeros(int(minus_zero.sum()), np.int64))   # floor(-0.0 * 4) is index 0
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, rtol=0, atol=1e-15)


def test_every_row_of_the_lone_cloud_has_its_own_voxel_under_every_transform():
    xyz, _ = K.lone_cloud()
    assert len(np.unique(K.keys_of(xyz), axis=0)) == K.N_LONE
    diagonal = K.VOXEL * np.sqrt(3.0)
    for T in (np.eye(4),) + tuple(K.transforms()):
        p = K.apply(T, xyz)
        d = np.linalg.norm(p[:, None, :] - p[None, :, :], axis=2) + np.eye(len(p)) * 1e9
        assert d.min() > 1.2 * diagonal                          # two rows cannot share a voxel, whatever the rounding
        assert len(np.unique(K.keys_of(p), axis=0)) == K.N_LONE
        assert np.abs(K.keys_of(p)).max() < 1 << 20


def test_the_transforms_are_what_they_claim():
    T, T2 = K.transforms()
    R = T[:3, :3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)
    assert np.abs(R - np.eye(3)).min() > 0.01                    # no entry of the identity survives: every product counts
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) and np.array_equal(T2[3], [0.0, 0.0, 0.0, 2.0])
    assert np.array_equal(T[:3], T2[:3])


def test_the_pair_fills_every_count_class_and_keeps_clear_of_the_voxel_faces():
    X, Y = K.pair()
    T = K.transforms()[0]
    assert X.shape == (K.N_X, 3) and Y.shape == (K.N_Y, 3)
    for p in (K.apply(T, X), Y):
        frac = p * (1.0 / K.VOXEL) - np.floor(p * (1.0 / K.VOXEL))
        assert frac.min() > 0.25 and frac.max() < 0.75           # >= 0.0625 from every face: no rounding decides a key
        c = _counts(K.keys_of(p))
        assert (c == 1).sum() >= 20 and (c == 2).sum() >= 20 and (c >= 3).sum() >= 20
    kx, ky = K.keys_of(K.apply(T, X)), K.keys_of(Y)
    both = {tuple(k) for k in kx} & {tuple(k) for k in ky}
    assert len(both) >= 100 and len({tuple(k) for k in kx}) > len(both) and len({tuple(k) for k in ky}) > len(both)
    cx = {tuple(k): c for k, c in zip(*np.unique(kx, axis=0, return_counts=True))}
    cy = {tuple(k): c for k, c in zip(*np.unique(ky, axis=0, return_counts=True))}
    combos = {(min(cx[k], 3), min(cy[k], 3)) for k in both}
    assert combos == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}   # min_points 1, 2, 3 each split the shared voxels
