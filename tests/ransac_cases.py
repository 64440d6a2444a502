"""Inputs shared by tests/test_ransac_host.py (which checks the precondition on them) and tests/test_gpu_ransac.py (which
runs them on the device), with the restatement's results computed once per process and left unchanged."""
import functools

import numpy as np

from tests import fpfh_cases
from tests import ransac_restatement as R

MARGIN = 1e-9            # every comparison of every iteration stays this far (relative) from its border
SIGMA_RATIO = 1e-6       # sigma_2 / sigma_1 of every survivor
MAXD, DIST, EDGE = 0.75, 0.75, 0.5
TILE, CHUNK = 256, R.CHUNK       # kRsTile, kRsChunk of csrc/kernels_ransac.hpp


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def make(K, frac, seed):
    """600 source points uniform in a 20 m box; the target is the source under yaw 0.4 rad and t = (1.5, -2.0, 0.3) with
    0.02 m noise, permuted into 650 target points (50 of them clutter); K correspondences, a fraction `frac` of them true,
    the rest with a random target index.  Returns (src (600, 3), tgt (650, 3), corres (K, 2) int32)."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-10.0, 10.0, size=(600, 3))
    c, s = np.cos(0.4), np.sin(0.4)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    moved = src @ Rz.T + np.array([1.5, -2.0, 0.3]) + rng.normal(scale=0.02, size=src.shape)
    tgt_all = np.concatenate([moved, rng.uniform(-10.0, 10.0, size=(50, 3))])
    perm = rng.permutation(650)
    tgt = tgt_all[perm]
    where = np.empty(650, np.int64)
    where[perm] = np.arange(650)
    a = rng.integers(0, 600, size=K)
    b = where[a]
    false = rng.random(K) >= frac
    b[false] = rng.integers(0, 650, size=int(false.sum()))
    return _frozen(src, tgt, np.stack([a, b], axis=1).astype(np.int32))


# name -> (K, frac, generator seed, keyword arguments of R.ransac / the device call)
def _case(K, frac, gseed, max_iteration, confidence, n=3, dist=DIST, edge=EDGE, seed=1):
    return (K, frac, gseed, dict(n=n, max_iteration=max_iteration, confidence=confidence, dist_thr=dist, edge_sim=edge,
                                 seed=seed))


CASES = {
    "k500-full": _case(500, 0.3, 21, 8192, 1.0),
    "k500-early": _case(500, 0.3, 21, 65536, 0.999),
    "k300-early": _case(300, 0.6, 22, 65536, 0.999),
    "k64": _case(64, 0.5, 23, 2048, 1.0),
    "k3": _case(3, 1.0, 24, 256, 0.999),      # count == K: est_k = 0 ends the loop after the first valid sample
    "k2": _case(2, 1.0, 24, 256, 1.0),
    "nothing": _case(300, 0.0, 25, 2048, 0.999, dist=0.01),
    "n4": _case(300, 0.6, 22, 4096, 0.999, n=4),
    "n6": _case(300, 0.6, 22, 4096, 0.999, n=6),
    "n8": _case(300, 0.6, 22, 4096, 0.999, n=8),
    "edge-only": _case(300, 0.6, 22, 1024, 1.0, dist=0.0),
    "dist-only": _case(300, 0.6, 22, 1024, 1.0, edge=0.0),
    "no-checker": _case(300, 0.6, 22, 1024, 1.0, dist=0.0, edge=0.0),
    "seed-0": _case(300, 0.6, 22, 1024, 0.999, seed=0),
    "seed-max": _case(300, 0.6, 22, 1024, 0.999, seed=2 ** 64 - 1),
}
for _k in (TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1):
    CASES[f"k{_k}"] = _case(_k, 0.4, 30 + _k % 7, 1024, 1.0)
EARLY = ("k500-early", "k300-early")


def inputs(name):
    K, frac, gseed, kw = CASES[name]
    return make(K, frac, gseed) + (kw,)


@functools.lru_cache(maxsize=None)
def expected(name):
    src, tgt, corres, kw = inputs(name)
    out = R.ransac(src, tgt, corres, MAXD, **kw)
    _frozen(out["T"], out["inliers"], out["iter_status"])
    return out


# ---- end to end on the scene: FPFH rows of fpfh_cases.scene() at (100, 2.5), the reading moved by a fixed rigid G -----------
def scene_G():
    a = np.deg2rad(40.0)
    G = np.eye(4)
    G[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    G[:3, 3] = [3.0 * np.cos(0.3), 3.0 * np.sin(0.3), 0.0]          # 3 m
    return G


def scene_features():
    """(reading FPFH rows, target FPFH rows) of the restatement: the same rows the device produces (test_gpu_fpfh)."""
    return fpfh_cases.expected("reading", 100, 2.5)["fpfh"], fpfh_cases.expected("target", 100, 2.5)["fpfh"]


@functools.lru_cache(maxsize=None)
def scene_clouds():
    """(reading moved by G, target) in fp64."""
    tgt, _, src, _ = fpfh_cases.scene()
    G = scene_G()
    moved = src.astype(np.float64) @ G[:3, :3].T + G[:3, 3]
    return _frozen(moved, tgt.astype(np.float64))


SCENE_KW = dict(n=3, max_iteration=16384, confidence=1.0, dist_thr=DIST, edge_sim=EDGE, seed=0)


@functools.lru_cache(maxsize=None)
def _scene_expected(corres_bytes, K):
    src, tgt = scene_clouds()
    corres = np.frombuffer(corres_bytes, np.int32).reshape(K, 2)
    out = R.ransac(src, tgt, corres, MAXD, **SCENE_KW)
    _frozen(out["T"], out["inliers"], out["iter_status"])
    return out


@functools.lru_cache(maxsize=None)
def scene_corres():
    """The correspondence set of the scene's features, mutual filter on: (K, 2) int32."""
    from tests import fpfh_restatement
    fa, fb = scene_features()
    c = np.ascontiguousarray(fpfh_restatement.correspondences(fa, fb), np.int32)
    c.setflags(write=False)
    return c


def scene_expected():
    c = scene_corres()
    return _scene_expected(c.tobytes(), c.shape[0])
