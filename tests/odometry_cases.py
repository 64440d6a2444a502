"""Inputs shared by tests/test_odometry_host.py (CPU) and tests/test_gpu_odometry.py (device): the special points and the
velocities of the undistortion tests, and their bar.  Every builder is deterministic and cached."""
import functools

import numpy as np

from tests import odometry_restatement as R

SIZES = (1, 63, 64, 65, 257, 4099)     # one point, the tails of a wave and of a workgroup, more than one workgroup

# ---- reg_undistort_scan ------------------------------------------------------------------------------------------------------------
SCAN_DURATION = 0.1
LINEAR = (0.7, -0.5, 0.6)              # >= 0.5 m/s per axis
ANGULAR = (0.4, -0.3, 0.5)             # >= 0.3 rad/s per axis; |omega| * scan_duration < 1 rad, the bar's domain
SPECIAL_POINTS = np.array([
    [3.0, 0.0, 1.0], [0.0, 2.0, -1.0], [-4.0, 0.0, 0.5], [0.0, -5.0, 2.0],              # the four axes
    [1.5, 2.5, 0.1], [-1.5, 2.5, 0.2], [-1.5, -2.5, 0.3], [1.5, -2.5, 0.4],             # the four quadrants
    [0.0, 0.0, 3.0],                                                                    # on the spin axis
    [2.0, 0.0, 0.7], [2.0, -0.0, 0.7],                                                  # y = +-0, x > 0: phase 0
    [2.0, -1e-300, 0.7]], np.float64)                                                   # y a tiny negative number: wraps to 2 pi
PHASE_ZERO_ROWS = (0, 9, 10)
TINY_Y_ROW = 11


@functools.lru_cache(maxsize=None)
def points(n, seed=12):
    out = np.random.default_rng(seed).uniform(-20.0, 20.0, size=(n, 3))
    k = min(n, len(SPECIAL_POINTS))
    out[:k] = SPECIAL_POINTS[:k]
    out.setflags(write=False)
    return out


def bar(xyz, clockwise, scan_duration=SCAN_DURATION, linear=LINEAR):
    """|delta|_inf <= 2^-42 (|x| + |y| + |z| + |t|_1) per point, t = phase * scan_duration * v that point's translation (the
    restatement's phase).  Derived in DESIGN.md 5x from library functions within 2 ulp: 8u on the angle, 8u on each sine and
    cosine, 56u per quaternion component, 250u per entry of R, below 260u |p|_1 on R p + t; 2048u = 2^-42 leaves a factor of
    about 8."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    t1 = np.abs(R.phase(p[:, 0], p[:, 1], clockwise) * np.float64(scan_duration)) * np.abs(np.asarray(linear, np.float64)).sum()
    return 2.0 ** -42 * (np.abs(p).sum(axis=1) + t1)
