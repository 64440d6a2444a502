"""A literal numpy restatement of the motion compensation's contract (include/o3dslam_reg.h): the per-point
undistortion of a raw scan.  Written from the header, one rounding per operation (numpy's elementwise operators on float64
arrays are IEEE doubles without contraction); every sum of three products is (a0 b0 + a1 b1) + a2 b2.  atan2, sin and cos
are numpy's, so the comparison with the library is within a derived bar, not bit for bit."""
import numpy as np

TWO_PI = np.float64(2.0) * np.float64(np.pi)


def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def phase(x, y, clockwise):
    """computePhase (MotionCompensation.cpp:120-139)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    a = np.arctan2(y, x)
    aw = np.where(a < 0.0, a + TWO_PI, a)
    f = aw / TWO_PI
    return np.where(aw == 0.0, np.float64(0.0), (np.float64(1.0) - f) if clockwise else f)


def quat_mul(a, b):
    """Hamilton product of (w, x, y, z) columns, every component summed left to right in Eigen's term order."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (((aw * bw - ax * bx) - ay * by) - az * bz,
            ((aw * bx + ax * bw) + ay * bz) - az * by,
            ((aw * by + ay * bw) + az * bx) - ax * bz,
            ((aw * bz + az * bw) + ax * by) - ay * bx)


def undistort(xyz, clockwise, scan_duration, linear_velocity, angular_velocity_rpy):
    """reg_undistort_scan on n x 3 rows."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    lin, rpy = np.asarray(linear_velocity, np.float64), np.asarray(angular_velocity_rpy, np.float64)
    with np.errstate(invalid="ignore"):
        s = phase(p[:, 0], p[:, 1], clockwise) * np.float64(scan_duration)
        t = [s * lin[k] for k in range(3)]
        e = [s * rpy[k] for k in range(3)]
        hr, hp, hy = e[0] * 0.5, e[1] * 0.5, e[2] * 0.5
        zero = np.zeros_like(s)
        qx = (np.cos(hr), np.sin(hr), zero, zero)
        qy = (np.cos(hp), zero, np.sin(hp), zero)
        qz = (np.cos(hy), zero, zero, np.sin(hy))
        q = quat_mul(quat_mul(qz, qy), qx)
        nn = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        w, x, y, z = (c / nn for c in q)
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        R = [[1.0 - (tyy + tzz), txy - twz, txz + twy],
             [txy + twz, 1.0 - (txx + tzz), tyz - twx],
             [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]
        out = np.stack([dot3(R[r][0], p[:, 0], R[r][1], p[:, 1], R[r][2], p[:, 2]) + t[r] for r in range(3)], axis=1)
    still = np.ones(len(p), bool)            # the identity motion copies the point
    for v in t + e:
        still &= v == 0.0
    out[still] = p[still]
    return out
