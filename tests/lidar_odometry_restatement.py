"""Literal numpy restatements of the host arithmetic of DESIGN.md 5y, in the operation order include/o3dslam_reg.h writes
out: the covariance Open3D's GeneralizedICP derives from a normal, the pose update cumulative * T^-1 and the branch table of
LidarOdometry::addRangeScan.  Explicit loops over np.float64 scalars: every product and every sum is rounded once, nothing is
contracted or reordered (no `@`, no np.linalg.inv)."""
import numpy as np

F = np.float64

ACCEPTED, POSE_UPDATED, REPLACE_CLOUD, POSE_FROM_INITIAL, ACCUMULATE, RECORD_STAMP, PREPROCESS, REGISTER = (
    1, 2, 4, 8, 16, 32, 64, 128)


def _dot3(a0, b0, a1, b1, a2, b2):
    p = a0 * b0
    q = a1 * b1
    s = p + q
    p = a2 * b2
    return s + p


def covariance_from_normal(normal, epsilon):
    """cov = Rx diag(eps, 1, 1) Rx^T with Rx = GetRotationFromE1ToX(normal); 3 x 3 float64."""
    with np.errstate(all="ignore"):
        x = [F(v) for v in normal]
        eps, zero, one = F(epsilon), F(0.0), F(1.0)
        v = [zero * x[2] - zero * x[1], zero * x[0] - one * x[2], one * x[1] - zero * x[0]]
        c = _dot3(one, x[0], zero, x[1], zero, x[2])
        R = [[one if i == j else zero for j in range(3)] for i in range(3)]
        if not (c < F(-0.99)):
            S = [[zero, -v[2], v[1]], [v[2], zero, -v[0]], [-v[1], v[0], zero]]
            f = one / (one + c)
            for i in range(3):
                for j in range(3):
                    s2 = _dot3(S[i][0], S[0][j], S[i][1], S[1][j], S[i][2], S[2][j])
                    a = R[i][j] + S[i][j]
                    R[i][j] = a + s2 * f
        M = [[R[i][0] * eps, R[i][1] * one, R[i][2] * one] for i in range(3)]
        out = np.empty((3, 3), F)
        for i in range(3):
            for j in range(3):
                out[i, j] = _dot3(M[i][0], R[j][0], M[i][1], R[j][1], M[i][2], R[j][2])
    return out


def covariances_from_normals(normals, epsilon):
    normals = np.asarray(normals, F).reshape(-1, 3)
    return np.stack([covariance_from_normal(n, epsilon) for n in normals]).reshape(-1, 9) if len(normals) else np.empty((0, 9), F)


def _det2(a, b, c, d):
    p = a * b
    q = c * d
    return p - q


def _t3(x, p, y, q, z, r):
    s = x * p
    s = s - y * q
    return s + z * r


def inverse4(T):
    """The general cofactor inverse of a 4 x 4 matrix (math layout), in the header's order."""
    a = [[F(T[r][c]) for c in range(4)] for r in range(4)]
    s0 = _det2(a[0][0], a[1][1], a[1][0], a[0][1])
    s1 = _det2(a[0][0], a[1][2], a[1][0], a[0][2])
    s2 = _det2(a[0][0], a[1][3], a[1][0], a[0][3])
    s3 = _det2(a[0][1], a[1][2], a[1][1], a[0][2])
    s4 = _det2(a[0][1], a[1][3], a[1][1], a[0][3])
    s5 = _det2(a[0][2], a[1][3], a[1][2], a[0][3])
    c5 = _det2(a[2][2], a[3][3], a[3][2], a[2][3])
    c4 = _det2(a[2][1], a[3][3], a[3][1], a[2][3])
    c3 = _det2(a[2][1], a[3][2], a[3][1], a[2][2])
    c2 = _det2(a[2][0], a[3][3], a[3][0], a[2][3])
    c1 = _det2(a[2][0], a[3][2], a[3][0], a[2][2])
    c0 = _det2(a[2][0], a[3][1], a[3][0], a[2][1])
    det = s0 * c5
    det = det - s1 * c4
    det = det + s2 * c3
    det = det + s3 * c2
    det = det - s4 * c1
    det = det + s5 * c0
    d = F(1.0) / det
    B = np.empty((4, 4), F)
    B[0, 0] = _t3(a[1][1], c5, a[1][2], c4, a[1][3], c3) * d
    B[0, 1] = -_t3(a[0][1], c5, a[0][2], c4, a[0][3], c3) * d
    B[0, 2] = _t3(a[3][1], s5, a[3][2], s4, a[3][3], s3) * d
    B[0, 3] = -_t3(a[2][1], s5, a[2][2], s4, a[2][3], s3) * d
    B[1, 0] = -_t3(a[1][0], c5, a[1][2], c2, a[1][3], c1) * d
    B[1, 1] = _t3(a[0][0], c5, a[0][2], c2, a[0][3], c1) * d
    B[1, 2] = -_t3(a[3][0], s5, a[3][2], s2, a[3][3], s1) * d
    B[1, 3] = _t3(a[2][0], s5, a[2][2], s2, a[2][3], s1) * d
    B[2, 0] = _t3(a[1][0], c4, a[1][1], c2, a[1][3], c0) * d
    B[2, 1] = -_t3(a[0][0], c4, a[0][1], c2, a[0][3], c0) * d
    B[2, 2] = _t3(a[3][0], s4, a[3][1], s2, a[3][3], s0) * d
    B[2, 3] = -_t3(a[2][0], s4, a[2][1], s2, a[2][3], s0) * d
    B[3, 0] = -_t3(a[1][0], c3, a[1][1], c1, a[1][2], c0) * d
    B[3, 1] = _t3(a[0][0], c3, a[0][1], c1, a[0][2], c0) * d
    B[3, 2] = -_t3(a[3][0], s3, a[3][1], s1, a[3][2], s0) * d
    B[3, 3] = _t3(a[2][0], s3, a[2][1], s1, a[2][2], s0) * d
    return B


def accumulate(cumulative, T):
    """cumulative * inverse(float32(T)), 4 x 4 float64 (math layout)."""
    with np.errstate(all="ignore"):
        B = inverse4(np.asarray(T, np.float32).astype(F))
        cum = np.asarray(cumulative, F)
        out = np.empty((4, 4), F)
        for i in range(4):
            for j in range(4):
                r = cum[i, 0] * B[0, j]
                r = r + cum[i, 1] * B[1, j]
                r = r + cum[i, 2] * B[2, j]
                r = r + cum[i, 3] * B[3, j]
                out[i, j] = r
    return out


def decide(has_previous, timestamp, last_stamp, use_odometry_topic, n_rows, fitness, min_fitness, initial_pending):
    """LidarOdometry::addRangeScan (Odometry.cpp:29-84) as the set of things that happen."""
    if not has_previous:
        return PREPROCESS | REPLACE_CLOUD | RECORD_STAMP | ACCEPTED | POSE_UPDATED
    if timestamp < last_stamp:
        return 0
    if use_odometry_topic:
        return ACCEPTED
    if not (fitness > min_fitness):
        return PREPROCESS | REGISTER | (REPLACE_CLOUD if n_rows > 0 else 0)
    return (PREPROCESS | REGISTER | ACCEPTED | POSE_UPDATED | REPLACE_CLOUD | RECORD_STAMP |
            (POSE_FROM_INITIAL if initial_pending else ACCUMULATE))
