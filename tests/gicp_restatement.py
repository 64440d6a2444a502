"""fp64 numpy restatement of the GICP factor (include/o3dslam_reg.h), written from the formula and not from the
kernel.  Test helper, not product code.

A pair (p, q) with covariances (Cp, Cq) at the pose T = [R | t]:

    r = q - T p                      T p evaluated in fp32 (NC4: ((T0 x + T1 y) + T2 z) + T3), everything else in fp64
    M = (Cq + R Cp R^T)^-1           R: the fp32 rotation entries of T, widened
    J = d r / d xi = [R skew(p), -R] for the right perturbation T <- T Exp(xi), xi = (omega, v), rotation first
    H = sum J^T M J,  b = sum J^T M r,  e = 1/2 sum r^T M r

Covariances arrive as 6 floats (xx, xy, xz, yy, yz, zz).  `ids[i]` is the matched reference point of reading point i, < 0
for none."""
import numpy as np


def sym3(c6):
    """n x 6 (xx xy xz yy yz zz) -> n x 3 x 3, fp64."""
    c = np.asarray(c6, np.float64)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)


def skew(p):
    """n x 3 -> n x 3 x 3 with skew(p) x = p cross x."""
    z = np.zeros(p.shape[0])
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], axis=1), np.stack([p[:, 2], z, -p[:, 0]], axis=1),
                     np.stack([-p[:, 1], p[:, 0], z], axis=1)], axis=1)


def transform_fp32(src, T):
    """T p with one rounding per fp32 operation in the contract's order, widened to fp64."""
    Tf = np.asarray(T, np.float32)
    x, y, z = (np.ascontiguousarray(src[:, k], np.float32) for k in range(3))
    rows = []
    for r in range(3):
        s = Tf[r, 0] * x + Tf[r, 1] * y
        s = s + Tf[r, 2] * z
        rows.append(s + Tf[r, 3])
    return np.stack(rows, axis=1).astype(np.float64)


def transform_exact(src, T):
    """T p in fp64 from the pose as given (no fp32 rounding of the pose or of the products)."""
    T = np.asarray(T, np.float64)
    return np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]


def information(src_cov6, tgt_cov6, T, ids):
    """M of every matched pair (k x 3 x 3) at the pose T."""
    m = ids >= 0
    R = np.asarray(T, np.float32)[:3, :3].astype(np.float64)
    return np.linalg.inv(sym3(tgt_cov6[ids[m]]) + R @ sym3(src_cov6[m]) @ R.T)


def residuals(src, tgt, T, ids, transform=transform_fp32):
    m = ids >= 0
    return np.asarray(tgt, np.float64)[ids[m]] - transform(src[m], T)


def normal_eq(src, src_cov6, tgt, tgt_cov6, T, ids, transform=transform_fp32):
    """H (6 x 6), b (6), e, count of the matched pairs at T."""
    m = ids >= 0
    R = np.asarray(T, np.float32)[:3, :3].astype(np.float64)
    M = information(src_cov6, tgt_cov6, T, ids)
    r = residuals(src, tgt, T, ids, transform)
    J = np.concatenate([R @ skew(np.asarray(src, np.float64)[m]), np.broadcast_to(-R, (int(m.sum()), 3, 3))], axis=2)
    MJ = M @ J
    H = np.einsum("nki,nkj->ij", J, MJ)
    b = np.einsum("nki,nk->i", MJ, r)
    e = 0.5 * float(np.einsum("ni,nij,nj->", r, M, r))
    return H, b, e, int(m.sum())


def cost(src, tgt, T, ids, M):
    """1/2 sum r^T M r with M frozen (as `information` gave it at the linearisation point) and T p in exact fp64: a smooth
    function of T whose gradient along T Exp(xi) at xi = 0 is b."""
    r = residuals(src, tgt, T, ids, transform_exact)
    return 0.5 * float(np.einsum("ni,nij,nj->", r, M, r))


def se3_exp(xi):
    """Exp of xi = (omega, v), rotation first: Rodrigues and the left Jacobian, fp64."""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        A, B, Cc = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
        Cc = (1.0 - A) / (th * th)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3) + B * K + Cc * (K @ K)) @ v
    return T
