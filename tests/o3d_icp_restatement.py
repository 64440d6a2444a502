"""fp64 numpy restatement of Open3D 0.15.1's RegistrationICP with TransformationEstimationPointToPlane (L2 loss) and
TransformationEstimationPointToPoint(with_scaling = false) -- the operators behind o3d_slam's RegistrationIcpPointToPlane /
RegistrationIcpPointToPoint (open3d_slam/src/CloudRegistration.cpp:54-101).  Open3D is not part of the reference tree:
restated from its published loop and estimations, PARITY UNPINNED.  Test helper, not product code.

Loop (RegistrationICP): evaluate the correspondences at T, then per iteration update = estimation(pcd, target, corres),
T = update * T, evaluate again; stop when |fitness - previous| < relative_fitness and |inlier_rmse - previous| <
relative_rmse, else after max_iteration updates.  The exact correspondences come from the oracle's kd-tree at the fp32
pose (d^2 <= max_dist^2), the per-pair algebra is fp64."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import oracle as orc

P2PL, P2P = 2, 3   # capi.COST_O3D_P2PL / COST_O3D_P2P


def zyx_to_T(x):
    """TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x3..5."""
    a, b, g = x[0], x[1], x[2]
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(g), -math.sin(g), 0], [math.sin(g), math.cos(g), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:6]
    return T


def umeyama(p, q):
    """Eigen::umeyama(p, q, false) with numpy's SVD: the rigid T minimising sum |T p - q|^2."""
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    S = (q - mq).T @ (p - mp) / p.shape[0]
    U, _, Vt = np.linalg.svd(S)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    R = U @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T


def p2pl_system(p, q, n):
    """J^T J, J^T r, sum r^2 of r = (p - q).n, J = [p x n, n] (p: transformed reading points)."""
    r = np.einsum("ij,ij->i", p - q, n)
    J = np.concatenate([np.cross(p, n), n], axis=1)
    return J.T @ J, J.T @ r, float(r @ r)


def record(cost, p, q, n=None, d2=None, origin=None):
    """The 32-double record the linearize kernel reduces (slot layout: csrc/reg_state.hpp)."""
    s = np.zeros(32)
    k = p.shape[0]
    if cost == P2PL:
        H, b, e = p2pl_system(p, q, n)
        s[:21] = H[np.triu_indices(6)]
        s[21:27] = b
        s[27] = e
    else:
        o = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
        pp, qq = p - o, q - o
        s[0:3] = pp.sum(axis=0)
        s[3:6] = qq.sum(axis=0)
        s[6:15] = (qq.T @ pp).reshape(9)
        s[15:18] = o * k
        s[27] = float(((p - q) ** 2).sum())
    s[28] = s[29] = k
    s[30] = float(np.sum(d2)) if d2 is not None else 0.0
    return s


@dataclass
class Result:
    iterations: int
    converged: bool
    max_iter_reached: bool
    fitness: float
    inlier_rmse: float
    ids: np.ndarray
    error: float
    T_last_eval: np.ndarray   # the pose of the last evaluation (its ids / fitness / rmse)


def transform(src, T):
    """T p as the device forms it (xf_point: fp32 pose, one rounding per fp32 operation, in this order), then fp64."""
    Tf = np.asarray(T, np.float32)
    x, y, z = (np.ascontiguousarray(src[:, k], np.float32) for k in range(3))
    rows = []
    for r in range(3):
        s = Tf[r, 0] * x + Tf[r, 1] * y
        s = s + Tf[r, 2] * z
        rows.append(s + Tf[r, 3])
    return np.stack(rows, axis=1).astype(np.float64)


def registration_icp(cost, tgt_xyz, tgt_nrm, src_xyz, T_init, max_dist, max_iter, rel_fitness=1e-6, rel_rmse=1e-6,
                     fixed_iters=0, tree=None, n_threads=1):
    """RegistrationICP(source, target, max_dist, T_init, estimation, ICPConvergenceCriteria(rel, rel, max_iter)).
    fixed_iters > 0: exactly that many updates, no convergence test (the C ABI's throughput mode)."""
    tree = tree if tree is not None else orc.KdTree(tgt_xyz)
    tgt = np.asarray(tgt_xyz, np.float64)
    nrm = None if tgt_nrm is None else np.asarray(tgt_nrm, np.float64)
    n = src_xyz.shape[0]
    T = np.asarray(T_init, np.float64).copy()
    rf, rr = float(np.float32(rel_fitness)), float(np.float32(rel_rmse))
    fit_prev = rmse_prev = 0.0
    updates, converged, maxed = 0, False, False
    limit = fixed_iters if fixed_iters > 0 else max_iter
    while True:
        Tf = T.astype(np.float32)
        ids, d2 = tree.knn(src_xyz, Tf, max_dist=max_dist, n_threads=n_threads)
        m = ids >= 0
        cnt = int(m.sum())
        if cnt == 0:
            raise RuntimeError("no correspondences")
        fit = cnt / float(np.float32(n))
        rmse = math.sqrt(float(d2[m].astype(np.float64).sum()) / cnt)
        p = transform(src_xyz[m], Tf)
        q = tgt[ids[m]]
        if cost == P2PL:
            H, b, err = p2pl_system(p, q, nrm[ids[m]])
        else:
            err = float(((p - q) ** 2).sum())
        if fixed_iters <= 0:
            if updates >= 1 and abs(fit - fit_prev) < rf and abs(rmse - rmse_prev) < rr:
                converged = True
                break
            if updates >= max_iter:
                maxed = True
                break
        fit_prev, rmse_prev = fit, rmse
        U = zyx_to_T(np.linalg.solve(H, -b)) if cost == P2PL else umeyama(p, q)
        T_eval = T
        T = U @ T
        updates += 1
        if fixed_iters > 0 and updates >= limit:
            return T, Result(updates, False, False, fit, rmse, ids, err, T_eval)
    return T, Result(updates, converged, maxed, fit, rmse, ids, err, T)
