"""CPU restatement of the pose covariance (PointToPlaneWithCovErrorMinimizer), the ErrorMinimizer statistics,
BoundTransformationChecker and degeneracyAwareness SolutionRemapping on top of tests/pm_chain_restatement.py (a plain
helper module, not a test).

  covariance_terms   PointToPlaneWithCov.cpp:106-150 vectorised: the per-pair terms in fp32 in the reference's expression
                     order, H = sum v v^T and M = sum (a a^T + b b^T) as fp64 sums of fp32 products
  covariance_loop    the same lines transcribed a second time, independently: a plain per-pair loop in Python floats (fp64)
  censi              cov = sigma^2 H^-1 M H^-1 (numpy.linalg, fp64)
  solution_remap     ICP.cpp:1621-1666, 2446-2501 with numpy.linalg.eigh
  bound_values       TransformationCheckersImpl.cpp:198-225 in fp32
"""
import math

import numpy as np

from oracle import oracle as orc
from tests.oracle_side import _m4, _xf
from tests.pm_chain_restatement import NT, Chain, Checkers, PmRestatement, _qdist, _quat, x_to_T

f32 = np.float32
IU = np.triu_indices(6)


class ExtrasChain(Chain):
    """Chain plus: with_cov / sigma; bound = (maxRotationNorm, maxTranslationNorm) or None and bound_after_counter (the
    Counter checker is listed before the Bound checker); sr = (threshold, use2019) or None."""

    def __init__(self, with_cov=False, sigma=0.01, bound=None, bound_after_counter=False, sr=None, **kw):
        super().__init__(**kw)
        self.with_cov, self.sigma, self.bound, self.bound_after_counter, self.sr = with_cov, sigma, bound, bound_after_counter, sr


class OutOfBounds(Exception):
    """BoundTransformationChecker's ConvergenceError."""

    def __init__(self, rot, trans, iteration, T):
        super().__init__(f"limit out of bounds: rot: {rot} tr: {trans}")
        self.rot, self.trans, self.iteration, self.T = rot, trans, iteration, T


def update_angles(dT):
    """alpha, beta, gamma, t of the last update (PointToPlaneWithCov.cpp:94-99): the angles in fp64 from the fp32 matrix,
    rounded to fp32 (the contract of include/o3dslam_reg.h)."""
    d = np.asarray(dT, f32).astype(np.float64)
    beta = f32(-math.asin(d[2, 0]))
    alpha = f32(math.atan2(d[2, 1], d[2, 2]))
    cb = math.cos(float(beta))
    gamma = f32(math.atan2(float(f32(d[1, 0] / cb)), float(f32(d[0, 0] / cb))))
    return alpha, beta, gamma, f32(dT[0][3]), f32(dT[1][3]), f32(dT[2][3])


def centre_pairs(P, Q):
    """compute_in_place (PointToPlane.cpp:281-284): both clouds minus their own mean over the pairs; the mean is an fp64
    sum rounded to fp32."""
    P, Q = np.asarray(P, f32), np.asarray(Q, f32)
    mp = (P.astype(np.float64).sum(0) / P.shape[0]).astype(f32)
    mq = (Q.astype(np.float64).sum(0) / Q.shape[0]).astype(f32)
    return (P - mp).astype(f32), (Q - mq).astype(f32)


def covariance_terms(P, Q, N, dT):
    """The 6-vectors v, a, b of every pair (n x 6 each, fp32) from the centred points P, Q and the normals N."""
    P, Q, N = np.asarray(P, f32), np.asarray(Q, f32), np.asarray(N, f32)
    alpha, beta, gamma, tx, ty, tz = update_angles(dT)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]
        rr = np.sqrt(s + P[:, 2] * P[:, 2])
        rd = P / rr[:, None]
        s = Q[:, 0] * Q[:, 0] + Q[:, 1] * Q[:, 1]
        fr = np.sqrt(s + Q[:, 2] * Q[:, 2])
        fd = Q / fr[:, None]
        n_a = N[:, 2] * rd[:, 1] - N[:, 1] * rd[:, 2]
        n_b = N[:, 0] * rd[:, 2] - N[:, 2] * rd[:, 0]
        n_g = N[:, 1] * rd[:, 0] - N[:, 0] * rd[:, 1]
        E = N[:, 0] * ((((P[:, 0] - gamma * P[:, 1]) + beta * P[:, 2]) + tx) - Q[:, 0])
        E = E + N[:, 1] * ((((gamma * P[:, 0] + P[:, 1]) - alpha * P[:, 2]) + ty) - Q[:, 1])
        E = E + N[:, 2] * (((((-beta) * P[:, 0] + alpha * P[:, 1]) + P[:, 2]) + tz) - Q[:, 2])
        Nr = N[:, 0] * ((rd[:, 0] - gamma * rd[:, 1]) + beta * rd[:, 2])
        Nr = Nr + N[:, 1] * ((gamma * rd[:, 0] + rd[:, 1]) - alpha * rd[:, 2])
        Nr = Nr + N[:, 2] * (((-beta) * rd[:, 0] + alpha * rd[:, 1]) + rd[:, 2])
        Nf = -((N[:, 0] * fd[:, 0] + N[:, 1] * fd[:, 1]) + N[:, 2] * fd[:, 2])
        g = E + rr * Nr
        v = np.stack([N[:, 0], N[:, 1], N[:, 2], rr * n_a, rr * n_b, rr * n_g], 1)
        a = np.stack([N[:, 0] * Nr, N[:, 1] * Nr, N[:, 2] * Nr, n_a * g, n_b * g, n_g * g], 1)
        b = np.stack([N[:, 0] * Nf, N[:, 1] * Nf, N[:, 2] * Nf, (fr * n_a) * Nf, (fr * n_b) * Nf, (fr * n_g) * Nf], 1)
    assert v.dtype == f32 and a.dtype == f32 and b.dtype == f32
    return v, a, b


def covariance_sums(P, Q, N, dT):
    """(H, M) 6x6 fp64: sums over the pairs of the fp32 products v_i v_j and a_i a_j, b_i b_j."""
    v, a, b = covariance_terms(P, Q, N, dT)
    H, M = np.zeros((6, 6)), np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = (v[:, i] * v[:, j]).astype(np.float64).sum()
            M[i, j] = M[j, i] = (a[:, i] * a[:, j]).astype(np.float64).sum() + (b[:, i] * b[:, j]).astype(np.float64).sum()
    return H, M


def censi(H, M, sigma):
    Hi = np.linalg.inv(H)
    return float(sigma) ** 2 * (Hi @ M @ Hi)


def covariance_loop(P, Q, N, dT, sigma):
    """PointToPlaneWithCov.cpp:94-161 transcribed line by line as a per-pair loop in Python floats (fp64); P, Q already
    centred.  Independent of covariance_terms."""
    T = np.asarray(dT, np.float64)
    beta = -math.asin(T[2, 0])
    alpha = math.atan2(T[2, 1], T[2, 2])
    gamma = math.atan2(T[1, 0] / math.cos(beta), T[0, 0] / math.cos(beta))
    t_x, t_y, t_z = T[0, 3], T[1, 3], T[2, 3]
    J_hessian = np.zeros((6, 6))
    cols_reading, cols_reference = [], []
    for rp, fp, nrm in zip(np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(N, np.float64)):
        reading_range = math.sqrt(rp[0] ** 2 + rp[1] ** 2 + rp[2] ** 2)
        reading_direction = rp / reading_range
        reference_range = math.sqrt(fp[0] ** 2 + fp[1] ** 2 + fp[2] ** 2)
        reference_direction = fp / reference_range
        n_alpha = nrm[2] * reading_direction[1] - nrm[1] * reading_direction[2]
        n_beta = nrm[0] * reading_direction[2] - nrm[2] * reading_direction[0]
        n_gamma = nrm[1] * reading_direction[0] - nrm[0] * reading_direction[1]
        E = nrm[0] * (rp[0] - gamma * rp[1] + beta * rp[2] + t_x - fp[0])
        E += nrm[1] * (gamma * rp[0] + rp[1] - alpha * rp[2] + t_y - fp[1])
        E += nrm[2] * (-beta * rp[0] + alpha * rp[1] + rp[2] + t_z - fp[2])
        N_reading = nrm[0] * (reading_direction[0] - gamma * reading_direction[1] + beta * reading_direction[2])
        N_reading += nrm[1] * (gamma * reading_direction[0] + reading_direction[1] - alpha * reading_direction[2])
        N_reading += nrm[2] * (-beta * reading_direction[0] + alpha * reading_direction[1] + reading_direction[2])
        N_reference = -(nrm[0] * reference_direction[0] + nrm[1] * reference_direction[1] + nrm[2] * reference_direction[2])
        tmp = np.array([nrm[0], nrm[1], nrm[2], reading_range * n_alpha, reading_range * n_beta, reading_range * n_gamma])
        J_hessian += np.outer(tmp, tmp)
        cols_reading.append([nrm[0] * N_reading, nrm[1] * N_reading, nrm[2] * N_reading,
                             n_alpha * (E + reading_range * N_reading), n_beta * (E + reading_range * N_reading),
                             n_gamma * (E + reading_range * N_reading)])
        cols_reference.append([nrm[0] * N_reference, nrm[1] * N_reference, nrm[2] * N_reference,
                               reference_range * n_alpha * N_reference, reference_range * n_beta * N_reference,
                               reference_range * n_gamma * N_reference])
    d2J_dZdX = np.concatenate([np.array(cols_reading).T, np.array(cols_reference).T], axis=1)
    inv_J_hessian = np.linalg.inv(J_hessian)
    covariance = d2J_dZdX @ d2J_dZdX.T
    covariance = inv_J_hessian @ covariance @ inv_J_hessian
    return (sigma * sigma) * covariance


def solution_remap(A, threshold, use2019, P_in):
    """One step on the fp32 normal matrix A: (P_out, categories, eigenvalues fp32 descending, condition number,
    return_prior)."""
    A = np.asarray(A, f32)
    if not A.any():
        return np.array(P_in, np.float64), np.zeros(6, np.int32), np.zeros(6, f32), float("nan"), True
    S = 0.5 * (A.astype(np.float64) + A.astype(np.float64).T)
    lam, U = np.linalg.eigh(S)
    order = np.argsort(-np.abs(lam), kind="stable")
    eig = np.abs(lam[order]).astype(f32)
    U = U[:, order]
    with np.errstate(divide="ignore"):
        cond = f32(eig[0]) / f32(eig[5])
    thr = cond if use2019 else f32(threshold)
    cat = (~(eig < thr)).astype(np.int32)
    P = np.array(P_in, np.float64)
    if (cat == 0).any():
        K = U[:, cat == 1]
        P = K @ K.T
    return P, cat, eig, float(cond), not P.any()


def min_norm_solve(A, b):
    """x (fp32) and the rank of the fp32 system: eigenvalues at or below 6 eps_fp32 of the largest count as zero."""
    S = 0.5 * (np.asarray(A, f32).astype(np.float64) + np.asarray(A, f32).astype(np.float64).T)
    lam, U = np.linalg.eigh(S)
    keep = np.abs(lam) > np.abs(lam).max() * 6.0 * 1.1920929e-07
    x = U[:, keep] @ ((U[:, keep].T @ np.asarray(b, f32).astype(np.float64)) / lam[keep])
    return x.astype(f32), int(keep.sum())


def bound_values(T):
    """(rotation, translation) of BoundTransformationChecker against the identity, in fp32 as the device (rot_to_quat /
    quat_angular_distance of host_math.hpp restated by tests/pm_chain_restatement.py in fp64, rounded)."""
    T = np.asarray(T, f32)
    rot = f32(_qdist(_quat(T), np.array([1.0, 0, 0, 0])))
    t = T[:3, 3]
    tr = np.sqrt(f32(f32(t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))
    return rot, f32(tr)


class PmExtrasRestatement(PmRestatement):
    """PmRestatement with SolutionRemapping in the solve, the Bound checker after the update, and the covariance /
    statistics of the last iteration.  `trace` keeps (categories, eigenvalues) of every iteration."""

    def register(self, T_init=None):
        c = self.c
        chk = Checkers(c.max_iter, c.min_rot, c.min_trans, c.smooth)
        T = np.eye(4, dtype=f32)
        it = 0
        self.P = np.eye(6)
        self.trace, self.returned_prior, self.last_dT, self.bound_last = [], False, None, None
        while True:
            dT, ids, d2, w, H, rank = self.step(T)
            self.last = dict(ids=ids, d2=d2, w=w, H=H, rank=rank, T_prev=T.copy())
            if c.sr is not None:
                dT = self._remap(H, T)
                if dT is None:
                    self.returned_prior = True
                    break
            self.last_dT = np.asarray(dT, f32)
            T = _m4(self.last_dT, T)
            it += 1
            if c.fixed_iters > 0:
                if it >= c.fixed_iters:
                    break
                continue
            go = chk.check(T)
            if c.bound is not None and not (c.bound_after_counter and chk.max_iter_reached):
                rot, tr = self.bound_last = bound_values(T)
                if rot > f32(c.bound[0]) or tr > f32(c.bound[1]):
                    raise OutOfBounds(rot, tr, it, T)
            if not go:
                break
        self.max_iter_reached = chk.max_iter_reached
        A = np.eye(4, dtype=f32)
        A[:3, 3] = self.c_ref
        B = np.eye(4, dtype=f32)
        B[:3, 3] = -self.c_read
        T_out = _m4(_m4(_m4(A, T), self.T0), B)
        if self.returned_prior:
            T_out = np.eye(4, dtype=f32) if T_init is None else np.asarray(T_init, f32)
        return T_out, it, T

    def step(self, T):
        """As PmRestatement.step for point-to-plane, with the solve of the device: the fp32 system, minimum norm below the
        rank threshold 6 eps_fp32 of the largest eigenvalue (a degenerate scene makes numpy.linalg.solve fail)."""
        c = self.c
        if c.minimizer == "point2point":
            return super().step(T)
        P = _xf(T, self.rd)
        ids, d2 = orc.knn_k(self.tree, P, c.knn, max_dist=c.max_dist, n_threads=NT)
        w = self.weights(T, ids, d2)
        self.last = dict(ids=ids, d2=d2, w=w, T_prev=np.array(T, f32))
        A, b = self._system(T)
        x, rank = min_norm_solve(A, b)
        return np.asarray(x_to_T(x), f32), ids, d2, w, A.astype(np.float64), rank

    def _system(self, T):
        """(A, b) of the last iteration as the loop builds them: fp64 sums, rounded to fp32."""
        l = self.last
        ii, kk = np.nonzero(l["w"] != 0)
        Pm = _xf(T, self.rd)[ii].astype(np.float64)
        Qm = self.tgt_c[l["ids"][ii, kk]].astype(np.float64)
        N = self.tgt_nrm[l["ids"][ii, kk]].astype(np.float64)
        ww = l["w"][ii, kk].astype(np.float64)
        F = np.concatenate([np.cross(Pm, N), N], axis=1)
        r = ((Pm - Qm) * N).sum(1)
        return ((F * ww[:, None]).T @ F).astype(f32), (-(F * (ww * r)[:, None]).sum(0)).astype(f32)

    def _remap(self, H, T):
        A, b = self._system(T)
        self.P, cat, eig, cond, prior = solution_remap(A, self.c.sr[0], self.c.sr[1], self.P)
        self.trace.append((cat, eig, cond))
        if prior:
            return None
        x, _ = min_norm_solve(A, b)
        return np.asarray(x_to_T((self.P @ x.astype(np.float64)).astype(f32)), f32)

    def pairs(self):
        """Centred (P, Q) and N of the kept pairs of the last iteration, in (i, k) order."""
        l = self.last
        ii, kk = np.nonzero((l["w"] != 0) & (l["ids"] >= 0))
        P = _xf(l["T_prev"], self.rd)[ii]
        Q = self.tgt_c[l["ids"][ii, kk]]
        Pc, Qc = centre_pairs(P, Q)
        return Pc, Qc, self.tgt_nrm[l["ids"][ii, kk]]

    def covariance(self):
        """(cov fp64 6x6, H, M) of the last iteration."""
        P, Q, N = self.pairs()
        H, M = covariance_sums(P, Q, N, self.last_dT)
        return censi(H, M, self.c.sigma), H, M

    def stats(self):
        l = self.last
        w = l["w"]
        nk = w.size
        used = w != 0
        P = _xf(l["T_prev"], self.rd)
        ii, kk = np.nonzero(used)
        ww = w[ii, kk].astype(np.float64)
        Q = self.tgt_c[l["ids"][ii, kk]].astype(np.float64)
        d = P[ii].astype(np.float64) - Q
        if self.c.minimizer == "point2point":
            res = float((ww * (d * d).sum(1)).sum())
        else:
            N = self.tgt_nrm[l["ids"][ii, kk]].astype(np.float64)
            res = float((ww * ((d * N).sum(1)) ** 2).sum())
        return dict(point_used_ratio=used.sum() / nk, weighted_point_used_ratio=float(w.astype(np.float64).sum()) / nk,
                    n_rejected_matches=int((~used).sum()), n_rejected_points=int((~used.any(1)).sum()), residual_error=res)
