"""CPU restatement of the libpointmatcher loop with the chain extension (a plain helper module, not a test).

Frames ICP.cpp:952-984,1345 (both clouds centred on their centroids, the prior folded into T0 = A T_init B); exact
k-NN by the oracle's kd-tree (orc.knn_k: ordered by (d2, id)); the filters as a product of weights -- TrimmedDist
(Matches.cpp:60-87), SurfaceNormal, MaxDist, RobustOutlierFilter (OutlierFiltersImpl.cpp:397-598, fp32 in the
reference's operation order, MAD by np.partition); fp64 weighted Kabsch (PointToPoint.cpp:62-100) or weighted
point-to-plane normal equations; T_iter <- dT T_iter; Counter + Differential checkers.  Queries are transformed with the
fp32 replay of tests/oracle_side.py, so the distances are bit-comparable with the device's."""
import math

import numpy as np

from oracle import oracle as orc
from tests.oracle_side import _m4, _rot, _xf

NT = max(1, min(orc.max_threads(), 16))
f32 = np.float32

BERG_TUNING = {"cauchy": 4.3040, "tukey": 7.0589, "huber": 2.0138}


def robust_weights(fct, k, scale, d, approximation=math.inf):
    """RobustOutlierFilter weights of the distances d (fp32 throughout, the reference's operation order)."""
    d = np.asarray(d, f32)
    k, scale = f32(k), f32(scale)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
        e2 = d / f32(scale * scale)
        k2 = f32(k * k)
        one = f32(1)
        if fct == "cauchy":
            w = one / (one + e2 / k2)
        elif fct == "welsch":
            w = np.exp(-e2 / k2)
        elif fct == "sc":
            a = k + e2
            w = np.where(e2 >= k, f32(4) * k2 * (one / (a * a)), one)
        elif fct == "gm":
            a = k + e2
            w = k2 * (one / (a * a))
        elif fct == "tukey":
            a = one - e2 / k2
            w = np.where(e2 >= k2, f32(0), a * a)
        elif fct == "huber":
            w = np.where(e2 >= k2, k * (one / np.sqrt(e2)), one)
        elif fct == "L1":
            w = one / np.sqrt(e2)
        elif fct == "student":
            dd = f32(3)
            p = np.power(one + e2 / k, -(k + dd) / f32(2))
            w = p * (k + dd) * (one / (k + e2))
        else:
            raise ValueError(fct)
        w = np.asarray(w, f32)
        w = np.where(w.astype(np.float64) <= 1e-50, f32(1e-50), w).astype(f32)
        if not math.isinf(approximation):
            sq = f32(float(approximation) ** 2)
            w = np.where(e2 >= sq, f32(0), w).astype(f32)
    return w


def quantile_index(n, ratio):
    if ratio == 1.0:
        return n - 1
    return min(int(f32(n) * f32(ratio)), n - 1)


def _normalize(n):
    n = np.asarray(n, f32)
    z = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]
    z = z + n[:, 2] * n[:, 2]
    s = np.sqrt(z)
    s = np.where(z > 0, s, f32(1))
    return (n / s[:, None]).astype(f32)


def kabsch(P, Q, w):
    """Weighted Kabsch in fp64: dT (4x4) with dT P ~ Q, and the rank of the cross-covariance."""
    w = np.asarray(w, np.float64)
    P = np.asarray(P, np.float64)
    Q = np.asarray(Q, np.float64)
    sw = w.sum()
    mp = (w[:, None] * P).sum(0) / sw
    mq = (w[:, None] * Q).sum(0) / sw
    S = ((w[:, None] * (Q - mq)).T @ (P - mp)) / sw
    U, D, Vt = np.linalg.svd(S)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        Vt = Vt.copy()
        Vt[2] *= -1
        R = U @ Vt
    dT = np.eye(4)
    dT[:3, :3] = R
    dT[:3, 3] = mq - R @ mp
    rank = int((D > 1e-10 * D[0]).sum()) if D[0] > 0 else 0
    return dT, rank


def x_to_T(x):
    """PointToPlane.cpp:327-381 restated in fp64: rotation AngleAxis(atan(|r|), r / |r|) of r = x[0:3], translation x[3:6]."""
    x = np.asarray(x, np.float64)
    r = x[:3]
    n = float(np.linalg.norm(r))
    T = np.eye(4)
    if n > 0:
        a = r / n
        ang = math.atan(n)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        T[:3, :3] = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    T[:3, 3] = x[3:6]
    return T


def _quat(T):
    T = np.asarray(T, np.float64)
    m = T[:3, :3]
    tr = np.trace(m)
    if tr > 0:
        t = math.sqrt(tr + 1)
        return np.array([0.5 * t, (m[2, 1] - m[1, 2]) * 0.5 / t, (m[0, 2] - m[2, 0]) * 0.5 / t, (m[1, 0] - m[0, 1]) * 0.5 / t])
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
    v = [0.0, 0.0, 0.0]
    v[i] = 0.5 * t
    t = 0.5 / t
    v[j] = (m[j, i] + m[i, j]) * t
    v[k] = (m[k, i] + m[i, k]) * t
    return np.array([(m[k, j] - m[j, k]) * t, *v])


def _qdist(a, b):
    bw, bx, by, bz = b[0], -b[1], -b[2], -b[3]
    w = a[0] * bw - a[1] * bx - a[2] * by - a[3] * bz
    x = a[0] * bx + a[1] * bw + a[2] * bz - a[3] * by
    y = a[0] * by + a[2] * bw + a[3] * bx - a[1] * bz
    z = a[0] * bz + a[3] * bw + a[1] * by - a[2] * bx
    return 2 * math.atan2(math.sqrt(x * x + y * y + z * z), abs(w))


class Checkers:
    """CounterTransformationChecker + DifferentialTransformationChecker (TransformationCheckersImpl.cpp:57-158)."""

    def __init__(self, max_iter, min_rot, min_trans, smooth):
        self.max_iter, self.min_rot, self.min_trans, self.smooth = max_iter, min_rot, min_trans, smooth
        self.hist = [np.eye(4)]
        self.count = 0
        self.converged = self.max_iter_reached = False

    def check(self, T):
        self.hist.append(np.asarray(T, np.float64))
        go = True
        if self.smooth > 0 and len(self.hist) > self.smooth:
            cr = ct = 0.0
            for i in range(len(self.hist) - 1, len(self.hist) - 1 - self.smooth, -1):
                a, b = self.hist[i], self.hist[i - 1]
                cr += abs(_qdist(_quat(a), _quat(b)))
                ct += float(np.linalg.norm(a[:3, 3] - b[:3, 3]))
            if cr / self.smooth < self.min_rot and ct / self.smooth < self.min_trans:
                go, self.converged = False, True
        self.count += 1
        if self.count >= self.max_iter:
            go, self.max_iter_reached = False, True
        return go


class Chain:
    """The configuration of one run (names as in the YAML)."""

    def __init__(self, knn=1, minimizer="point2plane", robust=None, tuning=1.0, scale="mad", nb_iter=0,
                 distance="point2point", approximation=math.inf, max_dist=math.inf, trim_ratio=None,
                 max_normal_angle=None, outlier_max_dist=None, max_iter=40, min_rot=0.001, min_trans=0.001, smooth=3,
                 fixed_iters=0):
        self.__dict__.update(locals())
        del self.__dict__["self"]


class PmRestatement:
    """One reference + reading; robust scale / iteration persist across register() calls as in the reference."""

    def __init__(self, tgt, tgt_nrm, chain: Chain):
        self.c = chain
        self.c_ref = orc.centroid(tgt)
        self.tgt_c = (np.asarray(tgt, f32) - self.c_ref).astype(f32)
        self.tgt_nrm = None if tgt_nrm is None else np.asarray(tgt_nrm, f32)
        self.tree = orc.KdTree(self.tgt_c)
        self.scale, self.iteration = f32(0), 1
        self.tuning = f32(BERG_TUNING.get(chain.robust, chain.tuning) if chain.scale == "berg" else chain.tuning)

    def set_reading(self, src, src_nrm=None, T_init=None):
        self.c_read = orc.centroid(src)
        A = np.eye(4, dtype=f32)
        A[:3, 3] = -self.c_ref
        B = np.eye(4, dtype=f32)
        B[:3, 3] = self.c_read
        self.T0 = _m4(_m4(A, np.eye(4, dtype=f32) if T_init is None else np.asarray(T_init, f32)), B)
        self.rd = _xf(self.T0, np.asarray(src, f32) - self.c_read)
        self.rdn = None if src_nrm is None else _rot(self.T0, np.asarray(src_nrm, f32))

    def weights(self, T, ids, d2):
        """Chain weights (n x knn) at T_iter for the matches (ids, d2); updates the robust state."""
        c = self.c
        valid = ids >= 0
        w = valid.astype(f32)
        fin = d2[valid]
        self.fail = False
        if c.trim_ratio is not None:
            if fin.size == 0:
                self.fail = True
            else:
                lim = np.partition(fin, quantile_index(fin.size, c.trim_ratio))[quantile_index(fin.size, c.trim_ratio)]
                w = np.where(d2 <= lim, w, f32(0)).astype(f32)
        if c.max_normal_angle is not None:
            nr = _normalize(_rot(T, self.rdn))
            idc = np.where(valid, ids, 0)
            nt = _normalize(self.tgt_nrm[idc.ravel()]).reshape(ids.shape + (3,))
            val = nr[:, None, 0] * nt[..., 0] + nr[:, None, 1] * nt[..., 1]
            val = val + nr[:, None, 2] * nt[..., 2]
            w = np.where(val < f32(math.cos(c.max_normal_angle)), f32(0), w).astype(f32)
        if c.outlier_max_dist is not None:
            w = np.where(d2 <= f32(c.outlier_max_dist) * f32(c.outlier_max_dist), w, f32(0)).astype(f32)
        if c.robust is not None:
            upd = self.iteration <= c.nb_iter or c.nb_iter == 0
            if c.scale == "mad" and upd:
                n = fin.size
                med = np.partition(fin, n // 2)[n // 2]
                dev = np.abs(fin - med).astype(f32)
                self.scale = f32(np.sqrt(np.partition(dev, n // 2)[n // 2]))
            elif c.scale == "berg" and upd:
                if self.iteration == 1:
                    q = np.partition(fin, quantile_index(fin.size, 0.5))[quantile_index(fin.size, 0.5)]
                    self.scale = f32(1.9 * float(np.sqrt(f32(q))))
                else:
                    self.scale = f32(f32(0.85) * f32(self.scale - f32(c.tuning)) + f32(c.tuning))
            elif c.scale == "none":
                self.scale = f32(1)
            self.iteration += 1
            dist = d2
            if c.distance == "point2plane":
                P = _xf(T, self.rd)
                idc = np.where(valid, ids, 0)
                Q = self.tgt_c[idc.ravel()].reshape(ids.shape + (3,))
                nh = _normalize(self.tgt_nrm[idc.ravel()]).reshape(ids.shape + (3,))
                dd = (P[:, None, :] - Q).astype(f32)
                t = nh[..., 0] * dd[..., 0] + nh[..., 1] * dd[..., 1]
                t = t + nh[..., 2] * dd[..., 2]
                dist = (t * t).astype(f32)
            rw = robust_weights(c.robust, self.tuning, self.scale, dist, c.approximation)
            w = np.where(valid, w * rw, f32(0)).astype(f32)
        return w

    def step(self, T):
        """One iteration at T_iter: (dT, ids, d2, w, H, rank)."""
        c = self.c
        P = _xf(T, self.rd)
        ids, d2 = orc.knn_k(self.tree, P, c.knn, max_dist=c.max_dist, n_threads=NT)
        w = self.weights(T, ids, d2)
        sel = w != 0
        ii, kk = np.nonzero(sel)
        Pm = P[ii].astype(np.float64)
        Qm = self.tgt_c[ids[ii, kk]].astype(np.float64)
        ww = w[ii, kk].astype(np.float64)
        H = None
        if c.minimizer == "point2point":
            dT, rank = kabsch(Pm, Qm, ww)
        else:
            N = self.tgt_nrm[ids[ii, kk]].astype(np.float64)
            F = np.concatenate([np.cross(Pm, N), N], axis=1)
            r = ((Pm - Qm) * N).sum(1)
            H = (F * ww[:, None]).T @ F
            b = -(F * (ww * r)[:, None]).sum(0)
            x = np.linalg.solve(H, b)
            dT = x_to_T(x)
            rank = 6
        return np.asarray(dT, f32), ids, d2, w, H, rank

    def register(self, T_init=None):
        c = self.c
        chk = Checkers(c.max_iter, c.min_rot, c.min_trans, c.smooth)
        T = np.eye(4, dtype=f32)
        it = 0
        while True:
            dT, ids, d2, w, H, rank = self.step(T)
            self.last = dict(ids=ids, d2=d2, w=w, H=H, rank=rank, T_prev=T.copy())
            T = _m4(dT, T)
            it += 1
            if c.fixed_iters > 0:
                if it >= c.fixed_iters:
                    break
            elif not chk.check(T):
                break
        A = np.eye(4, dtype=f32)
        A[:3, 3] = self.c_ref
        B = np.eye(4, dtype=f32)
        B[:3, 3] = -self.c_read
        T_out = _m4(_m4(_m4(A, T), self.T0), B)
        return T_out, it, T
