"""CPU restatement of degeneracyAwareness EqualityConstraints (X-ICP, ternary) on top of tests/pm_extras_restatement.py
(a plain helper module, not a test).  Sources: ICP.cpp:1143-1165, 1698-2125, 2158-2184, 2504-2795,
PointToPlane.cpp:459-505, 570-626.

  alignments          the data frame, the centre of the matched pairs and both alignment vectors in fp32 with one rounding
                      per operation, in the order oracle/icp_oracle.c uses for the first-iteration analysis
  contributions       combined (a >= cos minimal) / high (a > cos strong) as fp64 sums, with their pair counts
  decide              the ternary category of the six eigen-directions and the sanity rule
  partial_sums        the nine fp64 sums of fp32 products of one partial direction over its sample (+ the sums of |term|)
  partial_constraint  the 3x3 problem in the reference's expression order (partial-pivot LU, L^T L, fp64 least squares,
                      cofactor inverse of U); fp64=True evaluates the same sequence in fp64 throughout
  kkt_solve           the (6+c)x(6+c) system of PointToPlane.cpp:484-503 with the constraint values, fp64
  TernaryRestatement  the registration loop
"""
import math

import numpy as np

from oracle import oracle as orc
from tests.oracle_side import _m4, _xf
from tests.pm_chain_restatement import NT, Checkers, x_to_T
from tests.pm_extras_restatement import ExtrasChain, PmExtrasRestatement, bound_values, min_norm_solve, OutOfBounds

f32 = np.float32
LOCALIZABLE, PARTIAL_MIXED, PARTIAL_HIGH, NONE = 0, 1, 2, 3
YAML_THRESHOLDS = (250.0, 180.0, 35.0, 80.0, 45.0)   # high, enough, insufficient; minimal / strong angle [deg]


def cos_deg(deg):
    """cos of an angle threshold as the library forms it: fp64, rounded to fp32."""
    return f32(math.cos(float(f32(deg)) * 3.14159265358979323846 / 180.0))


class TernaryChain(ExtrasChain):
    """ExtrasChain plus ternary = (high, enough, insufficient, minimal angle, strong angle) or None."""

    def __init__(self, ternary=YAML_THRESHOLDS, **kw):
        super().__init__(**kw)
        self.ternary = ternary


def _dot3(a, b):
    """(a0 b0 + a1 b1) + a2 b2, one fp32 rounding per operation; a: n x 3, b: 3 or n x 3."""
    b = np.asarray(b, f32)
    s = a[:, 0] * b[..., 0] + a[:, 1] * b[..., 1]
    return (s + a[:, 2] * b[..., 2]).astype(f32)


def eigvecs_data_frame(V, Trd):
    """Eigenvectors V[r, k] (fp64) -> fp32 rows [k, r] in the data frame: v' = R^T v."""
    Vf = np.asarray(V, np.float64).astype(f32)
    out = np.zeros((3, 3), f32)
    for k in range(3):
        for r in range(3):
            s = f32(Trd[0, r] * Vf[0, k]) + f32(Trd[1, r] * Vf[1, k])
            out[k, r] = f32(s) + f32(Trd[2, r] * Vf[2, k])
    return out


def alignments(P, N, Trd, Vr, Vt):
    """|alignment . v_k| of every pair: (ar n x 3 rotation, at n x 3 translation), fp32.  P: matched reading points at
    T_iter, N: matched normals, Trd: T_refMean_dataIn, Vr / Vt: eigenvectors [r, k] in the optimisation frame."""
    P, N, Trd = np.asarray(P, f32), np.asarray(N, f32), np.asarray(Trd, f32)
    vr, vt = eigvecs_data_frame(Vr, Trd), eigvecs_data_frame(Vt, Trd)
    q = (P - Trd[:3, 3]).astype(f32)
    ps = np.stack([_dot3(q, Trd[:3, r]) for r in range(3)], 1)
    nn = np.stack([_dot3(N, Trd[:3, r]) for r in range(3)], 1)
    c = np.zeros(3, f32)
    if P.shape[0] > 0:
        c = (ps.astype(np.float64).sum(0) / P.shape[0]).astype(f32)
    ps = (ps - c).astype(f32)
    cr = np.stack([ps[:, 1] * nn[:, 2] - ps[:, 2] * nn[:, 1], ps[:, 2] * nn[:, 0] - ps[:, 0] * nn[:, 2],
                   ps[:, 0] * nn[:, 1] - ps[:, 1] * nn[:, 0]], 1).astype(f32)
    s2 = cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]
    nrm = np.sqrt(s2 + cr[:, 2] * cr[:, 2]).astype(f32)
    big = ~(nrm < f32(1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = np.where(big[:, None], cr / nrm[:, None], cr).astype(f32)
    ar = np.stack([np.abs(_dot3(cr, vr[k])) for k in range(3)], 1)
    at = np.stack([np.abs(_dot3(nn, vt[k])) for k in range(3)], 1)
    assert ar.dtype == f32 and at.dtype == f32
    return ar, at


def contributions(al, cos_min, cos_strong):
    """(combined[6], high[6], n_combined[6], n_high[6]) of the n x 6 alignments (rotation 0-2, translation 3-5)."""
    a64 = al.astype(np.float64)
    mc, mh = al >= f32(cos_min), al > f32(cos_strong)
    return (a64 * mc).sum(0), (a64 * mh).sum(0), mc.sum(0).astype(np.int64), mh.sum(0).astype(np.int64)


def decide(comb, high, n_comb, n_high, n_pairs, high_thr, enough_thr, insufficient_thr):
    """(categories[6], sane): decideLocalizabilityLevel's order of tests and the sanity rule of ICP.cpp:1956-1967."""
    hi, en, ins = float(f32(high_thr)), float(f32(enough_thr)), float(f32(insufficient_thr))
    cat, sane = np.zeros(6, np.int32), True
    for k in range(6):
        sample = None
        if comb[k] >= hi or high[k] >= en:
            cat[k] = LOCALIZABLE
        elif en <= comb[k] < hi:
            cat[k], sample = PARTIAL_MIXED, int(n_comb[k])
        elif high[k] >= ins:
            cat[k], sample = PARTIAL_HIGH, int(n_high[k])
        else:
            cat[k] = NONE
        if sample is not None and (sample < ins or sample > n_pairs):
            sane = False
    return cat, sane


def partial_terms(P, Q, N, rotation):
    """The nine fp32 products of every pair: f f^T (upper triangle, row by row) and f r, with f = p x n (rotation) or n
    (translation) and r = n . (p - q) as the normal equations form them."""
    P, Q, N = np.asarray(P, f32), np.asarray(Q, f32), np.asarray(N, f32)
    d = (P - Q).astype(f32)
    r = _dot3(d, N)
    if rotation:
        f = np.stack([P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1], P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2],
                      P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]], 1).astype(f32)
    else:
        f = N
    t = np.stack([f[:, 0] * f[:, 0], f[:, 0] * f[:, 1], f[:, 0] * f[:, 2], f[:, 1] * f[:, 1], f[:, 1] * f[:, 2],
                  f[:, 2] * f[:, 2], f[:, 0] * r, f[:, 1] * r, f[:, 2] * r], 1)
    assert t.dtype == f32
    return t


def partial_sums(P, Q, N, rotation, sample):
    """(sums9 fp64, sums of |term| fp64) over the pairs of `sample` (a boolean mask)."""
    t = partial_terms(P[sample], Q[sample], N[sample], rotation).astype(np.float64)
    return t.sum(0), np.abs(t).sum(0)


def _cof3(m, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return m[i1, j1] * m[i2, j2] - m[i1, j2] * m[i2, j1]


def partial_constraint(s9, v, fp64=False):
    """The constraint value v . x3 of solveSimpleOptimizationProblemForPartialConstraints from the nine sums (rounded once
    to fp32) in dtype D = fp32 (the reference) or, fp64=True, in fp64 throughout."""
    D = np.float64 if fp64 else f32
    a = [D(f32(x)) for x in s9[:6]]
    M = np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]], D)
    b = np.array([-D(f32(x)) for x in s9[6:9]], D)
    with np.errstate(all="ignore"):
        for k in range(3):   # Eigen's unblocked partial-pivot LU
            piv = k + int(np.argmax(np.abs(M[k:, k])))
            if M[piv, k] != 0:
                if piv != k:
                    M[[k, piv]] = M[[piv, k]]
                    b[[k, piv]] = b[[piv, k]]
                for i in range(k + 1, 3):
                    M[i, k] = M[i, k] / M[k, k]
            for i in range(k + 1, 3):
                for j in range(k + 1, 3):
                    M[i, j] = M[i, j] - M[i, k] * M[k, j]
        L = np.eye(3, dtype=D)
        L[1, 0], L[2, 0], L[2, 1] = M[1, 0], M[2, 0], M[2, 1]
        U = np.triu(M).astype(D)
        nA, nb = np.zeros((3, 3), D), np.zeros(3, D)
        for i in range(3):
            for j in range(3):
                s = L[0, i] * L[0, j] + L[1, i] * L[1, j]
                nA[i, j] = s + L[2, i] * L[2, j]
            s = L[0, i] * b[0] + L[1, i] * b[1]
            nb[i] = s + L[2, i] * b[2]
        y = np.linalg.lstsq(nA.astype(np.float64), nb.astype(np.float64), rcond=None)[0].astype(D)
        cof = np.array([[_cof3(U, i, j) for j in range(3)] for i in range(3)], D)
        det = (cof[0, 0] * U[0, 0] + cof[1, 0] * U[1, 0]) + cof[2, 0] * U[2, 0]
        invdet = D(1) / det
        inv = (cof.T * invdet).astype(D)   # inverse(r, c) = cofactor<c, r> / det
        x = np.array([(inv[r, 0] * y[0] + inv[r, 1] * y[1]) + inv[r, 2] * y[2] for r in range(3)], D)
        vv = np.asarray(v, f32).astype(D)
        val = (vv[0] * x[0] + vv[1] * x[1]) + vv[2] * x[2]
    assert isinstance(val, D)
    return val


def kkt_solve(A, b, Vr, Vt, cat, constraint):
    """x (fp64, 6) of the KKT system: A symmetrised in fp64, one row / column per direction with cat != LOCALIZABLE holding
    its eigenvector (fp64, optimisation frame) in its own 3-block, right-hand side its constraint value."""
    S = 0.5 * (np.asarray(A, f32).astype(np.float64) + np.asarray(A, f32).astype(np.float64).T)
    idx = [k for k in range(6) if cat[k] != LOCALIZABLE]
    c = len(idx)
    K, g = np.zeros((6 + c, 6 + c)), np.zeros(6 + c)
    K[:6, :6], g[:6] = S, np.asarray(b, f32).astype(np.float64)
    for m, k in enumerate(idx):
        v = np.zeros(6)
        if k < 3:
            v[:3] = np.asarray(Vr, np.float64)[:, k]
        else:
            v[3:] = np.asarray(Vt, np.float64)[:, k - 3]
        K[:6, 6 + m], K[6 + m, :6], g[6 + m] = v, v, float(constraint[k])
    return np.linalg.lstsq(K, g, rcond=None)[0][:6]


class TernaryRestatement(PmExtrasRestatement):
    """PmExtrasRestatement with EqualityConstraints in every iteration.  `trace` keeps the analysis of every iteration (a
    dict); fp64_partial evaluates the partial problems in fp64 throughout."""

    def __init__(self, tgt, tgt_nrm, chain, fp64_partial=False):
        super().__init__(tgt, tgt_nrm, chain)
        self.fp64_partial = fp64_partial

    def set_reading(self, src, src_nrm=None, T_init=None):
        super().set_reading(src, src_nrm, T_init)
        A = np.eye(4, dtype=f32)
        A[:3, 3] = -self.c_ref
        self.Trd = _m4(A, np.eye(4, dtype=f32) if T_init is None else np.asarray(T_init, f32))

    def analyse(self, T, A, ids, w):
        """The analysis of one iteration at T_iter on the fp32 system matrix A and the kept pairs."""
        hi, en, ins, amin, astrong = self.c.ternary
        keep = (ids[:, 0] >= 0) & (w[:, 0] != 0)
        P = _xf(T, self.rd)[keep]
        Q = self.tgt_c[ids[keep, 0]]
        N = self.tgt_nrm[ids[keep, 0]]
        Vr, Vt = orc.xicp_eigvecs(A)
        ar, at = alignments(P, N, self.Trd, Vr, Vt)
        al = np.concatenate([ar, at], 1)
        cmin, cstrong = cos_deg(amin), cos_deg(astrong)
        comb, high, nc, nh = contributions(al, cmin, cstrong)
        cat, sane = decide(comb, high, nc, nh, P.shape[0], hi, en, ins)
        vo = np.concatenate([np.asarray(Vr).astype(f32).T, np.asarray(Vt).astype(f32).T], 0)   # [k, r]
        constraint, psums, pabs = np.zeros(6, f32), np.zeros((6, 9)), np.zeros((6, 9))
        finite = True
        for k in range(6):
            if cat[k] not in (PARTIAL_MIXED, PARTIAL_HIGH):
                continue
            sample = al[:, k] >= cmin if cat[k] == PARTIAL_MIXED else al[:, k] > cstrong
            psums[k], pabs[k] = partial_sums(P, Q, N, k < 3, sample)
            val = partial_constraint(psums[k], vo[k], self.fp64_partial)
            constraint[k] = f32(val)
            finite = finite and bool(np.isfinite(val))
        return dict(cat=cat, sane=sane, comb=comb, high=high, n_comb=nc, n_high=nh, n_pairs=P.shape[0], vo=vo, Vr=Vr, Vt=Vt,
                    constraint=constraint, psums=psums, pabs=pabs, finite=finite, al=al)

    def register(self, T_init=None):
        c = self.c
        chk = Checkers(c.max_iter, c.min_rot, c.min_trans, c.smooth)
        T = np.eye(4, dtype=f32)
        it = 0
        self.trace, self.returned_prior, self.last_dT, self.bound_last = [], False, None, None
        while True:
            P = _xf(T, self.rd)
            ids, d2 = orc.knn_k(self.tree, P, 1, max_dist=c.max_dist, n_threads=NT)
            w = self.weights(T, ids, d2)
            self.last = dict(ids=ids, d2=d2, w=w, T_prev=T.copy())
            # the system as the device builds it: fp32 products, fp64 sums, rounded to fp32
            A, b, _, _ = orc.p2pl_normal_eq(self.rd, self.tgt_c, self.tgt_nrm, T, np.ascontiguousarray(ids[:, 0]),
                                            np.ascontiguousarray(d2[:, 0]), np.ascontiguousarray(w[:, 0]), n_threads=NT)
            an = self.analyse(T, A, ids, w)
            self.trace.append(an)
            if not an["sane"] or not an["finite"]:
                self.returned_prior = True
                break
            if (an["cat"] == LOCALIZABLE).all():
                x, _ = min_norm_solve(A, b)
            else:
                x = kkt_solve(A, b, an["Vr"], an["Vt"], an["cat"], an["constraint"]).astype(f32)
            self.last_dT = np.asarray(x_to_T(x), f32)
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
        A4 = np.eye(4, dtype=f32)
        A4[:3, 3] = self.c_ref
        B4 = np.eye(4, dtype=f32)
        B4[:3, 3] = -self.c_read
        T_out = _m4(_m4(_m4(A4, T), self.T0), B4)
        if self.returned_prior:
            T_out = np.eye(4, dtype=f32) if T_init is None else np.asarray(T_init, f32)
        return T_out, it, T
