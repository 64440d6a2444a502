"""The exact reference for the shipped point-to-plane chain, shared by the GPU tests (a plain helper module, not a test):
global centroid, kd-tree, TrimmedDist plus the normal-angle filter, fp64 normal equations -- the oracle's R1 / R2 replayed
once (numeric contract NC1-NC4), the kd-tree kept for several poses."""
import numpy as np

from oracle import oracle as orc

NT = max(1, min(orc.max_threads(), 64))


def _m4(A, B):
    C = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = np.float32(A[i, 0] * B[0, j])
            s = np.float32(s + np.float32(A[i, 1] * B[1, j]))
            s = np.float32(s + np.float32(A[i, 2] * B[2, j]))
            s = np.float32(s + np.float32(A[i, 3] * B[3, j]))
            C[i, j] = s
    return C


def _xf(T, P):
    T = T.astype(np.float32)
    P = P.astype(np.float32)
    out = np.empty_like(P)
    for i in range(3):
        s = T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]
        s = s + T[i, 2] * P[:, 2]
        out[:, i] = s + T[i, 3]
    return out


def _rot(T, P):
    T = T.astype(np.float32)
    P = P.astype(np.float32)
    out = np.empty_like(P)
    for i in range(3):
        s = T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]
        out[:, i] = s + T[i, 2] * P[:, 2]
    return out


class OracleSide:
    """R1 / R2 of the oracle replayed once (numeric contract NC1-NC4, T_init = I unless given), kd-tree kept for several poses.

    `src_xyz` / `src_nrm` replace the scene's reading (e.g. a reading with extra points appended); `trim_ratio=None`
    leaves TrimmedDist out (use_trimmed = 0); `T_init` is the prior R2 pre-transforms with (a rigid one: R3's
    re-orthogonalisation is not replayed)."""

    def __init__(self, sc, n_src=None, c_read=None, src_xyz=None, src_nrm=None, trim_ratio=0.9, T_init=None):
        src = sc.src_xyz[:n_src] if src_xyz is None else src_xyz
        snrm = sc.src_nrm[:n_src] if src_nrm is None else src_nrm
        self.c_ref = orc.centroid(sc.tgt_xyz)
        self.c_read = orc.centroid(src) if c_read is None else c_read
        self.tgt_c = sc.tgt_xyz - self.c_ref
        A = np.eye(4, dtype=np.float32)
        A[:3, 3] = -self.c_ref
        B = np.eye(4, dtype=np.float32)
        B[:3, 3] = self.c_read
        T0 = _m4(_m4(A, np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32)), B)
        self.rd = _xf(T0, src - self.c_read)
        self.rdn = _rot(T0, snrm)
        self.tgt_nrm = sc.tgt_nrm
        self.tree = orc.KdTree(self.tgt_c)
        self.filt = orc.make_filters(trim_ratio=trim_ratio, max_normal_angle=1.57)

    def linearize(self, T_iter):
        T_iter = np.asarray(T_iter, np.float32)
        ids, d2 = self.tree.knn(self.rd, T_iter, max_dist=0.5, n_threads=NT)
        w, limit = orc.weights(self.filt, self.rdn, self.tgt_nrm, T_iter, ids, d2, n_threads=NT)
        A6, b6, err, kept = orc.p2pl_normal_eq(self.rd, self.tgt_c, self.tgt_nrm, T_iter, ids, d2, w, n_threads=NT)
        return ids, d2, w, A6, b6, err, kept
