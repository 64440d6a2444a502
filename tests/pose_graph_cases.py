"""Seeded pose graphs for the pose-graph tests (CPU side; no device).  With NB = 48 the edge of the solver's diagonal tile
(kPgNB) and 96 that of a trailing-update tile, the node counts give 6 n = 42 (below one tile), 48 (exactly one), 54 (one
plus 6), 180 (several, the last one ragged) and 1206 (201 nodes: 25 tiles plus 6).

An edge's measurement that agrees with poses Ts, Tt is X = Tt^-1 Ts (zeta = lin6(X^-1 Tt^-1 Ts) = 0).  Odometry edges run
from node i to i + 1 and are certain; loop closures run from a later to an earlier node and are uncertain, as
OptimizationProblem builds them."""
import numpy as np

from tests import pose_graph_restatement as R


def pose_of(v):
    return R.pose_step(np.asarray(v, np.float64), np.eye(4))


def random_pose(rng, rot, trans):
    return pose_of(np.concatenate([rng.uniform(-rot, rot, 3), rng.uniform(-trans, trans, 3)]))


def measurement(Ts, Tt):
    return R.omm(R.rigid_inverse(Tt), Ts)


def information(rng, scale=500.0):
    A = rng.uniform(-1.0, 1.0, (6, 6))
    return scale * np.eye(6) + 0.05 * scale * (A @ A.T)


def ring_truth(n, radius):
    """n poses on a circle, heading along it, with a gentle roll and climb."""
    out = []
    for i in range(n):
        a = 2.0 * np.pi * i / n
        out.append(pose_of([0.05 * np.sin(3 * a), 0.03 * np.cos(2 * a), a + np.pi / 2, radius * np.cos(a), radius * np.sin(a),
                            0.2 * np.sin(a)]))
    return np.stack(out)


def integrate(first, Xs):
    """The nodes OptimizationProblem derives from odometry edges: Tt = Ts X^-1."""
    poses = [first]
    for X in Xs:
        poses.append(R.omm(poses[-1], R.rigid_inverse(X)))
    return np.stack(poses)


class Case:
    def __init__(self, name, graph, option=None, truth=None, wrong=()):
        self.name, self.graph, self.truth = name, graph, truth
        self.option = option or R.Option()
        self.criteria = R.Criteria()
        self.wrong = tuple(wrong)   # indices (into the input edge list) of the grossly wrong closures


def _chain(seed=11, n=7):
    rng = np.random.default_rng(seed)
    truth = np.stack([pose_of([0.02 * i, -0.03 * i, 0.25 * i, 1.5 * i, 0.3 * np.sin(i), 0.1 * i]) for i in range(n)])
    src, tgt = [], []
    for i in range(n - 1):
        src.append(i), tgt.append(i + 1)
    for i in range(n - 2):
        src.append(i), tgt.append(i + 2)
    X = [measurement(truth[s], truth[t]) for s, t in zip(src, tgt)]
    info = [information(rng) for _ in src]
    poses = truth.copy()
    for i in range(1, n):   # node 0 is the reference and stays
        poses[i] = R.omm(random_pose(rng, 0.03, 0.15), truth[i])
    return Case("a_chain", R.Graph(poses, src, tgt, X, info, [False] * len(src)), truth=truth)


def _ring(name, seed, n, closures, wrong=(), drift=(0.004, 0.03), option=None):
    rng = np.random.default_rng(seed)
    truth = ring_truth(n, 0.25 * n + 2.0)
    src, tgt, X, unc = [], [], [], []
    for i in range(n - 1):
        noisy = R.omm(random_pose(rng, drift[0], drift[1]), measurement(truth[i], truth[i + 1]))
        src.append(i), tgt.append(i + 1), X.append(noisy), unc.append(False)
    poses = integrate(truth[0], X)
    wrong_idx = []
    for k, (s, t) in enumerate(closures):
        Xc = R.omm(random_pose(rng, 0.005, 0.2), measurement(truth[s], truth[t]))   # noisy enough to leave confidence 1
        if k in wrong:
            Xc = R.omm(pose_of([0.3, -0.2, 0.8, 3.0, -2.0, 1.0]), Xc)
            wrong_idx.append(len(src))
        src.append(s), tgt.append(t), X.append(Xc), unc.append(True)
    info = [information(rng) for _ in src]
    return Case(name, R.Graph(poses, src, tgt, X, info, unc), option=option, truth=truth, wrong=wrong_idx)


def _certain(seed=17, n=30):
    rng = np.random.default_rng(seed)
    truth = ring_truth(n, 8.0)
    src, tgt = [], []
    for i in range(n - 1):
        src.append(i), tgt.append(i + 1)
    for i in range(0, n - 3, 2):
        src.append(i), tgt.append(i + 3)
    X = [R.omm(random_pose(rng, 0.003, 0.02), measurement(truth[s], truth[t])) for s, t in zip(src, tgt)]
    info = [information(rng) for _ in src]
    poses = integrate(truth[0], X[:n - 1])
    return Case("d_certain", R.Graph(poses, src, tgt, X, info, [False] * len(src)), truth=truth)


def _double(seed=19, n=5):
    rng = np.random.default_rng(seed)
    truth = ring_truth(n, 3.0)
    pairs = [(0, 1, False), (1, 2, False), (1, 2, False), (2, 3, False), (3, 4, False), (4, 0, True), (4, 0, True)]
    src, tgt, unc = [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs]
    X = [R.omm(random_pose(rng, 0.004, 0.2 if u else 0.03), measurement(truth[s], truth[t])) for s, t, u in zip(src, tgt, unc)]
    info = [information(rng) for _ in src]
    poses = integrate(truth[0], [X[0], X[1], X[3], X[4]])
    return Case("e_double", R.Graph(poses, src, tgt, X, info, unc), option=R.Option(max_correspondence_distance=1.0), truth=truth)


def _tiny():
    rng = np.random.default_rng(23)
    one = Case("f_one_node", R.Graph(pose_of([0.1, 0.2, 0.3, 1, 2, 3])[None], [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), []))
    truth = np.stack([np.eye(4), pose_of([0.0, 0.0, 0.4, 2.0, 0.0, 0.0])])
    poses = truth.copy()
    poses[1] = R.omm(random_pose(rng, 0.02, 0.1), truth[1])
    two = Case("f_two_nodes", R.Graph(poses, [0], [1], [measurement(truth[0], truth[1])], [information(rng)], [False]), truth=truth)
    return one, two


_LOOSE = dict(max_correspondence_distance=1.0)


def lm_cases():
    """Cases (a) to (f): the graphs of the LM and GlobalOptimization tests."""
    one, two = _tiny()
    return [
        _chain(),
        _ring("b_ring", 13, 8, [(7, 0)], option=R.Option(**_LOOSE)),
        _ring("c_ring_wrong", 15, 9, [(8, 0), (7, 1), (6, 2)], wrong=(2,), option=R.Option(**_LOOSE)),
        _certain(),
        _double(),
        one,
        two,
    ]


def large_case(n=201):
    """The closures of case (c) scaled up to a ring of n nodes (the largest system: 6 n = 1206)."""
    k = n // 9
    return _ring("g_large", 29, n, [(n - 1, 0), (n - 1 - k, k), (n - 1 - 2 * k, 2 * k)], wrong=(2,), drift=(0.0005, 0.004),
                 option=R.Option(**_LOOSE))


def by_name(name):
    for c in lm_cases() + [large_case()]:
        if c.name == name:
            return c
    raise KeyError(name)


SOLVER_SIZES = (42, 48, 54, 102, 1206)   # below one diagonal tile, one, one plus 6, a trailing tile plus 6, 25 tiles plus 6


def spd_system(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.uniform(-1.0, 1.0, (n, n))
    return B @ B.T / n + 0.1 * np.eye(n), rng.uniform(-1.0, 1.0, n)


def solver_systems():
    """(name, A, b): seeded SPD systems of the tile-boundary sizes, and H + lambda I of case (c) at its first LM step."""
    out = [(f"spd_{n}", *spd_system(n, 100 + n)) for n in SOLVER_SIZES]
    c = by_name("c_ring_wrong")
    g = c.graph.copy()
    w = R.line_process_weight(g.info, c.option.preference_loop_closure, c.option.max_correspondence_distance)
    _, _, _, ele = R.linearize(g, want_H=False)
    R.update_confidences(g, ele, w)
    H, b, _, _ = R.linearize(g)
    out.append(("c_ring_wrong_H_lambda", H + 1e-5 * float(np.max(np.diag(H))) * np.eye(H.shape[0]), b))
    return out


def backward_error(A, x, b):
    """The normwise backward error |A x - b| / (|A| |x| + |b|), 2-norms (Frobenius for A), the residual in long double."""
    r = np.array(A, np.longdouble) @ np.array(x, np.longdouble) - np.array(b, np.longdouble)
    return float(np.sqrt(np.sum(r * r))) / (float(np.linalg.norm(A)) * float(np.linalg.norm(x)) + float(np.linalg.norm(b)))


# Measured with this file and pose_graph_restatement.py (tests/test_pose_graph_host.py repeats the measurement):
# the normwise backward error of scipy.linalg.cho_solve on solver_systems(); the device's bar is 8 x the largest.
CHO_BACKWARD_ERRORS = {"spd_42": 2.66e-17, "spd_48": 2.8e-17, "spd_54": 2.06e-17, "spd_102": 1.66e-17, "spd_1206": 1.06e-17,
                       "c_ring_wrong_H_lambda": 9.09e-18}
SOLVER_BAR_FACTOR = 8.0
SOLVER_BAR = SOLVER_BAR_FACTOR * max(CHO_BACKWARD_ERRORS.values())   # 2.24e-16
# per LM case the largest spread between the restatement's three solvers (numpy solve, scipy cho_solve, long-double
# Cholesky) after GlobalOptimization: compensated poses (absolute), confidences (absolute), first / last residuals of both
# passes (relative); the device's bar is 16 x these.
SOLVER_SPREADS = {"a_chain": (2.66e-15, 0.0, 3.55e-09), "b_ring": (4e-15, 0.0, 1.63e-14),
                  "c_ring_wrong": (5.11e-15, 0.0, 8.95e-15), "d_certain": (1.15e-14, 0.0, 1.35e-14),
                  "e_double": (1.78e-15, 0.0, 5.29e-15), "f_one_node": (0.0, 0.0, 0.0), "f_two_nodes": (4.44e-16, 0.0, 1.18e-07)}
LM_BAR_FACTOR = 16.0


def measure_spreads(case):
    outs = [R.global_optimization(case.graph, case.option, case.criteria, s) for s in R.SOLVERS.values()]
    pose = conf = res = 0.0
    for i in range(len(outs)):
        for j in range(i):
            (ga, ra), (gb, rb) = outs[i], outs[j]
            pose = max(pose, float(np.abs(ga.poses - gb.poses).max()))
            if ga.E:
                conf = max(conf, float(np.abs(ga.confidence - gb.confidence).max()))
            for pa, pb in zip(ra, rb):
                for k in ("first_residual", "last_residual"):
                    if pa[k] != pb[k]:
                        res = max(res, abs(pa[k] - pb[k]) / max(abs(pa[k]), abs(pb[k])))
    return pose, conf, res, outs
