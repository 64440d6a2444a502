"""Seeded pose graphs for the pose-graph tests (CPU side; no device).  With NB = 48 the edge of the solver's diagonal tile
(kPgNB) and 96 that of a trailing-update tile, the node counts give 6 n = 42 (below one tile), 48 (exactly one), 54 (one
plus 6), 180 (several, the last one ragged) and 1206 (201 nodes: 25 tiles plus 6); lm_branch_cases() adds 72, 288 (three
whole trailing tiles, no padding), 300 and 1542 rows.

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
    def __init__(self, name, graph, option=None, truth=None, wrong=(), criteria=None):
        self.name, self.graph, self.truth = name, graph, truth
        self.option = option or R.Option()
        self.criteria = criteria or R.Criteria()
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


def _rough(name, seed, rot, trans, uncertain, n=12, criteria=None):
    """A ring of n nodes with odometry and two closures whose nodes start far from the truth: every initial pose is the
    true one perturbed by a random pose of up to rot rad and trans m, so that LM steps are rejected on the way."""
    rng = np.random.default_rng(seed)
    truth = ring_truth(n, 0.25 * n + 2.0)
    src, tgt, X, unc = [], [], [], []
    for i in range(n - 1):
        src.append(i), tgt.append(i + 1), unc.append(False)
        X.append(R.omm(random_pose(rng, 0.004, 0.03), measurement(truth[i], truth[i + 1])))
    for s, t in ((n - 1, 0), (n - 3, 2)):
        src.append(s), tgt.append(t), unc.append(uncertain)
        X.append(R.omm(random_pose(rng, 0.005, 0.2), measurement(truth[s], truth[t])))
    info = [information(rng) for _ in src]
    poses = np.stack([R.omm(random_pose(rng, rot, trans), truth[i]) for i in range(n)])
    return Case(name, R.Graph(poses, src, tgt, X, info, unc), option=R.Option(**_LOOSE), truth=truth, criteria=criteria)


DENSE_HOPS = (5, 7, 9, 11, 13, 15)


def _dense(seed=31, n=50):
    """Closures (i + h, i) for every i and every h of DENSE_HOPS on a ring of 50 nodes: E = 49 + 240 = 289 edges on
    M = 300 rows (Mp = 384), three of the closures grossly wrong."""
    closures = [(i + h, i) for h in DENSE_HOPS for i in range(n - h)]
    return _ring("k_dense", seed, n, closures, wrong=(3, 100, 200), option=R.Option(**_LOOSE))


def _thirds(name, seed, n, drift=(0.004, 0.03)):
    k = n // 9
    return _ring(name, seed, n, [(n - 1, 0), (n - 1 - k, k), (n - 1 - 2 * k, 2 * k)], wrong=(2,), drift=drift,
                 option=R.Option(**_LOOSE))


def lm_branch_cases():
    """Cases (h) to (m): rejected LM steps (lm_solves > outer_iterations, nu grown to 4), the two iteration caps, more than
    256 edges, three whole solver tiles without padding (M = 288), more than 256 nodes.  Held to the rules of lm_cases()."""
    return [
        _rough("h_rough_start", 51, 0.8, 3.0, False),
        _rough("h_rough_far", 57, 2.5, 10.0, True),
        _rough("i_cap_lm", 51, 1.5, 6.0, True, criteria=R.Criteria(max_iteration_lm=2)),
        _rough("j_cap_outer", 51, 0.8, 3.0, False, criteria=R.Criteria(max_iteration=3)),
        _dense(),
        _thirds("l_three_tiles", 37, 48),
        _thirds("m_nodes_257", 41, 257, drift=(0.0005, 0.004)),
    ]


def by_name(name):
    for c in lm_cases() + [large_case()] + lm_branch_cases():
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
# the same measurement on lm_branch_cases()
SOLVER_SPREADS.update({"h_rough_start": (3.42e-14, 0.0, 2.57e-14), "h_rough_far": (1.99e-09, 0.0, 2.57e-09),
                       "i_cap_lm": (4.9e-11, 0.0, 6.9e-13), "j_cap_outer": (2.2e-12, 0.0, 4.11e-12),
                       "k_dense": (1.55e-14, 3.67e-15, 2.66e-15), "l_three_tiles": (4.95e-13, 0.0, 8.32e-14),
                       "m_nodes_257": (2.53e-10, 4.45e-16, 1.36e-11)})
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


# ---- further solver systems (their own table: SOLVER_SIZES, CHO_BACKWARD_ERRORS and SOLVER_BAR above stay as they are) ----
# one node, two nodes; 96, 192, 288: whole tiles, Mp == M, no identity padding; 144: three panels, the trailing region of the
# last starts in mid-tile; 198: two tiles plus 6
MORE_SOLVER_SIZES = (6, 12, 96, 144, 192, 198, 288)


def graded_system(n=198, seed=401):
    """A = Q diag(logspace(0, -10, n)) Q^T, symmetrised: condition number 1e10.  The backward error of a Cholesky solve does
    not depend on the conditioning, so SOLVER_BAR holds."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0.0, -10.0, n)) @ Q.T
    return 0.5 * (A + A.T), rng.uniform(-1.0, 1.0, n)


def more_solver_systems():
    """Seed 100 + n as in solver_systems(), but 114 for n = 12: with seed 112 the reference itself reaches 3.43e-17, above
    the cap on MORE_CHO_BACKWARD_ERRORS, and such a system is replaced."""
    return [(f"spd_{n}", *spd_system(n, 114 if n == 12 else 100 + n)) for n in MORE_SOLVER_SIZES] + \
        [("graded_198", *graded_system())]


# scipy.linalg.cho_solve's backward error on more_solver_systems(), measured like CHO_BACKWARD_ERRORS; every one has to stay
# at or below SOLVER_BAR / 8 = 2.8e-17 (tests/test_pose_graph_host.py), so that SOLVER_BAR keeps its factor 8 over the
# reference on these systems too.
MORE_CHO_BACKWARD_ERRORS = {"spd_6": 1.77e-17, "spd_12": 1.96e-17, "spd_96": 2.08e-17, "spd_144": 1.78e-17, "spd_192": 1.55e-17,
                            "spd_198": 1.62e-17, "spd_288": 1.58e-17, "graded_198": 2.68e-17}


def exact_systems(n, seed=211):
    """(name, A, b, x) whose solution is exact in fp64: the identity; diag(4^k), integer k in [-8, 8] (square roots and
    divisions by powers of two are exact); a zero right-hand side."""
    rng = np.random.default_rng(seed + n)
    b = rng.uniform(-1.0, 1.0, n)
    d = 4.0 ** rng.integers(-8, 9, n)
    return [("identity", np.eye(n), b, b.copy()), ("diag_4^k", np.diag(d), b, b / d),
            ("zero_rhs", spd_system(n, 100 + n)[0], np.zeros(n), np.zeros(n))]


BAD_PIVOT_ROWS = (0, 47, 48, 95, 96, 143, 144, 197)   # first and last row of the panels at the tile borders, of 198 rows


def bad_pivot_system(r, n=198, seed=298):
    """spd_system(n, seed) with A[r, r] = L[r, :r] . L[r, :r] - 1, L its Cholesky factor: the pivots before row r stay as
    they were, pivot r is -1 (up to rounding), so the solver's status is r + 1."""
    A, b = spd_system(n, seed)
    L = np.linalg.cholesky(A)
    A[r, r] = float(np.dot(L[r, :r], L[r, :r])) - 1.0
    return A, b


def poisoned_systems(r=100, n=198, seed=298):
    """(name, A, b): a NaN, then +inf, on the diagonal at row r; a NaN at (r, r - 60), which reaches pivot r first: it
    enters row r of the factor alone, and of the pivots only pivot r takes row r."""
    out = []
    for name, at, v in (("nan_diagonal", (r, r), np.nan), ("inf_diagonal", (r, r), np.inf), ("nan_below", (r, r - 60), np.nan)):
        A, b = spd_system(n, seed)
        A[at] = v
        out.append((name, A, b))
    return out


# ---- the optimiser's bad-pivot contract ----
def first_lm_system(case):
    """H + lambda I and b of the first LM solve of a pass on the case's graph, and max diag H."""
    g = case.graph.copy()
    w = R.line_process_weight(g.info, case.option.preference_loop_closure, case.option.max_correspondence_distance)
    _, _, _, ele = R.linearize(g, want_H=False)
    R.update_confidences(g, ele, w)
    H, b, _, _ = R.linearize(g)
    top = float(np.max(np.diag(H)))
    return H + 1e-5 * top * np.eye(H.shape[0]), b, top


NEGATED_EDGE = 25   # the odometry edge 25 -> 26 of d_certain


def indefinite_cases():
    """Graphs whose H + lambda I is not positive definite, all finite, so reg_pose_graph_set accepts them: two nodes with one
    certain edge of information -information(rng) (pivot 0 fails), and d_certain with the information of edge 25 -> 26 negated.
    The options are those of c_ring_wrong, so that one object can run that case after the failure."""
    rng = np.random.default_rng(61)
    truth = np.stack([np.eye(4), pose_of([0.0, 0.0, 0.4, 2.0, 0.0, 0.0])])
    poses = truth.copy()
    poses[1] = R.omm(random_pose(rng, 0.02, 0.1), truth[1])
    two = Case("n_two_negative", R.Graph(poses, [0], [1], [measurement(truth[0], truth[1])], [-information(rng)], [False]),
               option=R.Option(**_LOOSE))
    g = _certain().graph
    assert (int(g.src[NEGATED_EDGE]), int(g.tgt[NEGATED_EDGE])) == (25, 26)
    g.info[NEGATED_EDGE] = -g.info[NEGATED_EDGE]
    return [two, Case("n_certain_negated", g, option=R.Option(**_LOOSE))]
