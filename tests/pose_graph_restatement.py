"""numpy restatement of the pose-graph contract of include/o3dslam_reg.h: Open3D's GlobalOptimization
(Levenberg-Marquardt with line processes, prune, second pass, reference compensation) as o3d_slam::OptimizationProblem::solve
runs it.  Open3D 0.15.1 is not vendored, so this file restates the issue's text, not Open3D's source: parity with Open3D is
unpinned.  The per-edge code follows the header's operation order (every product and sum written out, no BLAS call), so it is
comparable bit for bit with the library; H is dense; the linear solver is a parameter."""
import math

import numpy as np

STOP_NONE, STOP_RIGHT_TERM, STOP_INCREMENT, STOP_RESIDUAL_INCREMENT, STOP_MAX_ITERATION_LM, STOP_MIN_RESIDUAL, \
    STOP_MAX_ITERATION = range(7)


def omm(A, B):
    """(..., m, k) x (..., k, n), every entry summed left to right over k, one rounding per operation."""
    acc = A[..., :, 0, None] * B[..., None, 0, :]
    for k in range(1, A.shape[-1]):
        acc = acc + A[..., :, k, None] * B[..., None, k, :]
    return acc


def rigid_inverse(T):
    T = np.asarray(T, np.float64)
    O = np.zeros_like(T)
    R, t = T[..., :3, :3], T[..., :3, 3]
    O[..., :3, :3] = np.swapaxes(R, -1, -2)
    r = R[..., 0, :] * t[..., 0, None]
    r = r + R[..., 1, :] * t[..., 1, None]
    r = r + R[..., 2, :] * t[..., 2, None]
    O[..., :3, 3] = -r
    O[..., 3, 3] = 1.0
    return O


def lin6(M):
    return np.stack([(M[..., 2, 1] - M[..., 1, 2]) * 0.5, (M[..., 0, 2] - M[..., 2, 0]) * 0.5,
                     (M[..., 1, 0] - M[..., 0, 1]) * 0.5, M[..., 0, 3], M[..., 1, 3], M[..., 2, 3]], axis=-1)


def generator(k, sign=1.0):
    G = np.zeros((4, 4))
    if k == 0:
        G[1, 2], G[2, 1] = -sign, sign
    elif k == 1:
        G[0, 2], G[2, 0] = sign, -sign
    elif k == 2:
        G[0, 1], G[1, 0] = -sign, sign
    else:
        G[k - 3, 3] = sign
    return G


def edge_terms(Ts, Tt, X, want_jacobians=True):
    """zeta (..., 6) and Js, Jt (..., 6, 6; row = component of zeta, column = generator) of edges given as stacks."""
    A = omm(rigid_inverse(X), rigid_inverse(Tt))
    zeta = lin6(omm(A, Ts))
    if not want_jacobians:
        return zeta, None, None
    J = []
    for sign in (1.0, -1.0):
        cols = [lin6(omm(omm(A, np.broadcast_to(generator(k, sign), A.shape)), Ts)) for k in range(6)]
        J.append(np.stack(cols, axis=-1))
    return zeta, J[0], J[1]


def edge_records(Ts, Tt, X, info):
    """zeta, e^T L e, the four blocks (ss, st, ts, tt) and the two vectors (s, t), in the header's order."""
    zeta, Js, Jt = edge_terms(Ts, Tt, X)
    Ws, Wt = omm(info, Js), omm(info, Jt)
    v = omm(info, zeta[..., None])
    JsT, JtT = np.swapaxes(Js, -1, -2), np.swapaxes(Jt, -1, -2)
    blocks = [omm(JsT, Ws), omm(JsT, Wt), omm(JtT, Ws), omm(JtT, Wt)]
    vecs = [omm(JsT, v)[..., 0], omm(JtT, v)[..., 0]]
    ele = omm(zeta[..., None, :], v)[..., 0, 0]
    return zeta, ele, blocks, vecs


def edge_costs(Ts, Tt, X, info):
    zeta, _, _ = edge_terms(Ts, Tt, X, want_jacobians=False)
    v = omm(info, zeta[..., None])
    return zeta, omm(zeta[..., None, :], v)[..., 0, 0]


def pose_step(d, pose):
    sa, ca, sb, cb, sg, cg = math.sin(d[0]), math.cos(d[0]), math.sin(d[1]), math.cos(d[1]), math.sin(d[2]), math.cos(d[2])
    V = np.array([[cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa, d[3]],
                  [sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa, d[4]],
                  [-sb, cb * sa, cb * ca, d[5]],
                  [0.0, 0.0, 0.0, 1.0]])
    return omm(V, np.asarray(pose, np.float64))


def pose_vector(T):
    sy = math.sqrt(T[0, 0] * T[0, 0] + T[1, 0] * T[1, 0])
    if sy >= 1e-6:
        r = [math.atan2(T[2, 1], T[2, 2]), math.atan2(-T[2, 0], sy), math.atan2(T[1, 0], T[0, 0])]
    else:
        r = [math.atan2(-T[1, 2], T[1, 1]), math.atan2(-T[2, 0], sy), 0.0]
    return np.array(r + [T[0, 3], T[1, 3], T[2, 3]])


def line_process_weight(info, preference, max_correspondence_distance):
    n = len(info)
    if n == 0:
        return 0.0
    s = 0.0
    for e in range(n):
        s = s + float(info[e][5, 5])
    return (preference * (max_correspondence_distance * max_correspondence_distance)) * (s / float(n))


class Option:
    def __init__(self, max_correspondence_distance=10.0, preference_loop_closure=2.0, edge_prune_threshold=0.2,
                 reference_node=0):
        self.max_correspondence_distance = max_correspondence_distance
        self.preference_loop_closure = preference_loop_closure
        self.edge_prune_threshold = edge_prune_threshold
        self.reference_node = reference_node


class Criteria:
    def __init__(self, max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                 min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0,
                 lower_scale_factor=1.0 / 3.0):
        self.max_iteration = max_iteration
        self.min_relative_increment = min_relative_increment
        self.min_relative_residual_increment = min_relative_residual_increment
        self.min_right_term = min_right_term
        self.min_residual = min_residual
        self.max_iteration_lm = max_iteration_lm
        self.upper_scale_factor = upper_scale_factor
        self.lower_scale_factor = lower_scale_factor


class Graph:
    """poses (n, 4, 4); per edge src, tgt, X (E, 4, 4), info (E, 6, 6), uncertain, confidence."""

    def __init__(self, poses, src, tgt, X, info, uncertain, confidence=None):
        self.poses = np.array(poses, np.float64).reshape(-1, 4, 4)
        self.src = np.array(src, np.int32).reshape(-1)
        self.tgt = np.array(tgt, np.int32).reshape(-1)
        E = self.src.shape[0]
        self.X = np.array(X, np.float64).reshape(E, 4, 4)
        self.info = np.array(info, np.float64).reshape(E, 6, 6)
        self.uncertain = np.array(uncertain, bool).reshape(E)
        self.confidence = np.ones(E) if confidence is None else np.array(confidence, np.float64).reshape(E)

    @property
    def n(self):
        return self.poses.shape[0]

    @property
    def E(self):
        return self.src.shape[0]

    def copy(self):
        return Graph(self.poses, self.src, self.tgt, self.X, self.info, self.uncertain, self.confidence)

    def pruned(self, threshold):
        keep = ~self.uncertain | (self.confidence > threshold)
        return Graph(self.poses, self.src[keep], self.tgt[keep], self.X[keep], self.info[keep], self.uncertain[keep],
                     self.confidence[keep])


def residual_of(ele, conf, w):
    r = 0.0
    for e in range(len(ele)):
        l = float(conf[e])
        s = math.sqrt(l) - 1.0
        r = r + (l * float(ele[e]) + w * (s * s))
    return r


def linearize(g, w=None, want_H=True):
    """Dense H (6n x 6n), b, zeta, e^T L e at the graph's poses and confidences; sums in edge order."""
    n, E = g.n, g.E
    H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    if E == 0:
        return H, b, np.zeros((0, 6)), np.zeros(0)
    zeta, ele, blocks, vecs = edge_records(g.poses[g.src], g.poses[g.tgt], g.X, g.info)
    for e in range(E):
        s, t, l = 6 * int(g.src[e]), 6 * int(g.tgt[e]), g.confidence[e]
        if want_H:
            H[s:s + 6, s:s + 6] = H[s:s + 6, s:s + 6] + l * blocks[0][e]
            H[s:s + 6, t:t + 6] = H[s:s + 6, t:t + 6] + l * blocks[1][e]
            H[t:t + 6, s:s + 6] = H[t:t + 6, s:s + 6] + l * blocks[2][e]
            H[t:t + 6, t:t + 6] = H[t:t + 6, t:t + 6] + l * blocks[3][e]
        b[s:s + 6] = b[s:s + 6] - l * vecs[0][e]
        b[t:t + 6] = b[t:t + 6] - l * vecs[1][e]
    return H, b, zeta, ele


def update_confidences(g, ele, w):
    for e in range(g.E):
        if g.uncertain[e]:
            r = w / (w + float(ele[e]))
            g.confidence[e] = r * r


def solve_numpy(A, b):
    return np.linalg.solve(A, b)


def solve_cho(A, b):
    import scipy.linalg
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), b)


def solve_longdouble(A, b):
    """An unblocked Cholesky and the two substitutions in np.longdouble, rounded to double at the end."""
    n = A.shape[0]
    L = np.tril(np.array(A, np.longdouble))
    for j in range(n):   # left-looking: column j takes the columns before it in one product
        if j:
            L[j:, j] = L[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] = L[j + 1:, j] / L[j, j]
    y = np.array(b, np.longdouble)
    for j in range(n):
        y[j] = y[j] / L[j, j]
        y[j + 1:] = y[j + 1:] - L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] = y[j] / L[j, j]
        y[:j] = y[:j] - L[j, :j] * y[j]
    return np.array(y, np.float64)


def first_bad_pivot(A):
    """(row, pivots) of the unblocked long-double Cholesky of A's lower triangle: the first row whose pivot is not positive
    and finite (-1: none) and the pivots up to and including it."""
    n = A.shape[0]
    L = np.tril(np.array(A, np.longdouble))
    pivots = []
    for j in range(n):
        if j:
            L[j:, j] = L[j:, j] - L[j:, :j] @ L[j, :j]
        pivots.append(float(L[j, j]))
        if not (L[j, j] > 0 and L[j, j] < np.inf):
            return j, pivots
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] = L[j + 1:, j] / L[j, j]
    return -1, pivots


SOLVERS = {"numpy": solve_numpy, "cho": solve_cho, "longdouble": solve_longdouble}


def lm_pass(g, option, criteria, solver=solve_numpy):
    """One Levenberg-Marquardt pass, in place on g.  Returns the statistics; `decisions` lists every test as
    (name, left, right, outcome) for the precondition check, `trace` the accept / reject sequence."""
    c = criteria
    n = g.n
    w = line_process_weight(g.info, option.preference_loop_closure, option.max_correspondence_distance)
    decisions, trace = [], []

    def test(name, left, right):
        out = left < right
        decisions.append((name, float(left), float(right), bool(out)))
        return out

    def pose_vec():
        return np.concatenate([pose_vector(g.poses[i]) for i in range(n)])

    _, _, zeta, ele = linearize(g, want_H=False)
    current = residual_of(ele, g.confidence, w)
    first = current
    update_confidences(g, ele, w)
    H, b, _, _ = linearize(g)
    x = pose_vec()
    lam, nu = 1e-5 * float(np.max(np.diag(H))), 2.0
    stop = STOP_RIGHT_TERM if test("right_term", float(np.max(b)), c.min_right_term) else STOP_NONE
    solves = accepted = outer = 0
    it = 0
    while not stop:
        outer += 1
        lm_count = 0
        while True:
            delta = solver(H + lam * np.eye(6 * n), b)
            solves += 1
            nd, nx = math.sqrt(float(np.dot(delta, delta))), math.sqrt(float(np.dot(x, x)))
            if test("increment", nd, c.min_relative_increment * (nx + c.min_relative_increment)):
                stop = STOP_INCREMENT
                break
            trial = np.stack([pose_step(delta[6 * i:6 * i + 6], g.poses[i]) for i in range(n)])
            if g.E:
                zeta_t, ele_t = edge_costs(trial[g.src], trial[g.tgt], g.X, g.info)
            else:
                zeta_t, ele_t = np.zeros((0, 6)), np.zeros(0)
            new = residual_of(ele_t, g.confidence, w)
            rho = (current - new) / (float(np.dot(delta, lam * delta + b)) + 1e-3)
            decisions.append(("rho", float(rho), 0.0, bool(rho > 0.0)))
            trace.append(bool(rho > 0.0))
            if rho > 0.0:
                if test("residual_increment", current - new, c.min_relative_residual_increment * current):
                    stop = STOP_RESIDUAL_INCREMENT
                    break
                lam *= max(c.lower_scale_factor, min(c.upper_scale_factor, 1.0 - (2.0 * rho - 1.0) ** 3))
                nu = 2.0
                g.poses, zeta, ele, current = trial, zeta_t, ele_t, new
                accepted += 1
                x = pose_vec()
                update_confidences(g, ele, w)
                H, b, _, _ = linearize(g)
                if test("right_term", float(np.max(b)), c.min_right_term):
                    stop = STOP_RIGHT_TERM
                    break
            else:
                lam *= nu
                nu *= 2.0
            lm_count += 1
            if lm_count >= c.max_iteration_lm:
                stop = STOP_MAX_ITERATION_LM
            if rho > 0.0 or stop:
                break
        if stop:
            break
        if test("min_residual", current, c.min_residual):
            stop = STOP_MIN_RESIDUAL
        elif it >= c.max_iteration:
            stop = STOP_MAX_ITERATION
        it += 1
    valid = int(np.sum(g.confidence > option.edge_prune_threshold))
    return dict(outer_iterations=outer, lm_solves=solves, accepted_steps=accepted, stop_reason=stop, valid_edges=valid,
                first_residual=first, last_residual=current, last_lambda=lam, weight=w, decisions=decisions, trace=trace)


def global_optimization(graph, option=None, criteria=None, solver=solve_numpy):
    """GlobalOptimization: returns (the optimised, pruned, compensated graph, [pass 1 statistics, pass 2 statistics])."""
    option = option or Option()
    criteria = criteria or Criteria()
    g = graph.copy()
    r1 = lm_pass(g, option, criteria, solver)
    g = g.pruned(option.edge_prune_threshold)
    r2 = lm_pass(g, option, criteria, solver)
    g = g.pruned(option.edge_prune_threshold)
    ref = option.reference_node
    if 0 <= ref < g.n:
        C = omm(graph.poses[ref], rigid_inverse(g.poses[ref]))
        g.poses = np.stack([omm(C, g.poses[i]) for i in range(g.n)])
    return g, [r1, r2]


def decision_margin(d):
    """How far a decision is from its border: |rho| for the sign test of rho (rho is a ratio of order one: the actual over
    the predicted reduction), |left - right| / max(|left|, |right|) for every threshold test."""
    name, left, right, _ = d
    if name == "rho":
        return abs(left)
    m = max(abs(left), abs(right))
    return abs(left - right) / m if m > 0 else 0.0
