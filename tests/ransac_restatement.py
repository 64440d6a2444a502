"""A numpy restatement of the RANSAC-on-correspondences contract of include/o3dslam_reg.h (reg_ransac_correspondences;
DESIGN.md 5q): the counter-based sampler in vectorised uint64 arithmetic, the four per-iteration rules with np.linalg.svd
for the rigid fit, the inlier count and err2 in the contract's chunked order, and the sequential best / stop rule.  It is
the reference of tests/test_gpu_ransac.py and reports, next to the result, how far every comparison stayed from its
border (the precondition tests/test_ransac_host.py asserts)."""
import numpy as np

CHUNK = 1024            # kRsChunk of csrc/kernels_ransac.hpp: the summation order of err2 is part of the contract
DEGENERATE = 1e-12      # sigma_2 <= DEGENERATE * sigma_1: status -3
_M64 = (1 << 64) - 1
_G, _A, _B = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def draw_scalar(seed, ctr, K):
    """The sampler in Python integers, one draw (the definition the vectorised form is tested against)."""
    z = (seed + (ctr + 1) * _G) & _M64
    z = ((z ^ (z >> 30)) * _A) & _M64
    z = ((z ^ (z >> 27)) * _B) & _M64
    z ^= z >> 31
    return ((z >> 32) * K) >> 32


def draws(seed, i0, i1, n, K):
    """Indices of iterations i0 .. i1 - 1: (i1 - i0, n) int64."""
    with np.errstate(over="ignore"):
        ctr = np.arange(i0 * n, i1 * n, dtype=np.uint64)
        z = np.uint64(seed & _M64) + (ctr + np.uint64(1)) * np.uint64(_G)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_A)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_B)
        z = z ^ (z >> np.uint64(31))
        idx = ((z >> np.uint64(32)) * np.uint64(K)) >> np.uint64(32)
    return idx.astype(np.int64).reshape(-1, n)


def _norm(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _rel(a, b):
    """Distance of the comparison a <> b from its border, relative to b.  b == 0 counts as inf: a zero here is an exact zero
    (the distance between twice the same point, a product with it) on the device as in numpy, and so is its comparison."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b != 0, np.abs(a - b) / np.abs(b), np.inf)


def fit(S, T):
    """Rigid fits of I samples (I, n, 3) -> (R (I, 3, 3), t (I, 3), sigma (I, 3)); means and H in slot order."""
    n = S.shape[1]
    sm, tm = S[:, 0].copy(), T[:, 0].copy()
    for j in range(1, n):
        sm, tm = sm + S[:, j], tm + T[:, j]
    sm, tm = sm / float(n), tm / float(n)
    H = np.zeros((S.shape[0], 3, 3))
    for j in range(n):
        H = H + (S[:, j] - sm)[:, :, None] * (T[:, j] - tm)[:, None, :]
    U, sig, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, 1, 2)))
    d[d == 0] = 1.0
    D = np.zeros_like(H)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = V @ D @ np.swapaxes(U, 1, 2)
    t = tm - ((R[:, :, 0] * sm[:, None, 0] + R[:, :, 1] * sm[:, None, 1]) + R[:, :, 2] * sm[:, None, 2])
    return R, t, sig


def transform(R, t, s):
    """p = R s + t in the contract's order; R (.., 3, 3), t (.., 3), s broadcastable (.., 3)."""
    return np.stack([((R[..., r, 0] * s[..., 0] + R[..., r, 1] * s[..., 1]) + R[..., r, 2] * s[..., 2]) + t[..., r]
                     for r in range(3)], axis=-1)


def evaluate(R, t, P, maxd):
    """Inlier counts, err2 (chunked order) and the inlier mask of hypotheses (H, 3, 3), (H, 3) over P (K, 6)."""
    p = transform(R[:, None], t[:, None], P[None, :, :3])
    d = p - P[None, :, 3:]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    lim = maxd * maxd
    inl = d2 < lim
    w = np.where(inl, d2, 0.0)
    err2 = None
    for c0 in range(0, P.shape[0], CHUNK):
        part = np.cumsum(w[:, c0:c0 + CHUNK], axis=1)[:, -1]          # strictly sequential, ascending k
        err2 = part if err2 is None else err2 + part
    return inl.sum(axis=1).astype(np.int64), err2, inl, float(_rel(d2, lim).min()) if d2.size else np.inf


def statuses(P, idx, dist_thr, edge_sim, maxd):
    """Status of every sampled iteration (rules -1 .. -4; survivors get their inlier count), the survivors' fits and the
    margins of every comparison made."""
    I, n = idx.shape
    st = np.zeros(I, np.int64)
    S, T = P[idx, :3], P[idx, 3:]
    margin = {"edge": np.inf, "degenerate": np.inf, "distance": np.inf, "inlier": np.inf, "sigma_ratio": np.inf}
    srt = np.sort(idx, axis=1)
    st[(srt[:, 1:] == srt[:, :-1]).any(axis=1)] = -1
    if edge_sim > 0:
        live = st == 0
        fail = np.zeros(I, bool)
        for u in range(n):
            for v in range(u + 1, n):
                ds, dt = _norm(S[:, u] - S[:, v]), _norm(T[:, u] - T[:, v])
                fail |= (ds < dt * edge_sim) | (dt < ds * edge_sim)
                if live.any():
                    margin["edge"] = min(margin["edge"], float(_rel(ds, dt * edge_sim)[live].min()),
                                         float(_rel(dt, ds * edge_sim)[live].min()))
        st[live & fail] = -2
    live = np.nonzero(st == 0)[0]
    R, t, sig = fit(S[live], T[live])
    deg = sig[:, 1] <= DEGENERATE * sig[:, 0]
    if live.size:
        margin["degenerate"] = float(_rel(sig[:, 1], DEGENERATE * sig[:, 0]).min())
    st[live[deg]] = -3
    live, R, t, sig = live[~deg], R[~deg], t[~deg], sig[~deg]
    if dist_thr > 0 and live.size:
        d = transform(R[:, None], t[:, None], S[live]) - T[live]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        lim = dist_thr * dist_thr
        margin["distance"] = float(_rel(d2, lim).min())
        bad = (d2 > lim).any(axis=1)
        st[live[bad]] = -4
        live, R, t, sig = live[~bad], R[~bad], t[~bad], sig[~bad]
    cnt = err2 = np.zeros(0)
    if live.size:
        margin["sigma_ratio"] = float((sig[:, 1] / sig[:, 0]).min())
        cnt, err2, _, margin["inlier"] = evaluate(R, t, P, maxd)
        st[live] = cnt
    return st, live, R, t, cnt, err2, margin


def est_k_update(est_k, confidence, count, K, n):
    """The stop rule after a replacement: (new est_k, the quotient before truncation).  A quotient that is not >= 0 -- NaN
    from -inf / -inf at confidence 1 with count == K, -inf from a denominator that rounded to log(1) = 0 -- changes
    nothing."""
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.log(np.float64(1.0) - np.float64(confidence)) / np.log(np.float64(1.0) - np.float64(count / K) ** n)
    if x >= 0 and np.trunc(x) < est_k:
        return float(np.trunc(x)), float(x)
    return est_k, float(x)


def ransac(src, tgt, corres, maxd, n=3, max_iteration=100000, confidence=0.999, dist_thr=0.0, edge_sim=0.0, seed=0,
           block=8192):
    """The whole contract.  Returns a dict with the outputs of reg_ransac_correspondences plus `margin` (the smallest
    relative distance of any comparison from its border, per kind; `est_k_frac`, `err2_tie`) -- every iteration before the
    stop index takes part."""
    src, tgt = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    K = corres.shape[0]
    out = {"T": np.eye(4), "fitness": 0.0, "inlier_rmse": 0.0, "inliers": np.zeros((0, 2), np.int32), "n_iterations": 0,
           "n_validated": 0, "best_iteration": -1, "iter_status": np.zeros(0, np.int32), "margin": {}}
    if K < n:
        return out
    P = np.concatenate([src[corres[:, 0]], tgt[corres[:, 1]]], axis=1)
    margin = {"edge": np.inf, "degenerate": np.inf, "distance": np.inf, "inlier": np.inf, "sigma_ratio": np.inf,
              "est_k_frac": np.inf, "err2_tie": np.inf}
    est_k, best = float(max_iteration), None        # best: (count, err2, iteration, R, t, sample)
    status, stop, i0 = [], None, 0
    while stop is None:
        i1 = min(i0 + block, max_iteration)
        idx = draws(seed, i0, i1, n, K)
        st, live, R, t, cnt, err2, mg = statuses(P, idx, dist_thr, edge_sim, maxd)
        upto = i1                                   # iterations of this block that are run
        for j, li in enumerate(live):
            i = i0 + int(li)
            if i >= est_k:
                break
            if cnt[j] <= 0:
                continue
            if best is not None and cnt[j] == best[0] and not np.array_equal(idx[li], best[5]):
                margin["err2_tie"] = min(margin["err2_tie"], float(_rel(err2[j], best[1])))
            if best is None or cnt[j] > best[0] or (cnt[j] == best[0] and err2[j] < best[1]):
                best = (int(cnt[j]), float(err2[j]), i, R[j], t[j], idx[li].copy())
                est_k, x = est_k_update(est_k, confidence, best[0], K, n)
                if np.isfinite(x) and x != 0.0:     # 0 = finite / -inf is exact in every libm
                    margin["est_k_frac"] = min(margin["est_k_frac"], float(min(x - np.floor(x), np.ceil(x) - x)))
        if est_k <= i1:
            stop = int(max(est_k, (best[2] + 1) if best is not None else 0, i0))
            upto = stop
        # margins are taken over the whole block: a superset of the iterations that ran
        for k_, v in mg.items():
            margin[k_] = min(margin[k_], v)
        status.append(st[:upto - i0])
        i0 = i1
    status = np.concatenate(status).astype(np.int32)
    out.update(n_iterations=stop, n_validated=int((status >= 0).sum()), iter_status=status, margin=margin)
    if best is not None:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = best[3], best[4]
        _, _, inl, _ = evaluate(best[3][None], best[4][None], P, maxd)
        out.update(T=T, fitness=best[0] / K, inlier_rmse=float(np.sqrt(best[1] / best[0])), best_iteration=best[2],
                   inliers=corres[inl[0]].astype(np.int32))
    return out
