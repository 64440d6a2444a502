"""CPU restatement of MinDist, MedianDist and VarTrimmedDist outlier filters on top of tests/pm_chain_restatement.py (a
plain helper module, not a test).  Contract: include/o3dslam_reg.h (reg_pm_chain), DESIGN.md 5i.

All three act on the N x knn squared distances (+inf = no match) and multiply into the chain's weight:
  MinDist        w = [d2 >= f32(minDist) * f32(minDist)]
  MedianDist     w = [d2 <= f32(factor) * q], q = the finite distances' order statistic at int(f32(n_finite) * f32(0.5))
  VarTrimmedDist n = every entry; v = sorted finite entries > 0, m = |v|; candidates j in [floor(f32(minRatio) f32(n)),
                 min(floor(f32(maxRatio) f32(n)), m)); FRMS(j) = S(j) / (j + 1) / ((j + 1) / n)^(2 lambda) in fp64, S the
                 fp64 running sum of v; k = the first minimiser (m - 1 when the range is empty); optRatio = f32(k) / f32(n);
                 limit = the finite distances' (zeros included) order statistic at quantile_index(n_finite, optRatio).
`fork_rank` restates the reference's own arithmetic (fp32 sequential running sum, fp32 objective) for comparison."""
import numpy as np

from tests.pm_chain_restatement import Chain, PmRestatement, quantile_index

f32 = np.float32
REL = 1e-12   # near-optimality margin of a reported rank: covers another order of the fp64 additions only


class OutlierChain(Chain):
    """Chain + min_dist / median_factor / var_trim = (minRatio, maxRatio, lambda); None = filter off."""

    def __init__(self, min_dist=None, median_factor=None, var_trim=None, **kw):
        super().__init__(**kw)
        self.min_dist, self.median_factor, self.var_trim = min_dist, median_factor, var_trim


def var_range(n, m, min_ratio, max_ratio):
    lo = int(np.floor(f32(min_ratio) * f32(n)))
    hi = int(np.floor(f32(max_ratio) * f32(n)))
    return lo, min(hi, m)


def var_objective(d2, min_ratio, max_ratio, lam):
    """(lo, hi, m, FRMS over [lo, hi) in fp64) for the distances d2 (any shape)."""
    d = np.asarray(d2, f32).ravel()
    n = d.size
    v = np.sort(d[np.isfinite(d) & (d > 0)])
    lo, hi = var_range(n, v.size, min_ratio, max_ratio)
    if lo >= hi:
        return lo, hi, v.size, np.empty(0)
    S = np.cumsum(v[:hi].astype(np.float64))[lo:]
    ids = np.arange(lo + 1, hi + 1, dtype=np.float64)
    return lo, hi, v.size, S / ids / np.power(ids / np.float64(n), 2.0 * np.float64(f32(lam)))


def var_rank(d2, min_ratio, max_ratio, lam):
    """The contract's k: the first minimiser of the fp64 objective, m - 1 for an empty range, None when m == 0."""
    lo, hi, m, F = var_objective(d2, min_ratio, max_ratio, lam)
    if m == 0:
        return None
    return m - 1 if F.size == 0 else lo + int(np.argmin(F))


def var_rank_is_near_optimal(d2, k, min_ratio, max_ratio, lam):
    """A rank reported by the host or the device: inside the candidate range with FRMS64(k) <= min FRMS64 (1 + REL), or the
    empty-range fallback.  Returns (ok, FRMS64(k) / min - 1)."""
    lo, hi, m, F = var_objective(d2, min_ratio, max_ratio, lam)
    if F.size == 0:
        return k == m - 1, 0.0
    if not lo <= k < hi:
        return False, np.inf
    fmin = F.min()
    return bool(F[k - lo] <= fmin * (1 + REL)), float(F[k - lo] / fmin - 1)


def var_limit(d2, k):
    """(optRatio, limit) from a rank k: getDistsQuantile(optRatio) over the finite distances, zeros included."""
    d = np.asarray(d2, f32).ravel()
    fin = np.sort(d[np.isfinite(d)])
    ratio = f32(k) / f32(d.size)
    return ratio, fin[quantile_index(fin.size, float(ratio))]


def fork_rank(d2, min_ratio, max_ratio, lam):
    """The reference's arithmetic on the same candidates: fp32 sequential running sum, FRMS = S * (1 / id) *
    (1 / (id / n)^lambda)^2 in fp32 (OutlierFiltersImpl.cpp:186-214), clipped to the m entries that exist."""
    d = np.asarray(d2, f32).ravel()
    n = d.size
    v = np.sort(d[np.isfinite(d) & (d > 0)])
    lo, hi = var_range(n, v.size, min_ratio, max_ratio)
    if lo >= hi:
        return None
    S = np.cumsum(v[:hi], dtype=f32)[lo:]
    ids = np.arange(lo + 1, hi + 1).astype(f32)
    deno = np.power(ids / f32(n), f32(lam)).astype(f32)
    inv = (f32(1) / deno).astype(f32)
    F = (S * (f32(1) / ids)).astype(f32) * (inv * inv).astype(f32)
    return lo + int(np.argmin(F))


class PmOutliersRestatement(PmRestatement):
    """PmRestatement with the three filters in the product.  `var_k` (when set) replaces the restatement's own argmin by a
    reported rank, so that weights can be compared bit for bit at that rank; `last_var` keeps (k, ratio, limit)."""

    var_k = None
    last_var = None

    def weights(self, T, ids, d2):
        c = self.c
        w = super().weights(T, ids, d2)
        valid = ids >= 0
        fin = d2[valid]
        if c.min_dist is not None:
            w = np.where(d2 >= f32(c.min_dist) * f32(c.min_dist), w, f32(0)).astype(f32)
        if c.median_factor is not None:
            if fin.size == 0:
                self.fail = True
            else:
                qi = quantile_index(fin.size, 0.5)
                lim = f32(c.median_factor) * np.partition(fin, qi)[qi]
                w = np.where(d2 <= lim, w, f32(0)).astype(f32)
        if c.var_trim is not None:
            k = self.var_k if self.var_k is not None else var_rank(d2, *c.var_trim)
            if k is None:
                self.fail = True
            else:
                ratio, lim = var_limit(d2, k)
                self.last_var = (k, float(ratio), float(lim))
                w = np.where(d2 <= lim, w, f32(0)).astype(f32)
        return w
