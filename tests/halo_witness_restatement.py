"""Restatement in numpy of the witness points of the halo directory (kernels_build.hpp: the arg-min that
k_halo_gap_x / _y and k_halo_dir carry along, k_halo_rep, k_halo_witness).

An empty halo bin B names one real reference point: the representative of L, the nearest bin that has a run.
  * L minimises the squared whole-bin gap S1 = sum over the axes of max(|d| - 1, 0)^2 over the bins with a run inside the
    window the passes look at (|dx| <= R + 1, |dy| <= R, |dz| <= R).  Ties: axis by axis in the order z, y, x, the smallest
    |d| and, between -d and +d, the negative offset.
  * The representative of a bin is the listed point nearest the centre of the bin's box (float32, one rounding per
    operation), ties by the smallest sorted position.  The sort order of the device is not restated: a tie is reported, and
    the tests accept either point there.
The bound's S1 (halo_bound_restatement.py) is this S1 capped at R^2."""
import numpy as np

from halo_bound_restatement import F, HaloGrid, bin_coord

NONE = 1 << 40   # "no bin with a run in the window" (sums of gaps stay far below it)


def window_R(grid: HaloGrid, max_dist):
    return int(min(64.0, np.floor(float(F(max_dist) * grid.inv)) + 2.0))


def _shift(a, axis, d, fill):
    """out[i] = a[i + d] along `axis`, `fill` where i + d leaves the grid"""
    out = np.full(a.shape, fill, a.dtype)
    n = a.shape[axis]
    lo, hi = max(0, -d), min(n, n - d)
    if lo < hi:
        dst = [slice(None)] * 3
        src = [slice(None)] * 3
        dst[axis] = slice(lo, hi)
        src[axis] = slice(lo + d, hi + d)
        out[tuple(dst)] = a[tuple(src)]
    return out


def nearest_run_bin(listing, R):
    """Per bin [z, y, x]: (S1 uncapped, dz, dy, dx) of the nearest bin with a run under the tie rule; S1 == NONE: none in the
    window.  Three separable passes, each walking d upwards and replacing its choice only on a strictly smaller (S, |d|)."""
    shape = listing.shape
    S = np.where(listing, 0, NONE).astype(np.int64)
    off = {a: np.zeros(shape, np.int64) for a in (2, 1, 0)}
    for axis, reach in ((2, R + 1), (1, R), (0, R)):
        best = np.full(shape, NONE, np.int64)
        best_d = np.zeros(shape, np.int64)
        carried = {a: np.zeros(shape, np.int64) for a in (2, 1, 0) if a > axis}
        for d in range(-reach, reach + 1):
            g = max(abs(d) - 1, 0)
            src = _shift(S, axis, d, NONE)
            cand = np.where(src == NONE, NONE, src + g * g)
            better = (cand < best) | ((cand == best) & (cand != NONE) & (abs(d) < np.abs(best_d)))
            best = np.where(better, cand, best)
            best_d = np.where(better, d, best_d)
            for a in carried:
                carried[a] = np.where(better, _shift(off[a], axis, d, 0), carried[a])
        S = best
        off[axis] = best_d
        for a in carried:
            off[a] = carried[a]
    return S, off[0], off[1], off[2]


def listed_pairs(grid: HaloGrid, tgt_c):
    """(point, bin) pairs of the runs: every point with each bin whose box, grown by r_ins, contains it (halo_range)."""
    tgt_c = np.asarray(tgt_c, F)
    lo = [np.clip(bin_coord((tgt_c[:, k] - grid.r_ins).astype(F), grid.o[k], grid.inv), 0, grid.dims[k] - 1).astype(np.int64)
          for k in range(3)]
    hi = [np.clip(bin_coord((tgt_c[:, k] + grid.r_ins).astype(F), grid.o[k], grid.inv), 0, grid.dims[k] - 1).astype(np.int64)
          for k in range(3)]
    span = [int((hi[k] - lo[k]).max()) for k in range(3)]
    pts, bins = [], []
    for dz in range(span[2] + 1):
        for dy in range(span[1] + 1):
            for dx in range(span[0] + 1):
                ok = (lo[0] + dx <= hi[0]) & (lo[1] + dy <= hi[1]) & (lo[2] + dz <= hi[2])
                i = np.flatnonzero(ok)
                pts.append(i)
                bins.append(np.stack([lo[0][i] + dx, lo[1][i] + dy, lo[2][i] + dz], axis=1))
    return np.concatenate(pts), np.concatenate(bins)


def centre_d2(grid: HaloGrid, xyz, bins):
    """squared distance (float32, the kernel's order of operations) of points to the centres of `bins` (n x 3, x y z)"""
    d2 = None
    parts = []
    for k in range(3):
        c = (F(grid.o[k]) + ((bins[:, k].astype(F) + F(0.5)).astype(F) * grid.ch).astype(F)).astype(F)
        d = (xyz[:, k].astype(F) - c).astype(F)
        parts.append((d * d).astype(F))
    d2 = (parts[0] + parts[1]).astype(F)
    return (d2 + parts[2]).astype(F)


def representatives(grid: HaloGrid, tgt_c):
    """Per bin [z, y, x]: original index of the representative of its run (-1: no run), and whether another listed point is
    exactly as near the centre (then the device's choice depends on its sort order)."""
    tgt_c = np.asarray(tgt_c, F)
    pts, bins = listed_pairs(grid, tgt_c)
    d2 = centre_d2(grid, tgt_c[pts], bins)
    lin = (bins[:, 2] * grid.dims[1] + bins[:, 1]) * grid.dims[0] + bins[:, 0]
    order = np.lexsort((pts, d2, lin))
    lin, pts, d2 = lin[order], pts[order], d2[order]
    first = np.flatnonzero(np.concatenate([[True], lin[1:] != lin[:-1]]))
    nb = int(np.prod(grid.dims))
    rep = np.full(nb, -1, np.int64)
    tied = np.zeros(nb, bool)
    rep[lin[first]] = pts[first]
    nxt = np.minimum(first + 1, lin.size - 1)
    tied[lin[first]] = (nxt != first) & (lin[nxt] == lin[first]) & (d2[nxt] == d2[first])
    shape = tuple(grid.dims[::-1])
    return rep.reshape(shape), tied.reshape(shape)


def witness_table(grid: HaloGrid, tgt_c, max_dist):
    """Per bin [z, y, x]: witness as an original index (-1: none, -2: the bin has a run), whether it is subject to a tie of
    the representative, the uncapped S1 of its bin (NONE: none) and the offsets (dz, dy, dx) of L; plus R."""
    R = window_R(grid, max_dist)
    listing = grid.listing(tgt_c)
    S1, dz, dy, dx = nearest_run_bin(listing, R)
    rep, tied = representatives(grid, tgt_c)
    z, y, x = np.indices(listing.shape)
    has = S1 != NONE
    Lz, Ly, Lx = np.where(has, z + dz, 0), np.where(has, y + dy, 0), np.where(has, x + dx, 0)
    wit = np.where(has, rep[Lz, Ly, Lx], -1)
    wit = np.where(listing, -2, wit)
    wtied = np.where(has & ~listing, tied[Lz, Ly, Lx], False)
    return wit, wtied, np.where(listing, 0, S1), (dz, dy, dx), R


def gap2_between(b_from, b_to):
    """squared whole-bin gap between bins (n x 3 integer coordinates each)"""
    g = np.maximum(np.abs(np.asarray(b_to, np.int64) - np.asarray(b_from, np.int64)) - 1, 0)
    return (g * g).sum(axis=1)


def brute_nearest_run(listing, b, R):
    """Brute force over the window of bin b = (x, y, z): (smallest S1, set of (dz, dy, dx) that reach it), or (NONE, [])."""
    dimz, dimy, dimx = listing.shape
    x, y, z = (int(v) for v in b)
    x0, x1 = max(0, x - R - 1), min(dimx - 1, x + R + 1)
    y0, y1 = max(0, y - R), min(dimy - 1, y + R)
    z0, z1 = max(0, z - R), min(dimz - 1, z + R)
    sub = listing[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1]
    if not sub.any():
        return NONE, []
    zz, yy, xx = np.nonzero(sub)
    dz, dy, dx = zz + z0 - z, yy + y0 - y, xx + x0 - x
    S = (np.maximum(np.abs(dz) - 1, 0) ** 2 + np.maximum(np.abs(dy) - 1, 0) ** 2 + np.maximum(np.abs(dx) - 1, 0) ** 2)
    m = S.min()
    k = np.flatnonzero(S == m)
    return int(m), list(zip(dz[k].tolist(), dy[k].tolist(), dx[k].tolist()))


def tie_rule_pick(cands):
    """the stated tie rule among offsets (dz, dy, dx) of equal S1"""
    return min(cands, key=lambda d: (abs(d[0]), d[0], abs(d[1]), d[1], abs(d[2]), d[2]))
