"""Restatement in numpy of the empty-space bound of the halo directory (kernels_build.hpp:
k_halo_insert's occupancy bits, k_halo_gap_x / _y, k_halo_dir) and of the geometry of the halo grid (host_target.hpp:
build_halo), for the CPU test of the bound's argument and for placing test positions on bin borders.

lb(B) is a lower bound on the distance from ANY position that the bin function maps to halo bin B to ANY reference point.
With g = max(|d| - 1, 0) whole bins per axis between B and B + (dx, dy, dz):
  (a) a reference point inside that bin is at least c_h |g| away;
  (b) every reference point is listed by each bin whose box it is within rho_h of, so with S the smallest |g|^2 over the bins
      that list anything, it is at least c_h sqrt(S) + rho_h away (walk from the point towards B by less than rho_h: still
      inside a listing bin, and that much closer)."""
import numpy as np

F = np.float32


def bin_coord(v, o, inv):
    """bin_coord_f: floor(fl(fl(v - o) * inv)), one rounding per operation, as float32."""
    d = (np.asarray(v, F) - F(o)).astype(F)
    return np.floor((d * F(inv)).astype(F))


class HaloGrid:
    """Halo grid of a centred float32 cloud for halo-bin edge `ch` (= halo_ratio x the bin edge)."""

    def __init__(self, tgt_c, ch):
        tgt_c = np.asarray(tgt_c, F)
        self.o = tgt_c.min(axis=0)
        self.bmax = tgt_c.max(axis=0)
        self.ch = F(ch)
        self.inv = F(1.0) / F(ch)
        self.dims = np.array([int(np.floor(float(F(self.bmax[k] - self.o[k])) * float(self.inv))) + 1 for k in range(3)])
        self.max_abs = float(max(np.abs(self.o).max(), np.abs(self.bmax).max()))
        self.abs_margin = F(4e-7) * (F(1.0) + F(self.max_abs))
        self.rho_h = F(0.4) * self.ch * (F(1.0) - F(4e-3)) - F(2.0) * self.abs_margin
        self.r_ins = self.rho_h + F(1e-3) * self.rho_h + self.abs_margin

    def bins(self, pos):
        """(integer bin coordinates n x 3, inside mask) of float32 positions, unclamped."""
        pos = np.asarray(pos, F)
        b = np.stack([bin_coord(pos[:, k], self.o[k], self.inv) for k in range(3)], axis=1)
        inside = np.all((b >= 0) & (b < self.dims[None, :]), axis=1)
        return b.astype(np.int64), inside

    def occupancy(self, tgt_c):
        b, _ = self.bins(tgt_c)
        b = np.clip(b, 0, self.dims[None, :] - 1)
        occ = np.zeros(self.dims[::-1], bool)   # [z, y, x]
        occ[b[:, 2], b[:, 1], b[:, 0]] = True
        return occ


    def listing(self, tgt_c):
        """Bins whose run is non-empty: a point is listed in every bin whose box, grown by r_ins, contains it (halo_range)."""
        tgt_c = np.asarray(tgt_c, F)
        lo = [np.clip(bin_coord((tgt_c[:, k] - self.r_ins).astype(F), self.o[k], self.inv), 0, self.dims[k] - 1).astype(np.int64)
              for k in range(3)]
        hi = [np.clip(bin_coord((tgt_c[:, k] + self.r_ins).astype(F), self.o[k], self.inv), 0, self.dims[k] - 1).astype(np.int64)
              for k in range(3)]
        n = np.zeros(self.dims[::-1], bool)
        span = [int((hi[k] - lo[k]).max()) for k in range(3)]
        for dz in range(span[2] + 1):
            for dy in range(span[1] + 1):
                for dx in range(span[0] + 1):
                    n[np.minimum(lo[2] + dz, hi[2]), np.minimum(lo[1] + dy, hi[1]), np.minimum(lo[0] + dx, hi[0])] = True
        return n


def _gap_pass(S, axis, R):
    """min over d in [-R, R] of max(|d| - 1, 0)^2 + S shifted by d along `axis` (bins outside the grid hold no point)."""
    out = np.full(S.shape, R * R, np.int64)
    n = S.shape[axis]
    for d in range(-R, R + 1):
        g = max(abs(d) - 1, 0)
        lo, hi = max(0, -d), min(n, n - d)   # destination range whose source lo + d .. hi + d lies inside
        if lo >= hi:
            continue
        dst = [slice(None)] * 3
        src = [slice(None)] * 3
        dst[axis] = slice(lo, hi)
        src[axis] = slice(lo + d, hi + d)
        out[tuple(dst)] = np.minimum(out[tuple(dst)], S[tuple(src)] + g * g)
    return out


def _gap2(mask, R):
    """per bin: the smallest |g|^2 over the bins of `mask`, capped at R^2"""
    S = np.where(mask, 0, R * R).astype(np.int64)
    for axis in (2, 1, 0):
        S = _gap_pass(S, axis, R)
    return np.minimum(S, R * R)


def bound_table(grid: HaloGrid, occ, listing, max_dist):
    """lb per bin [z, y, x] (float32 metres) from the bins that hold a point (`occ`) and the bins that list one (`listing`);
    the device keeps it only for bins whose own run is empty."""
    R = int(min(64.0, np.floor(float(F(max_dist) * grid.inv)) + 2.0))
    S0, S1 = _gap2(occ, R), _gap2(listing, R)
    eps_bins = F(grid.dims.max()) * F(1.0 / 2097152.0)
    down = F(1.0) - F(1e-3)
    g0 = (np.sqrt(S0.astype(F)) * down - F(3.5) * eps_bins).astype(F)
    g1 = (np.sqrt(S1.astype(F)) * down - F(3.5) * eps_bins).astype(F)
    lb0 = (g0 * grid.ch - F(2.0) * grid.abs_margin).astype(F)
    lb1 = np.where(S1 > 0, (g1 * grid.ch + grid.rho_h * down - F(2.0) * grid.abs_margin).astype(F), F(0.0))
    lb = np.maximum(np.maximum(lb0, lb1), F(0.0)).astype(F)
    return np.where(listing, F(0.0), lb), R


def border_positions(grid: HaloGrid, rng, n):
    """Positions on (and one float step either side of) bin borders and the faces of the grid."""
    k = np.stack([rng.integers(0, grid.dims[a] + 1, n) for a in range(3)], axis=1)
    p = (grid.o[None, :] + k.astype(F) * grid.ch).astype(F)
    free = rng.random((n, 3)) < 0.5        # per axis: on a border, or anywhere
    anyw = (grid.o[None, :] + (rng.random((n, 3)) * (grid.bmax - grid.o)[None, :])).astype(F)
    p = np.where(free, anyw, p).astype(F)
    step = rng.integers(-1, 2, (n, 3))
    p = np.where(step < 0, np.nextafter(p, F(-np.inf)), np.where(step > 0, np.nextafter(p, F(np.inf)), p)).astype(F)
    return p
