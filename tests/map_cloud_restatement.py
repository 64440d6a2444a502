"""A literal Python restatement of the map cloud's contract (include/o3dslam_reg.h): Submap::insertScan, carve,
transform and centre on plain numpy rows.  Dicts keyed by integer triples, float64 scalars, sequential sums; one rounding
per operation (numpy's elementwise operators and Python floats are IEEE doubles without contraction).  The voxelisation, the
carve and the voxel down-sampling are the existing restatements (oracle.voxelize_within_volume, oracle.carve_indices,
scanprep_restatement.voxel_down_sample); what is added here is their refusals, the order of the steps and the state."""
import numpy as np

from oracle import oracle as orc
from tests import map_rows_cases as M
from tests import scanprep_restatement as S

LIMIT = 1 << 20        # voxel indices lie within +-(2^20 - 1)


class Refused(ValueError):
    """REG_BAD_ARGUMENT found on the data: the map must be left as it was."""


def transform_point(T, p):
    """w = ((T30 x + T31 y) + T32 z) + T33; x' = (((T00 x + T01 y) + T02 z) + T03) / w.  On the device: xform_point;
    transform_normal and transform_cov below: xform_dir, xform_cov (csrc/kernels_cloud64.hpp)."""
    x, y, z = (np.float64(v) for v in p)
    with np.errstate(invalid="ignore"):        # 0 * inf and NaN rows pass through as the arithmetic leaves them
        w = ((T[3, 0] * x + T[3, 1] * y) + T[3, 2] * z) + T[3, 3]
        return np.array([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]) / w for r in range(3)], np.float64)


def transform_normal(T, n):
    """(T (n, 0)).head<3>(): (T00 nx + T01 ny) + T02 nz"""
    x, y, z = (np.float64(v) for v in n)
    return np.array([(T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z for r in range(3)], np.float64)


def transform_cov(T, c9):
    """R C R^T with C(r, c) at 3 c + r: M = R C, M(r, c) = (R(r,0) C(0,c) + R(r,1) C(1,c)) + R(r,2) C(2,c); then
    C'(r, c) = (M(r,0) R(c,0) + M(r,1) R(c,1)) + M(r,2) R(c,2)."""
    C = lambda r, c: np.float64(c9[3 * c + r])
    out = np.empty(9, np.float64)
    for r in range(3):
        Mr = [(T[r, 0] * C(0, c) + T[r, 1] * C(1, c)) + T[r, 2] * C(2, c) for c in range(3)]
        for c in range(3):
            out[3 * c + r] = (Mr[0] * T[c, 0] + Mr[1] * T[c, 1]) + Mr[2] * T[c, 2]
    return out


def transform_cloud(T, xyz, normals=None, covs=None):
    T = np.asarray(T, np.float64)
    x = np.array([transform_point(T, p) for p in xyz], np.float64).reshape(-1, 3)
    n = None if normals is None else np.array([transform_normal(T, v) for v in normals], np.float64).reshape(-1, 3)
    c = None if covs is None else np.array([transform_cov(T, v) for v in np.asarray(covs).reshape(-1, 9)]).reshape(-1, 9)
    return x, n, c


def center(xyz):
    """GetCenter: the sequential sum of the rows in order, divided by n; zero for an empty cloud."""
    c = np.zeros(3, np.float64)
    for p in np.asarray(xyz, np.float64).reshape(-1, 3):
        c = c + p
    return c / np.float64(len(xyz)) if len(xyz) else c


def check_keys(xyz, mask, voxel, what):
    """The refusal of k_vox_classify (vox_index / vox_fits of csrc/kernels_cloud64.hpp): a row inside the
    volume whose index floor(p * (1 / voxel)) is not within +-(2^20 - 1) on every axis (a non-finite coordinate included)."""
    inv = np.float64(1.0) / np.float64(voxel)
    for p in np.asarray(xyz, np.float64)[mask]:
        for c in p:
            with np.errstate(invalid="ignore"):
                k = np.floor(c * inv)
            if not abs(k) < LIMIT:
                raise Refused(what)


def volume_at(crop, c):
    return None if crop is None else dict(crop, center=tuple(float(v) for v in c))


class MapCloud:
    """Submap::mapCloud_ with mapBuilderCropper_'s pose and nScansInsertedMap_."""

    def __init__(self, map_voxel=0.03, crop=None, carve_voxel=0.1, max_ray=20.0, truncation=0.1, min_dot=0.5, every=10,
                 has_normals=True, has_covs=False):
        self.map_voxel, self.crop = map_voxel, crop
        self.carve = dict(voxel_size=carve_voxel, max_ray=max_ray, truncation=truncation, min_dot=min_dot)
        self.every, self.has_normals, self.has_covs = every, has_normals, has_covs
        self.center = np.array((crop or {}).get("center", (0.0, 0.0, 0.0)), np.float64)
        self.scans = 0
        self.xyz = np.zeros((0, 3))
        self.nrm = np.zeros((0, 3)) if has_normals else None
        self.cov = np.zeros((0, 9)) if has_covs else None
        self.last_removed = None       # map rows the last carve removed (ascending)

    def _fields(self, nrm, cov):
        if (nrm is not None) != self.has_normals or (cov is not None) != self.has_covs:
            raise Refused("fields")

    def set(self, xyz, nrm=None, cov=None, voxel=0.0):
        self._fields(nrm, cov)
        if voxel > 0:
            try:
                self.xyz, self.nrm, self.cov = S.voxel_down_sample(xyz, voxel, nrm, cov)
            except ValueError as e:
                raise Refused(str(e)) from None
        else:
            self.xyz = np.array(xyz, np.float64).reshape(-1, 3)
            self.nrm = None if nrm is None else np.array(nrm, np.float64).reshape(-1, 3)
            self.cov = None if cov is None else np.array(cov, np.float64).reshape(-1, 9)

    def carve_due(self, perform):
        return bool(perform) and len(self.xyz) > 0 and self.scans % self.every == 1

    def insert_scan(self, raw, xyz, T, nrm=None, cov=None, perform_carving=True, carve_at_new_pose=False):
        """Returns dict(carved, n_carved, n_outside, n_voxels, n_rows); Refused leaves the object untouched.
        carve_at_new_pose: what the reference would do if setPose came before the carve -- only for showing that the two
        volumes differ on a case."""
        T = np.asarray(T, np.float64)
        self._fields(nrm, cov)
        if len(xyz) == 0:
            return dict(carved=0, n_carved=0, n_outside=0, n_voxels=0, n_rows=len(self.xyz))
        tx, tn, tc = transform_cloud(T, xyz, nrm, cov)
        mx, mn, mc = self.xyz, self.nrm, self.cov
        carved, removed = self.carve_due(perform_carving), np.zeros(0, np.int32)
        if carved and raw is not None and len(raw):
            rays = transform_cloud(T, raw)[0]                                  # the whole raw scan, not de-duplicated
            subset = M.mask_of(mx, volume_at(self.crop, T[:3, 3] if carve_at_new_pose else self.center))   # the PREVIOUS pose
            check_keys(mx, subset, self.carve["voxel_size"], "carve: key range")
            removed = orc.carve_indices(mx, rays, T[:3, 3], map_normals=mn, subset_mask=subset, **self.carve)
            keep = np.ones(len(mx), bool)
            keep[removed] = False
            mx, mn, mc = mx[keep], None if mn is None else mn[keep], None if mc is None else mc[keep]
        cat = lambda a, b: None if a is None else np.concatenate([a, b])
        cx, cn, cc = cat(mx, tx), cat(mn, tn), cat(mc, tc)
        new_center = T[:3, 3].copy()
        inside = M.mask_of(cx, volume_at(self.crop, new_center))
        if self.map_voxel > 0:
            check_keys(cx, inside, self.map_voxel, "voxelise: key range")
        ox, on, oc, n_outside = orc.voxelize_within_volume(cx, self.map_voxel, inside, cn, cc)
        self.xyz, self.nrm, self.cov = ox, on, oc
        self.center, self.scans, self.last_removed = new_center, self.scans + 1, removed
        return dict(carved=int(carved), n_carved=len(removed), n_outside=int(n_outside), n_voxels=len(ox) - int(n_outside),
                    n_rows=len(ox))

    def transform(self, T):
        self.xyz, self.nrm, self.cov = transform_cloud(T, self.xyz, self.nrm, self.cov)

    def get_center(self):
        return center(self.xyz)
