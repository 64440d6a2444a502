"""numpy restatement (fp32, operation by operation) of the descriptor-carrying data-point filters under the contract of
reg_filter_cloud (include/o3dslam_reg.h): ObservationDirection, OrientNormals, Shadow, SimpleSensorNoise,
IncidenceAngle, CutAtDescriptorThreshold, MaxDensity, and the chain runner that carries every descriptor through every
compaction.  norm = sqrt((x*x + y*y) + z*z), dot = (a0*b0 + a1*b1) + a2*b2; numpy's fp32 element-wise operations round
once per operation, as the device code does without contraction."""
import numpy as np

from tests import ssn_restatement as S

F32 = np.float32
RAND_MAX = 2147483647
CREATED = {"ObservationDirection": ("observationDirections", 3), "SimpleSensorNoise": ("simpleSensorNoise", 1),
           "IncidenceAngle": ("incidenceAngles", 1)}
# (minRadius, beamAngle, beamConst), SimpleSensorNoise.cpp:87-113
LASERS = {0: (0.012, 0.0068, 0.0008), 1: (0.028, 0.0013, 0.0001), 2: (0.018, 0.0006, 0.0015), 4: (0.004, 0.0053, -0.0092)}


class MissingField(KeyError):
    """The reference's InvalidField."""


def dot3(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def norm3(a):
    return np.sqrt(dot3(a, a))


def normalized(a):
    """Eigen's normalized(): v / norm where norm > 0, else v."""
    a = np.asarray(a, F32)
    n = norm3(a)
    out = a.copy()
    pos = n > 0
    out[pos] = a[pos] / n[pos, None]
    return out


def glibc_rand(seed: int, count: int) -> np.ndarray:
    """The first `count` values of glibc's rand() after srand(seed) (random_r TYPE_3), written from the algorithm."""
    seed = seed or 1
    r = [seed]
    for i in range(1, 31):
        hi, lo = divmod(r[-1], 127773)
        w = 16807 * lo - 2836 * hi
        r.append(w + 2147483647 if w < 0 else w)
    st = r + r[:3]
    for k in range(34, 344 + count):
        st.append((st[k - 31] + st[k - 3]) & 0xffffffff)
    return np.array([v >> 1 for v in st[344:344 + count]], np.int64)


def observation_direction(xyz, x=0.0, y=0.0, z=0.0):
    return np.array([x, y, z], F32)[None, :] - np.asarray(xyz, F32)[:, :3]


def orient_normals(normals, obs, towardCenter=1):
    s = dot3(obs, normals)
    flip = (s < 0) if towardCenter else (s > 0)
    out = np.asarray(normals, F32).copy()
    out[flip] = -out[flip]
    return out


def shadow_value(xyz, normals):
    return np.abs(dot3(normalized(normals), normalized(np.asarray(xyz, F32)[:, :3])))


def shadow_threshold(eps):
    return F32(np.sin(F32(eps)))


def simple_sensor_noise(xyz, sensorType=0):
    r = norm3(np.asarray(xyz, F32)[:, :3])
    if sensorType == 3:
        return (r * r) * F32(0.5 * 0.00285)
    lo, ang, const = (F32(v) for v in LASERS[sensorType])
    return np.maximum(lo, ang * r + const)


def incidence_dot(normals, obs):
    return dot3(normalized(obs), normals)


def max_density_keep(den, maxDensity, seed=1):
    den = np.asarray(den, F32).reshape(-1)
    n = den.size
    keep = np.ones(n, bool)
    if n == 0:
        return keep
    last = den.max()
    n_sat = int((den == last).sum())
    need = den > F32(maxDensity)
    r = glibc_rand(seed, int(need.sum())).astype(F32) / F32(RAND_MAX)
    a = F32(maxDensity) / den[need]
    sat = den[need] == last
    a[sat] = a[sat] * F32(1 - n_sat // n)
    keep[need] = r < a
    return keep


def filter_cloud(xyz, filters, descriptors=None):
    """Returns (xyz m x 3, src_idx, {name: m x span}); point filters go through ssn_restatement.point_filter_keep."""
    P = np.asarray(xyz, F32)[:, :3].copy()
    D = {k: np.asarray(v, F32).reshape(P.shape[0], -1).copy() for k, v in (descriptors or {}).items()}
    idx = np.arange(P.shape[0], dtype=np.int32)

    def need(name):
        if name not in D:
            raise MissingField(name)
        return D[name]

    for f in filters:
        t = f["type"]
        keep = None
        if P.shape[0] == 0:
            break
        if t == "ObservationDirection":
            D["observationDirections"] = observation_direction(P, f.get("x", 0), f.get("y", 0), f.get("z", 0))
        elif t == "OrientNormals":
            D["normals"] = orient_normals(need("normals"), need("observationDirections"), int(f.get("towardCenter", 1)))
        elif t == "SimpleSensorNoise":
            D["simpleSensorNoise"] = simple_sensor_noise(P, int(f.get("sensorType", 0)))[:, None]
        elif t == "IncidenceAngle":
            d = incidence_dot(need("normals"), need("observationDirections"))
            D["incidenceAngles"] = np.arccos(d.astype(np.float64)).astype(F32)[:, None]
        elif t == "Shadow":
            keep = shadow_value(P, need("normals")) > shadow_threshold(f.get("eps", 0.1))
        elif t == "CutAtDescriptorThreshold":
            v, thr = need(f.get("descName", "none"))[:, 0], F32(f.get("threshold", 0))
            keep = (v <= thr) if int(f.get("useLargerThan", 1)) else (v >= thr)
        elif t == "MaxDensity":
            keep = max_density_keep(need("densities")[:, 0], f.get("maxDensity", 10), int(f.get("seed", 1)))
        elif t != "Identity":
            keep = S.point_filter_keep(P, f).astype(bool)
        if keep is not None:
            P, idx = P[keep], idx[keep]
            D = {k: v[keep] for k, v in D.items()}
    return P, idx, D


def voxel_grid(xyz, vSize=(1.0, 1.0, 1.0), descriptors=None, average=True):
    """VoxelGrid with useCentroid 1 under reg_voxel_grid's contract.  The ordered sums are vectorised by rounds: round r
    adds the r-th member (input order) of every voxel that has one, so each voxel's sum is still sequential.
    Returns (xyz m x 3, first-member indices, {name: m x span}); raises ValueError where the device returns
    REG_BAD_ARGUMENT."""
    P = np.asarray(xyz, F32)[:, :3]
    n = P.shape[0]
    D = {k: np.asarray(v, F32).reshape(n, -1) for k, v in (descriptors or {}).items()}
    if not np.isfinite(P).all():
        raise ValueError("non-finite input")
    v = np.asarray(vSize, F32)
    min_bound = P.min(axis=0) / v
    d = (F32(1) + P.max(axis=0) / v) - min_bound
    if not np.all(d < F32(4294967296.0)):
        raise ValueError("2^32 or more cells along an axis")
    nd = [int(np.uint64(np.trunc(x))) for x in d]
    if nd[0] * nd[1] * nd[2] >= 2 ** 32:
        raise ValueError("nx * ny * nz >= 2^32")
    cell = np.floor(P / v - min_bound).astype(np.int64)
    key = cell[:, 0] + cell[:, 1] * nd[0] + cell[:, 2] * nd[0] * nd[1]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(n, bool)
    head[1:] = ks[1:] != ks[:-1]
    starts = np.nonzero(head)[0]
    counts = np.diff(np.append(starts, n))
    first = order[starts]
    by_first = np.argsort(first, kind="stable")                # output rows ascending by first-member index
    starts, counts, first = starts[by_first], counts[by_first], first[by_first]

    def reduce(A, avg):
        acc = A[first].copy()
        if avg:
            for r in range(1, int(counts.max()) if counts.size else 0):
                live = counts > r
                acc[live] = acc[live] + A[order[starts[live] + r]]
            acc = acc / counts.astype(F32)[:, None]
        return acc

    return reduce(P, True), first.astype(np.int32), {k: reduce(A, average) for k, A in D.items()}
