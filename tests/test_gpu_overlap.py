"""Voxel-overlap selection and the submap-pair constraint front on the device against the numpy restatement
(tests/overlap_restatement.py) and against the host path.

Bars: index lists, counts and order are exact (integer work on fp64 keys; every random input is first checked to keep
1e-9 away from a voxel face, so one differing rounding cannot move a point); a registration after
`reg_set_pair_overlap_f64` is the one `reg_set_target` + `reg_set_source` give on the host-selected, host-cast fp32 clouds
bit for bit (the same fp32 arrays reach the same code: derived, no tolerance)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from open3d_slam_private_amd import capi, icp, synth
from tests import overlap_restatement as R

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, EMPTY_TARGET, MISSING_FIELD = 6, 1, 7
MARGIN = 1e-9


def _reg():
    p = capi.default_params()
    p.cost = capi.COST_O3D_P2P
    return capi.Registration(p)


def _assert_margin(src, tgt, T, voxel):
    """A failing assertion here is a bug of the test's inputs, not of the device code."""
    assert R.integer_margin(R.transform_points(src, T), voxel) > MARGIN
    assert R.integer_margin(tgt, voxel) > MARGIN


def _check(reg, src, tgt, T, voxel, k, T_device="same"):
    want = R.overlap_indices(src, tgt, T, voxel, k)
    got = reg.overlap_indices(src, tgt, voxel, T if T_device == "same" else T_device, k)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert got[0].size == want[0].size and got[1].size == want[1].size
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return want


@functools.lru_cache(maxsize=None)
def _random_case():
    rng = np.random.default_rng(5)
    src, tgt = rng.uniform(-3, 3, size=(4096, 3)), rng.uniform(-3, 3, size=(5000, 3))
    T = R.rpy_transform(2.0, -3.0, 25.0, (0.3, -0.2, 0.1))
    _assert_margin(src, tgt, T, 0.5)
    _assert_margin(src, tgt, None, 0.5)
    for a in (src, tgt, T):
        a.setflags(write=False)
    return src, tgt, T


@pytest.mark.parametrize("k,want_counts", [(1, (3288, 3941)), (2, (2474, 2706)), (3, (1293, 1319))])
def test_random_clouds_under_a_transform(k, want_counts):
    src, tgt, T = _random_case()
    want = _check(_reg(), src, tgt, T, 0.5, k)
    assert (want[0].size, want[1].size) == want_counts


def test_random_clouds_at_identity_and_with_a_null_transform():
    src, tgt, _ = _random_case()
    reg = _reg()
    a = _check(reg, src, tgt, np.eye(4), 0.5, 1)
    b = _check(reg, src, tgt, None, 0.5, 1)
    assert (a[0].size, a[1].size) == (3888, 4546) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _check(reg, src, tgt, np.eye(4), 0.5, 1, T_device=None)              # identity through the formula == no transform pass


def test_single_points_and_empty_clouds():
    reg = _reg()
    p = np.array([[0.3, 0.3, 0.3]])
    assert [list(x) for x in _check(reg, p, p + 0.1, None, 0.5, 1)] == [[0], [0]]
    assert [x.size for x in _check(reg, p, p + 0.5, None, 0.5, 1)] == [0, 0]      # different voxels: REG_OK, 0 / 0
    assert [x.size for x in reg.overlap_indices(p[:0], p, 0.5)] == [0, 0]         # n = 0
    assert [x.size for x in reg.overlap_indices(p, p[:0], 0.5)] == [0, 0]         # m = 0
    assert [list(x) for x in _check(reg, p, p, None, 0.5, 1)] == [[0], [0]]       # and the handle still works


@pytest.mark.parametrize("n", [255, 256, 257])
def test_one_point_per_voxel_across_a_block_edge(n):
    rng = np.random.default_rng(n)
    cells = np.stack([np.arange(n) % 7, (np.arange(n) // 7) % 7, np.arange(n) // 49], axis=1) - 3.0
    src = (cells + rng.uniform(0.1, 0.9, size=(n, 3))) * 0.5
    tgt = (cells[::-1] + rng.uniform(0.1, 0.9, size=(n, 3))) * 0.5
    tgt[::3] += 100.0                                                          # every third target voxel has no source point
    _assert_margin(src, tgt, None, 0.5)
    want = _check(_reg(), src, tgt, None, 0.5, 1)
    assert want[0].size == want[1].size == n - len(range(0, n, 3))
    assert [x.size for x in _check(_reg(), src, tgt, None, 0.5, 2)] == [0, 0]


def test_many_points_in_one_voxel():
    rng = np.random.default_rng(3)
    src, tgt = rng.uniform(0.05, 0.45, size=(257, 3)) - 0.5, rng.uniform(0.05, 0.45, size=(257, 3)) - 0.5
    _assert_margin(src, tgt, None, 0.5)
    reg = _reg()
    for k in (1, 257):
        want = _check(reg, src, tgt, None, 0.5, k)
        assert np.array_equal(want[0], np.arange(257)) and np.array_equal(want[1], np.arange(257))
    assert [x.size for x in _check(reg, src, tgt, None, 0.5, 258)] == [0, 0]


@pytest.mark.parametrize("voxel", [0.25, 0.5])
def test_points_on_voxel_faces(voxel):
    """Lattice points exactly on the faces, negative coordinates included: multiples of 0.25 / 0.5 times the exact 4.0 / 2.0 are
    exact, so floor() decides alone (-0.5 -> voxel -1 at 0.5)."""
    src, tgt = R.face_lattice(voxel)
    want = _check(_reg(), src, tgt, None, voxel, 1)
    assert 0 < want[1].size < tgt.shape[0]


def test_layers_of_different_sizes():
    src, tgt, T = _random_case()
    reg = _reg()
    for s, t in ((src[:100], tgt), (src, tgt[:100])):
        want = _check(reg, s, t, T, 0.5, 1)
        assert 0 < want[0].size and 0 < want[1].size


def test_invalid_input_is_refused_and_the_handle_survives():
    src, tgt, T = _random_case()
    reg = _reg()

    def refused(s, t, voxel=0.5, k=1, Tm=None):
        with pytest.raises(capi.RegError) as e:
            reg.overlap_indices(s, t, voxel, Tm, k)
        assert e.value.status == BAD_ARGUMENT
        _check(reg, src[:300], tgt[:300], T, 0.5, 1)                      # a valid call on the same handle

    def with_value(a, v):
        b = a[:500].copy()
        b[123, 1] = v
        return b

    refused(with_value(src, 0.5 * (1 << 20) + 1.0), tgt)                  # key past 2^20
    refused(src, with_value(tgt, -0.5 * (1 << 20) - 1.0))
    for v in (np.nan, np.inf, -np.inf):
        refused(with_value(src, v), tgt)
        refused(src, with_value(tgt, v))
    far = np.eye(4)
    far[0, 3] = 1e6
    refused(src, tgt, Tm=far)                                             # the TRANSFORMED source leaves the key range
    refused(src, tgt, voxel=0.0)
    refused(src, tgt, voxel=float("inf"))
    refused(src, tgt, k=0)


def test_host_and_device_pointers_agree():
    src, tgt, T = _random_case()
    d_s, d_t = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(tgt.copy()).cuda()
    d_si = torch.full((src.shape[0],), -1, dtype=torch.int32, device="cuda")
    d_ti = torch.full((tgt.shape[0],), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    reg = _reg()
    host = reg.overlap_indices(src, tgt, 0.5, T, 2)
    ns, nt = reg.overlap_indices_device(d_s.data_ptr(), src.shape[0], d_t.data_ptr(), tgt.shape[0], 0.5, d_si.data_ptr(),
                                        d_ti.data_ptr(), T, 2)
    torch.cuda.synchronize()
    assert (ns, nt) == (host[0].size, host[1].size) == (2474, 2706)
    assert np.array_equal(d_si.cpu().numpy()[:ns], host[0]) and np.array_equal(d_ti.cpu().numpy()[:nt], host[1])
    assert np.all(d_si.cpu().numpy()[ns:] == -1) and np.all(d_ti.cpu().numpy()[nt:] == -1)   # nothing written past the counts


# ---- reg_set_pair_overlap_f64 against the host path -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    sc = synth.make_scene(3000, 40000, seed=8)
    s64, t64 = sc.src_xyz.astype(np.float64), sc.tgt_xyz.astype(np.float64)
    _assert_margin(s64, t64, None, 1.0)
    si, ti = R.overlap_indices(s64, t64, None, 1.0, 1)
    assert 0 < ti.size < t64.shape[0] and 0 < si.size <= s64.shape[0]     # the map extends beyond the scan: points are dropped
    return sc, s64, t64, si, ti


def _c9(c6):
    return np.ascontiguousarray(c6.astype(np.float64)[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]])


def _registered(reg):
    T, res = reg.register(np.eye(4))
    ids, d2, w = reg.correspondences()
    info, n_pairs = reg.information_matrix(T, 0.5)
    return T, res.iterations, ids, d2.view(np.uint32), w, info, n_pairs


def _assert_same_registration(a, b):
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]                    # pose, iteration count
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])   # ids, d2 bits, weights
    assert np.array_equal(a[5], b[5]) and a[6] == b[6] and a[6] > 0       # all 36 doubles of the information matrix, n_pairs


def test_pair_front_registers_like_the_host_path_point_to_plane():
    sc, s64, t64, si, ti = _scene()
    reg = capi.Registration(capi.shipped_params())
    kept = reg.set_pair_overlap_f64(s64, t64, 1.0, None, 1, src_normals=sc.src_nrm.astype(np.float64),
                                    tgt_normals=sc.tgt_nrm.astype(np.float64))
    assert kept == (si.size, ti.size) and 0 < kept[1] < t64.shape[0]
    assert np.array_equal(reg.target_source_indices(), ti) and np.array_equal(reg.source_source_indices(), si)
    ref = capi.Registration(capi.shipped_params())
    ref.set_target(t64[ti].astype(np.float32), sc.tgt_nrm[ti])
    ref.set_source(s64[si].astype(np.float32), sc.src_nrm[si])
    _assert_same_registration(_registered(reg), _registered(ref))
    # device pointers: the same selection, the same registration
    arrs = [torch.from_numpy(a.astype(np.float64)).cuda() for a in (s64, sc.src_nrm, t64, sc.tgt_nrm)]
    torch.cuda.synchronize()
    dev = capi.Registration(capi.shipped_params())
    assert dev.set_pair_overlap_f64_device(arrs[0].data_ptr(), s64.shape[0], arrs[2].data_ptr(), t64.shape[0], 1.0,
                                           src_nrm_ptr=arrs[1].data_ptr(), tgt_nrm_ptr=arrs[3].data_ptr()) == kept
    assert np.array_equal(dev.target_source_indices(), ti) and np.array_equal(dev.source_source_indices(), si)
    _assert_same_registration(_registered(dev), _registered(ref))
    # the index maps go with the entry point that made them
    reg.set_source(sc.src_xyz, sc.src_nrm)
    with pytest.raises(capi.RegError):
        reg.source_source_indices()
    assert np.array_equal(reg.target_source_indices(), ti)
    reg.set_target(sc.tgt_xyz, sc.tgt_nrm)
    with pytest.raises(capi.RegError):
        reg.target_source_indices()


def test_pair_front_registers_like_the_host_path_gicp():
    sc, s64, t64, si, ti = _scene()
    p = capi.default_params()
    p.cost = capi.COST_GICP
    p.use_trimmed = 0
    p.max_dist = 0.5
    reg = capi.Registration(p)
    T = R.rpy_transform(0.3, -0.2, 0.5, (0.05, -0.03, 0.02))
    _assert_margin(s64, t64, T, 1.0)
    si, ti = R.overlap_indices(s64, t64, T, 1.0, 1)
    kept = reg.set_pair_overlap_f64(s64, t64, 1.0, T, 1, src_covs=_c9(sc.src_cov), tgt_covs=_c9(sc.tgt_cov))
    assert kept == (si.size, ti.size) and 0 < kept[1] < t64.shape[0]
    assert np.array_equal(reg.target_source_indices(), ti) and np.array_equal(reg.source_source_indices(), si)
    ref = capi.Registration(p)
    ref.set_target(t64[ti].astype(np.float32), None, sc.tgt_cov[ti])
    ref.set_source(s64[si].astype(np.float32), None, sc.src_cov[si])
    _assert_same_registration(_registered(reg), _registered(ref))


def test_pair_front_empty_overlap_and_missing_fields():
    sc, s64, t64, _, _ = _scene()
    nrm_s, nrm_t = sc.src_nrm.astype(np.float64), sc.tgt_nrm.astype(np.float64)
    reg = capi.Registration(capi.shipped_params())

    def status(*a, **kw):
        with pytest.raises(capi.RegError) as e:
            reg.set_pair_overlap_f64(*a, **kw)
        return e.value.status

    assert status(s64 + 1000.0, t64, 1.0, src_normals=nrm_s, tgt_normals=nrm_t) == EMPTY_TARGET
    assert (reg.n_source_kept, reg.n_target_kept) == (0, 0)
    assert status(s64[:0], t64, 1.0, src_normals=nrm_s[:0], tgt_normals=nrm_t) == EMPTY_TARGET
    assert status(s64, t64, 1.0, src_normals=nrm_s) == MISSING_FIELD                 # point-to-plane: reference normals
    assert status(s64, t64, 1.0, tgt_normals=nrm_t) == MISSING_FIELD                 # SurfaceNormalOutlierFilter: reading normals
    assert status(s64, t64, 0.0, src_normals=nrm_s, tgt_normals=nrm_t) == BAD_ARGUMENT
    assert status(s64, t64, 1.0, None, 0, src_normals=nrm_s, tgt_normals=nrm_t) == BAD_ARGUMENT
    with pytest.raises(capi.RegError):                                               # nothing is left registered after a refusal
        reg.register(np.eye(4))
    p = capi.default_params()
    p.cost = capi.COST_GICP
    p.use_trimmed = 0
    g = capi.Registration(p)
    with pytest.raises(capi.RegError) as e:
        g.set_pair_overlap_f64(s64, t64, 1.0, tgt_covs=_c9(sc.tgt_cov))
    assert e.value.status == MISSING_FIELD
    assert reg.set_pair_overlap_f64(s64, t64, 1.0, src_normals=nrm_s, tgt_normals=nrm_t)[1] > 0   # the handle still works


# ---- buildConstraint / refineLoopClosure ------------------------------------------------------------------------------------
def _clouds():
    sc, s64, t64, si, ti = _scene()
    return icp.DataPoints(sc.src_xyz), icp.DataPoints(sc.tgt_xyz, normals=sc.tgt_nrm)


def _host_info(p, source, target, T, max_dist):
    reg = capi.Registration(p)
    reg.set_target(target.features, target.normals if p.cost == capi.COST_O3D_P2PL else None, target.covariances)
    reg.set_source(source.features, None, source.covariances)
    return reg.information_matrix(T, max_dist)[0]


def _assert_same_result(a, b):
    assert np.array_equal(a.transformation_, b.transformation_)
    assert a.fitness_ == b.fitness_ and a.inlier_rmse_ == b.inlier_rmse_
    assert np.array_equal(a.correspondence_set_, b.correspondence_set_) and a.correspondence_set_.shape[0] > 0


@pytest.mark.parametrize("overlap", [True, False])
def test_build_constraint_equals_the_operators_on_host_selected_clouds(overlap):
    sc, s64, t64, si, ti = _scene()
    source, target = _clouds()
    c, res = icp.buildConstraint(source, target, isComputeOverlap=overlap, icpMaxCorrespondenceDistance=0.5,
                                 voxelSizeOverlapCompute=1.0, isEstimateInformationMatrix=True, isSkipIcpRefinement=False,
                                 sourceIdx=3, targetIdx=4, withResult=True)
    hs = icp.DataPoints(sc.src_xyz[si]) if overlap else source
    ht = icp.DataPoints(sc.tgt_xyz[ti], normals=sc.tgt_nrm[ti]) if overlap else target
    op = icp.RegistrationIcpPointToPlane(0.5, 100)
    want = op.registerClouds(hs, ht, np.eye(4))
    _assert_same_result(res, want)
    assert np.array_equal(c.sourceToTarget_, want.transformation_)
    assert np.array_equal(c.informationMatrix_, _host_info(op.params(), hs, ht, want.transformation_, 0.5))
    assert (c.sourceSubmapIdx_, c.targetSubmapIdx_, c.isInformationMatrixValid_, c.isOdometryConstraint_) == (3, 4, True, True)
    assert not np.array_equal(c.sourceToTarget_, np.eye(4))


def test_build_constraint_without_refinement_and_without_information_matrix():
    sc, s64, t64, si, ti = _scene()
    source, target = _clouds()
    kw = dict(isComputeOverlap=True, icpMaxCorrespondenceDistance=0.5, voxelSizeOverlapCompute=1.0)
    c = icp.buildConstraint(source, target, isEstimateInformationMatrix=True, isSkipIcpRefinement=True, **kw)
    assert np.array_equal(c.sourceToTarget_, np.eye(4)) and c.isInformationMatrixValid_
    hs, ht = icp.DataPoints(sc.src_xyz[si]), icp.DataPoints(sc.tgt_xyz[ti], normals=sc.tgt_nrm[ti])
    op = icp.RegistrationIcpPointToPlane(0.5, 100)
    want = _host_info(op.params(), hs, ht, np.eye(4), 0.5)
    assert np.array_equal(c.informationMatrix_, want) and not np.array_equal(want, np.eye(6))
    c = icp.buildConstraint(source, target, isEstimateInformationMatrix=False, isSkipIcpRefinement=False, **kw)
    assert np.array_equal(c.informationMatrix_, np.eye(6)) and not c.isInformationMatrixValid_
    assert np.array_equal(c.sourceToTarget_, op.registerClouds(hs, ht, np.eye(4)).transformation_)


@pytest.mark.parametrize("kind", ["PointToPlaneIcp", "PointToPointIcp", "GeneralizedIcp"])
def test_refine_loop_closure_equals_the_operator_on_host_selected_clouds(kind):
    sc, s64, t64, _, _ = _scene()
    source, target = _clouds()
    source.covariances, target.covariances = sc.src_cov, sc.tgt_cov
    T0 = R.rpy_transform(0.1, -0.1, 0.2, (0.03, -0.02, 0.01)) @ sc.T_true     # a coarse alignment, as RANSAC would leave it
    _assert_margin(s64, t64, T0, 1.0)
    si, ti = R.overlap_indices(s64, t64, T0, 1.0, 1)
    op = icp.cloudRegistrationFactory(kind, maxCorrespondenceDistance_=0.5, maxNumIter_=30)
    c, res = icp.refineLoopClosure(source, target, T0, op, 1.0, 0.4, sourceIdx=7, targetIdx=2)
    hs = icp.DataPoints(sc.src_xyz[si], covariances=sc.src_cov[si])
    ht = icp.DataPoints(sc.tgt_xyz[ti], normals=sc.tgt_nrm[ti], covariances=sc.tgt_cov[ti])
    want = op.registerClouds(hs, ht, T0)
    _assert_same_result(res, want)
    assert np.array_equal(c.sourceToTarget_, want.transformation_) and res.fitness_ > 0.0
    p = op.params()
    if p.cost != capi.COST_GICP:
        hs.covariances = ht.covariances = None
    assert np.array_equal(c.informationMatrix_, _host_info(p, hs, ht, want.transformation_, 0.4))
    assert (c.sourceSubmapIdx_, c.targetSubmapIdx_, c.isInformationMatrixValid_, c.isOdometryConstraint_) == (7, 2, True, False)
    got = icp.computeIndicesOfOverlappingPoints(source, target, T0, 1.0, 1)
    assert np.array_equal(got[0], si) and np.array_equal(got[1], ti)


# ---- cleanup ----------------------------------------------------------------------------------------------------------------
def _free_bytes():
    hip = C.CDLL("libamdhip64.so.7")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_destroy_returns_the_workspace():
    capi.load_library()
    rng = np.random.default_rng(4)
    src, tgt = rng.uniform(-20, 20, size=(400_000, 3)), rng.uniform(-20, 20, size=(400_000, 3))

    def one():
        r = _reg()
        r.overlap_indices(src, tgt, 1.6)
        r.set_pair_overlap_f64(src, tgt, 1.6)
        r.source_source_indices()
        r.close()

    one()
    free0 = _free_bytes()
    for _ in range(4):
        one()
    assert free0 - _free_bytes() < 32 * 2**20
