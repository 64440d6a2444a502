"""Data-point filters on the device (reg_sampling_surface_normal, reg_filter_points) against the numpy restatement
(tests/ssn_restatement.py), and libpointmatcher's data-filter ICP goldens end to end through PointMatcherICP (GPU box)."""
import ctypes as C

import numpy as np
import pytest

from open3d_slam_private_amd import capi
from open3d_slam_private_amd.icp import DataPoints, PointMatcherICP
from tests import ssn_restatement as R
from tests.test_data_filters_host import _READING, golden_case, golden_yaml, restated_golden_run
from tests.test_oracle_golden import icp_test_relative_error

pytestmark = pytest.mark.gpu
F32 = np.float32
KEEP_ALL = dict(keep_normals=1, keep_densities=1, keep_eigen_values=1, keep_eigen_vectors=1)


def _ssn(reg, xyz, knn, method=1, ratio=0.5, box=np.inf, **keep):
    p = capi.default_ssn_params()
    p.knn, p.sampling_method, p.ratio, p.max_box_dim = knn, method, ratio, box
    for k, v in keep.items():
        setattr(p, k, v)
    return reg.sampling_surface_normal(xyz, p, want_leaf_id=True)


def _check_ssn(dev, ref, eig=True):
    assert dev["n_out"] == ref["n_out"] and dev["n_unfit"] == ref["n_unfit"]
    assert np.array_equal(dev["leaf_id"], ref["leaf_id"])
    assert np.array_equal(dev["src_idx"], ref["src_idx"])
    assert np.array_equal(dev["xyz"], ref["xyz"])   # bit-exact: sequential fp32 means
    if "densities" in dev:
        np.testing.assert_allclose(dev["densities"], ref["densities"], rtol=1e-6)
    if eig and dev["n_out"]:
        # DESIGN 5b tolerances of reg_estimate_normals: 1e-6 relative on eigenvalues, normals up to rounding
        lam_ref = ref["eigvals"].astype(np.float64)
        scale = np.maximum(np.abs(lam_ref).max(axis=1, keepdims=True), 1e-30)
        assert np.all(np.abs(dev["eigvals"] - lam_ref) <= 1e-5 * scale + 1e-12)
        dot = np.abs(np.sum(dev["normals"].astype(np.float64) * ref["normals"], axis=1))
        separated = (lam_ref[:, 1] - lam_ref[:, 0]) > 1e-3 * scale[:, 0]
        assert np.all(dot[separated] > 1 - 1e-5), dot[separated].min()
        assert np.array_equal(dev["normals"][separated], ref["normals"][separated]) or \
            np.abs(dev["normals"][separated] - ref["normals"][separated]).max() < 1e-4


@pytest.fixture(scope="module")
def reg():
    r = capi.Registration(capi.default_params())
    yield r
    r.close()


def _grid_cloud():
    g = np.stack(np.meshgrid(np.arange(24), np.arange(24), np.arange(12), indexing="ij"), -1).reshape(-1, 3).astype(F32)
    g = np.concatenate([g, g[::3]])   # duplicates
    g[g == 0] = -0.0                  # a mix of signed zeros
    g[::2][g[::2] == -0.0] = 0.0
    return g


@pytest.mark.parametrize("knn", [3, 10, 64])
def test_ssn_golden_cloud_matches_restatement(reg, knn):
    ref = np.load("tests/golden/cloud00000.npy")
    dev = _ssn(reg, ref, knn, **KEEP_ALL)
    want = R.sampling_surface_normal(ref, knn=knn, samplingMethod=1, keepNormals=True, keepDensities=True,
                                     keepEigenValues=True, keepEigenVectors=True)
    _check_ssn(dev, want)


def test_ssn_tie_heavy_grid_and_box_limit(reg):
    g = _grid_cloud()
    for method, ratio, box in ((1, 0.5, np.inf), (0, 1.0, np.inf), (1, 0.5, 1.5)):
        dev = _ssn(reg, g, 10, method, ratio, box, **KEEP_ALL)
        want = R.sampling_surface_normal(g, knn=10, samplingMethod=method, ratio=ratio, maxBoxDim=box,
                                         keepNormals=True, keepDensities=True, keepEigenValues=True)
        _check_ssn(dev, want)


def test_ssn_small_edge_clouds(reg):
    rng = np.random.default_rng(5)
    clouds = [np.ones((50, 3), F32), np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [6, 5, 5], [7, 6, 5]], F32),
              np.stack([rng.normal(size=120), np.zeros(120), np.zeros(120)], 1).astype(F32),
              rng.normal(size=(3, 3)).astype(F32)]
    for xyz in clouds:
        for keep in (dict(keep_normals=1), dict(keep_normals=0, keep_densities=1)):
            dev = _ssn(reg, xyz, 3, **keep)
            want = R.sampling_surface_normal(xyz, knn=3, samplingMethod=1, keepNormals=bool(keep.get("keep_normals")),
                                             keepDensities=bool(keep.get("keep_densities")))
            _check_ssn(dev, want, eig=False)


def test_ssn_one_million_point_map(reg):
    rng = np.random.default_rng(11)
    n = 1_000_000
    xyz = np.concatenate([rng.uniform(-40, 40, size=(n, 2)), rng.normal(scale=0.3, size=(n, 1))], 1).astype(F32)
    dev = _ssn(reg, xyz, 10, keep_normals=1)
    want = R.sampling_surface_normal(xyz, knn=10, samplingMethod=1)
    assert dev["n_out"] == want["n_out"] and dev["n_unfit"] == want["n_unfit"]
    assert np.array_equal(dev["leaf_id"], want["leaf_id"])
    assert np.array_equal(dev["src_idx"], want["src_idx"]) and np.array_equal(dev["xyz"], want["xyz"])
    dot = np.abs(np.sum(dev["normals"] * want["normals"], axis=1))
    assert np.quantile(dot, 0.999) > 1 - 1e-5


def _reading_cloud():
    rng = np.random.default_rng(8)
    P = rng.normal(scale=3.0, size=(20000, 3)).astype(F32)
    P[rng.random(20000) < 0.01, 1] = np.nan
    P[rng.random(20000) < 0.005, 2] = np.inf
    P[rng.random(20000) < 0.01, 0] = -0.0
    P[rng.random(20000) < 0.01, 0] = 0.0
    P[100:140, 0] = 1.0   # ties at a threshold
    return P


READING_CASES = [
    [{"type": "Identity"}], [{"type": "RemoveNaN"}],
    [{"type": "MaxDist", "dim": -1, "maxDist": 4.0}], [{"type": "MaxDist", "dim": 0, "maxDist": 1.0}],
    [{"type": "MinDist", "dim": -1, "minDist": -2.0}], [{"type": "MinDist", "dim": 2, "minDist": 0.0}],
    [{"type": "BoundingBox", "xMin": -1, "xMax": 1, "yMin": -2, "yMax": 2, "zMin": -1, "zMax": 3, "removeInside": 1}],
    [{"type": "BoundingBox", "xMin": 0.0, "xMax": 1, "removeInside": 0}],
    [{"type": "DistanceLimit", "dim": -1, "dist": 3.0, "removeInside": 0}],
    [{"type": "DistanceLimit", "dim": 1, "dist": 0.5, "removeInside": 1}],
    [{"type": "RemoveNaN"}, {"type": "MaxQuantileOnAxis", "dim": 0, "ratio": 0.72}],
    [{"type": "FixStepSampling", "startStep": 7, "phase": 3}],
    [{"type": "RemoveNaN"}, {"type": "MaxDist", "dim": -1, "maxDist": 6.0}, {"type": "MaxQuantileOnAxis", "dim": 2,
                                                                            "ratio": 0.5},
     {"type": "FixStepSampling", "startStep": 3, "phase": 2}, {"type": "MinDist", "dim": 0, "minDist": -1.0}],
]


@pytest.mark.parametrize("case", range(len(READING_CASES)))
def test_reading_filters_index_exact(reg, case):
    P = _reading_cloud()
    flt = READING_CASES[case]
    nrm = np.random.default_rng(1).normal(size=P.shape).astype(F32)
    cov = np.random.default_rng(2).normal(size=(P.shape[0], 6)).astype(F32)
    want_xyz, want_idx = R.filter_points(P, flt)
    ox, oi, on, oc = reg.filter_points(P, flt, normals=nrm, covs=cov)
    assert np.array_equal(oi, want_idx)
    assert np.array_equal(ox, want_xyz, equal_nan=True)
    assert np.array_equal(on, nrm[want_idx]) and np.array_equal(oc, cov[want_idx])


def test_quantile_on_a_nan_axis_is_refused(reg):
    with pytest.raises(capi.RegError) as e:
        reg.filter_points(_reading_cloud(), [{"type": "MaxQuantileOnAxis", "dim": 1, "ratio": 0.5}])
    assert e.value.status == 6


def test_host_and_device_pointer_paths_agree(reg):
    P = _reading_cloud()
    flt = READING_CASES[-1]
    hx, hi, _, _ = reg.filter_points(P, flt)
    n = P.shape[0]
    din, dx, di = capi.DeviceArray(P.nbytes), capi.DeviceArray(n * 12), capi.DeviceArray(n * 4)
    din.upload(P)
    m = reg.filter_points_device(din.value, 3, n, flt, dx.value, out_idx_ptr=di.value)
    assert m == hx.shape[0]
    assert np.array_equal(dx.download((m, 3)), hx, equal_nan=True) and np.array_equal(di.download(m, np.int32), hi)
    ref = np.load("tests/golden/cloud00000.npy")
    host = _ssn(reg, ref, 10, **KEEP_ALL)
    n = ref.shape[0]
    bufs = {k: capi.DeviceArray(n * w * 4) for k, w in (("in", 3), ("xyz", 3), ("nrm", 3), ("den", 1), ("eva", 3),
                                                        ("eve", 9), ("src", 1), ("lid", 1))}
    bufs["in"].upload(ref)
    p = capi.default_ssn_params()
    p.knn, p.sampling_method = 10, 1
    for k, v in KEEP_ALL.items():
        setattr(p, k, v)
    m, unfit = reg.sampling_surface_normal_device(bufs["in"].value, 3, n, p, bufs["xyz"].value, bufs["nrm"].value,
                                                  bufs["den"].value, bufs["eva"].value, bufs["eve"].value,
                                                  bufs["src"].value, bufs["lid"].value)
    assert (m, unfit) == (host["n_out"], host["n_unfit"])
    assert np.array_equal(bufs["xyz"].download((m, 3)), host["xyz"])
    assert np.array_equal(bufs["nrm"].download((m, 3)), host["normals"])
    assert np.array_equal(bufs["den"].download(m), host["densities"])
    assert np.array_equal(bufs["eva"].download((m, 3)), host["eigvals"])
    assert np.array_equal(bufs["eve"].download((m, 9)), host["eigvecs"])
    assert np.array_equal(bufs["src"].download(m, np.int32), host["src_idx"])
    assert np.array_equal(bufs["lid"].download(n, np.int32), host["leaf_id"])
    for b in bufs.values():
        b.free()


@pytest.mark.parametrize("name", sorted(_READING))
def test_golden_configs_end_to_end_on_the_device(name):
    ref, data, refT = golden_case(name)
    icp = PointMatcherICP()
    icp.loadFromYaml(golden_yaml(name))
    T = icp.compute(DataPoints(data), DataPoints(ref))
    rel = icp_test_relative_error(T, refT, data)
    assert rel < 0.05, rel                     # utest.cpp:146-159
    _, ores, _ = restated_golden_run(name)
    assert icp.last_result.iterations == ores.iterations
    assert icp.referenceFilteredCount == R.sampling_surface_normal(ref, knn=10, samplingMethod=1)["n_out"]
    want_idx = R.filter_points(data, [dict(f, phase=0) if f["type"] == "FixStepSampling" else f
                                      for f in _READING[name][1]])[1]
    assert np.array_equal(icp.readingFilteredIndices(), want_idx)


def _free_bytes():
    hip = C.CDLL("libamdhip64.so.7")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_destroy_returns_device_memory():
    capi.load_library()
    xyz = np.random.default_rng(4).normal(size=(400_000, 3)).astype(F32)

    def one():
        r = capi.Registration(capi.default_params())
        _ssn(r, xyz, 10)
        r.filter_points(xyz, [{"type": "MaxQuantileOnAxis", "dim": 0, "ratio": 0.5}])
        r.close()

    one()
    free0 = _free_bytes()
    for _ in range(4):
        one()
    assert free0 - _free_bytes() < 32 * 2**20


def test_bad_arguments_give_documented_codes(reg):
    xyz = np.random.default_rng(6).normal(size=(100, 3)).astype(F32)

    def status(fn):
        with pytest.raises(capi.RegError) as e:
            fn()
        return e.value.status

    assert status(lambda: _ssn(reg, xyz, 2)) == 6                     # knn < 3
    assert status(lambda: _ssn(reg, xyz, 65)) == 9                    # above the build's cap
    assert status(lambda: _ssn(reg, xyz, 10, 0, 0.5)) == 9            # std::rand subsampling
    bad = xyz.copy()
    bad[7, 1] = np.inf
    assert status(lambda: _ssn(reg, bad, 10)) == 6                    # non-finite input
    p = capi.default_ssn_params()
    p.struct_size = 8
    assert status(lambda: reg.sampling_surface_normal(xyz, p)) == 6   # struct_size
    assert status(lambda: reg.filter_points(xyz, [{"type": "FixStepSampling", "startStep": 3, "phase": 3}])) == 6
    assert status(lambda: reg.filter_points(xyz, [{"type": "MaxQuantileOnAxis", "dim": -1}])) == 6
    assert status(lambda: reg.filter_points(xyz, [{"type": "MaxDist", "dim": 3}])) == 6


# ---- the output paths that the calls above leave thin: absent outputs, scratch slices, zero rows, edge sizes ---------------
from tests import staged_output_cases as SO  # noqa: E402


@pytest.fixture(scope="module")
def so_reg():
    r = capi.Registration(capi.default_params())
    yield r
    r.close()


def test_ssn_output_subsets_equal_the_full_call(so_reg):
    """Each optional output alone (eigenvalues without normals among them) and none, host form, 300 points."""
    full = SO.check_subsets(so_reg, SO.OPS["ssn"](so_reg), SO.f32_inputs(300))
    assert 0 < full.counts["m"] < 300


def test_ssn_device_form_without_optional_outputs(so_reg):
    SO.check_device_without_optionals(so_reg, SO.OPS["ssn"](so_reg), SO.f32_inputs(300))


def test_ssn_writes_nothing_past_the_reported_rows(so_reg):
    SO.check_nothing_past_the_rows(so_reg, SO.OPS["ssn"](so_reg), SO.f32_inputs(300))


def test_ssn_larger_cloud_after_a_smaller_one(so_reg):
    SO.check_grown(so_reg, SO.OPS["ssn"], SO.f32_inputs)


def test_filter_points_output_subsets_equal_the_full_call(so_reg):
    full = SO.check_subsets(so_reg, SO.OPS["filter_points"](so_reg, SO.PM_CHAIN), SO.f32_inputs(300))
    assert 0 < full.counts["m"] < 300


def test_filter_points_device_form_without_optional_outputs(so_reg):
    SO.check_device_without_optionals(so_reg, SO.OPS["filter_points"](so_reg, SO.PM_CHAIN), SO.f32_inputs(300))


def test_filter_points_writes_nothing_past_the_reported_rows(so_reg):
    SO.check_nothing_past_the_rows(so_reg, SO.OPS["filter_points"](so_reg, SO.PM_CHAIN), SO.f32_inputs(300))


@pytest.mark.parametrize("form", ["host", "device"])
def test_filter_points_zero_rows_leave_the_outputs_untouched(so_reg, form):
    SO.check_zero_rows(so_reg, SO.OPS["filter_points"](so_reg, SO.BOX_OUT + SO.PM_CHAIN), SO.f32_inputs(300), form)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_filter_points_forms_agree_at_edge_sizes(so_reg, n):
    SO.check_forms_agree(so_reg, SO.OPS["filter_points"](so_reg, [{"type": "FixStepSampling", "startStep": 1}]),
                         SO.f32_inputs(n))
