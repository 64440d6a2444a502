"""CPU-only checks of the FPFH / feature-matching contract: hand-worked pair features and rows of the numpy
restatement (tests/fpfh_restatement.py), its neighbourhoods against the oracle's k-NN order, the two new exports and their
ctypes signatures against the header, the Python wrappers' argument validation (before any device is touched), and the
precondition the GPU tests lean on: on every input they use, the f0 bin coordinate of every pair stays 1e-9 away from the
interior bin borders (atan2 is the only operation whose last bit may differ between the device and libm)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from open3d_slam_private_amd import capi, icp
from oracle import oracle
from tests import fpfh_cases as K
from tests import fpfh_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bins(pi, ni, pj, nj):
    b = R.pair_bins(*(np.array(v, np.float32) for v in (pi, ni, pj, nj)))
    return tuple(int(v[0]) for v in b)


# ---- hand-worked pair features -----------------------------------------------------------------------------------------------
def test_neighbour_along_the_normal_and_duplicate_point_give_the_zero_feature():
    # d parallel to n1: v = d x n1 = 0, the feature is (0, 0, 0): 11 * pi / (2 pi) = 11 * 1 * 0.5 = 5.5 -> bin 5 of each third
    assert _bins((0, 0, 0), (0, 0, 1), (0, 0, 1), (0, 0, 1)) == (5, 5, 5)
    # L == 0
    assert _bins((1, 2, 3), (0, 0, 1), (1, 2, 3), (0, 1, 0)) == (5, 5, 5)
    x = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 0]], np.float32)       # point 2 is a twin of point 0
    nr = np.array([[0, 0, 1], [0, 0, 1], [0, 1, 0]], np.float32)
    out = R.compute_fpfh(x, nr, 3, 1.5)
    assert np.array_equal(np.nonzero(out["counts"][0])[0], [5, 16, 27]) and list(out["m"]) == [2, 2, 2]
    # point 0: neighbours in (d2, index) order are its twin (d2 == 0: skipped in the weighted sum) and point 1 (d2 == 1)
    assert list(out["ids"][0][:2]) == [2, 1]
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0 * 1.0 + 100.0           # acc = spfh[1] / 1, s = 100, scale = 1
    assert np.array_equal(out["fpfh"][0], want)


def test_both_outcomes_of_the_swap_and_the_tie():
    # |a1| = 0 < |a2| = 0.6: swap; n1 = (0.6, 0, 0.8), d = (-1, 0, 0), f2 = -0.6 -> 11 * 0.4 * 0.5 = 2.2;
    # v = (0, 1, 0), w = (-0.8, 0, 0.6), f1 = 0, f0 = atan2(0.6, 0.8) = 0.6435 -> 11 * 3.785 / 6.283 = 6.63
    assert _bins((0, 0, 0), (0, 0, 1), (1, 0, 0), (0.6, 0, 0.8)) == (6, 5, 2)
    # the roles exchanged: |a1| = 0.6 > |a2| = 0: no swap; f2 = 0.6 -> 8.8; v = (0, -1, 0), w = (0.8, 0, -0.6), f0 = -0.6435 -> 4.37
    assert _bins((0, 0, 0), (0.6, 0, 0.8), (1, 0, 0), (0, 0, 1)) == (4, 5, 8)
    # a1 == a2 == 0.5 exactly: no swap, f2 = +0.5 -> 8.25 (a swap would give -0.5 -> 2.75); v = (0, -1, 0), f1 = -0.5 -> 2.75
    f = R.pair_features(*(np.array(v, np.float32) for v in ((0, 0, 0), (0.5, 0, 0.5), (1, 0, 0), (0.5, 0.5, 0))))
    assert f[2][0] == 0.5 and f[1][0] == -0.5
    assert _bins((0, 0, 0), (0.5, 0, 0.5), (1, 0, 0), (0.5, 0.5, 0)) == (6, 2, 8)


def test_antiparallel_normals_land_in_the_end_bins_by_the_sign_of_y():
    # n1.n2 = -1 and w.n2 = +0: theta = +pi -> coordinate 11, clamped to bin 10
    assert _bins((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 0, -1)) == (10, 5, 5)
    # w = (-1, 0, 0), n2 = (0, -0, -1): every product of w.n2 is -0, theta = -pi -> coordinate 0, bin 0
    f = R.pair_features(*(np.array(v, np.float32) for v in ((0, 0, 0), (0, 0, 1), (-1, 0, 0), (0.0, -0.0, -1.0))))
    assert f[0][0] == -np.pi
    assert _bins((0, 0, 0), (0, 0, 1), (-1, 0, 0), (0.0, -0.0, -1.0)) == (0, 5, 5)


def test_three_point_cloud_by_hand():
    """Points on the x axis one apart, normals z, z and (0.6, 0, 0.8); radius 1.5.  Pairs (0,1), (1,0): both normals z, the
    feature is (0, 0, 0) -> bins 5 / 16 / 27.  Pairs (1,2), (2,1): the swap test above -> bins 6 / 16 / 24.
    counts: point 0 {5, 16, 27}, m = 1; point 1 {5, 6, 16 x 2, 24, 27}, m = 2; point 2 {6, 16, 24}, m = 1.
    spfh: point 0 100 each; point 1 50, 50, 100, 50, 50; point 2 100 each.  Every d2 is 1.
    point 0: acc = spfh[1], s_t = 100, scale 1: fpfh = spfh[1] + spfh[0]
    point 1: acc = spfh[0] + spfh[2], s_t = 200, scale 0.5
    point 2: acc = spfh[1]: fpfh = spfh[1] + spfh[2]"""
    x = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    nr = np.array([[0, 0, 1], [0, 0, 1], [0.6, 0, 0.8]], np.float32)
    out = R.compute_fpfh(x, nr, 3, 1.5)
    assert list(out["m"]) == [1, 2, 1]
    want = np.zeros((3, 33))
    want[0, [5, 6, 16, 24, 27]] = [150, 50, 200, 50, 150]
    want[1, [5, 6, 16, 24, 27]] = [100, 100, 200, 100, 100]
    want[2, [5, 6, 16, 24, 27]] = [50, 150, 200, 150, 50]
    assert np.array_equal(out["fpfh"], want)
    spfh = np.zeros((3, 33))
    spfh[0, [5, 16, 27]] = 100
    spfh[1, [5, 6, 16, 24, 27]] = [50, 50, 100, 50, 50]
    spfh[2, [6, 16, 24]] = 100
    assert np.array_equal(out["spfh"], spfh)
    # max_nn = 2 keeps the point and its nearest neighbour: point 1 keeps point 0 (tie in d2, lowest index)
    cut = R.compute_fpfh(x, nr, 2, 1.5)
    assert list(cut["m"]) == [1, 1, 1] and cut["ids"][1][0] == 0


# ---- the precondition of the GPU tests, and properties of whole rows ------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_inputs_of_the_gpu_tests_keep_f0_off_the_bin_borders(case):
    m = K.margin(*case)
    print(f"{case}: smallest distance of an f0 bin coordinate from an interior border {m:.3g}")
    assert m >= K.MARGIN
    e = K.expected(*case)
    sums = e["fpfh"].reshape(-1, 3, 11).sum(axis=2)
    has = e["m"] > 0
    if case[1] > 2:    # with max_nn = 2 the only neighbour of a duplicated point is its twin: nothing is accumulated
        assert np.all(np.abs(sums[has] - 200.0) < 1e-9)
    assert np.all(sums[~has] == 0.0) and np.all(e["spfh"][~has] == 0.0)
    assert np.array_equal(e["counts"].reshape(-1, 3, 11).sum(axis=2), np.repeat(e["m"][:, None], 3, axis=1))


def test_cases_cover_the_cap_and_the_empty_neighbourhoods():
    assert int((K.expected("target", 33, 2.5)["m"] == 32).sum()) == 3081
    m = K.expected("target", 100, 2.5)["m"]
    assert (int(m.min()), int(m.max())) == (7, 88)
    m = K.expected("target", 16, 1.0)["m"]
    assert (m == 0).any() and (m == 1).any()
    assert np.all(K.expected("cluster", 128, 1.0)["m"] == 127)


@pytest.mark.parametrize("k,radius", [(32, 2.5), (10, 1.0), (1, 0.5)])
def test_neighbourhoods_equal_the_oracles_knn_order(k, radius):
    x = K.scene()[0]
    ids = oracle.surface_normals(x, k, radius)[3]
    assert np.array_equal(ids, R.neighbourhoods(x, k, radius))


def test_nearest_breaks_ties_to_the_lowest_index_and_mutual_ascends():
    rng = np.random.default_rng(2)
    fb = rng.normal(size=(40, 5))
    fb[17] = fb[3]
    fa = np.concatenate([fb[[17, 5]], rng.normal(size=(6, 5))])
    nn_ab, nn_ba, mutual = R.match_features(fa, fb)
    assert nn_ab[0] == 3 and nn_ab[1] == 5 and nn_ba[3] == 0 and nn_ba[17] == 0
    assert np.all(np.diff(mutual[:, 0]) > 0) and [0, 3] in mutual.tolist() and [1, 5] in mutual.tolist()
    for a, b in ((fa, fb), (np.round(fb * 2) / 2, np.round(fb[:25] * 2) / 2), (fb[:, :1].round(), fb[:7, :1].round())):
        both = R.nearest_both(a, b, block=16)                             # the one-pass form against the definition
        assert np.array_equal(both[0], R.nearest(a, b)) and np.array_equal(both[1], R.nearest(b, a))
    assert R.correspondences(fa, fb[:1]).tolist() == [[a, 0] for a in range(8)]      # one mutual pair < ransac_n: every pair


# ---- exports and signatures ----------------------------------------------------------------------------------------------------
NEW = ("reg_compute_fpfh", "reg_match_features")
_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int, "double": C.c_double, "float": C.c_float}


def _header_params(name):
    hdr = open(os.path.join(ROOT, "include", "o3dslam_reg.h")).read()
    m = re.search(r"REG_API\s+reg_status\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in the header"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in args.split(",")]


def test_library_exports_the_new_entry_points_with_the_headers_signatures():
    lib = capi.load_library()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        params = _header_params(name)
        argtypes = getattr(lib, name).argtypes
        assert len(params) == len(argtypes), (name, params)
        for decl, ct in zip(params, argtypes):
            base = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
            if "*" in decl:
                if ct is not C.c_void_p:
                    assert ct._type_ is _CTYPES[base], (name, decl)       # typed pointer: must point at the right type
            else:
                assert ct is _CTYPES[base], (name, decl)
    assert len(_header_params("reg_compute_fpfh")) == 13 and len(_header_params("reg_match_features")) == 11


# ---- argument validation: before the device ---------------------------------------------------------------------------------
def test_python_wrappers_validate_before_touching_the_device():
    dp = icp.DataPoints(np.zeros((4, 3), np.float32), normals=np.zeros((4, 3), np.float32))
    for radius in (0.0, -1.0, float("nan"), float("inf"), "2.5"):
        with pytest.raises(icp.InvalidParameter):
            icp.ComputeFPFHFeature(dp, radius, 100)
    for max_nn in (1, 129, 0, -3, 2.5, True):
        with pytest.raises(icp.InvalidParameter):
            icp.ComputeFPFHFeature(dp, 2.5, max_nn)
    with pytest.raises(icp.InvalidField):
        icp.ComputeFPFHFeature(icp.DataPoints(dp.features), 2.5, 100)
    with pytest.raises(icp.InvalidParameter):
        icp.ComputeFPFHFeature(icp.DataPoints(np.zeros((4, 2), np.float32), normals=dp.normals), 2.5, 100)
    with pytest.raises(icp.InvalidParameter):
        icp.ComputeFPFHFeature(icp.DataPoints(dp.features, normals=np.zeros((3, 3), np.float32)), 2.5, 100)
    f = icp.Feature(np.zeros((33, 5)))
    assert (f.Dimension(), f.Num()) == (33, 5) and icp.Feature().data_.shape == (33, 0)
    with pytest.raises(icp.InvalidParameter):
        icp.CorrespondencesFromFeatures(f, icp.Feature(np.zeros((32, 5))))
    with pytest.raises(icp.InvalidParameter):
        icp.CorrespondencesFromFeatures(icp.Feature(np.zeros((65, 5))), icp.Feature(np.zeros((65, 5))))
    with pytest.raises(icp.InvalidParameter):
        icp.CorrespondencesFromFeatures(f, f, True, 0)
    with pytest.raises(icp.InvalidParameter):
        icp.CorrespondencesFromFeatures(np.zeros(33), f)
    P = icp.PlaceRecognitionParameters
    assert (P().normalEstimationRadius_, P().featureVoxelSize_, P().featureRadius_, P().featureKnn_, P().normalKnn_) == \
        (1.0, 0.5, 2.5, 100, 10)
    cloud = np.zeros((10, 3))
    for bad in (P(featureVoxelSize_=0.0), P(featureRadius_=float("inf")), P(featureKnn_=200), P(normalKnn_=33),
                P(normalKnn_=0), P(normalEstimationRadius_=0.0)):
        with pytest.raises(icp.InvalidParameter):
            icp.computeSubmapFeatures(cloud, bad)
    with pytest.raises(icp.InvalidParameter):
        icp.computeSubmapFeatures(np.zeros((10, 2)))
