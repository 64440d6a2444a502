"""reg_compute_fpfh and reg_match_features on the device against the numpy restatement
(tests/fpfh_restatement.py); the inputs are those of tests/fpfh_cases.py, whose precondition (no f0 bin coordinate within 1e-9
of an interior bin border) tests/test_fpfh_host.py asserts.

Bars: n_neighbours and spfh are exact (integer counts times one fp64 factor: np.array_equal); fpfh is within
1e-12 * max(1, |value|) (at most 127 non-negative terms added in the same order on both sides: the bar covers the division
and libm only; bit equality is expected and printed when seen); nn_ab, nn_ba, mutual and n_mutual are exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from open3d_slam_private_amd import capi, icp, synth
from tests import fpfh_cases as K
from tests import fpfh_restatement as R

pytestmark = pytest.mark.gpu

EMPTY_TARGET, EMPTY_SOURCE, BAD_ARGUMENT = 1, 2, 6
G = 4            # kFpfhWaves: query points per workgroup of the neighbourhood kernel
TILE, CHUNK = 32, 1024   # kMfTile, kMfChunk


def _reg():
    p = capi.default_params()
    p.cost = capi.COST_O3D_P2P
    return capi.Registration(p)


def _assert_fpfh(got, want, what):
    assert got["n_neighbours"].dtype == np.int32 and np.array_equal(got["n_neighbours"], want["m"]), what
    assert np.array_equal(got["spfh"], want["spfh"]), what
    err = np.abs(got["fpfh"] - want["fpfh"]) / np.maximum(1.0, np.abs(want["fpfh"]))
    print(f"{what}: fpfh max scaled error {err.max() if err.size else 0.0:.3g}, "
          f"bit-equal {np.array_equal(got['fpfh'], want['fpfh'])}, rescanned {got['n_rescanned']}")
    assert np.all(err <= 1e-12), what


def _run(reg, x, nr, max_nn, radius):
    return reg.compute_fpfh(x, nr, radius, max_nn, want_spfh=True, want_counts=True)


# ---- reg_compute_fpfh ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_fpfh_equals_the_restatement(case):
    cloud, max_nn, radius = case
    x, nr = K.CLOUDS[cloud]()
    got = _run(_reg(), x, nr, max_nn, radius)
    _assert_fpfh(got, K.expected(*case), str(case))
    if cloud == "cluster":
        assert got["n_rescanned"] > 0        # 2 000 candidates exceed the 1 024 keys of the on-chip list
    else:
        assert got["n_rescanned"] == 0


@pytest.mark.parametrize("n", [1, 2, G - 1, G, G + 1])
def test_fpfh_of_the_first_points(n):
    x, nr = K.scene()[0][:n], K.scene()[1][:n]
    # the first points of the scene lie far apart: a radius that makes them neighbours of each other
    radius = 60.0
    want = R.compute_fpfh(x, nr, 100, radius)
    assert R.f0_border_margin(x, nr, want["ids"], want["m"]) >= K.MARGIN
    got = _run(_reg(), x, nr, 100, radius)
    _assert_fpfh(got, want, f"first {n}")
    assert np.all(want["m"] == n - 1)
    if n == 1:
        assert not got["fpfh"].any() and not got["spfh"].any()


def test_fpfh_host_and_device_pointers_agree_and_sentinels_survive():
    x, nr = K.scene()[0][:1500], K.scene()[1][:1500]
    n = x.shape[0]
    reg = _reg()
    host = _run(reg, x, nr, 16, 1.0)
    x4 = np.concatenate([x, np.full((n, 1), 7.0, np.float32)], axis=1)        # stride 4
    d_x, d_n = torch.from_numpy(x4).cuda(), torch.from_numpy(nr.copy()).cuda()
    d_f = torch.full((n + 1, 33), -7.0, dtype=torch.float64, device="cuda")
    d_s = torch.full((n + 1, 33), -7.0, dtype=torch.float64, device="cuda")
    d_m = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    resc = reg.compute_fpfh_device(d_x.data_ptr(), 4, d_n.data_ptr(), 3, n, 1.0, 16, d_f.data_ptr(), d_s.data_ptr(),
                                   d_m.data_ptr())
    torch.cuda.synchronize()
    assert resc == host["n_rescanned"]
    f, s, m = d_f.cpu().numpy(), d_s.cpu().numpy(), d_m.cpu().numpy()
    assert np.array_equal(f[:n], host["fpfh"]) and np.array_equal(s[:n], host["spfh"]) and np.array_equal(m[:n], host["n_neighbours"])
    assert np.all(f[n] == -7.0) and np.all(s[n] == -7.0) and m[n] == -7
    # optional outputs left out: nothing but fpfh is written
    d_f2 = torch.full((n + 1, 33), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    reg.compute_fpfh_device(d_x.data_ptr(), 4, d_n.data_ptr(), 3, n, 1.0, 16, d_f2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_f2, d_f)
    only = reg.compute_fpfh(x, nr, 1.0, 16)
    assert set(only) == {"fpfh", "n_rescanned"} and np.array_equal(only["fpfh"], host["fpfh"])


def _status(reg, x, nr, max_nn, radius, n=None):
    x, nr = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(nr, np.float32)
    out = np.full((max(x.shape[0], 1), 33), -7.0)
    st = reg._lib.reg_compute_fpfh(reg._h, x.ctypes.data, 3, nr.ctypes.data, 3, x.shape[0] if n is None else n, 0, max_nn,
                                   radius, out.ctypes.data, None, None, None)
    return st, out


def test_fpfh_bad_arguments_leave_the_handle_usable():
    x, nr = K.scene()[0][:600].copy(), K.scene()[1][:600].copy()
    reg = _reg()
    good = _run(reg, x, nr, 16, 1.0)
    for what, bad_x, bad_n in (("nan x", 5, None), ("inf x", 7, None), ("nan n", None, 9), ("inf n", None, 11)):
        bx, bn = x.copy(), nr.copy()
        if bad_x is not None:
            bx[bad_x, 1] = np.nan if "nan" in what else np.inf
        if bad_n is not None:
            bn[bad_n, 2] = np.nan if "nan" in what else -np.inf
        st, out = _status(reg, bx, bn, 16, 1.0)
        assert st == BAD_ARGUMENT and "finite" in reg.last_error(), what
        assert np.all(out == -7.0), what
        assert np.array_equal(_run(reg, x, nr, 16, 1.0)["fpfh"], good["fpfh"]), what
    for max_nn, radius in ((1, 1.0), (129, 1.0), (16, 0.0), (16, float("inf")), (16, float("nan")), (16, -1.0)):
        st, out = _status(reg, x, nr, max_nn, radius)
        assert st == BAD_ARGUMENT and np.all(out == -7.0), (max_nn, radius)
    assert _status(reg, x, nr, 16, 1.0, n=0)[0] == EMPTY_SOURCE
    lib, h = reg._lib, reg._h
    out = np.zeros((600, 33))
    assert lib.reg_compute_fpfh(h, None, 3, nr.ctypes.data, 3, 600, 0, 16, 1.0, out.ctypes.data, None, None, None) == BAD_ARGUMENT
    assert lib.reg_compute_fpfh(h, x.ctypes.data, 3, None, 3, 600, 0, 16, 1.0, out.ctypes.data, None, None, None) == BAD_ARGUMENT
    assert lib.reg_compute_fpfh(h, x.ctypes.data, 3, nr.ctypes.data, 3, 600, 0, 16, 1.0, None, None, None, None) == BAD_ARGUMENT
    assert lib.reg_compute_fpfh(h, x.ctypes.data, 2, nr.ctypes.data, 3, 600, 0, 16, 1.0, out.ctypes.data, None, None, None) == BAD_ARGUMENT
    assert lib.reg_compute_fpfh(h, x.ctypes.data, 3, nr.ctypes.data, 2, 600, 0, 16, 1.0, out.ctypes.data, None, None, None) == BAD_ARGUMENT
    assert np.array_equal(_run(reg, x, nr, 16, 1.0)["fpfh"], good["fpfh"])
    with pytest.raises(icp.InvalidParameter):
        bx = x.copy()
        bx[0, 0] = np.nan
        icp.ComputeFPFHFeature(icp.DataPoints(bx, normals=nr), 1.0, 16)
    assert np.array_equal(icp.ComputeFPFHFeature(icp.DataPoints(x, normals=nr), 1.0, 16).data_, good["fpfh"].T)


def test_fpfh_calls_of_different_size_share_one_handle_with_a_registration():
    sc = synth.make_scene(3000, 6000, seed=5)
    p = capi.default_params()
    p.cost = capi.COST_O3D_P2PL
    p.use_trimmed = 0
    p.max_dist = 1.0
    reg = capi.Registration(p)
    reg.set_target(sc.tgt_xyz, sc.tgt_nrm)
    reg.set_source(sc.src_xyz)
    T0, res0 = reg.register(np.eye(4))
    x, nr = K.scene()[0], K.scene()[1]
    want = K.expected("target", 16, 1.0)
    big = _run(reg, x, nr, 16, 1.0)
    small = _run(reg, x[:700], nr[:700], 16, 1.0)
    again = _run(reg, x, nr, 16, 1.0)
    _assert_fpfh(big, want, "first call")
    assert np.array_equal(again["fpfh"], big["fpfh"]) and np.array_equal(again["spfh"], big["spfh"])
    ref = _run(_reg(), x[:700], nr[:700], 16, 1.0)
    assert np.array_equal(small["fpfh"], ref["fpfh"]) and np.array_equal(small["n_neighbours"], ref["n_neighbours"])
    T1, res1 = reg.register(np.eye(4))
    assert np.array_equal(T0, T1) and res0.iterations == res1.iterations and res0.fitness == res1.fitness


def _free_bytes():
    hip = C.CDLL("libamdhip64.so.7")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_destroy_returns_the_workspace():
    capi.load_library()
    rng = np.random.default_rng(4)
    x = rng.uniform(-40, 40, size=(150_000, 3)).astype(np.float32)
    x[:, 2] *= 0.02
    nr = np.tile(np.array([[0, 0, 1]], np.float32), (x.shape[0], 1))
    fa = rng.normal(size=(20_000, 33))

    def one():
        r = _reg()
        r.compute_fpfh(x, nr, 1.0, 64, want_spfh=True)
        r.match_features(fa, fa[:5000])
        r.close()

    one()
    free0 = _free_bytes()
    for _ in range(3):
        one()
    assert free0 - _free_bytes() < 32 * 2**20


# ---- reg_match_features --------------------------------------------------------------------------------------------------------
def _assert_match(reg, fa, fb, what=""):
    want = R.match_features(fa, fb)
    got = reg.match_features(fa, fb)
    for g, w, name in zip(got, want, ("nn_ab", "nn_ba", "mutual")):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, name)
    return want


def test_match_one_by_one():
    nn_ab, nn_ba, mutual = _assert_match(_reg(), np.array([[1.0, 2.0]]), np.array([[-1.0, 0.5]]))
    assert mutual.tolist() == [[0, 0]]


@pytest.mark.parametrize("dim", [1, 3, 33, 64])
@pytest.mark.parametrize("na,nb", [(TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (CHUNK - 1, CHUNK + 1), (CHUNK, CHUNK),
                                   (CHUNK + 1, CHUNK - 1), (257, 2 * CHUNK + TILE + 1)])
def test_match_around_the_tile_and_the_chunk(na, nb, dim):
    rng = np.random.default_rng(1000 * dim + na)
    # coarse values: equal distances, and so ties across tiles and chunks, are common at dim 1 and 3
    fa, fb = np.round(rng.normal(size=(na, dim)) * 4) / 4, np.round(rng.normal(size=(nb, dim)) * 4) / 4
    _assert_match(_reg(), fa, fb, (na, nb, dim))


def test_match_duplicate_rows_self_match_and_zero_rows():
    rng = np.random.default_rng(3)
    reg = _reg()
    fb = rng.normal(size=(2 * CHUNK + 100, 33))
    dup = rng.choice(fb.shape[0], 300, replace=False)
    fb[dup] = fb[(dup * 7 + 13) % fb.shape[0]]            # duplicate rows, many of them in another chunk
    fa = fb[rng.permutation(fb.shape[0])[:1500]].copy()
    nn_ab, _, _ = _assert_match(reg, fa, fb, "duplicates in B")
    assert np.array_equal(fb[nn_ab], fa)
    # A = B: every row is its own mutual match unless a duplicate row precedes it
    nn_ab, nn_ba, mutual = _assert_match(reg, fb, fb, "A = B")
    first = np.array([np.nonzero((fb == r).all(axis=1))[0][0] for r in fb])
    assert np.array_equal(nn_ab, first) and np.array_equal(nn_ba, first)
    assert np.array_equal(mutual[:, 0], np.nonzero(first == np.arange(fb.shape[0]))[0]) and np.array_equal(mutual[:, 0], mutual[:, 1])
    z = np.zeros((CHUNK + 5, 33))
    nn_ab, nn_ba, mutual = _assert_match(reg, z, z[:70], "zero rows")
    assert not nn_ab.any() and not nn_ba.any() and mutual.tolist() == [[0, 0]]


def test_match_fpfh_rows_of_the_scene():
    fa, fb = K.expected("reading", 100, 2.5)["fpfh"], K.expected("target", 100, 2.5)["fpfh"]
    _, _, mutual = _assert_match(_reg(), fa, fb, "scene")
    assert mutual.shape[0] == 825
    got = icp.CorrespondencesFromFeatures(icp.Feature(fa.T), icp.Feature(fb.T))
    assert got.dtype == np.int32 and np.array_equal(got, mutual)


def test_match_forward_only_device_pointers_and_sentinels():
    rng = np.random.default_rng(8)
    fa, fb = rng.normal(size=(700, 33)), rng.normal(size=(CHUNK + 300, 33))
    reg = _reg()
    want = R.match_features(fa, fb)
    nn_ab, nn_ba, mutual = reg.match_features(fa, fb, backward=False, mutual=False)
    assert nn_ba is None and mutual is None and np.array_equal(nn_ab, want[0])
    nn_ab, nn_ba, mutual = reg.match_features(fa, fb, backward=True, mutual=False)
    assert mutual is None and np.array_equal(nn_ab, want[0]) and np.array_equal(nn_ba, want[1])
    na, nb = fa.shape[0], fb.shape[0]
    d_a, d_b = torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda()
    d_ab = torch.full((na + 1,), -7, dtype=torch.int32, device="cuda")
    d_ba = torch.full((nb + 1,), -7, dtype=torch.int32, device="cuda")
    d_mu = torch.full((na, 2), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert reg.match_features_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, 33, d_ab.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_ab.cpu().numpy()[:na], want[0]) and int(d_ab[na]) == -7
    assert bool((d_ba == -7).all()) and bool((d_mu == -7).all())
    d_ab.fill_(-7)
    torch.cuda.synchronize()
    km = reg.match_features_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, 33, d_ab.data_ptr(), d_ba.data_ptr(), d_mu.data_ptr())
    torch.cuda.synchronize()
    assert km == want[2].shape[0] and km > 0
    assert np.array_equal(d_ab.cpu().numpy()[:na], want[0]) and np.array_equal(d_ba.cpu().numpy()[:nb], want[1])
    mu = d_mu.cpu().numpy()
    assert np.array_equal(mu[:km], want[2]) and np.all(mu[km:] == -7) and int(d_ab[na]) == -7 and int(d_ba[nb]) == -7
    # mutual without nn_ba: the backward search runs in the workspace
    d_mu.fill_(-7)
    torch.cuda.synchronize()
    assert reg.match_features_device(d_a.data_ptr(), na, d_b.data_ptr(), nb, 33, d_ab.data_ptr(), None, d_mu.data_ptr()) == km
    torch.cuda.synchronize()
    assert np.array_equal(d_mu.cpu().numpy()[:km], want[2])


def test_match_bad_arguments_and_the_python_fallback():
    reg = _reg()
    lib, h = reg._lib, reg._h
    fa, fb = np.zeros((4, 3)), np.ones((5, 3))
    ab, km = np.zeros(4, np.int32), C.c_int64(-1)
    call = lambda na, nb, dim, mu=None, kmp=None: lib.reg_match_features(h, fa.ctypes.data, na, fb.ctypes.data, nb, dim, 0,
                                                                         ab.ctypes.data, None, mu, kmp)
    assert call(4, 5, 0) == BAD_ARGUMENT and call(4, 5, 65) == BAD_ARGUMENT
    assert call(0, 5, 3) == EMPTY_SOURCE and call(4, 0, 3) == EMPTY_TARGET
    mu = np.zeros((4, 2), np.int32)
    assert call(4, 5, 3, mu.ctypes.data, None) == BAD_ARGUMENT          # mutual without n_mutual
    assert lib.reg_match_features(h, None, 4, fb.ctypes.data, 5, 3, 0, ab.ctypes.data, None, None, None) == BAD_ARGUMENT
    assert lib.reg_match_features(h, fa.ctypes.data, 4, fb.ctypes.data, 5, 3, 0, None, None, None, None) == BAD_ARGUMENT
    assert call(4, 5, 3, mu.ctypes.data, C.byref(km)) == 0 and km.value == 1 and mu[0].tolist() == [0, 0]
    # one mutual pair < ransac_n = 3: Open3D falls back to every (a, nearest b)
    rng = np.random.default_rng(6)
    a, b = rng.normal(size=(33, 9)), rng.normal(size=(33, 1))
    got = icp.CorrespondencesFromFeatures(icp.Feature(a), icp.Feature(b))
    assert got.dtype == np.int32 and got.tolist() == [[i, 0] for i in range(9)]
    assert icp.CorrespondencesFromFeatures(icp.Feature(a), icp.Feature(b), True, 1).shape == (1, 2)
    a2, b2 = rng.normal(size=(33, 50)), rng.normal(size=(33, 60))
    want = R.match_features(a2.T, b2.T)
    assert np.array_equal(icp.CorrespondencesFromFeatures(a2, b2, False), np.stack([np.arange(50), want[0]], axis=1))
    assert np.array_equal(icp.CorrespondencesFromFeatures(a2, b2), R.correspondences(a2.T, b2.T))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_compute_submap_features_equals_the_three_calls():
    sc = synth.make_scene(100, 40_000, seed=9)
    cloud = sc.tgt_xyz.astype(np.float64)
    prm = icp.PlaceRecognitionParameters()
    sparse, feature = icp.computeSubmapFeatures(cloud, prm)
    reg = _reg()
    vox, _, _, n_outside = reg.voxelize_within_volume(cloud, 0.5)
    assert n_outside == 0 and 1000 < vox.shape[0] < cloud.shape[0]
    pts = vox.astype(np.float32)
    nrm = reg.estimate_normals(pts, k=10, max_dist=1.0, viewpoint=np.zeros(3, np.float32))["normals"]
    out = reg.compute_fpfh(pts, nrm, 2.5, 100)
    assert np.array_equal(sparse.features, pts) and np.array_equal(sparse.normals, nrm)
    assert feature.data_.shape == (33, pts.shape[0]) and np.array_equal(feature.data_, out["fpfh"].T)
    assert np.isfinite(feature.data_).all() and feature.data_.any()


# ---- the output paths that the calls above leave thin: absent outputs, scratch slices, zero rows, edge sizes ---------------
from tests import staged_output_cases as SO  # noqa: E402


@pytest.fixture(scope="module")
def so_reg():
    r = capi.Registration(capi.default_params())
    yield r
    r.close()


def test_fpfh_output_subsets_equal_the_full_call(so_reg):
    SO.check_subsets(so_reg, SO.OPS["fpfh"](so_reg), SO.f32_inputs(300))


def test_fpfh_device_form_without_optional_outputs(so_reg):
    SO.check_device_without_optionals(so_reg, SO.OPS["fpfh"](so_reg), SO.f32_inputs(300))


def test_match_features_output_subsets_equal_the_full_call(so_reg):
    """Among the subsets: mutual without nn_ba (the backward search then runs into a scratch slice)."""
    full = SO.check_subsets(so_reg, SO.OPS["match_features"](so_reg, 257, 33), SO.feature_inputs(300, 257, 33))
    assert full.counts["km"] > 0


def test_match_features_device_form_without_optional_outputs(so_reg):
    SO.check_device_without_optionals(so_reg, SO.OPS["match_features"](so_reg, 257, 33), SO.feature_inputs(300, 257, 33))
