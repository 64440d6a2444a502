"""The libpointmatcher chain extension on the CPU: its restatement against the reference's own golden, the pure C ABI
checks, the robust weights and the point-to-point update shared with the device, and the YAML binding."""
import math

import numpy as np
import pytest

from open3d_slam_private_amd import capi
from open3d_slam_private_amd.icp import ICP, PointMatcherICP
from tests.pm_chain_restatement import Chain, PmRestatement, kabsch, robust_weights
from tests.test_oracle_golden import _ref_trans_case, icp_test_relative_error

GOLDEN_YAML = """
readingDataPointsFilters:
referenceDataPointsFilters:
matcher:
  KDTreeMatcher:
    knn: 10
    epsilon: 0
outlierFilters:
  - RobustOutlierFilter:
      robustFct: cauchy
      scaleEstimator: mad
      tuning: 1
errorMinimizer:
  PointToPointErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 40
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.01
      smoothLength: 4
inspector:
  NullInspector
logger:
  NullLogger
"""


def robust_golden():
    """libpointmatcher examples/data/icp_data/defaultRobustOutlierFilter.{yaml,ref_trans} (checked by TEST(icpTest,
    icpTest), utest.cpp:81-161): cloud.00001 -> cloud.00000, KDTreeMatcher knn 10, RobustOutlierFilter cauchy / mad /
    tuning 1, PointToPointErrorMinimizer, Counter 40, Differential 0.001 / 0.01 / 4.  The fixture holds the 16 numbers
    of the .ref_trans file as fp64 4 x 4."""
    ref, data, _ = _ref_trans_case()
    refT = np.load(__file__.rsplit("/", 1)[0] + "/golden/icp_data_robust_cauchy_p2p_ref_trans.npy")
    return ref, data, refT


GOLDEN_CHAIN = dict(knn=10, minimizer="point2point", robust="cauchy", tuning=1.0, scale="mad", max_iter=40,
                    min_rot=0.001, min_trans=0.01, smooth=4)


def test_restatement_reproduces_the_robust_point_to_point_golden():
    ref, data, refT = robust_golden()
    r = PmRestatement(ref, None, Chain(**GOLDEN_CHAIN))
    r.set_reading(data)
    T, iters, _ = r.register()
    rel = icp_test_relative_error(T, refT, data)
    assert rel < 0.05                       # the reference's criterion, utest.cpp:159
    # what the restatement reaches: 1.49e-2 in 22 iterations (the stored matrix is probably from an older filter)
    assert 1e-2 < rel < 2e-2, rel
    assert iters == 22


def _chain(**kw):
    c = capi.default_pm_chain()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_check_pm_chain_rules():
    p = capi.default_params()
    p.use_xicp = 0
    for k in range(1, 17):
        assert capi.check_pm_chain(p, _chain(knn=k)) == 0
    assert capi.check_pm_chain(p, _chain(knn=0)) == 6
    assert capi.check_pm_chain(p, _chain(knn=17)) == 6
    for f in range(8):
        for est in (0, 1, 2):
            for dist in (0, 1):
                for mini in (0, 1):
                    c = _chain(use_robust=1, robust_fct=f, scale_estimator=est, distance_type=dist, minimizer=mini, knn=3)
                    assert capi.check_pm_chain(p, c) == 0, (f, est, dist, mini)
    assert capi.check_pm_chain(p, _chain(use_robust=1, scale_estimator=3)) == 9     # std: refused
    assert capi.check_pm_chain(p, _chain(use_robust=1, robust_fct=8)) == 6
    assert capi.check_pm_chain(p, _chain(use_robust=1, tuning=0.0)) == 6
    assert capi.check_pm_chain(p, _chain(use_robust=1, nb_iter_for_scale=101)) == 6
    c = _chain(knn=2)
    c.struct_size = 12
    assert capi.check_pm_chain(p, c) == 6
    for cost in (1, 2, 3):
        q = capi.default_params()
        q.cost = cost
        assert capi.check_pm_chain(q, _chain(knn=2)) == 6
    x = capi.shipped_params()                     # use_xicp = 1
    assert capi.check_pm_chain(x, _chain()) == 0
    assert capi.check_pm_chain(x, _chain(knn=2)) == 9
    assert capi.check_pm_chain(x, _chain(use_robust=1)) == 9
    assert capi.check_pm_chain(x, _chain(minimizer=1)) == 9


def _d2_samples():
    rng = np.random.default_rng(3)
    return np.concatenate([np.array([0.0, 1e-8, 0.5, 1.0, 2.0, 3.0, 4.0], np.float32),
                           (rng.random(4000) ** 3 * 25).astype(np.float32)])


@pytest.mark.parametrize("fct", ["cauchy", "sc", "gm", "tukey", "huber", "L1"])
def test_robust_weights_bit_equal_to_the_fp32_formula(fct):
    d = _d2_samples()
    for tuning, scale in ((1.0, 1.0), (1.0, 0.37), (4.3040, 0.05), (2.5, 1.7)):
        w = capi.host_robust_weights(fct, tuning, scale, d)
        ref = robust_weights(fct, tuning, scale, d)
        assert np.array_equal(w.view(np.uint32), ref.view(np.uint32)), (fct, tuning, scale)


@pytest.mark.parametrize("fct", ["welsch", "student"])
def test_robust_weights_within_two_ulp(fct):
    d = _d2_samples()
    for tuning, scale in ((1.0, 1.0), (1.0, 0.37), (2.5, 1.7)):
        w = capi.host_robust_weights(fct, tuning, scale, d)
        ref = robust_weights(fct, tuning, scale, d)
        nz = (w != 0) | (ref != 0)
        ulp = np.abs(w[nz].view(np.int32).astype(np.int64) - ref[nz].view(np.int32).astype(np.int64))
        # welsch: expf within 2 ulp; student: powf, then two fp32 products (measured: 3 ulp against numpy on the host)
        assert ulp.max() <= (2 if fct == "welsch" else 4), (fct, ulp.max())


def test_robust_weights_zero_past_the_approximation():
    d = _d2_samples()
    for fct in capi.ROBUST_FCTS:
        w = capi.host_robust_weights(fct, 1.0, 0.5, d, approximation=1.5)
        e2 = d / np.float32(0.25)
        assert np.all(w[e2 >= np.float32(1.5 ** 2)] == 0)
        assert np.array_equal(w, robust_weights(fct, 1.0, 0.5, d, 1.5)) or fct in ("welsch", "student")


def _p2p_sums(P, Q, w):
    s = np.zeros(32)
    s[0:3] = (w[:, None] * P).sum(0)
    s[3:6] = (w[:, None] * Q).sum(0)
    s[6:15] = ((w[:, None] * Q).T @ P).reshape(9)
    s[28] = w.sum()
    return s


def test_pm_p2p_update_is_weighted_kabsch():
    rng = np.random.default_rng(5)
    P = rng.normal(size=(500, 3))
    w = rng.random(500)
    ang = 0.3
    R = np.array([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, math.cos(0.2), -math.sin(0.2)], [0, math.sin(0.2), math.cos(0.2)]])
    Rt = R @ Rx
    t = np.array([0.4, -1.0, 0.25])
    Q = P @ Rt.T + t                                    # exact pairs: the known transform comes back
    U, rank = capi.host_pm_p2p_update(_p2p_sums(P, Q, w))
    assert rank == 3
    assert np.abs(U[:3, :3] - Rt).max() < 1e-10 and np.abs(U[:3, 3] - t).max() < 1e-10
    Qn = Q + rng.normal(scale=0.05, size=Q.shape)       # noisy pairs: equal to numpy's weighted Kabsch
    U, _ = capi.host_pm_p2p_update(_p2p_sums(P, Qn, w))
    K, _ = kabsch(P, Qn, w)
    assert np.abs(U - K).max() < 1e-9
    Qr = P * np.array([1.0, 1.0, -1.0])                 # a reflection: the best proper rotation, as the reference's flip
    U, _ = capi.host_pm_p2p_update(_p2p_sums(P, Qr, w))
    K, _ = kabsch(P, Qr, w)
    assert abs(np.linalg.det(U[:3, :3]) - 1) < 1e-9
    assert np.abs(U - K).max() < 1e-9
    line = np.outer(rng.normal(size=50), [1.0, 2.0, 0.5])   # rank <= 1: finite
    U, rank = capi.host_pm_p2p_update(_p2p_sums(line, line + 0.1, np.ones(50)))
    assert rank <= 1 and np.all(np.isfinite(U))
    U, rank = capi.host_pm_p2p_update(_p2p_sums(np.zeros((4, 3)), np.ones((4, 3)), np.ones(4)))
    assert rank == 0 and np.all(np.isfinite(U))
    with pytest.raises(capi.RegError):
        capi.host_pm_p2p_update(np.zeros(32))


def test_pointmatcher_icp_binds_the_golden_yaml():
    icp = PointMatcherICP()
    icp.loadFromYaml(GOLDEN_YAML)
    p, c = icp.params, icp.chain
    assert p.knn == 1 and p.cost == 0 and math.isinf(p.max_dist) and p.epsilon == 0
    assert p.use_trimmed == 0 and p.use_surface_normal == 0 and p.use_max_dist_filter == 0 and p.use_xicp == 0
    assert p.max_iter == 40 and p.smooth_len == 4
    assert abs(p.min_diff_rot - 0.001) < 1e-9 and abs(p.min_diff_trans - 0.01) < 1e-9
    assert c.knn == 10 and c.minimizer == capi.PM_POINT_TO_POINT and c.use_robust == 1
    assert c.robust_fct == capi.ROBUST_FCTS["cauchy"] and c.tuning == 1.0
    assert c.scale_estimator == capi.SCALE_ESTIMATORS["mad"] and c.nb_iter_for_scale == 0
    assert c.distance_type == capi.DISTANCE_TYPES["point2point"] and math.isinf(c.approximation)
    with pytest.raises((NotImplementedError, Exception)):
        ICP().loadFromYaml(GOLDEN_YAML)
    icp2 = PointMatcherICP()
    with pytest.raises(NotImplementedError):
        icp2.loadFromYaml(GOLDEN_YAML.replace("scaleEstimator: mad", "scaleEstimator: std"))
