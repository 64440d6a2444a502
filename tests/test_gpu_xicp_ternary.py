"""degeneracyAwareness EqualityConstraints (X-ICP, ternary) on the device against tests/xicp_ternary_restatement.py.

PARITY UNPINNED against the reference itself: its localizability unit tests are empty (utest/ui/localizability).  Pinned
here: device == restatement.  Bars: categories and pair counts identical; the information sums within 1e-9 relative (the
same fp32 terms, fp64 sums in different orders; the bar of tests/test_gpu_xicp.py); every partial sum within
1e-9 max(1, sum |term|); constraint values within 2 d + 1e-6 |value| of the fp32 restatement, d = the fp32 / fp64 spread
of the restatement on that input (what rounding alone does to an ill-conditioned 3x3); iteration counts equal; the pose
within 1e-4 m / 1e-4 rad plus the pose spread of the restatement's two modes on that scene.

The sign of an eigenvector is a free choice of the eigen-solver (it cancels in the KKT system): constraint values are
compared after aligning the restatement's eigenvector with the device's.

The sanity rule (ICP.cpp:1956-1967): with unit reference normals a <= 1, a partial sample holds at least sum(a) >=
insufficient pairs and the rule cannot fail under ordered thresholds.  Nothing normalises the matched normal, though:
the device case scales the reference normals by 30 (tests/xicp_ternary_scenes.py: slanted_scaled)."""
import numpy as np
import pytest

from open3d_slam_private_amd import capi, synth
from open3d_slam_private_amd.icp import DataPoints, PointMatcherICP
from tests import xicp_ternary_scenes as scenes
from tests.test_gpu_pm_extras import register_raw
from tests.test_pm_extras_host import SHIPPED
from tests.xicp_ternary_restatement import LOCALIZABLE, PARTIAL_HIGH, PARTIAL_MIXED, partial_constraint

pytestmark = pytest.mark.gpu
f32 = np.float32


def _reg(ternary=True, chain_kw=None, **pk):
    p = capi.shipped_params()
    p.use_xicp = 0
    for k, v in pk.items():
        setattr(p, k, v)
    reg = capi.Registration(p)
    if chain_kw:
        c = capi.default_pm_chain_v3()
        for k, v in chain_kw.items():
            setattr(c, k, v)
        reg.set_pm_chain(c)
    if ternary:
        reg.set_ternary_xicp(capi.default_ternary_xicp(True))
    return reg


def _run(name, **pk):
    tgt, tn, src, sn, _ = scenes.scene(name)
    reg = _reg(**pk)
    reg.set_target(tgt, tn)
    reg.set_source(src, sn)
    T, res = reg.register(np.eye(4))
    return reg, T, res


def _fields(g):
    """Every field of the getter's struct as bytes."""
    return bytes(g)


@pytest.mark.parametrize("name", scenes.SCENES)
def test_first_iteration_matches_the_restatement(name):
    reg, T, res = _run(name, fixed_iters=1)
    g = reg.get_ternary_xicp()
    a = scenes.restated(name, 1)[0].trace[0]
    cat = list(g.category)
    print(name, "device categories", cat, "combined", list(g.combined), "high", list(g.high), "constraint", list(g.constraint))
    assert res.iterations == 1 and g.iteration == 1 and g.sane == 1
    assert cat == list(a["cat"]) and g.n_pairs == a["n_pairs"]
    assert list(g.n_combined) == list(a["n_comb"]) and list(g.n_high) == list(a["n_high"])
    assert list(res.localizable) == [1 if c == LOCALIZABLE else 0 for c in cat]
    assert res.n_constraints == sum(c != LOCALIZABLE for c in cat)
    vo = np.array([list(g.eigenvectors[0]), list(g.eigenvectors[1])], f32).reshape(6, 3)
    for k in range(6):
        assert abs(g.combined[k] - a["comb"][k]) <= 1e-9 * max(1.0, a["comb"][k])
        assert abs(g.high[k] - a["high"][k]) <= 1e-9 * max(1.0, a["high"][k])
        assert res.xicp_combined[k] == g.combined[k] and res.xicp_high[k] == g.high[k]
        sign = 1.0 if float(vo[k] @ a["vo"][k]) >= 0 else -1.0
        assert np.abs(vo[k] - sign * a["vo"][k]).max() <= 1e-5
        ps = np.array(list(g.partial_sums[k]))
        if cat[k] in (PARTIAL_MIXED, PARTIAL_HIGH):
            assert np.all(np.abs(ps - a["psums"][k]) <= 1e-9 * np.maximum(1.0, a["pabs"][k]))
            r32 = sign * float(partial_constraint(a["psums"][k], a["vo"][k]))
            d = abs(r32 - sign * float(partial_constraint(a["psums"][k], a["vo"][k], fp64=True)))
            print(f"  direction {k}: device {g.constraint[k]:.9g} restatement {r32:.9g} d {d:.3g}")
            assert abs(g.constraint[k] - r32) <= 2 * d + 1e-6 * abs(r32)
            # the device's own value is the host form on the device's own sums, bit for bit
            hv, ok = capi.host_partial_constraint(ps, vo[k])
            assert ok and f32(hv).view(np.uint32) == f32(g.constraint[k]).view(np.uint32)
        else:
            assert not ps.any() and g.constraint[k] == 0.0


@pytest.mark.parametrize("name", scenes.SCENES)
def test_checkers_decide_like_the_restatement(name):
    reg, T, res = _run(name)
    r, T_r, it_r = scenes.restated(name)
    _, T_64, _ = scenes.restated(name, 0, True)
    g = reg.get_ternary_xicp()
    spread = synth.pose_error(T_r, T_64)
    dt, dr = synth.pose_error(T, T_r)
    print(f"{name}: {res.iterations} iterations, last categories {list(g.category)}, pose vs restatement {dt:.3g} m {dr:.3g} rad, "
          f"fp32 / fp64 spread of the restatement {spread[0]:.3g} m {spread[1]:.3g} rad")
    assert res.iterations == it_r and g.iteration == it_r
    assert list(g.category) == list(r.trace[-1]["cat"])
    assert dt <= 1e-4 + spread[0] and dr <= 1e-4 + spread[1]
    assert reg.get_minimizer_stats().returned_prior == 0


def test_partial_direction_recovers_what_a_constrained_one_leaves_at_the_prior():
    _, T0, _ = _run("corridor0")
    _, T100, _ = _run("corridor100")
    print("x of the corridor: E = 0:", T0[0, 3], "E = 100:", T100[0, 3])
    assert abs(T100[0, 3] - 0.10) < abs(T0[0, 3] - 0.10)
    assert abs(T0[0, 3]) < 2e-3 and abs(T100[0, 3] - 0.10) < 1e-2


def test_inert_when_every_direction_is_localizable():
    sc = synth.make_scene(8000, 80000, seed=9)
    bound = dict(use_bound=1, max_rotation_norm=float("inf"), max_translation_norm=float("inf"))
    out = []
    for ternary in (True, False):
        reg = _reg(ternary, bound)
        reg.set_target(sc.tgt_xyz, sc.tgt_nrm)
        reg.set_source(sc.src_xyz, sc.src_nrm)
        out.append(reg.register(np.eye(4)))
        if ternary:
            g = reg.get_ternary_xicp()
            assert list(g.category) == [LOCALIZABLE] * 6 and g.iteration == out[0][1].iterations
    (T1, r1), (T0, r0) = out
    assert list(r1.localizable) == [1] * 6 and r1.n_constraints == 0
    assert r1.iterations == r0.iterations and np.array_equal(T1.view(np.uint32), T0.view(np.uint32))


@pytest.mark.parametrize("name", ["slanted", "floor_strip"])
def test_two_registrations_return_identical_bits(name):
    tgt, tn, src, sn, _ = scenes.scene(name)
    reg = _reg()
    reg.set_target(tgt, tn)
    reg.set_source(src, sn)
    T1, r1 = reg.register(np.eye(4))
    g1 = _fields(reg.get_ternary_xicp())
    T2, r2 = reg.register(np.eye(4))
    g2 = _fields(reg.get_ternary_xicp())
    assert np.array_equal(T1.view(np.uint32), T2.view(np.uint32)) and r1.iterations == r2.iterations
    assert g1 == g2


def test_failed_detection_returns_the_prior():
    """Exact, unperturbed normals: the sample of the corridor axis gives a rank-1 A3, its constraint value is not finite."""
    tgt, tn, src, sn, _ = scenes.corridor(100, exact_normals=True)
    reg = _reg()
    reg.set_target(tgt, tn)
    reg.set_source(src, sn)
    T_init = np.eye(4, dtype=f32)
    T_init[:3, 3] = (0.01, -0.02, 0.005)
    st, T, res = register_raw(reg, T_init)
    g = reg.get_ternary_xicp()
    print("categories", list(g.category), "constraint", list(g.constraint), "iterations", res.iterations)
    assert st == 0 and g.category[5] == PARTIAL_HIGH and not np.isfinite(g.constraint[5])
    assert reg.get_minimizer_stats().returned_prior == 1
    assert np.array_equal(T.view(np.uint32), T_init.view(np.uint32)) and res.iterations == 0


def test_sanity_rule_returns_the_prior():
    """insufficient_thr above the sample count of a PARTIAL_MIXED direction (reference normals scaled by 30, so that its
    combined sum exceeds its pair count and the thresholds stay ordered): the prior, as for a failed detection."""
    tgt, tn, src, sn, _ = scenes.scene("slanted_scaled")
    thr = scenes.sanity_thresholds()
    r, _, it_r = scenes.restated("slanted_scaled", 0, False, thr)
    a = r.trace[0]
    assert r.returned_prior and it_r == 0 and not a["sane"]
    reg = _reg(False)
    t = capi.default_ternary_xicp(True)
    t.high_information, t.enough_information, t.insufficient_information = thr[:3]
    reg.set_ternary_xicp(t)
    reg.set_target(tgt, tn)
    reg.set_source(src, sn)
    T_init = np.eye(4, dtype=f32)
    st, T, res = register_raw(reg, T_init)
    g = reg.get_ternary_xicp()
    print("categories", list(g.category), "combined", g.combined[5], "pairs", g.n_combined[5], "thresholds", thr)
    assert list(g.category) == list(a["cat"]) and g.category[5] == PARTIAL_MIXED
    assert g.n_combined[5] == a["n_comb"][5] and g.n_combined[5] < thr[2] and g.sane == 0
    assert abs(g.combined[5] - a["comb"][5]) <= 1e-9 * a["comb"][5]
    assert st == 0 and res.iterations == 0 and reg.get_minimizer_stats().returned_prior == 1
    assert np.array_equal(T.view(np.uint32), T_init.view(np.uint32))
    assert not np.array(list(g.partial_sums[5])).any() and g.constraint[5] == 0.0   # no partial problem was set up
    # the same scene under thresholds its sample meets registers
    reg.set_ternary_xicp(capi.default_ternary_xicp(True))
    _, res2 = reg.register(np.eye(4))
    assert res2.iterations >= 1 and reg.get_minimizer_stats().returned_prior == 0 and reg.get_ternary_xicp().sane == 1


def test_state_switches_and_refusals():
    tgt, tn, src, sn, _ = scenes.scene("corridor100")
    reg = _reg()
    reg.set_target(tgt, tn)
    reg.set_source(src, sn)
    T1, r1 = reg.register(np.eye(4))
    g1 = _fields(reg.get_ternary_xicp())
    with pytest.raises(capi.RegError) as e:
        reg.dist_begin(None)                              # no distributed path while the method is on
    assert e.value.status == 9                            # REG_UNSUPPORTED
    reg.set_ternary_xicp(None)
    with pytest.raises(capi.RegError) as e:
        reg.get_ternary_xicp()
    assert e.value.status == 5                            # REG_NOT_CONFIGURED
    T_off, r_off = reg.register(np.eye(4))
    assert list(r_off.localizable) == [1] * 6 and r_off.n_constraints == 0
    reg.set_ternary_xicp(capi.default_ternary_xicp(True))
    T2, r2 = reg.register(np.eye(4))
    assert np.array_equal(T1.view(np.uint32), T2.view(np.uint32)) and g1 == _fields(reg.get_ternary_xicp())
    # a later chain that does not run with the method fails and leaves the handle as it was
    for kw, status in ((dict(knn=2), 9), (dict(use_robust=1), 9), (dict(minimizer=capi.PM_POINT_TO_POINT), 9),
                       (dict(degeneracy_method=capi.DEGENERACY_SOLUTION_REMAPPING), 6)):
        c = capi.default_pm_chain_v3()
        for k, v in kw.items():
            setattr(c, k, v)
        with pytest.raises(capi.RegError) as e:
            reg.set_pm_chain(c)
        assert e.value.status == status, kw
    T3, _ = reg.register(np.eye(4))
    assert np.array_equal(T1.view(np.uint32), T3.view(np.uint32))
    # the method refused on a handle whose chain / parameters do not run with it
    for kw, pk, status in ((dict(knn=2), {}, 9), (dict(use_robust=1), {}, 9), (dict(minimizer=capi.PM_POINT_TO_POINT), {}, 9),
                           (dict(degeneracy_method=capi.DEGENERACY_SOLUTION_REMAPPING), {}, 6), (None, dict(use_xicp=1), 6)):
        other = _reg(False, kw, **pk)
        with pytest.raises(capi.RegError) as e:
            other.set_ternary_xicp(capi.default_ternary_xicp(True))
        assert e.value.status == status, (kw, pk)
    # Bound checker and the 0 / 1 outlier filters run with it
    ok = _reg(True, dict(use_bound=1, max_rotation_norm=1.0, max_translation_norm=1.0, use_min_dist_filter=1,
                         outlier_min_dist=1e-4), use_max_dist_filter=1, outlier_max_dist=0.4)
    ok.set_target(tgt, tn)
    ok.set_source(src, sn)
    _, r_ok = ok.register(np.eye(4))
    assert r_ok.iterations >= 1 and ok.get_ternary_xicp().iteration == r_ok.iterations


def test_shipped_yaml_registers_with_its_equality_constraints_block():
    lines = SHIPPED.split("\n")
    k0 = lines.index("  OptimizedEqualityConstraints:")
    for k in range(k0, k0 + 5):
        lines[k] = "#" + lines[k]
    k1 = lines.index("  #EqualityConstraints:")
    for k in range(k1, k1 + 6):
        lines[k] = lines[k].replace("#", "", 1)
    icp = PointMatcherICP()
    icp.loadFromYaml("\n".join(lines))
    tgt, tn, src, sn, _ = scenes.scene("corridor100")
    T = icp.compute(DataPoints(src, sn), DataPoints(tgt, tn), np.eye(4))
    _, T_r, it_r = scenes.restated("corridor100")
    loc = icp.localizability
    dt, dr = synth.pose_error(T, T_r)
    assert icp.last_result.iterations == it_r and loc.iteration == it_r and dt <= 1e-4 and dr <= 1e-4
    assert list(loc.category) == list(scenes.restated("corridor100")[0].trace[-1]["cat"])
