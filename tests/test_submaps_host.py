"""CPU-only checks of the submap collection: the pure host functions of the library against the literal
restatement (tests/submaps_restatement.py), the parameter validation and struct layouts, and -- on the restatement alone --
that the scripted walk of tests/submaps_cases.py reaches every outcome of updateActiveSubmap with fitness values far from
the threshold, so that the device test (tests/test_gpu_submaps.py) compares what it is meant to compare."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from open3d_slam_private_amd import capi
from tests import submaps_cases as K
from tests import submaps_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT, BAD_TRANSFORM = 6, 4


# ---- reg_host_submaps_decide: the full enumeration of its discrete inputs, distances on both sides of the radius and on it ----
def test_decide_equals_the_restatement_on_the_full_enumeration():
    radius = 2.0
    below, above = np.nextafter(radius, 0.0), np.nextafter(radius, 10.0)
    dists = (0.0, below, radius, above, 7.5)
    n = 0
    for force, merged, initial, points, closest_active, adjacent, fit in itertools.product(
            (0, 1), (0, 4, 5, 6), (0, 1), (99, 100, 101), (0, 1), (0, 1), (None, False, True)):
        for dc, da in itertools.product(dists, dists):
            want = R.decide(force, merged, 5, initial, points, 100, closest_active, dc, da, radius, adjacent, fit)
            got = capi.host_submaps_decide(force, merged, 5, initial, points, 100, closest_active, dc, da, radius, adjacent,
                                           -1 if fit is None else int(fit))
            assert got == want, (force, merged, initial, points, closest_active, adjacent, fit, dc, da)
            n += 1
    assert n == 2 * 4 * 2 * 3 * 2 * 2 * 3 * 25
    # every action and both flags occur in the enumeration (the comparison above is not vacuous)
    seen = {R.decide(f, m, 5, 0, p, 100, c, dc, da, radius, a, fit)
            for f, m, p, c, a, fit, dc, da in itertools.product((0, 1), (0, 5), (99, 101), (0, 1), (0, 1), (None, False, True),
                                                                dists, dists)}
    assert {d & 3 for d in seen} == {0, 1, 2, 3} and any(d & 4 for d in seen) and any(d & 8 for d in seen)


def test_decide_on_the_radius_itself_and_with_nan():
    # distance_to_closest == radius is NOT within range (strictly less); distance_to_active == radius has NOT travelled
    assert capi.host_submaps_decide(0, 9, 5, 0, 0, 100, 0, 2.0, 0.0, 2.0, 0, 0) == R.CREATE
    assert capi.host_submaps_decide(0, 9, 5, 0, 0, 100, 0, 1.0, 2.0, 2.0, 0, 0) == R.KEEP
    assert capi.host_submaps_decide(0, 9, 5, 0, 0, 100, 0, 1.0, np.nextafter(2.0, 3.0), 2.0, 0, 0) == R.CREATE
    assert capi.host_submaps_decide(0, 9, 5, 0, 0, 100, 0, float("nan"), 0.0, 2.0, 1, 1) == R.CREATE   # NaN < radius is false


# ---- getDistanceToNearestLoopClosureSubmap ---------------------------------------------------------------------------------------
def _graph(n, edges, marked):
    a = R.AdjacencyMatrix()
    for e in edges:
        a.addEdge(*e)
    for m in marked:
        a.markAsLoopClosureSubmap(m)
    return a, a.matrix(n)


@pytest.mark.parametrize("n,edges,marked", [
    (5, [(0, 1), (1, 2), (2, 3), (3, 4)], []),                       # a chain without marks: ends at the last node popped
    (5, [(0, 1), (1, 2), (2, 3), (3, 4)], [4]),                      # a chain with the mark at its end
    (5, [(0, 1), (1, 2), (2, 3), (3, 4)], [2]),
    (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], [3]),      # a cycle
    (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], [1, 4]),
    (7, [(0, 1), (0, 2), (1, 3), (2, 4), (4, 5), (3, 5), (5, 6)], [6]),
    (4, [(0, 1), (2, 3)], [3]),                                      # the mark is in another component
])
def test_adjacency_distance_equals_the_restatement(n, edges, marked):
    a, (adj, marks) = _graph(n, edges, marked)
    for node in range(n):
        if node in a.isLoopClosureSubmap_:
            assert capi.host_adjacency_distance(adj, marks, node) == a.getDistanceToNearestLoopClosureSubmap(node), node


def test_adjacency_distance_special_cases():
    a, (adj, marks) = _graph(3, [], [])
    assert capi.host_adjacency_distance(adj, marks, 1) == R.INT_MAX == a.getDistanceToNearestLoopClosureSubmap(1)   # no marks at all
    a, (adj, marks) = _graph(3, [(0, 1)], [0])
    assert capi.host_adjacency_distance(adj, marks, 0) == 0          # the mark on the node itself
    assert capi.host_adjacency_distance(adj, marks, 1) == 0          # one hop: max(0, 1 - 1)
    assert capi.host_adjacency_distance(adj, marks, 2) == -1         # no entry: the reference throws
    with pytest.raises(KeyError):
        a.getDistanceToNearestLoopClosureSubmap(2)
    assert capi.host_adjacency_distance(adj, marks, 3) == -1 and capi.host_adjacency_distance(adj, marks, -1) == -1
    a, (adj, marks) = _graph(5, [(0, 1), (1, 2), (2, 3), (3, 4)], [4])
    assert [capi.host_adjacency_distance(adj, marks, k) for k in range(5)] == [3, 2, 1, 0, 0]


# ---- the transform plan ------------------------------------------------------------------------------------------------------------
PARENTS = [0, 0, 1, 2, 2, 4, 5, 1]     # a tree: 0 - 1 - 2 - (3, 4 - 5 - 6), 1 - 7


@pytest.mark.parametrize("ids", [[0, 1, 2, 3, 4, 5, 6, 7], [0], [0, 1], [0, 2, 1], [0, 1, 2, 4], [0, 0, 1], [0, 1, 9], []])
def test_transform_plan_equals_the_restatement(ids):
    try:
        want = R.transform_plan(PARENTS, ids)
    except (IndexError, RuntimeError):
        want = None
    st, plan = capi.host_submaps_transform_plan(PARENTS, ids)
    if want is None:
        assert st == BAD_TRANSFORM
    else:
        assert st == 0 and plan.tolist() == want


def test_transform_plan_cases_by_hand():
    st, plan = capi.host_submaps_transform_plan(PARENTS, [0, 1])
    # unlisted 2..7 walk up to 1 (or through 2, 4, 5 to 1): all read position 1, which here is submap 1's own increment
    assert st == 0 and plan.tolist() == [0, 1, 1, 1, 1, 1, 1, 1]
    st, plan = capi.host_submaps_transform_plan(PARENTS, [1, 0])
    # the oddity: position = parent INDEX, so the children of 1 read position 1 = the increment listed for submap 0
    assert st == 0 and plan.tolist() == [1, 0, 1, 1, 1, 1, 1, 1]
    assert capi.host_submaps_transform_plan(PARENTS, [1, 2])[0] == BAD_TRANSFORM       # 0 unlisted and its own parent: stuck
    assert capi.host_submaps_transform_plan(PARENTS, [0, 4])[0] == BAD_TRANSFORM       # 5 reads position 4 of a list of 2
    assert capi.host_submaps_transform_plan(PARENTS, [])[0] == 0
    assert capi.host_submaps_transform_plan([0, 5], [0])[0] == BAD_ARGUMENT            # a parent out of range


# ---- parameters, struct sizes, the header -----------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults():
    assert capi.submaps_struct_sizes() == tuple(C.sizeof(c) for c in (capi.SubmapsParams, capi.SubmapsInfo, capi.SubmapInfo,
                                                                      capi.SubmapsInsertResult, capi.SubmapFeatureParams))
    f = capi.default_submap_feature_params()                      # Parameters.hpp:121-126
    assert (f.normal_knn, f.feature_knn, f.feature_voxel_size, f.normal_radius, f.feature_radius) == (10, 100, 0.5, 1.0, 2.5)
    p = capi.default_submaps_params()
    assert p.struct_size == C.sizeof(capi.SubmapsParams) and p.map.struct_size == C.sizeof(capi.MapCloudParams)
    # Parameters.hpp:103-110,138-139 and magic.hpp:16
    assert (p.radius, p.min_num_range_data, p.max_num_points, p.min_seconds_between_features, p.revisit_min_fitness,
            p.num_scans_overlap) == (20.0, 5, 400000, 5.0, 0.4, 3)
    assert (p.voxel_expansion_factor, p.loop_closure_search_radius, p.min_submaps_between_loop_closures, p.max_submaps) == (2.5, 20.0, 2, 64)
    assert capi.check_submaps_params(p) == 0


@pytest.mark.parametrize("field,value", [("num_scans_overlap", 0), ("max_submaps", 0), ("max_submaps", 4097), ("max_num_points", -1),
                                         ("radius", float("nan")), ("revisit_min_fitness", float("nan")),
                                         ("voxel_expansion_factor", 0.0), ("voxel_expansion_factor", float("inf")),
                                         ("voxel_expansion_factor", 1e-320), ("struct_size", 8)])
def test_parameter_validation(field, value):
    p = capi.default_submaps_params()
    setattr(p, field, value)
    assert capi.check_submaps_params(p) == BAD_ARGUMENT
    q = capi.default_submaps_params()
    q.map.map_voxel_size = 0.0                  # the occupancy voxel would be zero
    assert capi.check_submaps_params(q) == BAD_ARGUMENT


def test_header_declares_the_structs_as_the_bindings_mirror_them():
    hdr = open(os.path.join(ROOT, "include", "o3dslam_reg.h")).read()
    for name, cls in (("reg_submaps_params", capi.SubmapsParams), ("reg_submaps_info", capi.SubmapsInfo),
                      ("reg_submap_info", capi.SubmapInfo), ("reg_submaps_insert_result", capi.SubmapsInsertResult)):
        end = hdr.index("} " + name + ";")
        body = hdr[hdr.rindex("typedef struct {", 0, end):end]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [m for decl in re.findall(r"^\s+(?:int32_t|int64_t|double|reg_map_cloud_params|reg_map_cloud_insert_result)\s+([^;]+);",
                                          body, re.M) for m in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl)]
        assert names == [f[0] for f in cls._fields_], name


# ---- the Mapper's initial guess ------------------------------------------------------------------------------------------------------
def _rigid(rng, scale):
    from open3d_slam_private_amd import synth
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_R(*rng.uniform(-3.0, 3.0, size=3))
    T[:3, 3] = rng.uniform(-scale, scale, size=3)
    return T


def test_initial_guess_is_the_restatement_and_within_the_conditioning_bar_of_extended_precision():
    """Bar: four levels of 4 x 4 products of rigid matrices (the inverse of calib feeds A and B, B^-1 A, prev M).  An entry of
    one product carries at most gamma_4 = 4 eps times the sum of |a| |b| over its four terms, which is at most 3 + S for
    rotation entries <= 1 and translations that add up to at most S = |t_prev| + 2 (|t_odom| + |t_calib|) each; an error made
    at one level passes through at most three more rotations whose rows have absolute sums <= sqrt(3) < 2.  So every entry is
    within 4 levels x 4 eps x (3 + S) x 2^3 = 128 eps (3 + S) of the exact result, here taken from 80-bit arithmetic."""
    rng = np.random.default_rng(11)
    eps = np.finfo(np.float64).eps
    for scale in (0.5, 30.0, 2000.0):
        for _ in range(10):
            prev, op, on, cal = (_rigid(rng, scale) for _ in range(4))
            got = capi.host_mapper_initial_guess(prev, op, on, cal)
            assert np.array_equal(got.view(np.uint64), R.mapper_initial_guess(prev, op, on, cal).view(np.uint64))
            L = lambda T: np.asarray(T, np.longdouble)
            inv = lambda T: np.block([[T[:3, :3].T, -(T[:3, :3].T @ T[:3, 3:])], [np.zeros((1, 3), np.longdouble), np.ones((1, 1), np.longdouble)]])
            ci = inv(L(cal))
            exact = L(prev) @ (inv(L(op) @ ci) @ (L(on) @ ci))
            S = np.linalg.norm(prev[:3, 3]) + 2 * (np.linalg.norm(op[:3, 3]) + np.linalg.norm(on[:3, 3]) + 2 * np.linalg.norm(cal[:3, 3]))
            assert float(np.max(np.abs(L(got) - exact))) <= 128 * eps * (3 + S)
    eye = np.eye(4)
    assert np.array_equal(capi.host_mapper_initial_guess(eye, eye, eye), eye)


# ---- the occupancy clouds and the walk, on the restatement alone ---------------------------------------------------------------------
def test_occupancy_clouds_hold_what_they_are_meant_to():
    v = 2.5 * K.OCC_VOXEL
    x = K.occ_cloud(4099, 1)
    f, ok = R.voxel_indices(x, v)
    assert np.isnan(x).any() and np.isinf(x).any() and (~ok).sum() >= 4 and (x < 0).any()
    assert np.any(np.all(np.abs(x[ok]) / v == np.round(np.abs(x[ok]) / v), axis=1))          # a row on voxel faces on every axis
    assert len({tuple(r) for r in x[ok]}) < ok.sum()                                         # duplicates
    assert len(R.occupancy_set(x, v)) < ok.sum()                                             # several rows per voxel
    assert R.occupancy_set(K.occ_cloud(1, 1), v) and not R.occupancy_set(np.array([[np.nan, 0, 0]]), v)
    c, fit = R.switch_fitness(set(), np.zeros((0, 3)), np.eye(4), v)
    assert c == 0 and np.isnan(fit) and not fit > 0.4                                        # the empty scan fails the check


def test_walk_reaches_every_outcome_with_fitness_far_from_the_threshold():
    col, decisions, fitness = K.host_walk()
    assert len(decisions) == len(K.WALK_X) == 14 and all(1500 <= n <= 3000 for n in K.WALK_N)
    seen = set(col.branches)
    assert seen == set(R.BRANCHES) - {"initial_map"}, set(R.BRANCHES) - seen      # isUseInitialMap_ has its own short walk
    assert any(d & R.SET_FORCE_FLAG for d in decisions) and any(d & R.FORCED for d in decisions)
    k = next(i for i, d in enumerate(decisions) if d & R.SET_FORCE_FLAG)
    assert decisions[k + 1] & R.FORCED                                            # max_num_points acts at the NEXT call
    checked = [f for f in fitness if f is not None]
    thr = K.PARAMS["revisit_min_fitness"]
    assert any(f[1] > thr for f in checked) and any(not f[1] > thr for f in checked)
    assert all(abs(f[1] - thr) >= 0.05 for f in checked), checked
    assert len(col.submaps_) == 7 <= K.PARAMS["max_submaps"]
    assert any(len(s.voxelMap_) == 0 and s.isCenterComputed_ for s in col.submaps_)          # a finished submap without features
    rep = [i for i, _ in col.finishedSubmapsIdxs_]
    assert len(rep) > len(set(rep))                                               # a submap is finished twice (it was revisited)


def test_initial_map_walk_keeps_the_first_submap():
    p = dict(K.PARAMS, is_use_initial_map=1)
    col = R.SubmapCollection(p, K.HostMap)
    for raw, scan, T, stamp in K.walk()[:3]:
        col.insertScan(raw, scan, T, stamp)
    assert col.branches == ["few_scans", "initial_map", "initial_map"] and col.activeSubmapIdx_ == 0
    assert col.submaps_[0].map.scans == 2                  # the first scan became the map (Submap.cpp:47-52): not counted
