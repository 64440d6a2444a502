"""Parity at the FULL sizes of BASELINE.json's single-GPU configurations ("correspondence ids bit-exact vs
oracle exact-NN on iteration 0 and on the last iteration on the benchmark clouds"), plus the 20 M-point map of C4.
GPU box only; the oracle side runs on the box's host cores (OpenMP kd-tree search).

  C2  100 k -> 1 M      ids / d2 / weights bit-exact at iteration 0 and at the pose of the last iteration, A, b 1e-6
  C3  200 k -> 5 M      the same
  C4  20 M-point map    table build at that scale (brick directory, halo bins), ids bit-exact for one rank's 25 k-point
                        slice of an 8-way split and for the whole 200 k-point reading
"""
import numpy as np
import pytest

from oracle import oracle as orc
from open3d_slam_private_amd import capi, synth
from oracle_side import NT, OracleSide

pytestmark = pytest.mark.gpu

ITERS = 20


def _compare(reg, side, T_iter, what):
    ids, d2, w, A6, b6, err, kept = side.linearize(T_iter)
    H, b, gerr, gcnt = reg.linearize(T_iter)
    gids, gd2, gw = reg.correspondences()
    assert np.array_equal(gids, ids), f"{what}: {(gids != ids).sum()} of {ids.size} correspondence ids differ"
    assert np.array_equal(gd2.view(np.uint32), d2.view(np.uint32)), f"{what}: squared distances not bit-exact"
    assert np.array_equal(gw, w), f"{what}: {(gw != w).sum()} weights differ"
    assert gcnt == kept
    scale = np.abs(A6).max()
    assert np.abs(H - A6).max() <= 1e-6 * scale, (what, np.abs(H - A6).max(), scale)
    assert np.abs(b - b6).max() <= 1e-6 * np.abs(b6).max() + 1e-9 * scale, (what, np.abs(b - b6).max())
    assert abs(gerr - err) <= 1e-9 * max(err, 1e-30)
    return int((ids >= 0).sum()), int(kept)


def _full_size_case(n_src, n_tgt, seed):
    sc = synth.make_scene(n_src, n_tgt, seed=seed)
    p = capi.shipped_params()
    p.use_xicp = 0                      # SURVEY 8d's measured chain (bench.py's headline)
    p.fixed_iters = ITERS
    reg = capi.Registration(p)
    reg.set_target(sc.tgt_xyz, sc.tgt_nrm)
    reg.set_source(sc.src_xyz, sc.src_nrm)
    side = OracleSide(sc)
    # iteration 0
    reg.prepare(np.eye(4))
    matched0, kept0 = _compare(reg, side, np.eye(4, dtype=np.float32), "iteration 0")
    # the benchmark's 20-iteration registration, then the correspondences at the pose of its LAST iteration: the fused
    # kernel's own ids / d2 / weights (what iteration 19 used) ...
    T, res = reg.register(np.eye(4))
    assert res.iterations == ITERS
    assert res.n_tail_launches >= 1 and res.n_tail_iterations >= 5     # the settled tail ran in the persistent kernel
    last_ids, last_d2, last_w = reg.correspondences()
    # ... round 3: reg_result.T_iter_prev is the pose iteration 19 actually RAN at, so the persistent tail kernel's OWN output
    # (temporal-coherence shortcut, its own searches, band classification + exact limit) is compared bit for bit with the
    # oracle evaluated at that pose -- not a replay on the select-based path
    T_prev = np.array(res.T_iter_prev, np.float32).reshape(4, 4).T.copy()
    o_ids, o_d2, o_w, oA, ob, o_err, o_kept = side.linearize(T_prev)
    assert np.array_equal(last_ids, o_ids), f"tail kernel, last iteration: {(last_ids != o_ids).sum()} ids differ"
    assert np.array_equal(last_d2.view(np.uint32), o_d2.view(np.uint32)), "tail kernel, last iteration: d2 not bit-exact"
    assert np.array_equal(last_w, o_w), f"tail kernel, last iteration: {(last_w != o_w).sum()} weights differ"
    assert res.n_inliers == o_kept
    H_last = np.array(res.H_last, np.float32).reshape(6, 6)
    assert np.abs(H_last - oA).max() <= 1e-6 * np.abs(oA).max()
    # and one more linearisation at the final pose on the select-based path (iteration 20's matches)
    T_last = np.array(res.T_iter_last, np.float32).reshape(4, 4).T.copy()
    matched, kept = _compare(reg, side, T_last, "last iteration")
    assert matched >= matched0 and kept > 0.85 * matched
    assert (last_ids >= 0).sum() >= matched0
    # whole-registration parity with the oracle on the same clouds
    To, ores = orc.icp_p2pl(sc.tgt_xyz, sc.tgt_nrm, sc.src_xyz, sc.src_nrm, max_dist=0.5, trim_ratio=0.9,
                            max_normal_angle=1.57, fixed_iters=ITERS, n_threads=NT)
    dt, dr = synth.pose_error(T, To)
    assert dt <= 1e-4 and dr <= 1e-4, (dt, dr)
    et, er = synth.pose_error(T, sc.T_true)
    assert et < 5e-3 and er < 1e-3, (et, er)
    reg.close()


def test_c2_full_size_ids_bit_exact_first_and_last_iteration():
    _full_size_case(100_000, 1_000_000, 1234 + 2)


def test_c3_full_size_ids_bit_exact_first_and_last_iteration():
    _full_size_case(200_000, 5_000_000, 1234 + 3)


def test_c4_map_20M_table_build_and_slice_ids_bit_exact():
    """BASELINE configs[3]: the 20 M-point map every rank replicates.  One GPU here: the table build at that scale, then
    (a) ONE rank's 25 k-point slice of an 8-way split (centred on the centroid of the WHOLE reading, as the distributed
    path does) and (b) the whole 200 k-point reading, ids / d2 / weights bit-exact against the kd-tree oracle."""
    n_src, n_tgt, seed = 200_000, 20_000_000, 1234 + 4
    sc = synth.make_scene(n_src, n_tgt, seed=seed)
    p = capi.shipped_params()
    p.use_xicp = 0
    p.fixed_iters = ITERS
    reg = capi.Registration(p)
    reg.set_target(sc.tgt_xyz, sc.tgt_nrm)
    info = reg.target_info()
    assert info.n_points == n_tgt and info.n_bricks > 0
    # (b) whole reading
    reg.set_source(sc.src_xyz, sc.src_nrm)
    side = OracleSide(sc)
    reg.prepare(np.eye(4))
    _compare(reg, side, np.eye(4, dtype=np.float32), "c4 whole reading, iteration 0")
    T, res = reg.register(np.eye(4))
    # the tail kernel's own last iteration at the pose it ran at (see _full_size_case)
    last_ids, last_d2, last_w = reg.correspondences()
    T_prev = np.array(res.T_iter_prev, np.float32).reshape(4, 4).T.copy()
    o_ids, o_d2, o_w, *_ = side.linearize(T_prev)
    assert res.n_tail_launches >= 1
    assert np.array_equal(last_ids, o_ids) and np.array_equal(last_d2.view(np.uint32), o_d2.view(np.uint32))
    assert np.array_equal(last_w, o_w)
    T_last = np.array(res.T_iter_last, np.float32).reshape(4, 4).T.copy()
    _compare(reg, side, T_last, "c4 whole reading, last iteration")
    et, er = synth.pose_error(T, sc.T_true)
    assert et < 5e-3 and er < 1e-3, (et, er)
    # (a) rank 3 of 8: points [75 k, 100 k), global centroid
    lo, hi = 3 * n_src // 8, 4 * n_src // 8
    reg.set_source(sc.src_xyz[lo:hi], sc.src_nrm[lo:hi])
    reg.prepare_centroid(np.eye(4), side.c_read)
    ids_all, d2_all, w_all, *_ = side.linearize(T_last)
    H, b, gerr, gcnt = reg.linearize(T_last)
    gids, gd2, gw = reg.correspondences()
    assert np.array_equal(gids, ids_all[lo:hi])
    assert np.array_equal(gd2.view(np.uint32), d2_all[lo:hi].view(np.uint32))
    reg.close()


def test_c2_full_size_gicp_registration_vs_oracle():
    """BASELINE configs[1] with the GICP cost (separate search / linearise kernels): 20 iterations at full C2 size, pose
    against the fp64 oracle (OpenMP) on the same clouds and covariances.  GICP parity is unpinned against the reference
    (Open3D's arithmetic is not in its tree): this is oracle == HIP only, tolerance 1e-4 m / 1e-4 rad."""
    sc = synth.make_scene(100_000, 1_000_000, seed=1234 + 2)
    tcov, scov = sc.tgt_cov, sc.src_cov
    p = capi.default_params()
    p.cost = capi.COST_GICP
    p.use_trimmed = 0
    p.max_dist = 0.5
    p.fixed_iters = ITERS
    reg = capi.Registration(p)
    reg.set_target(sc.tgt_xyz, None, tcov)
    reg.set_source(sc.src_xyz, None, scov)
    T, res = reg.register(np.eye(4))
    assert res.iterations == ITERS
    To, ores = orc.icp_gicp(sc.tgt_xyz, tcov, sc.src_xyz, scov, np.eye(4), max_dist=0.5, fixed_iters=ITERS, n_threads=NT)
    dt, dr = synth.pose_error(T, To)
    assert dt <= 1e-4 and dr <= 1e-4, (dt, dr)
    et, er = synth.pose_error(T, sc.T_true)
    assert et < 5e-3 and er < 1e-3, (et, er)
    # correspondences of the last iteration: the search is the point-to-plane path's, ids against the kd-tree at T_last
    T_last = np.array(res.T_iter_last, np.float32).reshape(4, 4).T.copy()
    gids, gd2, _ = reg.correspondences()
    tree = orc.KdTree(sc.tgt_xyz)
    reg.close()
    # GICP works in the caller's frame (no centring).  Round 3: iterations 1 .. 19 ran inside the persistent tail kernel
    # (k_tail<true>: coherence shortcut, its own searches, fp64 GICP factors); the ids / d2 it left are those of its LAST
    # iteration, which ran at reg_result.T_iter_prev -- bit-exact against the kd-tree at that pose
    assert res.n_tail_launches == 1 and res.n_tail_iterations == ITERS - 1
    T_prev = np.array(res.T_iter_prev, np.float32).reshape(4, 4).T.copy()
    ids_p, d2_p = tree.knn(sc.src_xyz, T_prev, max_dist=0.5, n_threads=NT)
    assert np.array_equal(gids, ids_p), f"GICP tail, last iteration: {(gids != ids_p).sum()} ids differ"
    assert np.array_equal(gd2.view(np.uint32), d2_p.view(np.uint32)), "GICP tail, last iteration: d2 not bit-exact"
    assert res.n_matched == int((ids_p >= 0).sum())
    ids_o, d2_o = tree.knn(sc.src_xyz, T_last, max_dist=0.5, n_threads=NT)
    agree = float((gids == ids_o).mean())
    assert agree > 0.995, agree


def test_c5_eight_full_size_c2_registrations_in_parallel_threads(monkeypatch):
    """BASELINE configs[4] on ONE GPU: 8 independent handles, each with its own stream, registering 8 different full-size C2
    problems (seed + i) at the same time from 8 host threads.  Every pose within 1e-4 m / 1e-4 rad of the oracle's for ITS
    problem.  Twice: with the default policy (a registration takes the persistent tail kernel only when it is alone on the
    device, so the batch runs on the three-launch iteration) and with O3D_TAIL_ALWAYS (one registration at a time holds the
    device's tail lock, the others fall back: the lock changes hands between rounds)."""
    import threading
    n_src, n_tgt, K = 100_000, 1_000_000, 8
    scenes = [synth.make_scene(n_src, n_tgt, seed=4321 + i) for i in range(K)]
    oracle_T = [orc.icp_p2pl(sc.tgt_xyz, sc.tgt_nrm, sc.src_xyz, sc.src_nrm, max_dist=0.5, trim_ratio=0.9, max_normal_angle=1.57,
                             fixed_iters=ITERS, n_threads=NT)[0] for sc in scenes]
    for always in (False, True):
        if always:
            monkeypatch.setenv("O3D_TAIL_ALWAYS", "1")     # read when the handle is created
        regs = []
        for sc in scenes:
            p = capi.shipped_params()
            p.use_xicp = 0
            p.fixed_iters = ITERS
            r = capi.Registration(p)
            r.set_target(sc.tgt_xyz, sc.tgt_nrm)
            r.set_source(sc.src_xyz, sc.src_nrm)
            regs.append(r)
        out = [None] * K
        errs = []
        start = threading.Barrier(K)

        def work(i):
            try:
                start.wait()
                for _ in range(3):   # several rounds: the lock changes hands
                    out[i] = regs[i].register(np.eye(4))
            except Exception as e:   # noqa: BLE001
                errs.append((i, repr(e)))

        ths = [threading.Thread(target=work, args=(i,)) for i in range(K)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errs, errs
        n_tail = 0
        for i in range(K):
            T, res = out[i]
            assert res.iterations == ITERS
            n_tail += int(res.n_tail_launches > 0)
            dt, dr = synth.pose_error(T, oracle_T[i])
            assert dt <= 1e-4 and dr <= 1e-4, (always, i, dt, dr)
            regs[i].close()
        if always:
            assert n_tail >= 1
    # alone on the device, the same handle does take the tail
    p = capi.shipped_params()
    p.use_xicp = 0
    p.fixed_iters = ITERS
    r = capi.Registration(p)
    r.set_target(scenes[0].tgt_xyz, scenes[0].tgt_nrm)
    r.set_source(scenes[0].src_xyz, scenes[0].src_nrm)
    T, res = r.register(np.eye(4))
    assert res.n_tail_launches >= 1
    dt, dr = synth.pose_error(T, oracle_T[0])
    assert dt <= 1e-4 and dr <= 1e-4
    r.close()
