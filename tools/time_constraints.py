"""Timings of DESIGN.md 5zc on one GPU: one pose-graph constraint between two submaps of the resident collection, (a) built where
the maps live -- reg_submaps_build_constraint -- against (b) the path without it: both map clouds exported to the host and
icp.buildConstraint / icp.refineLoopClosure on a throw-away handle, which uploads them again.  Measured for an odometry
constraint (buildOdometryConstraint's arguments with refinement, from the identity) and for a refined loop candidate (from an
initial transform, overlap at it).  The world is a ground disc of 25 m with four walls, sampled with --scans points per scan
at a map voxel of 0.07 m; three scans per submap.  The two paths alternate inside every repetition; times are host clocks
around calls that end in a stream synchronise.
usage: python tools/time_constraints.py [--scans 400000] [--warmup 2] [--reps 7] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open3d_slam_private_amd import capi, icp, synth  # noqa: E402

VOXEL, REACH = 0.07, 25.0


def scan(n, seed):
    """Ground (70 %) and four walls at +-20 m (30 %), with their normals."""
    rng = np.random.default_rng(seed)
    g = int(0.7 * n)
    r, a = REACH * np.sqrt(rng.random(g)), rng.uniform(0.0, 2.0 * np.pi, g)
    ground = np.stack([r * np.cos(a), r * np.sin(a), rng.normal(0.0, 0.01, g) - 1.5], axis=1)
    w = n - g
    side, u, z = rng.integers(0, 4, w), rng.uniform(-20.0, 20.0, w), rng.uniform(-1.5, 4.0, w)
    d = 20.0 + rng.normal(0.0, 0.01, w)
    sx, sy = np.array([1.0, -1.0, 0.0, 0.0])[side], np.array([0.0, 0.0, 1.0, -1.0])[side]
    walls = np.stack([np.where(sx != 0.0, sx * d, u), np.where(sy != 0.0, sy * d, u), z], axis=1)
    nr = np.concatenate([np.tile([0.0, 0.0, 1.0], (g, 1)), np.stack([-sx, -sy, np.zeros(w)], axis=1)])
    return np.ascontiguousarray(np.concatenate([ground, walls])), np.ascontiguousarray(nr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=400_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    crop = dict(type=capi.CROP_MAX_RADIUS, center=(0.0, 0.0, 0.0), radius_max=40.0)
    mp = capi.default_map_cloud_params(crop, has_normals=True, map_voxel_size=VOXEL, carve_every_n_scans=10)
    sp = capi.default_submaps_params(mp, min_num_range_data=1, max_num_points=10_000_000, radius=1000.0, is_carving_enabled=0,
                                     num_scans_overlap=1)
    reg = capi.Registration(capi.shipped_params())
    dev = capi.Submaps(reg, sp)
    for s in range(3):                                             # three finished submaps, a few centimetres apart
        T = np.eye(4)
        T[:3, 3] = (0.03 * s, -0.02 * s, 0.0)
        for j in range(3):
            x, nr = scan(a.scans, 10 * s + j)
            dev.insert_scan(None, x, T, 100 * s + j, nr)
        dev.force_new_submap()
    rows = [int(dev.submap_info(k).n_rows) for k in range(3)]
    odo = dev.default_odometry_constraint_params(refine=True)
    T0 = np.eye(4)
    T0[:3, :3] = synth.rpy_to_R(0.001, -0.002, 0.004)
    T0[:3, 3] = (0.05, -0.03, 0.01)
    loop = capi.constraint_params(capi.COST_O3D_P2PL, 30, True, False, True, odo.overlap_voxel_size, 0.3, 0.3)
    t = dict(resident_odometry=[], exported_odometry=[], resident_loop=[], exported_loop=[])
    dp = lambda e: icp.DataPoints(e["xyz"], normals=e["normals"])
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        r = dev.build_constraint(0, 1, odo)
        t1 = time.perf_counter()
        c = icp.buildConstraint(dp(dev.export_submap(0)), dp(dev.export_submap(1)), isComputeOverlap=True,
                                icpMaxCorrespondenceDistance=odo.icp_max_correspondence_distance,
                                voxelSizeOverlapCompute=odo.overlap_voxel_size, isEstimateInformationMatrix=True, isSkipIcpRefinement=False)
        t2 = time.perf_counter()
        rl = dev.build_constraint(2, 0, loop, T0)
        t3 = time.perf_counter()
        cl, _ = icp.refineLoopClosure(dp(dev.export_submap(2)), dp(dev.export_submap(0)), T0, icp.RegistrationIcpPointToPlane(0.3, 30),
                                      odo.overlap_voxel_size, 0.3)
        t4 = time.perf_counter()
        assert np.array_equal(r.T_matrix(), c.sourceToTarget_) and np.array_equal(r.information_matrix(), c.informationMatrix_)
        assert np.array_equal(rl.T_matrix(), cl.sourceToTarget_) and np.array_equal(rl.information_matrix(), cl.informationMatrix_)
        if k >= a.warmup:
            for name, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                t[name].append(v)
    ms = lambda v: dict(median_ms=round(1e3 * float(np.median(v)), 3), min_ms=round(1e3 * min(v), 3), max_ms=round(1e3 * max(v), 3))
    out = dict(scan_points=a.scans, map_rows=rows, reps=a.reps, warmup=a.warmup, odometry_iterations=int(r.iterations),
               loop_iterations=int(rl.iterations), selected=[int(r.n_source_selected), int(r.n_target_selected)],
               **{name: ms(v) for name, v in t.items()})
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    dev.close(), reg.close()


if __name__ == "__main__":
    main()
