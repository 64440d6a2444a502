"""Sweep of the search-structure knobs (env switches read at reg_create) on one workload:
  O3D_BIN_OCC    points per occupied bin the automatic bin edge aims at (default 8)
  O3D_HALO_RATIO halo-bin edge / bin edge (default 1.25; 1.5 when this sweep was run)
  O3D_HALO_RHO   exactness radius of the halo level / halo-bin edge (default 0.25)
Prints, per combination: registration time (min / median of 6), search-kernel times from the per-dispatch HIP events,
table size, build time; the final pose must be identical for every combination (the search is exact for any table).
usage: python tools/tools_sweep_tables.py c3 "8,4,16" "1.5,1.0,2.0" "0.25,0.35,0.5" """
import itertools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open3d_slam_private_amd import capi, synth
from bench import WORKLOADS, ITERS

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
occs = [float(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "8").split(",")]
ratios = [float(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "1.5").split(",")]
rhos = [float(v) for v in (sys.argv[4] if len(sys.argv) > 4 else "0.25").split(",")]
n_src_override = int(sys.argv[5]) if len(sys.argv) > 5 else None
n_src, n_tgt, seed = WORKLOADS[wl]
sc = synth.make_scene(n_src, n_tgt, seed=seed)
if n_src_override:
    n_src = n_src_override
dev = torch.device("cuda", 0)
d_t, d_tn = torch.from_numpy(sc.tgt_xyz).to(dev), torch.from_numpy(sc.tgt_nrm).to(dev)
d_s, d_sn = torch.from_numpy(sc.src_xyz[:n_src].copy()).to(dev), torch.from_numpy(sc.src_nrm[:n_src].copy()).to(dev)
torch.cuda.synchronize()
T0 = None
print(f"workload {wl}: {n_src} -> {n_tgt}", flush=True)
for occ, ratio, rho in itertools.product(occs, ratios, rhos):
    os.environ["O3D_BIN_OCC"], os.environ["O3D_HALO_RATIO"], os.environ["O3D_HALO_RHO"] = str(occ), str(ratio), str(rho)
    p = capi.shipped_params()
    p.use_xicp = 0
    p.fixed_iters = ITERS
    p.profile_loop = 0
    try:
        reg = capi.Registration(p)
        reg.set_target_device(d_t.data_ptr(), 3, n_tgt, d_tn.data_ptr(), 3)
        reg.set_source_device(d_s.data_ptr(), 3, n_src, d_sn.data_ptr(), 3)
        info = reg.target_info()
        ms = []
        for k in range(8):
            T, res = reg.register(np.eye(4))
            if k >= 2:
                ms.append(res.loop_ms)
        reg.close()
        p.profile_loop = 1
        reg = capi.Registration(p)
        reg.set_target_device(d_t.data_ptr(), 3, n_tgt, d_tn.data_ptr(), 3)
        reg.set_source_device(d_s.data_ptr(), 3, n_src, d_sn.data_ptr(), 3)
        reg.register(np.eye(4))
        _, pr = reg.register(np.eye(4))
        reg.close()
    except capi.RegError as e:
        print(f"occ {occ:5.1f} ratio {ratio:4.2f} rho {rho:4.2f}: {e}", flush=True)
        continue
    if T0 is None:
        T0 = T
    same = bool(np.array_equal(T, T0))
    km = pr.prof_ms[0] / max(pr.prof_launches[0], 1) * 1e3
    kf = (pr.prof_ms[1] + pr.prof_ms[2]) / max(pr.prof_launches[1], 1) * 1e3
    kf1 = pr.prof_ms[1] / max(pr.prof_launches[1], 1) * 1e3
    print(f"occ {occ:5.1f} ratio {ratio:4.2f} rho {rho:4.2f}: cell {info.cell_size:.4f} table {info.table_bytes / 1e6:8.1f} MB "
          f"build {res.target_build_ms:7.2f} ms | loop min {min(ms):.3f} med {sorted(ms)[len(ms) // 2]:.3f} ms | "
          f"k_match {pr.prof_launches[0]:2d} x {km:6.1f} us, k_iter_fused {pr.prof_launches[1]:2d} x {kf:6.1f} us (check {kf1:5.1f}) | "
          f"stalls {res.n_band_stalls} same pose {same}", flush=True)
