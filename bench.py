#!/usr/bin/env python3
"""Headline benchmark: ICP iterations/sec of scan-to-map registration on MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c2|c3|c4|tiny] [--mode strong|weak|replicas]
                  [--dump-outputs DIR]

A "step" is ONE registration of the synthetic scan against the synthetic map with exactly ITERS (=20) Gauss-Newton
iterations of the reference's chain (param/icp.yaml: knn 1, maxDist 0.5, TrimmedDist 0.9, SurfaceNormal 1.57,
point-to-plane): R2 reading prep + 20 x (R3 transform, R4 exact 1-NN, R5 trimmed quantile + normal filter, R7 normal
equations, R8 6x6 solve, R9 pose update) + R10.  Inputs are resident in HBM before the timed region; the target
voxel-bin build (== kd-tree build of the reference) is excluded on both sides and reported as target_build_ms, the
per-scan reading upload + ordering as source_prep_ms.

N = 1 (default): workload C3 = 200k -> 5M points, the largest single-GPU configuration of BASELINE.json and the size its
        metric is quoted on ("100k->5M-pt scan-to-map").  The same line carries, as secondary objects the driver times
        too: C2 (100k -> 1M), the C4 map on one GPU (whole 200k reading and one rank's 25k slice against the 20M-point
        map), 8 registrations in flight on 8 HIP streams (C5 analogue), the GICP cost, and the shipped chain with its
        degeneracyAwareness (R8x) switched on.
N > 1: workload C4 as BASELINE.json states it: ONE 200k-point reading split into N contiguous slices (200k/N points per
        rank), the 20M-point map replicated on every GPU, per iteration the ranks exchange the trimmed-quantile data and
        the 32-double (H, b, e, counts) record over RCCL.  STRONG scaling: `value` = ITERS * K / t, whole-reading
        iterations per second.  `--mode weak` (explicit) keeps the reading at 200k points PER RANK instead.

--mode replicas (any N): BASELINE.json configs[4] -- 64 independent C2-shaped registrations (seed + i), 64 / N per rank, 8 in
        flight per GPU (one handle + HIP stream + host thread each), NO collectives; a "step" is one pass over the 64
        registrations, `value` the aggregate ICP iterations/s of all ranks; every timed pose is checked against the same
        problem registered alone on its GPU afterwards.  WEAK scaling (per-GPU work is fixed at 64 / N ... of a fixed batch:
        "strong" in the batch, reported as such).

Prints ONE JSON line (rank 0).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ITERS = 20
WORKLOADS = {"c2": (100_000, 1_000_000, 1234 + 2), "c3": (200_000, 5_000_000, 1234 + 3),
             "c4": (200_000, 20_000_000, 1234 + 4), "tiny": (10_000, 100_000, 1234 + 1)}
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_MEASURED_GBS = 6290.0   # ... and 6.29 TB/s measured (float4 copy): the secondary denominator SURVEY 8d asks for
# algorithmic bytes per reading point and launch:
#   k_match_g8  : src xyz 12 + matched tgt xyz 12 + pos 4 + d2 4 written            = 32
#   fused_pair  : src xyz 12 + src normal 12 + matched tgt xyz 12 + tgt normal 12 (P2Pl) = 48
#                 (k_coh_check + k_coh_search: the fused iteration's search + linearisation, two launches)
#   k_tail      : the persistent settled-tail kernel, per ITERATION it runs: the same 48 (its per-point state never leaves LDS)
KERNEL_BYTES_PER_POINT = {"k_match_g8": 32, "fused_pair": 48}
ITER_BYTES_PER_POINT = 64    # P2Pl 48 B + 16 B (id, d2 written and re-read) for the split-kernel variant


def chain_params(capi, device, xicp=0):
    """The measured chain: the shipped icp.yaml with epsilon 0, fixed 20 iterations; R8x off unless asked."""
    p = capi.shipped_params()
    p.fixed_iters = ITERS
    p.device = device
    p.use_xicp = xicp
    return p


def cpu_baseline(sc, threads, legs=("omp", "1t")):
    """The oracle (faithful C restatement; the reference itself cannot be built here) timed on the host cores: same
    clouds, same chain, same 20 iterations on both legs, kd-tree build excluded.  Returns (figures, T of the OpenMP leg)."""
    from oracle import oracle as orc
    out = {}
    T_omp = None
    for name, nt in (("omp", threads), ("1t", 1)):
        if name not in legs:
            continue
        T, r = orc.icp_p2pl(sc.tgt_xyz, sc.tgt_nrm, sc.src_xyz, sc.src_nrm, max_dist=0.5, trim_ratio=0.9,
                            max_normal_angle=1.57, fixed_iters=ITERS, n_threads=nt)
        out[name] = ITERS / r.loop_seconds
        if name == "omp":
            T_omp = T
    return out, T_omp


DUMP_LIMIT_BYTES = 64 << 20
# What reg_register / reg_dist_register hand back besides the pose: RegResult fields that are results of the computation.
# Timings (loop_ms, target_build_ms, source_prep_ms, prof_*) and statistics of how the loop ran (band stalls, tail launches
# and iterations) are left out: they differ from run to run or between builds that compute the same thing.  `error` is an fp64
# sum whose reduction order is not fixed: its last bits can differ between two runs (measured: 4e-15 of 14.05 at C3).
RESULT_FIELDS = ("iterations", "converged", "max_iter_reached", "rank_last", "n_inliers", "n_matched", "error", "fitness",
                 "inlier_rmse", "H_last", "b_last", "T_iter_last", "T_iter_prev", "n_constraints", "localizable",
                 "xicp_combined", "xicp_high", "rotation_corrected")
COLUMN_MAJOR_4X4 = ("T_iter_last", "T_iter_prev")


def step_outputs(T, res):
    """The arrays a caller of the timed step receives: the pose and the result fields above, as float32 / float64.
    4x4 transforms in math layout (the ABI stores them column-major), H_last as 6x6."""
    out = {"pose": np.asarray(T, dtype=np.float32).reshape(4, 4)}
    for name in RESULT_FIELDS:
        v = getattr(res, name)
        a = np.array(v[:] if hasattr(v, "__len__") else v, dtype=np.float64)   # exact for the int32 / int64 / float fields
        if name in COLUMN_MAJOR_4X4:
            a = a.reshape(4, 4).T.copy()
        elif name == "H_last":
            a = a.reshape(6, 6)
        out[name] = a
    return out


def dump_outputs(directory, arrays):
    """--dump-outputs: one DIR/<name>.npy per array (float32 / float64 only, DUMP_LIMIT_BYTES in all)."""
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(directory, name + ".npy"), a)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


class stdout_to_stderr:
    """RCCL prints a version banner on fd 1 when a communicator is created; this script's stdout carries exactly ONE JSON
    line, so fd 1 points at stderr while groups are being set up."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)


class DeviceScene:
    """A synthetic scene resident in HBM (torch tensors are only the allocation: plumbing)."""

    def __init__(self, torch, dev, sc, lo=0, hi=None, with_cov=False):
        self.sc = sc
        self.n_tgt = sc.tgt_xyz.shape[0]
        hi = sc.src_xyz.shape[0] if hi is None else hi
        self.n_src = hi - lo
        self.tgt = torch.from_numpy(sc.tgt_xyz).to(dev)
        self.tnrm = torch.from_numpy(sc.tgt_nrm).to(dev)
        self.src = torch.from_numpy(np.ascontiguousarray(sc.src_xyz[lo:hi])).to(dev)
        self.snrm = torch.from_numpy(np.ascontiguousarray(sc.src_nrm[lo:hi])).to(dev)
        self.tcov = self.scov = None
        if with_cov:
            self.tcov = torch.from_numpy(sc.tgt_cov).to(dev)
            self.scov = torch.from_numpy(np.ascontiguousarray(sc.src_cov[lo:hi])).to(dev)
        torch.cuda.synchronize()

    def make_reg(self, capi, p, n_src=None):
        reg = capi.Registration(p)
        if p.cost == capi.COST_GICP:
            reg.set_target_device(self.tgt.data_ptr(), 3, self.n_tgt, None, 3, self.tcov.data_ptr())
            reg.set_source_device(self.src.data_ptr(), 3, n_src or self.n_src, None, 3, self.scov.data_ptr())
        else:
            reg.set_target_device(self.tgt.data_ptr(), 3, self.n_tgt, self.tnrm.data_ptr(), 3)
            reg.set_source_device(self.src.data_ptr(), 3, n_src or self.n_src, self.snrm.data_ptr(), 3)
        return reg


def time_registrations(torch, reg, T_init, steps, warmup=2):
    for _ in range(warmup):
        out = reg.register(T_init)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = reg.register(T_init)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_profile(capi, ds, local_rank):
    """One more registration with begin/end HIP events attached to every search-kernel dispatch on the handle's own
    stream (profile_loop) -> average launch duration over the SAME 20-iteration trajectory the timed region ran;
    rocprofv3 --kernel-trace of this command must agree."""
    p = chain_params(capi, local_rank)
    p.profile_loop = 1
    preg = ds.make_reg(capi, p)
    T_init = np.eye(4, dtype=np.float32)
    preg.register(T_init)
    _, pres = preg.register(T_init)
    kern = {}
    for idx, name in ((0, "k_match_g8"), (1, "k_coh_check"), (2, "k_coh_search")):
        if pres.prof_launches[idx]:
            kern[name] = {"launches": int(pres.prof_launches[idx]), "total_ms": float(pres.prof_ms[idx]),
                          "avg_ms": float(pres.prof_ms[idx]) / int(pres.prof_launches[idx])}
    if pres.prof_launches[3]:
        # the persistent tail: ONE launch runs many iterations; avg_ms is per ITERATION (what a fused pair + update launch was)
        its = max(int(pres.n_tail_iterations), 1)
        kern["k_tail"] = {"launches": int(pres.prof_launches[3]), "total_ms": float(pres.prof_ms[3]), "iterations": its,
                          "avg_ms": float(pres.prof_ms[3]) / its, "avg_ms_is": "per iteration (search + linearisation + exchange "
                          "+ band select + solve + update of every settled iteration)"}
    if "k_coh_check" in kern:
        # the fused iteration's search + linearisation = the pair of launches (shortcut test + queued full searches)
        tot = kern["k_coh_check"]["total_ms"] + kern.get("k_coh_search", {"total_ms": 0.0})["total_ms"]
        kern["fused_pair"] = {"launches": kern["k_coh_check"]["launches"], "total_ms": tot,
                              "avg_ms": tot / kern["k_coh_check"]["launches"], "kernels": "k_coh_check + k_coh_search"}
    preg.close()
    return kern


def pmc_traffic(workload, dom):
    """HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process; the number comes from the
    committed rocprofv3 --pmc passes of THIS command (tools/collect_profiles.sh; FETCH_SIZE doubled as the gfx950 guide
    prescribes and as the stream-kernel calibration in that file confirms)."""
    for name in ("r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
        try:
            pj = json.load(open(os.path.join(ROOT, "profiles", name)))
            if pj.get("workload", "c2") != workload:
                continue
            for kname, kv in pj["kernels"].items():
                if kname.startswith(dom):
                    return kv.get("hbm_bytes_per_iteration_corrected", kv["hbm_bytes_per_launch_corrected"]), (f"STATIC: read from the committed profiles/{name} (rocprofv3 --pmc passes of "
                                                                  "this command, 2*FETCH_SIZE + WRITE_SIZE per launch), not measured in this run")
        except (OSError, KeyError, ValueError):
            pass
    return None, None


def run_replicas(args, torch, capi, synth, dist, dev, rank, local_rank, world):
    """BASELINE.json configs[4]: `--replicas` (64) independent C2-shaped registrations (seed + i), split over the ranks, 8 in
    flight per GPU -- one handle, one HIP stream and one host thread each -- and no collective (replicas only; the
    reference analogue is the per-submap-pair loop of PlaceRecognition.cpp:71-111).  One step = one pass over the whole batch."""
    import gc
    import threading
    n_src, n_tgt, seed0 = WORKLOADS["c2"]
    total = args.replicas
    mine = list(range(rank, total, world))          # round-robin: equal shares whenever world divides the batch
    S = min(args.streams, max(1, len(mine)))
    T_init = np.eye(4, dtype=np.float32)
    keep, regs = [], []
    for i in mine:
        sc = synth.make_scene(n_src, n_tgt, seed=seed0 + 100 + i)
        dsi = DeviceScene(torch, dev, sc)
        regs.append(dsi.make_reg(capi, chain_params(capi, local_rank)))
        dsi.sc = None                                # host copies are not needed any more
        keep.append(dsi)
        del sc
    groups = [list(range(k, len(regs), S)) for k in range(S)]
    poses = [None] * len(regs)

    def one_pass_all(n_pass):
        go = threading.Barrier(S + 1)
        errs = []

        def work(idx):
            try:
                go.wait()
                for _ in range(n_pass):
                    for j in idx:
                        poses[j] = regs[j].register(T_init)[0]
            except Exception as e:   # noqa: BLE001
                errs.append(repr(e))
            finally:
                go.wait()

        ths = [threading.Thread(target=work, args=(g,)) for g in groups]
        for th in ths:
            th.start()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        go.wait()
        t0 = time.perf_counter()
        go.wait()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        for th in ths:
            th.join()
        if errs:
            raise SystemExit("replica registration failed: " + errs[0])
        return el

    gc.collect()
    gc.disable()
    one_pass_all(max(1, args.warmup))
    elapsed = one_pass_all(args.steps)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # every timed pose against the same problem registered ALONE on this GPU (single stream, nothing else in flight)
    timed = [np.array(p) for p in poses]
    dmax = 0.0
    for j, r in enumerate(regs):
        Tj = r.register(T_init)[0]
        dmax = max(dmax, float(np.abs(np.asarray(Tj) - timed[j]).max()))
    ok = dmax <= 2e-6
    # ... and a sample of them against the truth of its scene is implicit in tests/test_gpu_fullsize.py (oracle parity of C2)
    if dist is not None:
        t = torch.tensor([dmax], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dmax = float(t.item())
        ok = dmax <= 2e-6
    for r in regs:
        r.close()
    if rank == 0:
        line = {
            "metric": "ICP iterations/sec (batched submap registrations, one per HIP stream)",
            "value": total * ITERS * args.steps / elapsed, "unit": "iter/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"c5: {total} independent registrations {n_src} -> {n_tgt} points (seed + i), {ITERS} iterations "
                                   "each, icp.yaml chain as the headline; one step = one pass over the batch",
                       "registrations": total, "registrations_per_gpu": len(mine), "streams_per_gpu": S,
                       "n_source": n_src, "n_target": n_tgt, "iterations_per_registration": ITERS,
                       "parallelism": f"replicas only: {total} registrations over {world} GPU(s), {S} handles / HIP streams / host "
                                      "threads in flight per GPU, no collective"},
            "poses_equal_single_stream": bool(ok), "max_abs_pose_diff_vs_single_stream": dmax,
            "ms_per_registration_amortised": 1e3 * elapsed / (args.steps * max(len(mine), 1)),
            "note": "total work (the 64-registration batch) is fixed as N grows: per-GPU efficiency = value(N) / (N * value(1))",
        }
        print(json.dumps(line), flush=True)
    if rank == 0 and args.dump_outputs:
        # this rank's share of the batch, as its last timed pass left it (registration i of the batch = seed + 100 + i)
        dump_outputs(args.dump_outputs, {"poses": np.stack(timed).astype(np.float32),
                                         "registration_ids": np.array(mine, dtype=np.float64)})
    if not ok:
        raise SystemExit(f"replicas: a timed pose differs from its single-stream registration by {dmax}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help="default: c3 on one GPU, c4 (200k -> 20M, reading split over the ranks) on N > 1")
    ap.add_argument("--mode", default="strong", choices=("strong", "weak", "replicas"),
                    help="N > 1 only.  strong (default, = BASELINE config C4): ONE reading split into N slices; "
                         "weak: every rank holds a full-size slice of an N-times larger reading; replicas (any N): BASELINE "
                         "configs[4], 64 independent C2 registrations split over the ranks, 8 streams per GPU, no collectives")
    ap.add_argument("--replicas", type=int, default=64, help="--mode replicas: registrations in the batch (all ranks together)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the secondary objects (C2, C4 map, batched, GICP, R8x)")
    ap.add_argument("--streams", type=int, default=8,
                    help="secondary measurement (config 5 analogue): S independent C2 registrations in flight, one handle "
                         "+ HIP stream + host thread each; reported under \"batched\", never as `value`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (pose and result fields; "
                         "--mode replicas: the poses of the batch) as DIR/<name>.npy; same arguments, same inputs")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with WORLD_SIZE={args.gpus} (got {world})")

    import gc
    import torch  # plumbing only: device buffers, streams, torch.distributed
    from open3d_slam_private_amd import capi, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the registration path has no CPU fallback")
    backend = os.environ.get("O3D_BENCH_BACKEND", "nccl")   # "gloo": rehearsal of the N>1 path on a 1-GPU box
    if backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()   # rehearsal: several ranks share the one GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        with stdout_to_stderr():
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
                dist.barrier()          # forms the communicator now (its banner goes to stderr)
            else:
                dist.init_process_group(backend)

    if args.mode == "replicas":
        run_replicas(args, torch, capi, synth, dist, dev, rank, local_rank, world)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    force_dist = os.environ.get("O3D_BENCH_FORCE_DIST") == "1"   # rehearsal: N>1 code path with one rank
    multi = world > 1 or force_dist
    workload = args.workload or ("c4" if multi else "c3")
    n_src, n_tgt, seed = WORKLOADS[workload]
    if multi and args.mode == "weak":
        sc = synth.make_scene(n_src * world, n_tgt, seed=seed)
        lo, hi = rank * n_src, (rank + 1) * n_src
    else:
        sc = synth.make_scene(n_src, n_tgt, seed=seed)
        lo, hi = (rank * n_src) // world, ((rank + 1) * n_src) // world
    n_global = sc.src_xyz.shape[0]
    n_local = hi - lo
    ds = DeviceScene(torch, dev, sc, lo, hi)
    T_init = np.eye(4, dtype=np.float32)

    p = chain_params(capi, local_rank)
    reg = capi.Registration(p)
    loop_kind = None
    if not multi:
        reg.set_target_device(ds.tgt.data_ptr(), 3, n_tgt, ds.tnrm.data_ptr(), 3)
        reg.set_source_device(ds.src.data_ptr(), 3, n_local, ds.snrm.data_ptr(), 3)

        def step():
            return reg.register(T_init)
    else:
        # The multi-GPU loop lives behind the C ABI (reg_dist_register, host_rccl.hpp): C++ steering, the library's kernels
        # and RCCL collectives on the handle's own stream, no host synchronisation inside an iteration.  torch.distributed
        # is only used to hand rank 0's ncclUniqueId to the other ranks and for the barrier / max-over-ranks timing.
        reg.set_target_device(ds.tgt.data_ptr(), 3, n_tgt, ds.tnrm.data_ptr(), 3)
        reg.set_source_device(ds.src.data_ptr(), 3, n_local, ds.snrm.data_ptr(), 3)
        if backend == "nccl":
            uid = [capi.dist_unique_id() if rank == 0 else None]
            if dist is not None:
                dist.broadcast_object_list(uid, src=0)
            with stdout_to_stderr():
                reg.dist_init(uid[0], rank, world)
                reg.dist_register(T_init)     # first collectives (lazy channel set-up) before anything is timed
            loop_kind = "reg_dist_register: C++ loop, RCCL"
        else:
            # rehearsal on a 1-GPU box (several ranks share the GPU, where RCCL refuses to form a group): same C++ loop,
            # bytes moved by the torch.distributed backend through host staging
            from open3d_slam_private_amd.distributed import host_staged_transport
            ar, ag = host_staged_transport(dist, dev)
            reg.dist_init_custom(ar, ag, rank, world)
            loop_kind = f"reg_dist_register: C++ loop, {backend} host-staged transport (rehearsal)"

        def step():
            return reg.dist_register(T_init)
    info = reg.target_info()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # CPython's cyclic collector is off while anything is timed (as timeit does): the first full collection of a process that
    # imported torch takes 40-55 ms and comes around the 250th registration (tools/tools_sustained2.py)
    gc.collect()
    gc.disable()
    for _ in range(args.warmup):
        out = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    T_final, res_final = out[0], out[1]
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, step_outputs(T_final, res_final))

    # ---- kernel-level numbers (outside the timed region) ----
    kern = {}
    if not multi:
        kern = kernel_profile(capi, ds, local_rank)
    else:
        prof = reg.profile_kernels(np.eye(4, dtype=np.float32), reps=20)
        kern["k_match_g8"] = {"launches": 20, "total_ms": 20 * prof["match_ms"], "avg_ms": prof["match_ms"]}
    dom = max((k for k in kern if k in KERNEL_BYTES_PER_POINT), key=lambda k: kern[k]["total_ms"])
    bytes_pp = KERNEL_BYTES_PER_POINT[dom]
    achieved = n_local * bytes_pp / (kern[dom]["avg_ms"] * 1e-3) / 1e9
    traffic, traffic_src = pmc_traffic(workload, dom) if not multi else (None, None)

    # ---- N > 1: the SAME workload (whole reading, same map) on rank 0's GPU alone, plain single-GPU loop: the denominator
    #      of an honest strong-scaling figure (N = 1 of this script is the C3 headline, a different workload)
    single = None
    if multi and rank == 0:
        ds1 = DeviceScene(torch, dev, sc)
        r1 = ds1.make_reg(capi, chain_params(capi, local_rank))
        s_steps = max(3, args.steps // 4)
        t1, (T1, _res1) = time_registrations(torch, r1, T_init, s_steps)
        single = {"value": ITERS * s_steps / t1, "unit": "iter/s", "ms_per_registration": 1e3 * t1 / s_steps,
                  "n_source": int(sc.src_xyz.shape[0]), "same_pose_as_group": bool(np.array_equal(T1, T_final)),
                  "note": "whole reading against the same map on ONE GPU (reg_register), timed after the group's run"}
        r1.close()
        del ds1
        torch.cuda.empty_cache()

    # ---- secondary objects (single GPU only; never `value`) ----
    extras = {}
    if not multi and not args.no_extras:
        x_steps = max(3, args.steps // 4)
        # (1) the shipped chain with its degeneracyAwareness (R8x: first-iteration localizability analysis + constrained
        #     solve) ON -- reg_shipped_params() as it comes; the headline chain is SURVEY 8d's (without it)
        xreg = ds.make_reg(capi, chain_params(capi, local_rank, xicp=1))
        tx, (Tx, xres) = time_registrations(torch, xreg, T_init, x_steps)
        extras["xicp"] = {"value": ITERS * x_steps / tx, "unit": "iter/s", "ms_per_registration": 1e3 * tx / x_steps,
                          "workload": workload, "localizable": list(xres.localizable),
                          "n_constraints": int(xres.n_constraints),
                          "same_pose_as_plain_chain": bool(np.array_equal(Tx, T_final))}
        xreg.close()
        # (1a) the shipped chain as the mapper runs it: its own transformation checkers decide when to stop
        #      (Differential 0.001 / 0.008 / 3, Counter 30) instead of the metric's fixed 20 iterations
        pc = capi.shipped_params()
        pc.device = local_rank
        creg = ds.make_reg(capi, pc)
        tc, (Tc, cres) = time_registrations(torch, creg, T_init, x_steps)
        ct, cr = synth.pose_error(Tc, sc.T_true)
        extras["shipped_checkers"] = {"ms_per_registration": 1e3 * tc / x_steps, "iterations": int(cres.iterations),
                                      "iter_per_s": int(cres.iterations) * x_steps / tc, "workload": workload,
                                      "converged": bool(cres.converged), "pose_vs_truth": {"trans_m": ct, "rot_rad": cr}}
        # ... and from a prior as good as the mapper's odometry usually is (0.2 deg / 2 cm off the truth instead of the
        #     benchmark's 2 deg / 0.19 m): the first searches stay inside the halo level
        Tn = np.array(sc.T_true, np.float64)
        dT = np.eye(4)
        dT[:3, :3] = synth.rpy_to_R(np.radians(0.1), np.radians(-0.1), np.radians(0.2))
        dT[:3, 3] = (0.015, -0.01, 0.005)
        T_near = (dT @ Tn).astype(np.float32)
        tn, (Tnr, nres) = time_registrations(torch, creg, T_near, x_steps)
        nt, nr = synth.pose_error(Tnr, sc.T_true)
        extras["shipped_checkers_near_prior"] = {"ms_per_registration": 1e3 * tn / x_steps, "iterations": int(nres.iterations),
                                                 "prior_error": "0.2 deg, 2 cm", "workload": workload,
                                                 "pose_vs_truth": {"trans_m": nt, "rot_rad": nr}}
        # ... and from priors far off (3 deg / 25 cm, sigma per axis: 5 deg / 0.4 m typical): registrations that sit on a plateau of
        #     the trimmed limit before they snap in -- the case the pose-step gate of the loop is for
        frng = np.random.default_rng(1)
        f_t, f_it, f_stalls = [], [], 0
        for _ in range(12):
            dT = np.eye(4)
            dT[:3, :3] = synth.rpy_to_R(*frng.normal(scale=0.05, size=3))
            dT[:3, 3] = frng.normal(scale=0.25, size=3)
            T_far = (dT @ Tn).astype(np.float32)
            creg.register(T_far)
            torch.cuda.synchronize()
            tf0 = time.perf_counter()
            Tfr, fres = creg.register(T_far)
            torch.cuda.synchronize()
            f_t.append(time.perf_counter() - tf0)
            f_it.append(int(fres.iterations))
            f_stalls += int(fres.n_band_stalls)
        extras["shipped_checkers_far_priors"] = {"ms_per_registration_mean": 1e3 * float(np.mean(f_t)),
                                                 "ms_per_registration_median": 1e3 * float(np.median(f_t)),
                                                 "iterations_mean": float(np.mean(f_it)), "band_stalls_per_registration": f_stalls / 12.0,
                                                 "priors": "12 draws, rotation sigma 0.05 rad per axis, translation sigma 0.25 m per axis",
                                                 "workload": workload}
        creg.close()
        # (1b) the GICP cost (the north star's cost function; parity unpinned) on the headline clouds
        if True:
            tcov = torch.from_numpy(sc.tgt_cov).to(dev)
            scov = torch.from_numpy(np.ascontiguousarray(sc.src_cov[lo:hi])).to(dev)
            pgh = capi.default_params()
            pgh.cost = capi.COST_GICP
            pgh.use_trimmed = 0
            pgh.max_dist = 0.5
            pgh.fixed_iters = ITERS
            pgh.device = local_rank
            gh = capi.Registration(pgh)
            gh.set_target_device(ds.tgt.data_ptr(), 3, n_tgt, None, 3, tcov.data_ptr())
            gh.set_source_device(ds.src.data_ptr(), 3, n_local, None, 3, scov.data_ptr())
            tgh, (Tgh, _gres) = time_registrations(torch, gh, T_init, x_steps)
            ght, ghr = synth.pose_error(Tgh, sc.T_true)
            extras["gicp_headline_clouds"] = {"value": ITERS * x_steps / tgh, "unit": "iter/s",
                                              "ms_per_registration": 1e3 * tgh / x_steps, "workload": workload,
                                              "pose_vs_truth": {"trans_m": ght, "rot_rad": ghr}}
            gh.close()
            del tcov, scov
            torch.cuda.empty_cache()
        if workload != "tiny":
            # (2) C2 (BASELINE configs[1]): 100k -> 1M
            n2, m2, s2 = WORKLOADS["c2"]
            sc2 = synth.make_scene(n2, m2, seed=s2)
            ds2 = DeviceScene(torch, dev, sc2, with_cov=True)
            r2 = ds2.make_reg(capi, chain_params(capi, local_rank))
            t2, (T2, res2) = time_registrations(torch, r2, T_init, args.steps)
            e2t, e2r = synth.pose_error(T2, sc2.T_true)
            k2 = kernel_profile(capi, ds2, local_rank)
            extras["c2"] = {"value": ITERS * args.steps / t2, "unit": "iter/s", "ms_per_registration": 1e3 * t2 / args.steps,
                            "workload": f"c2: {n2} -> {m2}", "pose_vs_truth": {"trans_m": e2t, "rot_rad": e2r},
                            "kernels": k2, "target_build_ms": float(res2.target_build_ms),
                            "source_prep_ms": float(res2.source_prep_ms)}
            # (3) config 5 analogue on one GPU: S independent C2 registrations in flight, one HIP stream + host thread each
            if args.streams > 1:
                import threading
                regs = []
                for _ in range(args.streams):
                    r = ds2.make_reg(capi, chain_params(capi, local_rank))
                    r.register(T_init)
                    regs.append(r)
                per = max(2, args.steps // 2)
                rates = []
                lastT = [None] * args.streams
                for _rep in range(3):       # the aggregate depends on how the streams land on the hardware queues: 3 runs
                    go = threading.Barrier(args.streams + 1)

                    def work(r, i):
                        go.wait()
                        for _ in range(per):
                            lastT[i] = r.register(T_init)[0]   # ctypes releases the GIL: the host threads really run in parallel
                        go.wait()

                    ths = [threading.Thread(target=work, args=(r, i)) for i, r in enumerate(regs)]
                    for th in ths:
                        th.start()
                    torch.cuda.synchronize()
                    go.wait()
                    tb0 = time.perf_counter()
                    go.wait()
                    tb = time.perf_counter() - tb0
                    for th in ths:
                        th.join()
                    rates.append(args.streams * per * ITERS / tb)
                rates.sort()
                # every stream's pose against the single-stream registration of the same clouds (T2): a registration that is not
                # alone on the device runs the three-launch iteration instead of the persistent tail -- same ids, sums equal up
                # to the fp64 summation order
                dmax = max(float(np.abs(np.asarray(Ti) - np.asarray(T2)).max()) for Ti in lastT)
                assert dmax <= 2e-6, f"batched registrations disagree with the single-stream pose by {dmax}"
                extras["batched"] = {"streams": args.streams, "registrations": args.streams * per, "workload": "c2",
                                     "iter_per_s": rates[1], "iter_per_s_min_max_of_3": [rates[0], rates[2]],
                                     "ms_per_registration_amortised": 1e3 * ITERS / rates[1],
                                     "max_abs_pose_diff_vs_single_stream": dmax}
                for r in regs:
                    r.close()
            # (4) the GICP cost (the north star's cost function; SURVEY 8d: 72 B/pt + 16 B/pt for the split kernels) on
            #     the C2 clouds, covariances from the analytic normals
            pg = capi.default_params()
            pg.cost = capi.COST_GICP
            pg.use_trimmed = 0
            pg.max_dist = 0.5
            pg.fixed_iters = ITERS
            pg.device = local_rank
            greg = ds2.make_reg(capi, pg)
            tg, (Tg, gres) = time_registrations(torch, greg, T_init, x_steps)
            gt, gr = synth.pose_error(Tg, sc2.T_true)
            extras["gicp"] = {"value": ITERS * x_steps / tg, "unit": "iter/s", "ms_per_registration": 1e3 * tg / x_steps,
                              "workload": "c2", "bytes_per_point": 88,
                              "achieved_GBs_end_to_end": n2 * 88 * ITERS * x_steps / tg / 1e9,
                              "pose_vs_truth": {"trans_m": gt, "rot_rad": gr},
                              "note": "GICP parity is unpinned against the reference (Open3D 0.15.1 arithmetic not in "
                                      "tree); checked against the float64 oracle in tests/test_gpu_parity.py"}
            greg.close()
            r2.close()
            del ds2, sc2
            torch.cuda.empty_cache()
            # (5) the C4 map (20M points) on ONE GPU: the whole 200k reading, and one rank's slice of an 8-way split
            if workload != "c4":
                n4, m4, s4 = WORKLOADS["c4"]
                sc4 = synth.make_scene(n4, m4, seed=s4)
                ds4 = DeviceScene(torch, dev, sc4)
                r4 = ds4.make_reg(capi, chain_params(capi, local_rank))
                t4, (T4, res4) = time_registrations(torch, r4, T_init, x_steps)
                e4t, e4r = synth.pose_error(T4, sc4.T_true)
                i4 = r4.target_info()
                r4s = ds4.make_reg(capi, chain_params(capi, local_rank), n_src=n4 // 8)
                t4s, _ = time_registrations(torch, r4s, T_init, x_steps)
                extras["c4_one_gpu"] = {
                    "value": ITERS * x_steps / t4, "unit": "iter/s", "ms_per_registration": 1e3 * t4 / x_steps,
                    "workload": f"c4 map on one GPU: {n4} -> {m4}", "pose_vs_truth": {"trans_m": e4t, "rot_rad": e4r},
                    "target_build_ms": float(res4.target_build_ms), "cell_size_m": i4.cell_size,
                    "table_MB": i4.table_bytes / 1e6,
                    "one_rank_slice": {"points": n4 // 8, "iter_per_s": ITERS * x_steps / t4s,
                                       "ms_per_registration": 1e3 * t4s / x_steps,
                                       "note": "what ONE of 8 ranks computes per registration, no collectives: "
                                               "(this / value) / 8 bounds the 8-GPU strong-scaling efficiency from above"}}
                r4.close()
                r4s.close()
                del ds4, sc4
                torch.cuda.empty_cache()

    if rank == 0:
        if multi and args.mode == "weak":
            value = world * ITERS * args.steps / elapsed     # n_src-point iteration units
            scaling = "weak"
        else:
            value = ITERS * args.steps / elapsed              # whole-reading iterations
            scaling = "strong" if multi else None             # N = 1: the label means nothing
        line = {
            "metric": "ICP iterations/sec (scan-to-map)",
            "value": value, "unit": "iter/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": scaling,
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{workload}: scan-to-map point-to-plane ICP {n_global} -> {n_tgt} points, "
                                   f"{ITERS} iterations/registration, icp.yaml chain (exact 1-NN, maxDist 0.5, "
                                   "Trimmed 0.9, SurfaceNormal 1.57), degeneracyAwareness off (SURVEY 8d; with it: \"xicp\")",
                       "n_source": n_global, "n_source_per_gpu": n_local, "n_target": n_tgt, "iterations_per_step": ITERS,
                       "parallelism": (f"reading point-partitioned x{world} ({args.mode} scaling), map replicated, {loop_kind}"
                                       if multi else "single GPU"),
                       "dist_loop": (reg.dist_info() if multi else None),
                       "use_xicp": 0, "cell_size_m": info.cell_size, "n_bricks": info.n_bricks,
                       "table_MB": info.table_bytes / 1e6},
            "roofline": {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "peak_measured": HBM_MEASURED_GBS,
                         "frac_of_measured_peak": achieved / HBM_MEASURED_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": n_local * bytes_pp,
                         "kernel_ms": kern[dom]["avg_ms"], "launches": kern[dom]["launches"],
                         "bytes_per_point": bytes_pp,
                         "limiter": "latency of dependent round trips, then Infinity-Cache/HBM fetches of the candidate "
                                    "records an exact search has to look at (DESIGN.md section 6, profiles/)"},
            "roofline_tail": (None if multi or "k_tail" not in kern else {
                "bound": "hbm", "kernel": "k_tail (persistent settled tail), per iteration",
                "achieved": n_local * 48 / (kern["k_tail"]["avg_ms"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": n_local * 48 / (kern["k_tail"]["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "traffic": pmc_traffic(workload, "k_tail")[0], "algorithmic_bytes_per_iteration": n_local * 48,
                "iteration_ms": kern["k_tail"]["avg_ms"], "iterations": kern["k_tail"]["iterations"],
                "launches": kern["k_tail"]["launches"],
                "note": "replaces k_coh_check + k_coh_search + k_reduce_update of every settled iteration (round 2: roofline_fused)"}),
            "roofline_fused": (None if multi or "fused_pair" not in kern else {
                "bound": "hbm", "kernel": "k_coh_check + k_coh_search (settled iterations: search + linearisation)",
                "achieved": n_local * 48 / (kern["fused_pair"]["avg_ms"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": n_local * 48 / (kern["fused_pair"]["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "traffic": pmc_traffic(workload, "fused_pair")[0], "algorithmic_bytes_per_launch": n_local * 48,
                "kernel_ms": kern["fused_pair"]["avg_ms"], "launches": kern["fused_pair"]["launches"]}),
            "kernels": kern,
            "roofline_iteration": {"bytes_per_point": ITER_BYTES_PER_POINT,
                                   "achieved_GBs_end_to_end": n_global * ITER_BYTES_PER_POINT * ITERS * args.steps / elapsed / 1e9},
            "target_build_ms": float(res_final.target_build_ms) if not multi else None,
            "source_prep_ms": float(res_final.source_prep_ms) if not multi else None,
            "band_stalls_last_step": int(res_final.n_band_stalls) if not multi else None,
            "tail_iterations_last_step": int(res_final.n_tail_iterations) if not multi else None,
        }
        line.update(extras)
        if single is not None:
            line["single_gpu_same_workload"] = single
            # whole-reading iterations/s of the group over those of one GPU
            line["speedup_vs_single_gpu_same_workload"] = (value / world if scaling == "weak" else value) / single["value"]
        if not args.no_cpu_baseline:
            cores = os.cpu_count() or 1
            threads = min(cores, 64)
            if world == 1:
                cb, T_oracle = cpu_baseline(sc, threads)
                line["cpu_baseline"] = {"value": cb["omp"], "unit": "iter/s", "cores": threads, "kind": "port",
                                        "cpu": cpu_model(),
                                        "sample": f"same {n_global}->{n_tgt} clouds and chain, {ITERS} iterations once per leg, "
                                                  "OpenMP oracle (parallel search, parallel exact quantile select, parallel "
                                                  "weights and normal equations; kd-tree build excluded)",
                                        "value_1thread": cb["1t"],
                                        "note_1thread": "the reference's own loop is single-threaded (no OpenMP in "
                                                        "libpointmatcher/pointmatcher): nth_element-class quantile"}
                line["speedup_vs_cpu_omp"] = value / cb["omp"]
            else:
                # N > 1: no baseline leg (the contract asks for it at N = 1 only); the oracle runs once, as the checker of
                # the pose every rank returned
                _, T_oracle = cpu_baseline(sc, threads, legs=("omp",))
            # final-pose parity against the oracle on the same inputs (whole reading)
            dt, dr = synth.pose_error(T_final, T_oracle)
            et, er = synth.pose_error(T_final, sc.T_true)
            line["pose_vs_oracle"] = {"trans_m": dt, "rot_rad": dr}
            line["pose_vs_truth"] = {"trans_m": et, "rot_rad": er}
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()      # rank 0 was still timing its single-GPU denominator: nobody tears the group down before it is done
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
