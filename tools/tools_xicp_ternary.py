"""Device time of degeneracyAwareness EqualityConstraints at the C2 size (100 k -> 1 M), fixed_iters = 20 on
the chain's generic iteration:
  off                 a chain with a MinDist filter that rejects nothing: the generic chain iteration without the method
  on_all_localizable  the 24 sums and the decision; the partial-sums kernel gated off on the device
  on_partial          high and enough thresholds at 1.2 times the weakest direction's combined sum of the run before, so
                      that it is PARTIAL_HIGH while the stronger directions stay localizable
  on_none             the insufficient threshold raised as well: that direction NONE, the constrained solve without a
                      partial problem (an extra case that splits the cost of on_partial)
The categories of the last iteration are printed.  The reference normals are perturbed by N(0, 0.03) per component: the
scene's exact plane normals would make the sampled 3x3 problem singular.
usage: python tools/tools_xicp_ternary.py [--reps 10]   (GPU)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from open3d_slam_private_amd import capi, synth


def run(sc, ternary, reps):
    p = capi.shipped_params()
    p.use_xicp, p.fixed_iters = 0, 20
    reg = capi.Registration(p)
    c = capi.default_pm_chain_v3()
    c.use_min_dist_filter, c.outlier_min_dist = 1, 1e-7
    reg.set_pm_chain(c)
    if ternary is not None:
        reg.set_ternary_xicp(ternary)
    reg.set_target(sc.tgt_xyz, sc.tgt_nrm)
    reg.set_source(sc.src_xyz, sc.src_nrm)
    per_iter = []
    for _ in range(reps + 2):          # two warm-up registrations
        _, res = reg.register(np.eye(4))
        per_iter.append(1000.0 * res.loop_ms / max(1, res.iterations))
    out = dict(iter_us_min=float(np.min(per_iter[2:])), iter_us_median=float(np.median(per_iter[2:])), iterations=int(res.iterations))
    if ternary is not None:
        g = reg.get_ternary_xicp()
        out.update(categories=list(g.category), combined=[float(v) for v in g.combined], n_combined=list(g.n_combined))
    reg.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    sc = synth.make_scene(100_000, 1_000_000, seed=1)
    nrm = sc.tgt_nrm.astype(np.float64) + np.random.default_rng(3).normal(scale=0.03, size=sc.tgt_nrm.shape)
    sc.tgt_nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    out = {"off": run(sc, None, args.reps)}
    # thresholds no sum reaches from below: every direction localizable
    t = capi.default_ternary_xicp(True)
    out["on_all_localizable"] = run(sc, t, args.reps)
    weakest = min(out["on_all_localizable"]["combined"])
    t = capi.default_ternary_xicp(True)
    t.high_information, t.enough_information, t.insufficient_information = 1.2 * weakest, 1.2 * weakest, 35.0
    out["on_partial"] = run(sc, t, args.reps)
    # the same direction non-localizable (constraint value 0): the constrained solve without the partial problem
    t.insufficient_information = 1.2 * weakest
    out["on_none"] = run(sc, t, args.reps)
    for k, r in out.items():
        print(f"{k:20s} {r['iter_us_min']:8.1f} / {r['iter_us_median']:8.1f} us per iteration (min / median of {args.reps}), "
              f"{r['iterations']} iterations, categories {r.get('categories')}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
