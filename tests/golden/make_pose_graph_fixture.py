"""Writes tests/golden/pose_graph_case_c.txt: case (c) of tests/pose_graph_cases.py (the ring with three loop closures, one
grossly wrong) with what the numpy restatement computes for it, as hexadecimal floats, for examples/pose_graph_host_check.cpp.
Run from the repository root: python tests/golden/make_pose_graph_fixture.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402

from tests import pose_graph_cases as K  # noqa: E402
from tests import pose_graph_restatement as R  # noqa: E402


def row(a):
    return " ".join(float(v).hex() for v in np.asarray(a, np.float64).reshape(-1))


def main():
    c = K.by_name("c_ring_wrong")
    g = c.graph
    zeta, Js, Jt = R.edge_terms(g.poses[g.src], g.poses[g.tgt], g.X)
    w = R.line_process_weight(g.info, c.option.preference_loop_closure, c.option.max_correspondence_distance)
    lines = [f"{g.n} {g.E}", row([c.option.preference_loop_closure, c.option.max_correspondence_distance, w])]
    lines += [row(p) for p in g.poses]
    for e in range(g.E):
        lines.append(f"{int(g.src[e])} {int(g.tgt[e])} {int(g.uncertain[e])}")
        lines += [row(g.X[e]), row(g.info[e]), row(zeta[e]), row(Js[e]), row(Jt[e])]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_graph_case_c.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
