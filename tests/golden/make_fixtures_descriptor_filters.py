"""Writes the fixture of the descriptor-filter tests from libpointmatcher's example data:

  icp_data_max_density_ref_trans.npy (4, 4) float64
                    the 16 numbers of icp_data/defaultMaxDensityDataPointsFilter.ref_trans: the expected transform of
                    "SurfaceNormal knn 10 keepDensities -> MaxDensity 0.3 on the reading, SurfaceNormal knn 10 on the
                    reference, KDTreeMatcher knn 1, TrimmedDist 0.75, PointToPlane, Counter 40, Differential
                    0.001 / 0.01 / 4" on cloud.00001 -> cloud.00000 (utest.cpp:81-161, criterion :146-159)

defaultShadowDataPointsFilter.ref_trans is checked to hold the numbers already stored as
icp_data_surface_normal_p2pl_ref_trans.npy (make_fixtures.py), so the Shadow golden needs no file of its own.

usage: python make_fixtures_descriptor_filters.py <libpointmatcher>/examples/data
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def main(data_dir):
    icp_data = os.path.join(data_dir, "icp_data")
    g = np.loadtxt(os.path.join(icp_data, "defaultMaxDensityDataPointsFilter.ref_trans"), dtype=np.float64)
    assert g.shape == (4, 4), g.shape
    shared = np.load(os.path.join(OUT, "icp_data_surface_normal_p2pl_ref_trans.npy"))
    shadow = np.loadtxt(os.path.join(icp_data, "defaultShadowDataPointsFilter.ref_trans"), dtype=np.float64)
    assert np.array_equal(shadow, shared) and not np.array_equal(g, shared)
    np.save(os.path.join(OUT, "icp_data_max_density_ref_trans.npy"), g)
    print("wrote icp_data_max_density_ref_trans.npy to", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
