"""Converts the three stored transforms of libpointmatcher's data-filter ICP goldens into tests/golden/*.npy (DATA only:
the 16 numbers of each .ref_trans file).  Run where a libpointmatcher checkout is available:

    python tools/make_filter_goldens.py <libpointmatcher>/examples/data/icp_data

  A  default{Identity,MaxDist,RemoveNaN,BoundingBox,DistanceLimit,PointToPlaneMinDist}DataPointsFilter.ref_trans
     (byte-identical)                               -> icp_data_ssn_reading_identity_ref_trans.npy
  B  defaultMaxQuantileOnAxisDataPointsFilter       -> icp_data_ssn_max_quantile_ref_trans.npy
  C  defaultFixStepSamplingDataPointsFilter         -> icp_data_ssn_fix_step_ref_trans.npy
"""
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
GROUPS = {
    "icp_data_ssn_reading_identity_ref_trans.npy": ["Identity", "MaxDist", "RemoveNaN", "BoundingBox", "DistanceLimit",
                                                    "PointToPlaneMinDist"],
    "icp_data_ssn_max_quantile_ref_trans.npy": ["MaxQuantileOnAxis"],
    "icp_data_ssn_fix_step_ref_trans.npy": ["FixStepSampling"],
}


def main(icp_data):
    for out, names in GROUPS.items():
        raw = [open(os.path.join(icp_data, f"default{n}DataPointsFilter.ref_trans"), "rb").read() for n in names]
        assert all(r == raw[0] for r in raw), f"{names}: the stored transforms differ"
        T = np.loadtxt(os.path.join(icp_data, f"default{names[0]}DataPointsFilter.ref_trans"), dtype=np.float64)
        assert T.shape == (4, 4)
        np.save(os.path.join(OUT, out), T)
        print(out, "<-", ", ".join(names))


if __name__ == "__main__":
    main(sys.argv[1])
