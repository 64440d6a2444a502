"""The input of test_knn_search_rescans_a_box_that_overflows_the_list (tests/test_gpu_pm_chain.py), shared with
tools/neigh_digest.py: a reference cloud with a blob of 3 040 points inside one level-0 bin box of the k-NN search and a
reading of which 64 points lie inside the blob."""
import math

import numpy as np

CELL_SIZE, MAX_DIST = 0.25, 0.5
N_NEAR = 64          # the first N_NEAR reading points lie in the blob
N_BLOB = 3040        # the first N_BLOB reference points are the blob (3 000 + 40 twins)
NEAR_RADIUS = 2e-3   # every blob point lies within this distance of every near reading point


def clouds():
    """(reference xyz (5040, 3), reference normals, reading xyz (128, 3), reading normals), fp32."""
    rng = np.random.default_rng(17)
    centre = np.array([1.3, -0.7, 0.4])
    half = 1e-3 / math.sqrt(3.0) * 0.999          # a cube inside the 1 mm ball around the centre
    blob = centre + rng.uniform(-half, half, size=(3000, 3))
    twins = blob[rng.choice(3000, 40, replace=False)]   # exact duplicates: equal d2, the lower index comes first
    ref = np.concatenate([blob, twins, rng.uniform(-5, 5, size=(2000, 3))]).astype(np.float32)
    nrm = rng.normal(size=ref.shape)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    near = centre + rng.uniform(-half, half, size=(N_NEAR, 3))
    rd = np.concatenate([near, rng.uniform(-5, 5, size=(64, 3))]).astype(np.float32)
    rd_nrm = np.tile(np.array([[0, 0, 1]], np.float32), (rd.shape[0], 1))
    return ref, nrm, rd, rd_nrm
