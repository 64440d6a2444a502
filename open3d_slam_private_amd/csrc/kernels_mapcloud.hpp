// kernels_mapcloud.hpp -- the scan-matching map of a submap (Submap::mapCloud_, Submap.cpp:39-144): rows of fp64
// points, normals and covariances in the reference's point order.  In-order compaction of the carve's survivors, the
// transform-and-append of a scan, the whole-map transform, centre.  The carve and the voxelisation are the kernels of
// kernels_mapprep.hpp.  fp64, one rounding per operation (the build forbids contraction).
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

struct McCols {   // one cloud: n x 3 points, n x 3 normals or null, n x 9 covariances or null (Matrix3d: (r, c) at 3 c + r)
    double *xyz, *nrm, *cov;
};

// One row through T (row-major DmT): the formula of reg_overlap_indices and k_dm_keys,
//   w = ((T30 x + T31 y) + T32 z) + T33,  x' = (((T00 x + T01 y) + T02 z) + T03) / w;  normals (T (n, 0)).head<3>();
//   covariances R C R^T as M = R C, C' = M R^T, each element ((a0 b0 + a1 b1) + a2 b2).
__device__ __forceinline__ void mc_transform_row(const DmT& T, const McCols& in, int64_t i, const McCols& out, int64_t o) {
    const double x = in.xyz[3 * i], y = in.xyz[3 * i + 1], z = in.xyz[3 * i + 2];
    double a = T.m[12] * x;
    double b = T.m[13] * y;
    double w = a + b;
    a = T.m[14] * z;
    w = w + a;
    w = w + T.m[15];
    for (int r = 0; r < 3; ++r) {
        a = T.m[4 * r] * x;
        b = T.m[4 * r + 1] * y;
        double s = a + b;
        a = T.m[4 * r + 2] * z;
        s = s + a;
        s = s + T.m[4 * r + 3];
        out.xyz[3 * o + r] = s / w;
    }
    if (in.nrm) {
        const double nx = in.nrm[3 * i], ny = in.nrm[3 * i + 1], nz = in.nrm[3 * i + 2];
        for (int r = 0; r < 3; ++r) {
            a = T.m[4 * r] * nx;
            b = T.m[4 * r + 1] * ny;
            double s = a + b;
            a = T.m[4 * r + 2] * nz;
            out.nrm[3 * o + r] = s + a;
        }
    }
    if (in.cov) {
        const double* C = in.cov + 9 * i;
        for (int r = 0; r < 3; ++r) {
            double M[3];   // row r of R C
            for (int c = 0; c < 3; ++c) {
                a = T.m[4 * r] * C[3 * c];
                b = T.m[4 * r + 1] * C[3 * c + 1];
                double s = a + b;
                a = T.m[4 * r + 2] * C[3 * c + 2];
                M[c] = s + a;
            }
            for (int c = 0; c < 3; ++c) {
                a = M[0] * T.m[4 * c];
                b = M[1] * T.m[4 * c + 1];
                double s = a + b;
                a = M[2] * T.m[4 * c + 2];
                out.cov[9 * o + 3 * c + r] = s + a;
            }
        }
    }
}

// removeByIds (helpers.cpp, after the carve): the rows without a mark, in their order.  offs = exclusive scan of mark, so
// row i lands at i - offs[i].  mark == null: every row survives (a plain copy).
__global__ void k_mc_compact(McCols in, int64_t n, const uint32_t* __restrict__ mark, const uint32_t* __restrict__ offs,
                             McCols out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t o = i;
    if (mark) {
        if (mark[i]) return;
        o = i - (int64_t)offs[i];
    }
    for (int k = 0; k < 3; ++k) out.xyz[3 * o + k] = in.xyz[3 * i + k];
    if (in.nrm)
        for (int k = 0; k < 3; ++k) out.nrm[3 * o + k] = in.nrm[3 * i + k];
    if (in.cov)
        for (int k = 0; k < 9; ++k) out.cov[9 * o + k] = in.cov[9 * i + k];
}

// o3d_slam::transform (helpers.cpp:283-318) of n rows, written at row `base` of out: `mapCloud_ += *transformedCloud` with
// base = the rows of the map, the transformed raw scan and PointCloud::Transform with base = 0
__global__ void k_mc_transform_append(McCols in, int64_t n, DmT T, McCols out, int64_t base) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    mc_transform_row(T, in, i, out, base + i);
}

// GetCenter: the sequential sum of the rows in order, divided by n.  An order-fixed sum: one thread.
__global__ void k_mc_center(const double* __restrict__ xyz, int64_t n, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double c[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) c[k] = c[k] + xyz[3 * i + k];
    const double d = (double)n;
    for (int k = 0; k < 3; ++k) out[k] = c[k] / d;
}
