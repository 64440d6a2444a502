// kernels_mapcloud.hpp -- the scan-matching map of a submap (Submap::mapCloud_, Submap.cpp:39-144): rows of fp64
// points, normals and covariances (Cols64) in the reference's point order.  The transform-and-append of a scan and the
// whole-map transform, centre.  The in-order compaction of the carve's survivors is k_gather_rows<9, false> and the
// transform formulas are those of kernels_cloud64.hpp; the carve and the voxelisation are the kernels of
// kernels_mapprep.hpp.  fp64, one rounding per operation (the build forbids contraction).
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// o3d_slam::transform (helpers.cpp:283-318) of n rows, written at row `base` of out: `mapCloud_ += *transformedCloud` with
// base = the rows of the map, the transformed raw scan and PointCloud::Transform with base = 0
__global__ void k_mc_transform_append(Cols64 in, int64_t n, Xform64 T, Cols64 out, int64_t base) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t o = base + i;
    xform_point(T, in.xyz[3 * i], in.xyz[3 * i + 1], in.xyz[3 * i + 2], out.xyz + 3 * o);
    if (in.nrm) xform_dir(T, in.nrm[3 * i], in.nrm[3 * i + 1], in.nrm[3 * i + 2], out.nrm + 3 * o);
    if (in.aux) xform_cov(T, in.aux + 9 * i, out.aux + 9 * o);
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
