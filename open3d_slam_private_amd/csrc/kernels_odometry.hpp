// kernels_odometry.hpp -- the first step of the odometry worker (SlamWrapper.cpp:716-756): the constant-velocity
// motion compensation of a raw scan (MotionCompensation.cpp:82-139).  The kernel calls the host-and-device formula of
// host_math.hpp (undistort_point), the only copy of it.  fp64, one rounding per operation (the build forbids contraction).
// And the covariances Open3D's GeneralizedICP derives from normals, again through the one formula of
// host_math.hpp (cov_from_normal).
// Part of the single translation unit reg_core.hip (included there, after kernels_mapcloud.hpp; not a standalone header).
#pragma once

struct UndistortCfg {   // by value: the velocities stay in SGPRs
    int clockwise;
    double scan_duration, lin[3], rpy[3];
};

// one thread per point: out[i] = motion(phase(p_i)) p_i; in and out may be the same array (a thread reads its row first)
__global__ void k_undistort(const double* xyz, int64_t n, UndistortCfg c, double* out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double o[3];
    undistort_point(p, c.clockwise, c.scan_duration, c.lin, c.rpy, o);
    out[3 * i] = o[0];
    out[3 * i + 1] = o[1];
    out[3 * i + 2] = o[2];
}

// GICP covariances from normals: one point per thread through cov_from_normal (host_math.hpp).  A thread's
// row is 72 bytes, so the rows of a workgroup go through LDS (row stride 9 doubles: odd, no bank conflict) and leave as
// consecutive doubles: every store instruction of a wave covers 512 contiguous bytes.  Launched with 256 threads.
__global__ void __launch_bounds__(256) k_cov_from_normals(const double* nrm, int64_t n, double eps, double* out) {
    __shared__ double rows[256 * 9];
    const int64_t base = blockIdx.x * (int64_t)256;
    const int64_t i = base + threadIdx.x;
    if (i < n) {
        const double x[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
        double c[9];
        cov_from_normal(x, eps, c);
#pragma unroll
        for (int k = 0; k < 9; ++k) rows[threadIdx.x * 9 + k] = c[k];
    }
    __syncthreads();
    const int64_t left = n - base;   // > 0: the grid is ceil(n / 256)
    const int total = (int)(left < 256 ? left : 256) * 9;
    for (int k = threadIdx.x; k < total; k += 256) out[base * 9 + k] = rows[k];
}
