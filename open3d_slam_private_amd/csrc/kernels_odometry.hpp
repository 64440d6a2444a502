// kernels_odometry.hpp -- the first step of the odometry worker (SlamWrapper.cpp:716-756): the constant-velocity
// motion compensation of a raw scan (MotionCompensation.cpp:82-139).  The kernel calls the host-and-device formula of
// host_math.hpp (undistort_point), the only copy of it.  fp64, one rounding per operation (the build forbids contraction).
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
