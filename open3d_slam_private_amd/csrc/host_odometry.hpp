// host_odometry.hpp -- the first step of the odometry worker on the device: reg_undistort_scan
// (ConstantVelocityMotionCompensation::undistortInputPointCloud, MotionCompensation.cpp:64-139) and its host form
// Part of the single translation unit reg_core.hip (included there, after host_mapcloud.hpp; not a standalone header).
#pragma once

static bool od_undistort_ok(const reg_undistort_params* u) {
    if (!u || u->struct_size != (int32_t)sizeof(reg_undistort_params) || !(u->scan_duration > 0.0) ||
        !std::isfinite(u->scan_duration))
        return false;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(u->linear_velocity[k]) || !std::isfinite(u->angular_velocity_rpy[k])) return false;
    return true;
}
static UndistortCfg od_undistort_cfg(const reg_undistort_params* u) {
    UndistortCfg c;
    c.clockwise = u->spinning_clockwise ? 1 : 0;
    c.scan_duration = u->scan_duration;
    for (int k = 0; k < 3; ++k) {
        c.lin[k] = u->linear_velocity[k];
        c.rpy[k] = u->angular_velocity_rpy[k];
    }
    return c;
}
static const char* kOdUndistortMsg = "undistort params of the wrong struct_size, scan_duration not finite and > 0, or a non-finite velocity";

extern "C" {

reg_status reg_host_undistort_point(const double p[3], const reg_undistort_params* u, double out[3]) {
    if (!p || !out || !od_undistort_ok(u)) return REG_BAD_ARGUMENT;
    undistort_point(p, u->spinning_clockwise ? 1 : 0, u->scan_duration, u->linear_velocity, u->angular_velocity_rpy, out);
    return REG_OK;
}

reg_status reg_undistort_scan(reg_handle* h, const double* xyz, int64_t n, int on_device, const reg_undistort_params* u,
                              double* out_xyz) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!od_undistort_ok(u) || !dm_cloud_args_ok(xyz, n) || (n > 0 && !out_xyz)) {
        h->err = std::string("reg_undistort_scan: 0 <= n <= 2^31 - 1, points and an output for n > 0; ") + kOdUndistortMsg;
        return REG_BAD_ARGUMENT;
    }
    if (n == 0) return REG_OK;   // nothing to do, with or without a device
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d_xyz = nullptr;
    HIPCHK(h, staged_input(h, h->od_in, xyz, (size_t)n * 3, on_device, &d_xyz));
    StagedOut so(h, h->od_out, on_device);
    const int s_o = so.add(out_xyz, 3);
    HIPCHK(h, so.reserve((size_t)n));
    k_undistort<<<grid_for(n), 256, 0, h->stream>>>(d_xyz, n, od_undistort_cfg(u), so.at<double>(s_o));
    HIPCHK(h, so.copy_back((size_t)n));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return REG_OK;
}

}  // extern "C"
