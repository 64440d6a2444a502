// host_odometry.hpp -- the odometry worker on the device.  DESIGN.md 5x: reg_undistort_scan
// (ConstantVelocityMotionCompensation::undistortInputPointCloud, MotionCompensation.cpp:64-139) and its host form.
// reg_covariances_from_normals (Open3D's GICP covariances) and reg_odometry (LidarOdometry, Odometry.cpp:22-141)
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

static bool od_epsilon_ok(double eps) { return std::isfinite(eps) && eps > 0.0; }
static void od_identity(double T[16]) {
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

// One side of the double-buffered previous cloud.  add_scan builds the new cloud in the spare side and swaps at the end, so
// a call that fails leaves the object as it was.
struct OdSide {
    DevBuf xyz, nrm, cov;
    int64_t n = 0;
    bool has_nrm = false, has_cov = false;
};
struct reg_odometry {
    reg_handle* h = nullptr;
    reg_odometry_params prm;
    double cum[16];            // odomToRangeSensorCumulative_, column-major
    double init[16];           // initialTransform_
    bool init_pending = false; // isInitialTransformSet_
    bool has_stamp = false;
    int64_t last_stamp = 0;    // lastMeasurementTimestamp_ [ns]
    uint64_t corr_epoch = 0;   // the handle's src_epoch after this object's last registration (0: none)
    int cur = 0;               // the side that holds cloudPrev_
    OdSide side[2];
    Event ev[4];               // preprocess and registration time; created by the first scan
};

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

reg_status reg_get_source_count(const reg_handle* h, int64_t* n_rows) {
    if (!h || !n_rows) return REG_BAD_ARGUMENT;
    *n_rows = h->n;
    return REG_OK;
}

reg_status reg_host_covariance_from_normal(const double normal[3], double epsilon, double out_cov[9]) {
    if (!normal || !out_cov || !od_epsilon_ok(epsilon)) return REG_BAD_ARGUMENT;
    cov_from_normal(normal, epsilon, out_cov);
    return REG_OK;
}

reg_status reg_covariances_from_normals(reg_handle* h, const double* normals, int64_t n, int on_device, double epsilon,
                                        double* out_covs) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!od_epsilon_ok(epsilon) || !dm_cloud_args_ok(normals, n) || (n > 0 && !out_covs)) {
        h->err = "reg_covariances_from_normals: epsilon finite and > 0, 0 <= n <= 2^31 - 1, normals and an output for n > 0";
        return REG_BAD_ARGUMENT;
    }
    if (n == 0) return REG_OK;   // nothing to do, with or without a device
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d_nrm = nullptr;
    HIPCHK(h, staged_input(h, h->od_in, normals, (size_t)n * 3, on_device, &d_nrm));
    StagedOut so(h, h->od_out, on_device);
    const int s_o = so.add(out_covs, 9);
    HIPCHK(h, so.reserve((size_t)n));
    k_cov_from_normals<<<grid_for(n), 256, 0, h->stream>>>(d_nrm, n, epsilon, so.at<double>(s_o));
    HIPCHK(h, so.copy_back((size_t)n));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return REG_OK;
}

void reg_default_odometry_params(reg_odometry_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_odometry_params);
    p->use_odometry_topic = 1;   // Parameters.hpp:83 and the shipped Lua
    reg_scan_params sp;          // SCAN_CROPPING_PARAMETERS / SCAN_PROCESSING_PARAMETERS / ICP_PARAMETERS, one copy
    reg_default_scan_params(&sp);
    p->crop = sp.wide;
    p->voxel_size = sp.voxel_size;
    p->down_sampling_ratio = sp.down_sampling_ratio;
    p->seed = sp.seed;
    p->normal_knn = sp.normal_knn;
    p->normal_radius = sp.normal_radius;
    p->gicp_epsilon = 1e-3;   // Open3D's RegistrationGeneralizedICP default
    p->min_fitness = 0.1;     // Odometry.cpp:56
}

void reg_odometry_struct_sizes(int32_t sizes[3]) {
    if (!sizes) return;
    sizes[0] = (int32_t)sizeof(reg_odometry_params);
    sizes[1] = (int32_t)sizeof(reg_odometry_result);
    sizes[2] = (int32_t)sizeof(reg_odometry_info);
}

reg_status reg_check_odometry_params(const reg_params* p, const reg_odometry_params* o) {
    if (!p || !o || p->struct_size != (int32_t)sizeof(reg_params) || o->struct_size != (int32_t)sizeof(reg_odometry_params))
        return REG_BAD_ARGUMENT;
    if (p->cost != REG_COST_GICP && !cost_is_o3d(p->cost)) return REG_BAD_ARGUMENT;   // cloudRegistrationFactory's three
    CropCfg c;
    if (!crop_cfg(&o->crop, &c) || !std::isfinite(o->voxel_size) || !sp_ratio_ok(o->down_sampling_ratio) || o->normal_knn < 0 ||
        o->normal_knn > kPcaMaxK || (o->normal_knn > 0 && !(o->normal_radius > 0.0)) || !od_epsilon_ok(o->gicp_epsilon) ||
        !std::isfinite(o->min_fitness))
        return REG_BAD_ARGUMENT;
    return REG_OK;
}

int32_t reg_host_odometry_decide(int32_t has_previous, int64_t timestamp_ns, int64_t last_stamp_ns, int32_t use_odometry_topic,
                                 int64_t n_rows, double fitness, double min_fitness, int32_t initial_pending) {
    if (!has_previous)   // Odometry.cpp:31-37
        return REG_ODOM_PREPROCESS | REG_ODOM_REPLACE_CLOUD | REG_ODOM_RECORD_STAMP | REG_ODOM_ACCEPTED | REG_ODOM_POSE_UPDATED;
    if (timestamp_ns < last_stamp_ns) return 0;            // :39-42
    if (use_odometry_topic) return REG_ODOM_ACCEPTED;      // :45-48
    const int32_t ran = REG_ODOM_PREPROCESS | REG_ODOM_REGISTER;
    if (!(fitness > min_fitness)) return ran | (n_rows > 0 ? REG_ODOM_REPLACE_CLOUD : 0);   // :56-71 (a NaN fitness fails)
    return ran | REG_ODOM_ACCEPTED | REG_ODOM_POSE_UPDATED | REG_ODOM_REPLACE_CLOUD | REG_ODOM_RECORD_STAMP |
           (initial_pending ? REG_ODOM_POSE_FROM_INITIAL : REG_ODOM_ACCUMULATE);             // :73-82
}

reg_status reg_host_odometry_accumulate(double cumulative[16], const float T[16]) {
    if (!cumulative || !T) return REG_BAD_ARGUMENT;
    double Td[16];
    for (int k = 0; k < 16; ++k) Td[k] = (double)T[k];
    odometry_accumulate(cumulative, Td);
    return REG_OK;
}

reg_status reg_odometry_create(reg_handle* h, const reg_odometry_params* p, reg_odometry** out) {
    if (!h || !out) return REG_BAD_ARGUMENT;
    *out = nullptr;
    if (reg_check_odometry_params(&h->prm, p) != REG_OK) {
        h->err = "reg_odometry_create: params missing or of the wrong struct_size, a cost other than GICP / O3D_P2PL / O3D_P2P, "
                 "an unknown crop type, voxel_size / min_fitness not finite, ratio outside [0, 1], normal_knn outside [0, 32], "
                 "normal_radius <= 0 with normal_knn > 0, or gicp_epsilon not finite and > 0";
        return REG_BAD_ARGUMENT;
    }
    reg_odometry* o = new reg_odometry();   // holds no device memory until the first scan
    o->h = h;
    o->prm = *p;
    od_identity(o->cum);
    *out = o;
    return REG_OK;
}

void reg_odometry_destroy(reg_odometry* o) {
    if (!o) return;
    if (o->h->device_ok && hipSetDevice(o->h->prm.device) == hipSuccess) (void)hipStreamSynchronize(o->h->stream);
    delete o;
}

reg_status reg_odometry_clear(reg_odometry* o) {
    if (!o) return REG_BAD_ARGUMENT;
    o->side[0].n = o->side[1].n = 0;
    o->has_stamp = o->init_pending = false;
    o->last_stamp = 0;
    o->corr_epoch = 0;
    od_identity(o->cum);
    return REG_OK;
}

reg_status reg_odometry_get_info(const reg_odometry* o, reg_odometry_info* info) {
    if (!o || !info || info->struct_size != (int32_t)sizeof(reg_odometry_info)) return REG_BAD_ARGUMENT;
    const OdSide& s = o->side[o->cur];
    info->has_cloud = s.n > 0;
    info->has_normals = s.n > 0 && s.has_nrm;
    info->has_covariances = s.n > 0 && s.has_cov;
    info->has_stamp = o->has_stamp;
    info->initial_pending = o->init_pending;
    info->n_rows = s.n;
    info->last_stamp_ns = o->last_stamp;
    std::memcpy(info->cumulative, o->cum, sizeof(o->cum));
    return REG_OK;
}

reg_status reg_odometry_set_initial_transform(reg_odometry* o, const double T[16], int32_t* applied) {
    if (!o || !T) return REG_BAD_ARGUMENT;
    if (applied) *applied = 0;
    if (o->init_pending) return REG_OK;   // "initial transform already set. Skipping." (Odometry.cpp:115-120)
    std::memcpy(o->init, T, sizeof(o->init));
    std::memcpy(o->cum, T, sizeof(o->cum));   // :124
    o->init_pending = true;
    if (applied) *applied = 1;
    return REG_OK;
}

reg_status reg_odometry_add_scan(reg_odometry* o, const double* xyz, const double* normals, int64_t n, int on_device,
                                 int64_t timestamp_ns, reg_odometry_result* res) {
    if (!o) return REG_BAD_ARGUMENT;
    reg_handle* h = o->h;
    if (!res || res->struct_size != (int32_t)sizeof(reg_odometry_result) || !dm_cloud_args_ok(xyz, n)) {
        h->err = "reg_odometry_add_scan: result missing or of the wrong struct_size, or not 0 <= n <= 2^31 - 1 with points for n > 0";
        return REG_BAD_ARGUMENT;
    }
    std::memset(res, 0, sizeof(*res));
    res->struct_size = (int32_t)sizeof(reg_odometry_result);
    m4_identity(res->T);
    std::memcpy(res->cumulative, o->cum, sizeof(o->cum));
    const OdSide& prev = o->side[o->cur];
    const reg_odometry_params& p = o->prm;
    // which branch, before any work: rows and fitness are not known yet and matter only where a registration runs
    const int32_t plan = reg_host_odometry_decide(prev.n > 0, timestamp_ns, o->last_stamp, p.use_odometry_topic, 0, 0.0,
                                                  p.min_fitness, o->init_pending);
    if (!(plan & REG_ODOM_PREPROCESS)) {
        res->accepted = (plan & REG_ODOM_ACCEPTED) != 0;
        return REG_OK;
    }
    const bool wants_normals = h->prm.cost != REG_COST_O3D_P2P;   // the point-to-point operator estimates nothing
    const bool estimate = !normals && wants_normals && p.normal_knn > 0;
    if (wants_normals && !normals && !estimate) {
        h->err = "InvalidField: the operator needs normals, the scan brings none and normal_knn is 0";
        return REG_MISSING_FIELD;
    }
    if (n == 0) {
        h->err = "reg_odometry_add_scan: the scan is empty";
        return REG_EMPTY_SOURCE;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    for (Event& e : o->ev)
        if (!e.e) HIPCHK(h, e.create());

    // preprocess (Odometry.cpp:22-27) into the spare side
    HIPCHK(h, hipEventRecord(o->ev[0], h->stream));
    const double* cur[3] = {xyz, normals, nullptr};
    for (int k = 0; k < 2; ++k) HIPCHK(h, staged_input(h, h->sp_in[k], cur[k], (size_t)n * kSpWidth[k], on_device, &cur[k]));
    CropCfg crop;
    crop_cfg(&p.crop, &crop);
    int64_t m = n;
    const reg_status fs = sp_front(h, cur, &m, crop, p.voxel_size, estimate, false, p.normal_knn, p.normal_radius,
                                   p.down_sampling_ratio, p.seed, &res->n_crop, &res->n_voxels);
    res->n_selected = fs == REG_OK ? m : 0;
    if (fs != REG_OK || m == 0) {
        if (fs == REG_OK || fs == REG_EMPTY_SOURCE) h->err = "reg_odometry_add_scan: the scan is empty after preprocessing";
        return fs == REG_OK ? REG_EMPTY_SOURCE : fs;
    }
    OdSide& next = o->side[o->cur ^ 1];
    const bool nrm = cur[1] != nullptr, cov = h->prm.cost == REG_COST_GICP;
    HIPCHK(h, dm_grow(next.xyz, (size_t)m, 24));
    if (nrm) HIPCHK(h, dm_grow(next.nrm, (size_t)m, 24));
    if (cov) HIPCHK(h, dm_grow(next.cov, (size_t)m, 72));
    HIPCHK(h, hipMemcpyAsync(next.xyz.p, cur[0], (size_t)m * 24, hipMemcpyDeviceToDevice, h->stream));
    if (nrm) HIPCHK(h, hipMemcpyAsync(next.nrm.p, cur[1], (size_t)m * 24, hipMemcpyDeviceToDevice, h->stream));
    if (cov) k_cov_from_normals<<<grid_for(m), 256, 0, h->stream>>>(next.nrm.as<double>(), m, p.gicp_epsilon, next.cov.as<double>());
    HIPCHK(h, hipEventRecord(o->ev[1], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // a host scan may go once this returns
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventElapsedTime(&res->prep_ms, o->ev[0], o->ev[1]));

    int32_t act = plan;
    if (plan & REG_ODOM_REGISTER) {
        // registerClouds(cloudPrev_, *preProcessed, I): the previous cloud is the reading, the new one the reference
        HIPCHK(h, hipEventRecord(o->ev[2], h->stream));
        REGCHK(reg_set_target_f64(h, next.xyz.as<double>(), nrm ? next.nrm.as<double>() : nullptr,
                                  cov ? next.cov.as<double>() : nullptr, m, 1, nullptr, nullptr));
        REGCHK(reg_set_source_f64(h, prev.xyz.as<double>(), prev.has_nrm ? prev.nrm.as<double>() : nullptr,
                                  prev.has_cov ? prev.cov.as<double>() : nullptr, prev.n, 1));
        float T_init[16];
        m4_identity(T_init);
        reg_result rr;
        REGCHK(reg_register(h, T_init, res->T, &rr));
        HIPCHK(h, hipEventRecord(o->ev[3], h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipEventElapsedTime(&res->register_ms, o->ev[2], o->ev[3]));
        res->registered = 1;
        res->n_source = prev.n;
        res->n_target = m;
        res->fitness = rr.fitness;
        res->inlier_rmse = rr.inlier_rmse;
        res->iterations = rr.iterations;
        o->corr_epoch = h->src_epoch;
        act = reg_host_odometry_decide(1, timestamp_ns, o->last_stamp, p.use_odometry_topic, m, rr.fitness, p.min_fitness,
                                       o->init_pending);
    }
    // from here on nothing can fail: the state changes together
    if (act & REG_ODOM_POSE_FROM_INITIAL) {
        std::memcpy(o->cum, o->init, sizeof(o->cum));
        o->init_pending = false;
    }
    if (act & REG_ODOM_ACCUMULATE) (void)reg_host_odometry_accumulate(o->cum, res->T);
    if (act & REG_ODOM_REPLACE_CLOUD) {
        next.n = m;
        next.has_nrm = nrm;
        next.has_cov = cov;
        o->cur ^= 1;   // the hand-over: a swap of the sides
    }
    if (act & REG_ODOM_RECORD_STAMP) {
        o->last_stamp = timestamp_ns;
        o->has_stamp = true;
    }
    res->accepted = (act & REG_ODOM_ACCEPTED) != 0;
    res->pose_updated = (act & REG_ODOM_POSE_UPDATED) != 0;
    std::memcpy(res->cumulative, o->cum, sizeof(o->cum));
    return REG_OK;
}

reg_status reg_odometry_export_cloud(reg_odometry* o, int on_device, double* xyz, double* normals, double* covs,
                                     int64_t capacity_rows, int64_t* n_out) {
    if (!o) return REG_BAD_ARGUMENT;
    reg_handle* h = o->h;
    const OdSide& s = o->side[o->cur];
    if (n_out) *n_out = 0;
    if (capacity_rows < s.n) {
        h->err = "reg_odometry_export_cloud: capacity_rows is below the number of rows";
        return REG_BAD_ARGUMENT;
    }
    if (n_out) *n_out = s.n;
    if (s.n == 0) return REG_OK;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, copy_out(h, xyz, s.xyz.p, (size_t)s.n * 24, on_device));   // the columns are the export's layout already
    if (s.has_nrm) HIPCHK(h, copy_out(h, normals, s.nrm.p, (size_t)s.n * 24, on_device));
    if (s.has_cov) HIPCHK(h, copy_out(h, covs, s.cov.p, (size_t)s.n * 72, on_device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

reg_status reg_odometry_get_correspondences(reg_odometry* o, int64_t capacity_rows, int32_t* ids, float* d2) {
    if (!o) return REG_BAD_ARGUMENT;
    reg_handle* h = o->h;
    if (o->corr_epoch == 0 || o->corr_epoch != h->src_epoch || h->n <= 0) {
        h->err = "reg_odometry_get_correspondences: the handle's reading is not one this object installed";
        return REG_NOT_CONFIGURED;
    }
    if (capacity_rows < h->n) {
        h->err = "reg_odometry_get_correspondences: capacity_rows is below the rows of the reading";
        return REG_BAD_ARGUMENT;
    }
    return reg_get_correspondences(h, ids, d2, nullptr);
}

}  // extern "C"
