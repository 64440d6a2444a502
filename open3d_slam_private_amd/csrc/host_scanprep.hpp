// host_scanprep.hpp -- the scan front end on the device: reg_voxel_down_sample, reg_random_down_sample,
// reg_process_scan (ScanToMapIcp::processForScanMatchingAndMerging, ScanToMapRegistration.cpp:36-69)
// Part of the single translation unit reg_core.hip (included there, after the other host headers; not a standalone header).
#pragma once

static const size_t kSpWidth[3] = {3, 3, 9};   // doubles per row of points_, normals_, covariances_

// VoxelDownSample of a device cloud into device arrays of n rows (d_onrm / d_ocov are written iff d_nrm / d_cov are given)
static reg_status sp_voxel_device(reg_handle* h, const double* d_xyz, const double* d_nrm, const double* d_cov, int64_t n,
                                  double voxel, double* d_oxyz, double* d_onrm, double* d_ocov, int64_t* n_vox) {
    HIPCHK(h, h->sp.reserve((size_t)n));
    HIPCHK(h, h->sp_misc.reserve(256));
    const int rows = (int)std::min<int64_t>(grid_for(n), kSpMinRows);
    HIPCHK(h, h->sp_part.reserve(((size_t)rows * 3 + 6) * 8));
    double *part = h->sp_part.as<double>(), *bound = part + (size_t)rows * 3;   // bound: min_bound[3], origin[3]
    const RunArrays a = h->sp.arrays();
    HIPCHK(h, hipMemsetAsync(h->sp_misc.p, 0, 4, h->stream));
    k_sp_min_partial<<<rows, 256, 0, h->stream>>>(d_xyz, n, part);
    k_sp_min_final<<<1, 256, 0, h->stream>>>(part, rows, voxel, bound);
    k_sp_vox_keys<<<grid_for(n), 256, 0, h->stream>>>(d_xyz, n, bound + 3, voxel, a.keys, a.vals, h->sp_misc.as<uint32_t>());
    uint32_t bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, h->sp_misc.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad) {
        h->err = (bad & 1u) ? "reg_voxel_down_sample: non-finite coordinate"
                            : "reg_voxel_down_sample: voxel_size too small for the extent of the cloud (voxel index exceeds 2^21)";
        return REG_BAD_ARGUMENT;
    }
    uint32_t tail[2];
    REGCHK(sort_runs(h, a, n, tail));
    k_vox_reduce<false><<<grid_for(n), 256, 0, h->stream>>>(a.sorted, a.svals, n, a.heads, a.run, d_xyz, d_nrm, d_cov, 0, d_oxyz,
                                                            d_onrm, d_ocov);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    *n_vox = flag_total(tail);
    return REG_OK;
}

// Flags (sp.heads) and their exclusive scan (sp.run) of the `count` smallest (key, index) pairs among n
static reg_status sp_random_flags(reg_handle* h, int64_t n, int64_t count, uint64_t seed) {
    HIPCHK(h, h->sp.heads.reserve((size_t)n * 4));
    HIPCHK(h, h->sp.run.reserve((size_t)n * 4));
    uint32_t* flags = h->sp.heads.as<uint32_t>();
    if (count >= n) {   // ratio == 1 copies through
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)flags, 1, (size_t)n, h->stream));
    } else {
        HIPCHK(h, hipMemsetAsync(flags, 0, (size_t)n * 4, h->stream));
        if (count > 0) {
            HIPCHK(h, h->sp.reserve((size_t)n));   // (heads and run are there already)
            const RunArrays a = h->sp.arrays();
            k_sp_rand_keys<<<grid_for(n), 256, 0, h->stream>>>(seed, n, a.keys, a.vals);
            REGCHK(sort_pairs(h, h->rp_tmp, a.keys, a.sorted, a.vals, a.svals, (size_t)n, 0, 64));
            k_sp_rand_mark<<<grid_for(count), 256, 0, h->stream>>>(a.svals, count, flags);
        }
    }
    REGCHK(scan_excl(h, h->rp_tmp, flags, h->sp.run.as<uint32_t>(), (size_t)n));
    return REG_OK;
}

// Stages 1-4 of the front end on a device cloud: crop, VoxelDownSample, estimateNormalsOrCovariancesIfNeeded, RandomDownSample.
// cur[3] (points, normals, covariances; null: absent) and *rows are the cloud on entry and on return; the result lies in the
// handle's sp_a / sp_b / sp_c buffers (or is the input itself when no stage moved it).  An empty crop is REG_EMPTY_SOURCE.
static reg_status sp_front(reg_handle* h, const double* cur[3], int64_t* rows, const CropCfg& crop, double voxel, bool estimate,
                           bool est_cov, int knn, double radius, double ratio, uint64_t seed, int64_t* n_crop, int64_t* n_vox) {
    int64_t m = *rows;
    // 1. crop, order-preserving
    if (crop.type != REG_CROP_NONE) {
        HIPCHK(h, h->sp.heads.reserve((size_t)m * 4));
        HIPCHK(h, h->sp.run.reserve((size_t)m * 4));
        uint32_t *flags = h->sp.heads.as<uint32_t>(), *offs = h->sp.run.as<uint32_t>();
        k_crop_flags<<<grid_for(m), 256, 0, h->stream>>>(cur[0], m, crop, flags);
        int64_t kept = 0;
        REGCHK(scan_total(h, flags, offs, m, &kept));
        if (kept > 0) {
            double* o[3] = {nullptr, nullptr, nullptr};
            for (int k = 0; k < 3; ++k)
                if (cur[k]) {
                    HIPCHK(h, h->sp_a[k].reserve((size_t)kept * kSpWidth[k] * 8));
                    o[k] = h->sp_a[k].as<double>();
                }
            k_gather_rows<9, true><<<grid_for(m), 256, 0, h->stream>>>(cols64_in(cur[0], cur[1], cur[2]), m, flags, offs,
                                                                       Cols64{o[0], o[1], o[2]}, nullptr);
            for (int k = 0; k < 3; ++k) cur[k] = o[k];
        }
        m = kept;
    }
    *n_crop = m;
    if (m == 0) {
        *rows = 0;
        h->err = "ScanToMapIcp::wideCropped cropped size is zero";   // ScanToMapRegistration.cpp:67
        return REG_EMPTY_SOURCE;
    }
    // 2. VoxelDownSample (helpers.cpp:108-111: voxel_size <= 0 skips it)
    if (voxel > 0.0) {
        double* o[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < 3; ++k)
            if (cur[k]) {
                HIPCHK(h, h->sp_b[k].reserve((size_t)m * kSpWidth[k] * 8));
                o[k] = h->sp_b[k].as<double>();
            }
        int64_t kept = 0;
        REGCHK(sp_voxel_device(h, cur[0], cur[1], cur[2], m, voxel, o[0], o[1], o[2], &kept));
        for (int k = 0; k < 3; ++k) cur[k] = o[k];
        m = kept;
    }
    *n_vox = m;
    // 3. estimateNormalsOrCovariancesIfNeeded: a cloud that brings normals keeps them (CloudRegistration.cpp:27,64)
    if (estimate) {
        HIPCHK(h, h->sp_f32[0].reserve((size_t)m * 12));
        HIPCHK(h, h->sp_f32[1].reserve((size_t)m * 12));
        if (est_cov) HIPCHK(h, h->sp_f32[2].reserve((size_t)m * 24));
        float *fx = h->sp_f32[0].as<float>(), *fn = h->sp_f32[1].as<float>(), *fc = est_cov ? h->sp_f32[2].as<float>() : nullptr;
        k_cast_cloud_f64<<<grid_for(m), 256, 0, h->stream>>>(cur[0], nullptr, nullptr, m, fx, nullptr, nullptr);
        reg_normals_out no;
        std::memset(&no, 0, sizeof(no));
        no.normals = fn;
        no.covs = fc;
        const float origin[3] = {0.f, 0.f, 0.f};
        REGCHK(reg_estimate_normals(h, fx, 3, m, 1, knn, (float)radius, origin, 1, &no, nullptr));
        HIPCHK(h, h->sp_b[1].reserve((size_t)m * 24));
        if (est_cov) HIPCHK(h, h->sp_b[2].reserve((size_t)m * 72));
        double *on = h->sp_b[1].as<double>(), *oc = est_cov ? h->sp_b[2].as<double>() : nullptr;
        k_sp_widen<<<grid_for(m), 256, 0, h->stream>>>(fn, fc, m, on, oc);
        cur[1] = on;
        if (est_cov) cur[2] = oc;
    }
    // 4. RandomDownSample (helpers.cpp:100-103: ratio >= 1 skips it)
    if (ratio < 1.0) {
        const int64_t count = (int64_t)(ratio * (double)m);
        if (count > 0) {
            REGCHK(sp_random_flags(h, m, count, seed));
            double* o[3] = {nullptr, nullptr, nullptr};
            for (int k = 0; k < 3; ++k)
                if (cur[k]) {
                    HIPCHK(h, h->sp_c[k].reserve((size_t)count * kSpWidth[k] * 8));
                    o[k] = h->sp_c[k].as<double>();
                }
            k_gather_rows<9, true><<<grid_for(m), 256, 0, h->stream>>>(cols64_in(cur[0], cur[1], cur[2]), m,
                                                                       h->sp.heads.as<uint32_t>(), h->sp.run.as<uint32_t>(),
                                                                       Cols64{o[0], o[1], o[2]}, nullptr);
            for (int k = 0; k < 3; ++k) cur[k] = o[k];
        }
        m = count;
    }
    *rows = m;
    return REG_OK;
}

static bool sp_ratio_ok(double ratio) { return ratio >= 0.0 && ratio <= 1.0; }   // false for NaN

extern "C" {

uint64_t reg_host_scan_key(uint64_t seed, uint64_t index) { return splitmix_key(seed, index); }

void reg_default_scan_params(reg_scan_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_scan_params);
    // SCAN_CROPPING_PARAMETERS / SCAN_PROCESSING_PARAMETERS / ICP_PARAMETERS of param/default/parameter_structure_definitions.lua
    p->wide.type = p->narrow.type = REG_CROP_MIN_MAX_RADIUS;
    p->wide.radius_min = p->narrow.radius_min = 2.0;
    p->wide.radius_max = p->narrow.radius_max = 100.0;
    p->wide.min_z = p->narrow.min_z = -50.0;
    p->wide.max_z = p->narrow.max_z = 50.0;
    p->voxel_size = 0.01;
    p->down_sampling_ratio = 1.0;
    p->seed = 0;
    p->normal_knn = 20;
    p->normal_radius = 1.0;
}

reg_status reg_voxel_down_sample(reg_handle* h, const double* xyz, const double* normals, const double* covs, int64_t n,
                                 int on_device, double voxel_size, double* out_xyz, double* out_normals, double* out_covs,
                                 int64_t* n_out) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_out) *n_out = 0;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) {
        h->err = "reg_voxel_down_sample: voxel_size must be finite and > 0";
        return REG_BAD_ARGUMENT;
    }
    if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!xyz || !out_xyz)) || (normals && !out_normals) || (covs && !out_covs))
        return REG_BAD_ARGUMENT;
    if (n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d_in[3] = {xyz, normals, covs};
    double* const user[3] = {out_xyz, out_normals, out_covs};
    StagedOut so(h, h->sp_b[0], on_device);   // slot k: points, normals, covariances; an output goes with its input
    for (int k = 0; k < 3; ++k) {
        HIPCHK(h, staged_input(h, h->sp_in[k], d_in[k], (size_t)n * kSpWidth[k], on_device, &d_in[k]));
        so.add(d_in[k] ? user[k] : nullptr, kSpWidth[k]);
    }
    HIPCHK(h, so.reserve((size_t)n));
    int64_t n_vox = 0;
    REGCHK(sp_voxel_device(h, d_in[0], d_in[1], d_in[2], n, voxel_size, so.at<double>(0), so.at<double>(1), so.at<double>(2),
                           &n_vox));
    if (!on_device) {   // (the device form is synchronised by sp_voxel_device)
        HIPCHK(h, so.copy_back((size_t)n_vox));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (n_out) *n_out = n_vox;
    return REG_OK;
}

reg_status reg_random_down_sample(reg_handle* h, const double* xyz, const double* normals, const double* covs, int64_t n,
                                  int on_device, double ratio, uint64_t seed, int32_t* out_idx, double* out_xyz,
                                  double* out_normals, double* out_covs, int64_t* n_out) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_out) *n_out = 0;
    if (!sp_ratio_ok(ratio)) {
        h->err = "reg_random_down_sample: ratio must lie in [0, 1]";
        return REG_BAD_ARGUMENT;
    }
    if (n < 0 || n > 0x7fffffffLL || (xyz && !out_xyz) || (normals && !out_normals) || (covs && !out_covs)) return REG_BAD_ARGUMENT;
    if (n == 0) return REG_OK;
    const int64_t count = (int64_t)(ratio * (double)n);   // the fp64 product, truncated
    if (count == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d_in[3] = {xyz, normals, covs};
    double* const user[3] = {out_xyz, out_normals, out_covs};
    StagedOut so(h, h->sp_c[0], on_device);   // slot k: points, normals, covariances (each with its input); slot 3: indices
    for (int k = 0; k < 3; ++k) {
        HIPCHK(h, staged_input(h, h->sp_in[k], d_in[k], (size_t)n * kSpWidth[k], on_device, &d_in[k]));
        so.add(d_in[k] ? user[k] : nullptr, kSpWidth[k]);
    }
    const int s_idx = so.add(out_idx, 1);
    HIPCHK(h, so.reserve((size_t)count));
    REGCHK(sp_random_flags(h, n, count, seed));
    k_gather_rows<9, true><<<grid_for(n), 256, 0, h->stream>>>(
        cols64_in(d_in[0], d_in[1], d_in[2]), n, h->sp.heads.as<uint32_t>(), h->sp.run.as<uint32_t>(),
        Cols64{so.at<double>(0), so.at<double>(1), so.at<double>(2)}, so.at<int32_t>(s_idx));
    HIPCHK(h, so.copy_back((size_t)count));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_out) *n_out = count;
    return REG_OK;
}

reg_status reg_process_scan(reg_handle* h, const double* xyz, const double* normals, const double* covs, int64_t n,
                            int on_device, const reg_scan_params* p, double* merge_xyz, double* merge_normals,
                            double* merge_covs, reg_scan_result* res) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    // whatever happens below, the previous reading is gone
    h->n = 0;
    h->src_kept = 0;
    h->prepared = false;
    h->have_match = false;
    h->pm_have_match = false;
    if (!p || p->struct_size != (int32_t)sizeof(reg_scan_params) || !res || res->struct_size != (int32_t)sizeof(reg_scan_result)) {
        h->err = "reg_process_scan: params / result missing or of the wrong struct_size";
        return REG_BAD_ARGUMENT;
    }
    std::memset(res, 0, sizeof(*res));
    res->struct_size = (int32_t)sizeof(reg_scan_result);
    CropCfg wide, narrow;
    if (!crop_cfg(&p->wide, &wide) || !crop_cfg(&p->narrow, &narrow) || !std::isfinite(p->voxel_size) ||
        !(p->down_sampling_ratio >= 0.0) || !std::isfinite(p->down_sampling_ratio) || p->normal_knn < 0 ||
        p->normal_knn > kPcaMaxK || (p->normal_knn > 0 && !(p->normal_radius > 0.0))) {
        h->err = "reg_process_scan: bad parameter (finite voxel_size, ratio >= 0, 0 <= normal_knn <= 32, normal_radius > 0)";
        return REG_BAD_ARGUMENT;
    }
    if (n <= 0) {
        h->err = "The reading point cloud is empty.";
        return REG_EMPTY_SOURCE;
    }
    if (!xyz || !merge_xyz || n > 0x7fffffffLL) return REG_BAD_ARGUMENT;
    // the fields the merge cloud will carry: given, or estimated by stage 3 (normals; covariances for GICP only)
    const bool estimate = !normals && p->normal_knn > 0;
    const bool est_cov = estimate && !covs && h->prm.cost == REG_COST_GICP;
    const bool has_nrm = normals || estimate, has_cov = (covs != nullptr) || est_cov;
    if (const reg_status fs = check_source_fields(h, has_nrm, has_cov)) return fs;
    HIPCHK(h, hipSetDevice(h->prm.device));
    if (!h->ev_p0.e) HIPCHK(h, h->ev_p0.create());
    if (!h->ev_p1.e) HIPCHK(h, h->ev_p1.create());
    HIPCHK(h, hipEventRecord(h->ev_p0, h->stream));
    const double* cur[3] = {xyz, normals, covs};   // the cloud as it stands after each stage (device pointers)
    for (int k = 0; k < 3; ++k) HIPCHK(h, staged_input(h, h->sp_in[k], cur[k], (size_t)n * kSpWidth[k], on_device, &cur[k]));
    int64_t m = n;
    // 1-4. wide crop (mapBuilderCropper_), voxel grid, normals / covariances, random selection
    REGCHK(sp_front(h, cur, &m, wide, p->voxel_size, estimate, est_cov, p->normal_knn, p->normal_radius, p->down_sampling_ratio,
                    p->seed, &res->n_wide, &res->n_voxels));
    res->n_merge = m;
    res->has_normals = cur[1] != nullptr;
    res->has_covs = cur[2] != nullptr;
    if (m == 0) {
        h->err = "ScanToMapIcp::wideCropped cropped size is zero";
        return REG_EMPTY_SOURCE;
    }
    // 5. the merge cloud (merge_) goes to the caller's arrays
    double* merge[3] = {merge_xyz, merge_normals, merge_covs};
    for (int k = 0; k < 3; ++k)
        if (cur[k]) HIPCHK(h, copy_out(h, merge[k], cur[k], (size_t)m * kSpWidth[k] * 8, on_device));
    // 6. narrow crop (scanMatcherCropper_ at the identity pose) + open3dToPointmatcher: match_ becomes the reading
    HIPCHK(h, h->sp.heads.reserve((size_t)m * 4));
    HIPCHK(h, h->sp.run.reserve((size_t)m * 4));
    uint32_t *flags = h->sp.heads.as<uint32_t>(), *offs = h->sp.run.as<uint32_t>();
    k_crop_flags<<<grid_for(m), 256, 0, h->stream>>>(cur[0], m, narrow, flags);
    int64_t kept = 0;
    REGCHK(scan_total(h, flags, offs, m, &kept));
    res->n_match = kept;
    if (kept == 0) {
        h->err = "ScanToMapIcp::narrow cropped size is zero";   // ScanToMapRegistration.cpp:66
        return REG_EMPTY_SOURCE;
    }
    HIPCHK(h, h->r_xyz.reserve((size_t)kept * 12));
    if (cur[1]) HIPCHK(h, h->r_nrm.reserve((size_t)kept * 12));
    if (cur[2]) HIPCHK(h, h->r_cov.reserve((size_t)kept * 24));
    HIPCHK(h, h->ov_sidx.reserve((size_t)kept * 4));
    k_crop_gather<<<grid_for(m), 256, 0, h->stream>>>(cur[0], cur[1], cur[2], m, flags, offs, h->r_xyz.as<float>(),
                                                      cur[1] ? h->r_nrm.as<float>() : nullptr,
                                                      cur[2] ? h->r_cov.as<float>() : nullptr, h->ov_sidx.as<int32_t>());
    HIPCHK(h, hipGetLastError());
    REGCHK(reg_set_source(h, h->r_xyz.as<float>(), 3, cur[1] ? h->r_nrm.as<float>() : nullptr, 3,
                          cur[2] ? h->r_cov.as<float>() : nullptr, kept, 1));
    h->src_kept = kept;
    HIPCHK(h, hipEventRecord(h->ev_p1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventElapsedTime(&res->scan_prep_ms, h->ev_p0, h->ev_p1));
    return REG_OK;
}

}  // extern "C"
