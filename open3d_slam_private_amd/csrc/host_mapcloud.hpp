// host_mapcloud.hpp -- the scan-matching map of a submap on the device: reg_map_cloud (Submap::mapCloud_) with
// set (Submap.cpp:47-52), insert_scan (Submap.cpp:54-95: transform, carve, append, setPose, voxelise), set_target
// (cropSubmap + initReference), transform, centre, export
// Part of the single translation unit reg_core.hip (included there, after host_densemap.hpp; not a standalone header).
#pragma once

// One side of the double-buffered columns.  Every mutating call builds its result in the spare side and swaps at the end,
// so a call that fails leaves the map as it was.
struct McSide {
    DevBuf xyz, nrm, cov;
};
struct reg_map_cloud {
    reg_handle* h = nullptr;
    reg_map_cloud_params prm;
    double center[3] = {0, 0, 0};   // mapBuilderCropper_'s pose: the creation centre, then the translation of the last insert
    int64_t n = 0;                  // rows
    int64_t scans = 0;              // nScansInsertedMap_
    int cur = 0;                    // the side that holds the map
    McSide side[2];
};

static hipError_t mc_reserve(McSide& s, size_t rows, bool nrm, bool cov) {
    hipError_t e = dm_grow(s.xyz, rows, 24);
    if (e == hipSuccess && nrm) e = dm_grow(s.nrm, rows, 24);
    if (e == hipSuccess && cov) e = dm_grow(s.cov, rows, 72);
    return e;
}
static Cols64 mc_cols(McSide& s, bool nrm, bool cov) {
    return Cols64{s.xyz.as<double>(), nrm ? s.nrm.as<double>() : nullptr, cov ? s.cov.as<double>() : nullptr};
}
static Cols64 mc_cur(reg_map_cloud* m) { return mc_cols(m->side[m->cur], m->prm.has_normals, m->prm.has_covariances); }
static Cols64 mc_spare(reg_map_cloud* m) { return mc_cols(m->side[m->cur ^ 1], m->prm.has_normals, m->prm.has_covariances); }
static reg_crop mc_crop_at(const reg_map_cloud* m, const double c[3]) {
    reg_crop crop = m->prm.crop;
    for (int k = 0; k < 3; ++k) crop.center[k] = c[k];
    return crop;
}
// 0 <= n <= 2^31 - 1, points for n > 0, exactly the fields of the map
static bool mc_cloud_ok(const reg_map_cloud* m, const double* xyz, const double* nrm, const double* cov, int64_t n) {
    return dm_cloud_args_ok(xyz, n) && (n == 0 || ((nrm != nullptr) == (m->prm.has_normals != 0) &&
                                                   (cov != nullptr) == (m->prm.has_covariances != 0)));
}
static const char* kMcCloudMsg = ": 0 <= n <= 2^31 - 1, points for n > 0 and exactly the fields the map was created with";

extern "C" {

void reg_default_map_cloud_params(reg_map_cloud_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_map_cloud_params);
    p->has_normals = 1;               // the merge cloud of the shipped point-to-plane configuration
    p->carve_every_n_scans = 10;      // SpaceCarvingParameters, Parameters.hpp:88-95
    p->map_voxel_size = 0.03;         // MapBuilderParameters, Parameters.hpp:97-101
    p->crop.type = REG_CROP_MAX_RADIUS;   // ScanCroppingParameters, Parameters.hpp:51-57
    p->crop.radius_min = 0.0;
    p->crop.radius_max = 20.0;
    p->crop.min_z = -10.0;
    p->crop.max_z = 10.0;
    p->carve_voxel_size = 0.1;
    p->carve_max_ray = 20.0;
    p->carve_truncation = 0.1;
    p->carve_min_dot = 0.5;
}

reg_status reg_map_cloud_create(reg_handle* h, const reg_map_cloud_params* p, reg_map_cloud** out) {
    if (!h || !out) return REG_BAD_ARGUMENT;
    *out = nullptr;
    CropCfg c;
    if (!p || p->struct_size != (int32_t)sizeof(reg_map_cloud_params) || !crop_cfg(&p->crop, &c) ||
        p->map_voxel_size != p->map_voxel_size || !(p->carve_voxel_size > 0.0) || !std::isfinite(p->carve_voxel_size) ||
        p->carve_max_ray != p->carve_max_ray || p->carve_truncation != p->carve_truncation ||
        p->carve_min_dot != p->carve_min_dot || p->carve_every_n_scans < 1) {
        h->err = "reg_map_cloud_create: params missing, of the wrong struct_size, an unknown crop type, a NaN, "
                 "carve_voxel_size not finite and > 0, or carve_every_n_scans < 1";
        return REG_BAD_ARGUMENT;
    }
    reg_map_cloud* m = new reg_map_cloud();   // holds no device memory until the first cloud
    m->h = h;
    m->prm = *p;
    m->prm.has_normals = p->has_normals ? 1 : 0;
    m->prm.has_covariances = p->has_covariances ? 1 : 0;
    for (int k = 0; k < 3; ++k) m->center[k] = p->crop.center[k];
    *out = m;
    return REG_OK;
}

void reg_map_cloud_destroy(reg_map_cloud* m) {
    if (!m) return;
    if (m->h->device_ok && hipSetDevice(m->h->prm.device) == hipSuccess) (void)hipStreamSynchronize(m->h->stream);
    delete m;
}

reg_status reg_map_cloud_clear(reg_map_cloud* m) {
    if (!m) return REG_BAD_ARGUMENT;
    m->n = 0;   // the points go; the cropper pose and the scan counter stay, as a cleared mapCloud_ leaves them
    return REG_OK;
}

reg_status reg_map_cloud_get_info(const reg_map_cloud* m, reg_map_cloud_info* info) {
    if (!m || !info || info->struct_size != (int32_t)sizeof(reg_map_cloud_info)) return REG_BAD_ARGUMENT;
    info->has_normals = m->prm.has_normals;
    info->has_covariances = m->prm.has_covariances;
    info->reserved = 0;
    info->n_rows = m->n;
    info->capacity = (int64_t)(m->side[m->cur].xyz.cap / 24);
    info->scans_inserted = m->scans;
    for (int k = 0; k < 3; ++k) info->crop_center[k] = m->center[k];
    return REG_OK;
}

reg_status reg_map_cloud_set(reg_map_cloud* m, const double* xyz, const double* normals, const double* covs, int64_t n,
                             int on_device, double voxel_size) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (!mc_cloud_ok(m, xyz, normals, covs, n) || voxel_size != voxel_size || std::isinf(voxel_size)) {
        h->err = std::string("reg_map_cloud_set") + kMcCloudMsg + "; voxel_size finite";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n == 0) {
        m->n = 0;
        return REG_OK;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d[3] = {xyz, normals, covs};
    for (int k = 0; k < 3; ++k) HIPCHK(h, staged_input(h, h->mc_in[k], d[k], (size_t)n * kSpWidth[k], on_device, &d[k]));
    HIPCHK(h, mc_reserve(m->side[m->cur ^ 1], (size_t)n, d[1], d[2]));
    const Cols64 out = mc_spare(m);
    int64_t rows = n;
    if (voxel_size > 0.0) {   // voxelize(mapVoxelSize_, &mapCloud_): PointCloud::VoxelDownSample
        REGCHK(sp_voxel_device(h, d[0], d[1], d[2], n, voxel_size, out.xyz, out.nrm, out.aux, &rows));
    } else {
        k_gather_rows<9, false><<<grid_for(n), 256, 0, h->stream>>>(cols64_in(d[0], d[1], d[2]), n, nullptr, nullptr, out,
                                                                    nullptr);   // no flags: a plain copy
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
    }
    m->cur ^= 1;
    m->n = rows;
    return REG_OK;
}

reg_status reg_map_cloud_insert_scan(reg_map_cloud* m, const double* raw_xyz, int64_t n_raw, const double* scan_xyz,
                                     const double* scan_normals, const double* scan_covs, int64_t n_scan, int on_device,
                                     const double T_map_to_sensor[16], int perform_carving, reg_map_cloud_insert_result* res) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (res) {
        if (res->struct_size != (int32_t)sizeof(reg_map_cloud_insert_result)) {
            h->err = "reg_map_cloud_insert_scan: result of the wrong struct_size";
            return REG_BAD_ARGUMENT;
        }
        res->carved = 0;
        res->n_carved = res->n_outside = res->n_voxels = 0;
        res->n_rows = m->n;
    }
    const double* T = T_map_to_sensor;
    if (!T || !mc_cloud_ok(m, scan_xyz, scan_normals, scan_covs, n_scan) || !dm_cloud_args_ok(raw_xyz, n_raw) ||
        m->n + n_scan > kDmMaxRows) {
        h->err = std::string("reg_map_cloud_insert_scan: T missing, a bad raw scan, map + scan beyond 2^31 - 1 rows, or a scan not") +
                 kMcCloudMsg;
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_scan == 0) return REG_OK;   // Submap.cpp:41-43
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double *d_raw = raw_xyz, *d[3] = {scan_xyz, scan_normals, scan_covs};
    for (int k = 0; k < 3; ++k) HIPCHK(h, staged_input(h, h->mc_in[k], d[k], (size_t)n_scan * kSpWidth[k], on_device, &d[k]));
    const Xform64 t = xform_rows(T);
    const bool nrm = m->prm.has_normals, cov = m->prm.has_covariances;
    const Cols64 in = mc_cur(m);

    // carve (Submap.cpp:130-144): the rule, the whole transformed raw scan as rays, the volume at the pose of the PREVIOUS insert
    const bool carve = perform_carving && m->n > 0 && (m->scans % m->prm.carve_every_n_scans) == 1;
    int64_t n_cand = 0, n_carved = 0;
    if (carve && n_raw > 0) {
        HIPCHK(h, staged_input(h, h->mc_in[3], d_raw, (size_t)n_raw * 3, on_device, &d_raw));
        HIPCHK(h, h->mc_raw.reserve((size_t)n_raw * 24));
        k_mc_transform_append<<<grid_for(n_raw), 256, 0, h->stream>>>(cols64_in(d_raw, nullptr, nullptr), n_raw, t,
                                                                      Cols64{h->mc_raw.as<double>(), nullptr, nullptr}, 0);
        const double sensor[3] = {T[12], T[13], T[14]};   // mapToRangeSensor.translation()
        const reg_crop prev = mc_crop_at(m, m->center);
        CropCfg c;
        crop_cfg(&prev, &c);
        REGCHK(carve_marks(h, in.xyz, in.nrm, m->n, h->mc_raw.as<double>(), n_raw, sensor, c, m->prm.carve_voxel_size,
                           m->prm.carve_max_ray, m->prm.carve_truncation, m->prm.carve_min_dot, &n_cand, &n_carved));
    }

    // removeByIds + operator+=: survivors in order, then the transformed scan, into the handle's working cloud
    const int64_t n_left = m->n - n_carved, n_cat = n_left + n_scan;
    HIPCHK(h, dm_grow(h->mc_cat[0], (size_t)n_cat, 24));
    if (nrm) HIPCHK(h, dm_grow(h->mc_cat[1], (size_t)n_cat, 24));
    if (cov) HIPCHK(h, dm_grow(h->mc_cat[2], (size_t)n_cat, 72));
    const Cols64 cat{h->mc_cat[0].as<double>(), nrm ? h->mc_cat[1].as<double>() : nullptr,
                     cov ? h->mc_cat[2].as<double>() : nullptr};
    if (m->n > 0)
        k_gather_rows<9, false><<<grid_for(m->n), 256, 0, h->stream>>>(in, m->n, n_carved > 0 ? h->v_fout.as<uint32_t>() : nullptr,
                                                                       n_carved > 0 ? h->v_oout.as<uint32_t>() : nullptr, cat,
                                                                       nullptr);   // the carve's marks leave
    k_mc_transform_append<<<grid_for(n_scan), 256, 0, h->stream>>>(cols64_in(d[0], d[1], d[2]), n_scan, t, cat, n_left);

    // setPose (Submap.cpp:85), then voxelizeInsideCroppingVolume from the working cloud into the spare side
    const double center[3] = {T[12], T[13], T[14]};
    const reg_crop volume = mc_crop_at(m, center);
    HIPCHK(h, mc_reserve(m->side[m->cur ^ 1], (size_t)n_cat, nrm, cov));
    const Cols64 out = mc_spare(m);
    int64_t n_out = 0, n_outside = 0;
    REGCHK(reg_voxelize_within_volume(h, cat.xyz, cat.nrm, cat.aux, n_cat, 1, &volume, m->prm.map_voxel_size, out.xyz, out.nrm,
                                      out.aux, &n_out, &n_outside));
    m->cur ^= 1;
    m->n = n_out;
    m->scans += 1;
    for (int k = 0; k < 3; ++k) m->center[k] = center[k];
    if (res) {
        res->carved = carve ? 1 : 0;
        res->n_carved = n_carved;
        res->n_outside = n_outside;
        res->n_voxels = n_out - n_outside;
        res->n_rows = n_out;
    }
    return REG_OK;
}

reg_status reg_map_cloud_set_target(reg_map_cloud* m, const reg_crop* crop, int64_t* n_kept) {
    if (!m) return REG_BAD_ARGUMENT;
    if (n_kept) *n_kept = 0;
    const Cols64 in = mc_cur(m);   // cropSubmap + open3dToPointmatcher + initReference: reg_set_target_f64 of the resident arrays
    return reg_set_target_f64(m->h, in.xyz, in.nrm, in.aux, m->n, 1, crop, n_kept);
}

reg_status reg_map_cloud_transform(reg_map_cloud* m, const double T[16]) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (!T) {
        h->err = "reg_map_cloud_transform: T is missing";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (m->n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, mc_reserve(m->side[m->cur ^ 1], (size_t)m->n, m->prm.has_normals, m->prm.has_covariances));
    k_mc_transform_append<<<grid_for(m->n), 256, 0, h->stream>>>(mc_cur(m), m->n, xform_rows(T), mc_spare(m), 0);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    m->cur ^= 1;
    return REG_OK;
}

reg_status reg_map_cloud_center(reg_map_cloud* m, double center[3]) {
    if (!m || !center) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    center[0] = center[1] = center[2] = 0.0;   // an empty cloud: Open3D's GetCenter returns zero
    if (m->n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, h->dm_misc.reserve(256));
    double* d_out = (double*)((char*)h->dm_misc.p + 64);
    k_mc_center<<<1, 64, 0, h->stream>>>(mc_cur(m).xyz, m->n, d_out);
    HIPCHK(h, hipMemcpyAsync(center, d_out, 24, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return REG_OK;
}

reg_status reg_map_cloud_export(reg_map_cloud* m, int on_device, double* xyz, double* normals, double* covs, int64_t capacity_rows,
                                int64_t* n_out) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (n_out) *n_out = 0;
    if (capacity_rows < m->n) {
        h->err = "reg_map_cloud_export: capacity_rows is below the number of rows";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_out) *n_out = m->n;
    if (m->n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const Cols64 in = mc_cur(m);   // the columns are the export's layout already: plain copies
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (xyz) HIPCHK(h, hipMemcpyAsync(xyz, in.xyz, (size_t)m->n * 24, kind, h->stream));
    if (normals && in.nrm) HIPCHK(h, hipMemcpyAsync(normals, in.nrm, (size_t)m->n * 24, kind, h->stream));
    if (covs && in.aux) HIPCHK(h, hipMemcpyAsync(covs, in.aux, (size_t)m->n * 72, kind, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

}  // extern "C"
