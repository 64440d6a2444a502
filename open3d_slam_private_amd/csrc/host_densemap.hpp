// host_densemap.hpp -- the dense map on the device: reg_dense_map (o3d_slam::VoxelizedPointCloud, Voxel.cpp:38-114)
// with insert, insert_scan (Submap.cpp:99-106), carve (helpers.cpp:360-390), transform, centre, export; reg_dedup_voxels
// Part of the single translation unit reg_core.hip (included there, after the other host headers; not a standalone header).
#pragma once

// One side of the double-buffered columns.  Every mutating call builds its result in the spare side and swaps at the end,
// so a call that fails leaves the map as it was.
struct DmSide {
    DevBuf key, cnt, pos, nrm, col;
};
struct reg_dense_map {
    reg_handle* h = nullptr;
    double voxel = 0.0, inv = 0.0;   // inv = 1.0 / voxel (VoxelHashMap.hpp:43-45)
    int64_t n = 0;                   // voxels
    int cur = 0;                     // the side that holds the map
    bool has_nrm = false, has_col = false;   // sticky (isHasNormals_ / isHasColors_)
    DmSide side[2];
};

constexpr int64_t kDmMaxRows = 0x7fffffffLL;
constexpr size_t kDmMinRows = 1024;
constexpr int kDmCarveLanes = 16;   // lanes per ray of k_dm_carve_bricks (8, 16 and 64 were measured)

// grows geometrically: at least `rows` rows of `row_bytes`, at least twice what the buffer held
static hipError_t dm_grow(DevBuf& b, size_t rows, size_t row_bytes) {
    if (b.cap >= rows * row_bytes) return hipSuccess;
    const size_t want = std::max(std::max(rows, 2 * (b.cap / row_bytes)), kDmMinRows);
    return b.reserve(std::min<size_t>(want, (size_t)kDmMaxRows) * row_bytes);
}
static hipError_t dm_reserve_spare(reg_dense_map* m, size_t rows, bool nrm, bool col) {
    DmSide& s = m->side[m->cur ^ 1];
    hipError_t e = dm_grow(s.key, rows, 8);
    if (e == hipSuccess) e = dm_grow(s.cnt, rows, 4);
    if (e == hipSuccess) e = dm_grow(s.pos, rows, 24);
    if (e == hipSuccess && nrm) e = dm_grow(s.nrm, rows, 24);
    if (e == hipSuccess && col) e = dm_grow(s.col, rows, 24);
    return e;
}
static DmCols dm_cols(reg_dense_map* m, int side, bool nrm, bool col) {
    DmSide& s = m->side[side];
    return DmCols{s.key.as<uint64_t>(), s.cnt.as<int32_t>(), s.pos.as<double>(), nrm ? s.nrm.as<double>() : nullptr,
                  col ? s.col.as<double>() : nullptr};
}
static void dm_swap(reg_dense_map* m, int64_t n, bool nrm, bool col) {
    m->cur ^= 1;
    m->n = n;
    m->has_nrm = nrm;
    m->has_col = col;
}

// keys (+ transformed cloud when T is given) of a device cloud, sorted with their indices, run heads and run ids.
// Leaves the sorted keys and values, the run heads and the run ids of h->dm filled; *runs = number of distinct keys.  One
// synchronisation.
static reg_status dm_sorted_keys(reg_handle* h, const char* who, const double* d_xyz, const double* d_nrm, int64_t n,
                                 const double* T, double inv, int64_t* runs) {
    HIPCHK(h, h->dm.reserve((size_t)n));
    HIPCHK(h, h->dm_misc.reserve(256));
    if (T) {
        HIPCHK(h, h->dm_tf[0].reserve((size_t)n * 24));
        if (d_nrm) HIPCHK(h, h->dm_tf[1].reserve((size_t)n * 24));
    }
    const RunArrays a = h->dm.arrays();
    HIPCHK(h, hipMemsetAsync(h->dm_misc.p, 0, 4, h->stream));
    k_dm_keys<<<grid_for(n), 256, 0, h->stream>>>(d_xyz, d_nrm, n, T ? 1 : 0, xform_rows(T), inv, h->dm_tf[0].as<double>(),
                                                  h->dm_tf[1].as<double>(), a.keys, a.vals, h->dm_misc.as<uint32_t>());
    uint32_t bad = 0, tail[2];
    HIPCHK(h, hipMemcpyAsync(&bad, h->dm_misc.p, 4, hipMemcpyDeviceToHost, h->stream));
    REGCHK(sort_runs(h, a, n, tail));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (bad) {
        h->err = std::string(who) + ((bad & 1u) ? ": non-finite coordinate" : ": voxel index outside +-2^20");
        return REG_BAD_ARGUMENT;
    }
    *runs = flag_total(tail);
    return REG_OK;
}

// VoxelizedPointCloud::insert of a device cloud (n > 0), after the optional transform
static reg_status dm_insert_device(reg_dense_map* m, const char* who, const double* d_xyz, const double* d_nrm,
                                   const double* d_col, int64_t n, const double* T, int64_t* n_new_out) {
    reg_handle* h = m->h;
    int64_t runs = 0;
    REGCHK(dm_sorted_keys(h, who, d_xyz, d_nrm, n, T, m->inv, &runs));
    const double* px = T ? h->dm_tf[0].as<double>() : d_xyz;
    const double* pn = d_nrm ? (T ? h->dm_tf[1].as<double>() : d_nrm) : nullptr;
    HIPCHK(h, h->dm_rank.reserve((size_t)runs * 4));
    HIPCHK(h, h->dm_new.reserve((size_t)runs * 4));
    HIPCHK(h, h->dm_newoff.reserve((size_t)runs * 4));
    HIPCHK(h, h->dm_newkeys.reserve((size_t)runs * 8));
    HIPCHK(h, h->dm_mark.reserve((size_t)std::max<int64_t>(m->n, 1) * 4));
    const RunArrays a = h->dm.arrays();   // as dm_sorted_keys left them
    const uint64_t* sorted = a.sorted;
    const uint32_t *svals = a.svals, *heads = a.heads, *run = a.run;
    uint32_t *rank = h->dm_rank.as<uint32_t>(), *is_new = h->dm_new.as<uint32_t>(), *new_off = h->dm_newoff.as<uint32_t>();
    uint32_t* touched = h->dm_mark.as<uint32_t>();
    uint64_t* new_keys = h->dm_newkeys.as<uint64_t>();
    const DmCols in = dm_cols(m, m->cur, m->has_nrm, m->has_col);
    if (m->n > 0) HIPCHK(h, hipMemsetAsync(touched, 0, (size_t)m->n * 4, h->stream));
    k_dm_rank<<<grid_for(n), 256, 0, h->stream>>>(sorted, n, heads, run, in.key, m->n, rank, is_new, touched);
    int64_t n_new = 0;
    REGCHK(scan_total(h, is_new, new_off, runs, &n_new));
    HIPCHK(h, hipGetLastError());
    const int64_t total = m->n + n_new;
    if (total > kDmMaxRows) {
        h->err = std::string(who) + ": the map would exceed 2^31 - 1 voxels";
        return REG_BAD_ARGUMENT;
    }
    const bool nrm = m->has_nrm || pn, col = m->has_col || d_col;
    HIPCHK(h, dm_reserve_spare(m, (size_t)total, nrm, col));
    const DmCols out = dm_cols(m, m->cur ^ 1, nrm, col);
    if (n_new > 0) k_dm_new_keys<<<grid_for(n), 256, 0, h->stream>>>(sorted, n, heads, run, is_new, new_off, new_keys);
    if (m->n > 0) k_dm_copy<<<grid_for(m->n), 256, 0, h->stream>>>(in, m->n, touched, new_keys, n_new, out);
    k_dm_accumulate<<<grid_for(n), 256, 0, h->stream>>>(sorted, svals, n, heads, run, rank, is_new, new_off, new_keys, n_new, px,
                                                        pn, d_col, in, out);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    dm_swap(m, total, nrm, col);
    *n_new_out = n_new;
    return REG_OK;
}

static bool dm_cloud_args_ok(const double* xyz, int64_t n) { return n >= 0 && n <= kDmMaxRows && (n == 0 || xyz); }

// the running sum -r, +v, +v, ... while <= r (VoxelHashMap.cpp:25-27); false: more than kDmMaxOffsets
static bool dm_offsets(double r, double v, DmOffsets* o) {
    o->n = 0;
    for (double d = -r; d <= r; d += v) {
        if (o->n == kDmMaxOffsets) return false;
        o->d[o->n++] = d;
    }
    for (int k = o->n; k < kDmMaxOffsets; ++k) o->d[k] = 0.0;
    return true;
}

// the scan parameters reg_dense_map_insert_scan accepts: struct_size, a known crop type, no NaN colour bound
static bool dm_scan_params_ok(const reg_dense_scan_params* p, CropCfg* crop) {
    bool ok = p && p->struct_size == (int32_t)sizeof(reg_dense_scan_params) && crop_cfg(&p->crop, crop);
    for (int k = 0; ok && k < 3; ++k) ok = !(p->rgb_min[k] != p->rgb_min[k]) && !(p->rgb_max[k] != p->rgb_max[k]);
    return ok;
}
// the arguments reg_dense_map_carve refuses, without a device: the bounds of the longest loop a lane can run -- offsets per
// axis, samples per ray (the reference loops forever at r <= 0)
static bool dm_carve_params_ok(const reg_dense_carve_params* p, double voxel, DmOffsets* off) {
    if (!p || p->struct_size != (int32_t)sizeof(reg_dense_carve_params)) return false;
    const double r = p->neighborhood_radius, step = 2.0 * r;
    return r > 0.0 && std::isfinite(r) && p->max_ray > 0.0 && std::isfinite(p->max_ray) && std::isfinite(p->truncation) &&
           std::isfinite(step) && dm_offsets(r, voxel, off) && !(p->max_ray / step > 65536.0);
}
static reg_status dm_carve_args(reg_dense_map* m, const char* who, const double* scan_xyz, int64_t n_scan, const double* sensor,
                                const reg_dense_carve_params* p, DmOffsets* off) {
    reg_handle* h = m->h;
    if (!p || p->struct_size != (int32_t)sizeof(reg_dense_carve_params) || !sensor || !dm_cloud_args_ok(scan_xyz, n_scan)) {
        h->err = std::string(who) + ": params / sensor missing, a wrong struct_size, or a bad scan";
        return REG_BAD_ARGUMENT;
    }
    if (!dm_carve_params_ok(p, m->voxel, off)) {
        h->err = std::string(who) + ": neighborhood_radius and max_ray finite and > 0, truncation finite, at most 16 offsets per "
                                    "axis, max_ray / (2 neighborhood_radius) <= 65536";
        return REG_BAD_ARGUMENT;
    }
    return REG_OK;
}
// the erase marks of `rows` voxels (or the de-duplication flags of `rows` scan points), the keep flags and the scans of both
static reg_status dm_reserve_marks(reg_handle* h, size_t rows) {
    for (DevBuf* b : {&h->dm_mark, &h->dm_off1, &h->dm_keep, &h->dm_off2}) HIPCHK(h, b->reserve(rows * 4));
    return REG_OK;
}
// Erases the voxels whose mark (h->dm_mark, enqueued on the stream) is set: builds the rest in the spare side, swaps, and
// reports the erased keys in ascending order.  A failure leaves the map as it was.
static reg_status dm_erase_marked(reg_dense_map* m, int on_device, int32_t* removed_keys, int64_t* n_removed) {
    reg_handle* h = m->h;
    const int64_t n = m->n;
    uint32_t *mark = h->dm_mark.as<uint32_t>(), *rem_off = h->dm_off1.as<uint32_t>();
    uint32_t *keep = h->dm_keep.as<uint32_t>(), *keep_off = h->dm_off2.as<uint32_t>();
    const DmCols in = dm_cols(m, m->cur, m->has_nrm, m->has_col);
    int64_t removed = 0;
    REGCHK(scan_total(h, mark, rem_off, n, &removed));
    HIPCHK(h, hipGetLastError());
    if (removed == 0) return REG_OK;
    StagedOut so(h, h->dm_out, on_device);
    const int s_keys = so.add(removed_keys, 3);
    HIPCHK(h, so.reserve((size_t)removed));
    HIPCHK(h, dm_reserve_spare(m, (size_t)(n - removed), m->has_nrm, m->has_col));
    const DmCols out = dm_cols(m, m->cur ^ 1, m->has_nrm, m->has_col);
    k_dm_keep_flags<<<grid_for(n), 256, 0, h->stream>>>(mark, n, keep);
    REGCHK(scan_excl(h, h->rp_tmp, keep, keep_off, (size_t)n));
    k_dm_erase<<<grid_for(n), 256, 0, h->stream>>>(in, n, mark, keep_off, rem_off, out, so.at<int32_t>(s_keys));
    HIPCHK(h, so.copy_back((size_t)removed));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    dm_swap(m, n - removed, m->has_nrm, m->has_col);
    if (n_removed) *n_removed = removed;
    return REG_OK;
}

template <int kLanes>
static void dm_launch_carve_bricks(reg_handle* h, const double* rays, int64_t n_rays, const double* sensor,
                                   const reg_dense_carve_params* p, double voxel, const DmOffsets& off, const uint64_t* rkeys,
                                   int64_t n_res, int64_t n_bricks, unsigned long long* stats) {
    const double r = p->neighborhood_radius;
    k_dm_carve_bricks<kLanes><<<grid_for(n_rays, 256 / kLanes), 256, 0, h->stream>>>(
        rays, n_rays, sensor[0], sensor[1], sensor[2], 2.0 * r, p->max_ray, p->truncation, r, voxel, voxel * 0.5, off, rkeys, n_res,
        h->dm_bkeys.as<uint64_t>(), h->dm_bmask.as<uint64_t>(), n_bricks, h->dm_mark.as<uint32_t>(), stats);
}

// Submap::carve for the dense map on a device scan (n > 0): transform (T given), first-wins de-duplication at the map's voxel
// size, the carve of the kept points through the coarse level, erase.  Arguments are checked by the caller.
static reg_status dm_carve_scan_device(reg_dense_map* m, const char* who, const double* d_scan, int64_t n_scan, const double* sensor,
                                       const reg_dense_carve_params* p, const DmOffsets& off, const double* T, int on_device,
                                       int32_t* removed_keys, int64_t* n_removed) {
    reg_handle* h = m->h;
    const int64_t n = m->n, rows = std::max(n_scan, n);
    HIPCHK(h, h->dm.reserve((size_t)rows));   // both sorts of this call: no buffer moves while a kernel reads it
    int64_t n_rays = 0;
    REGCHK(dm_sorted_keys(h, who, d_scan, nullptr, n_scan, T, m->inv, &n_rays));   // the refusals of reg_dedup_voxels
    h->dm_last[0] = h->dm_last[1] = h->dm_last[2] = 0;
    h->dm_last[3] = n_rays;
    if (n == 0) return REG_OK;
    const double* px = T ? h->dm_tf[0].as<double>() : d_scan;
    REGCHK(dm_reserve_marks(h, (size_t)rows));
    HIPCHK(h, h->dm_crop[0].reserve((size_t)n_rays * 24));
    const RunArrays a = h->dm.arrays();
    uint32_t *flags = h->dm_keep.as<uint32_t>(), *offs = h->dm_off2.as<uint32_t>();
    double* rays = h->dm_crop[0].as<double>();
    HIPCHK(h, hipMemsetAsync(flags, 0, (size_t)n_scan * 4, h->stream));
    k_dm_dedup_mark<<<grid_for(n_scan), 256, 0, h->stream>>>(a.heads, a.svals, n_scan, flags);
    REGCHK(scan_excl(h, h->rp_tmp, flags, offs, (size_t)n_scan));
    k_gather_rows<3, true><<<grid_for(n_scan), 256, 0, h->stream>>>(cols64_in(px, nullptr, nullptr), n_scan, flags, offs,
                                                                    Cols64{rays, nullptr, nullptr}, nullptr);
    const uint64_t* rkeys = dm_cols(m, m->cur, false, false).key;
    HIPCHK(h, hipMemsetAsync(h->dm_mark.p, 0, (size_t)n * 4, h->stream));
    const int lanes = h->dm_carve_lanes;
    if (lanes < 0) {   // measurement only (reg_debug_dense_carve): the lookups of reg_dense_map_carve
        const double r = p->neighborhood_radius;
        k_dm_carve<<<grid_for(n_rays, 4), 256, 0, h->stream>>>(rays, n_rays, sensor[0], sensor[1], sensor[2], 2.0 * r, p->max_ray,
                                                               p->truncation, r, m->voxel, m->voxel * 0.5, off, rkeys, n,
                                                               h->dm_mark.as<uint32_t>());
        return dm_erase_marked(m, on_device, removed_keys, n_removed);
    }
    // the coarse level of the map as it stands
    uint32_t tail[2];
    k_dm_brick_keys<<<grid_for(n), 256, 0, h->stream>>>(rkeys, n, a.keys, a.vals);
    REGCHK(sort_runs(h, a, n, tail));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    const int64_t n_bricks = flag_total(tail);
    HIPCHK(h, dm_grow(h->dm_bkeys, (size_t)n_bricks, 8));
    HIPCHK(h, dm_grow(h->dm_bmask, (size_t)n_bricks, 64));
    k_dm_brick_masks<<<grid_for(n), 256, 0, h->stream>>>(a.sorted, a.svals, n, a.heads, a.run, rkeys, h->dm_bkeys.as<uint64_t>(),
                                                         h->dm_bmask.as<uint64_t>());
    unsigned long long* stats = nullptr;
    if (h->dm_carve_stats) {
        HIPCHK(h, h->dm_stats.reserve(16));
        HIPCHK(h, hipMemsetAsync(h->dm_stats.p, 0, 16, h->stream));
        stats = h->dm_stats.as<unsigned long long>();
    }
    switch (lanes ? lanes : kDmCarveLanes) {
        case 8: dm_launch_carve_bricks<8>(h, rays, n_rays, sensor, p, m->voxel, off, rkeys, n, n_bricks, stats); break;
        case 16: dm_launch_carve_bricks<16>(h, rays, n_rays, sensor, p, m->voxel, off, rkeys, n, n_bricks, stats); break;
        default: dm_launch_carve_bricks<64>(h, rays, n_rays, sensor, p, m->voxel, off, rkeys, n, n_bricks, stats); break;
    }
    h->dm_last[0] = n_bricks;
    if (stats) {
        unsigned long long got[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(got, stats, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->dm_last[1] = (int64_t)got[0];
        h->dm_last[2] = (int64_t)got[1];
    }
    return dm_erase_marked(m, on_device, removed_keys, n_removed);
}

extern "C" {

int32_t reg_host_dense_offsets(double neighborhood_radius, double voxel_size, double* offsets) {
    DmOffsets o;
    if (!(neighborhood_radius > 0.0) || !std::isfinite(neighborhood_radius) || !(voxel_size > 0.0) || !std::isfinite(voxel_size) ||
        !dm_offsets(neighborhood_radius, voxel_size, &o))
        return -1;
    if (offsets)
        for (int k = 0; k < o.n; ++k) offsets[k] = o.d[k];
    return o.n;
}

reg_status reg_dense_map_create(reg_handle* h, double voxel_size, reg_dense_map** out) {
    if (!h || !out) return REG_BAD_ARGUMENT;
    *out = nullptr;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) {
        h->err = "reg_dense_map_create: voxel_size must be finite and > 0";
        return REG_BAD_ARGUMENT;
    }
    reg_dense_map* m = new reg_dense_map();   // holds no device memory until the first insert
    m->h = h;
    m->voxel = voxel_size;
    m->inv = 1.0 / voxel_size;
    *out = m;
    return REG_OK;
}

void reg_dense_map_destroy(reg_dense_map* m) {
    if (!m) return;
    if (m->h->device_ok && hipSetDevice(m->h->prm.device) == hipSuccess) (void)hipStreamSynchronize(m->h->stream);
    delete m;
}

reg_status reg_dense_map_clear(reg_dense_map* m) {
    if (!m) return REG_BAD_ARGUMENT;
    m->n = 0;   // VoxelHashMap::clear drops the voxels; the has-field flags stay, as isHasNormals_ / isHasColors_ do
    return REG_OK;
}

reg_status reg_dense_map_get_info(const reg_dense_map* m, reg_dense_map_info* info) {
    if (!m || !info || info->struct_size != (int32_t)sizeof(reg_dense_map_info)) return REG_BAD_ARGUMENT;
    info->has_normals = m->has_nrm;
    info->has_colors = m->has_col;
    info->reserved = 0;
    info->n_voxels = m->n;
    info->capacity = (int64_t)(m->side[m->cur].key.cap / 8);
    info->voxel_size = m->voxel;
    return REG_OK;
}

reg_status reg_dense_map_insert(reg_dense_map* m, const double* xyz, const double* normals, const double* colors, int64_t n,
                                int on_device, const double T[16], int64_t* n_voxels, int64_t* n_new) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (n_voxels) *n_voxels = m->n;
    if (n_new) *n_new = 0;
    if (!dm_cloud_args_ok(xyz, n)) {
        h->err = "reg_dense_map_insert: 0 <= n <= 2^31 - 1 and a cloud for n > 0";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d[3] = {xyz, normals, colors};
    for (int k = 0; k < 3; ++k) HIPCHK(h, staged_input(h, h->dm_in[k], d[k], (size_t)n * 3, on_device, &d[k]));
    int64_t added = 0;
    REGCHK(dm_insert_device(m, "reg_dense_map_insert", d[0], d[1], d[2], n, T, &added));
    if (n_voxels) *n_voxels = m->n;
    if (n_new) *n_new = added;
    return REG_OK;
}

void reg_default_dense_scan_params(reg_dense_scan_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_dense_scan_params);
    p->crop.type = REG_CROP_NONE;
    for (int k = 0; k < 3; ++k) p->rgb_min[k] = 0.0, p->rgb_max[k] = 1.0;
}

reg_status reg_dense_map_insert_scan(reg_dense_map* m, const double* xyz, const double* normals, const double* colors, int64_t n,
                                     int on_device, const reg_dense_scan_params* p, const double T_map_to_sensor[16],
                                     int64_t* n_inserted, int64_t* n_voxels) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (n_inserted) *n_inserted = 0;
    if (n_voxels) *n_voxels = m->n;
    CropCfg crop;
    if (!dm_scan_params_ok(p, &crop)) {
        h->err = "reg_dense_map_insert_scan: params missing, of the wrong struct_size, an unknown crop type or a NaN colour bound";
        return REG_BAD_ARGUMENT;
    }
    if (!dm_cloud_args_ok(xyz, n)) {
        h->err = "reg_dense_map_insert_scan: 0 <= n <= 2^31 - 1 and a cloud for n > 0";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d[3] = {xyz, normals, colors};
    for (int k = 0; k < 3; ++k) HIPCHK(h, staged_input(h, h->dm_in[k], d[k], (size_t)n * 3, on_device, &d[k]));
    int64_t kept = n;
    if (crop.type != REG_CROP_NONE || d[2]) {   // denseMapCropper_->crop, then colorCropper_.crop: one order-preserving pass
        HIPCHK(h, h->dm_keep.reserve((size_t)n * 4));
        HIPCHK(h, h->dm_off2.reserve((size_t)n * 4));
        uint32_t *flags = h->dm_keep.as<uint32_t>(), *offs = h->dm_off2.as<uint32_t>();
        k_dm_scan_flags<<<grid_for(n), 256, 0, h->stream>>>(d[0], d[2], n, crop, p->rgb_min[0], p->rgb_min[1], p->rgb_min[2],
                                                            p->rgb_max[0], p->rgb_max[1], p->rgb_max[2], flags);
        REGCHK(scan_total(h, flags, offs, n, &kept));
        HIPCHK(h, hipGetLastError());
        if (kept > 0 && kept < n) {
            double* o[3] = {nullptr, nullptr, nullptr};
            for (int k = 0; k < 3; ++k)
                if (d[k]) {
                    HIPCHK(h, h->dm_crop[k].reserve((size_t)kept * 24));
                    o[k] = h->dm_crop[k].as<double>();
                }
            k_gather_rows<3, true><<<grid_for(n), 256, 0, h->stream>>>(cols64_in(d[0], d[1], d[2]), n, flags, offs,
                                                                       Cols64{o[0], o[1], o[2]}, nullptr);
            for (int k = 0; k < 3; ++k) d[k] = o[k];
        }
    }
    if (kept == 0) return REG_OK;
    int64_t added = 0;
    REGCHK(dm_insert_device(m, "reg_dense_map_insert_scan", d[0], d[1], d[2], kept, T_map_to_sensor, &added));
    if (n_inserted) *n_inserted = kept;
    if (n_voxels) *n_voxels = m->n;
    return REG_OK;
}

void reg_default_dense_carve_params(reg_dense_carve_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_dense_carve_params);
    p->neighborhood_radius = 0.1;   // SpaceCarvingParameters, Parameters.hpp:88-95
    p->max_ray = 20.0;
    p->truncation = 0.1;
}

reg_status reg_dense_map_carve(reg_dense_map* m, const double* scan_xyz, int64_t n_scan, int on_device, const double sensor[3],
                               const reg_dense_carve_params* p, int32_t* removed_keys, int64_t* n_removed) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (n_removed) *n_removed = 0;
    DmOffsets off;
    REGCHK(dm_carve_args(m, "reg_dense_map_carve", scan_xyz, n_scan, sensor, p, &off));
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_scan == 0 || m->n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d_scan = scan_xyz;
    HIPCHK(h, staged_input(h, h->dm_in[0], d_scan, (size_t)n_scan * 3, on_device, &d_scan));
    const int64_t n = m->n;
    REGCHK(dm_reserve_marks(h, (size_t)n));
    const double r = p->neighborhood_radius;
    HIPCHK(h, hipMemsetAsync(h->dm_mark.p, 0, (size_t)n * 4, h->stream));
    k_dm_carve<<<grid_for(n_scan, 4), 256, 0, h->stream>>>(d_scan, n_scan, sensor[0], sensor[1], sensor[2], 2.0 * r, p->max_ray,
                                                           p->truncation, r, m->voxel, m->voxel * 0.5, off,
                                                           dm_cols(m, m->cur, false, false).key, n, h->dm_mark.as<uint32_t>());
    return dm_erase_marked(m, on_device, removed_keys, n_removed);
}

reg_status reg_dense_map_carve_scan(reg_dense_map* m, const double* scan_xyz, int64_t n_scan, int on_device, const double sensor[3],
                                    const reg_dense_carve_params* p, const double T[16], int32_t* removed_keys,
                                    int64_t* n_removed) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (n_removed) *n_removed = 0;
    DmOffsets off;
    REGCHK(dm_carve_args(m, "reg_dense_map_carve_scan", scan_xyz, n_scan, sensor, p, &off));
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_scan == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d_scan = scan_xyz;
    HIPCHK(h, staged_input(h, h->dm_in[0], d_scan, (size_t)n_scan * 3, on_device, &d_scan));
    return dm_carve_scan_device(m, "reg_dense_map_carve_scan", d_scan, n_scan, sensor, p, off, T, on_device, removed_keys,
                                n_removed);
}

reg_status reg_debug_dense_carve(reg_handle* h, int32_t lanes_per_ray, int32_t collect_stats, int64_t last[4]) {
    if (!h || !(lanes_per_ray == 0 || lanes_per_ray == -1 || lanes_per_ray == 8 || lanes_per_ray == 16 || lanes_per_ray == 64))
        return REG_BAD_ARGUMENT;
    if (last)
        for (int k = 0; k < 4; ++k) last[k] = h->dm_last[k];
    h->dm_carve_lanes = lanes_per_ray;
    h->dm_carve_stats = collect_stats != 0;
    return REG_OK;
}

reg_status reg_dense_map_transform(reg_dense_map* m, const double T[16]) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (!T) {
        h->err = "reg_dense_map_transform: T is missing";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (m->n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, dm_reserve_spare(m, (size_t)m->n, m->has_nrm, m->has_col));
    k_dm_transform<<<grid_for(m->n), 256, 0, h->stream>>>(dm_cols(m, m->cur, m->has_nrm, m->has_col), m->n, xform_rows(T),
                                                          dm_cols(m, m->cur ^ 1, m->has_nrm, m->has_col));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    dm_swap(m, m->n, m->has_nrm, m->has_col);
    return REG_OK;
}

reg_status reg_dense_map_center(reg_dense_map* m, double center[3]) {
    if (!m || !center) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    center[0] = center[1] = center[2] = 0.0;   // an empty map: 0 / 1e-6
    if (m->n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, h->dm_misc.reserve(256));
    double* d_out = (double*)((char*)h->dm_misc.p + 64);
    k_dm_center<<<1, 64, 0, h->stream>>>(dm_cols(m, m->cur, false, false), m->n, d_out);
    HIPCHK(h, hipMemcpyAsync(center, d_out, 24, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return REG_OK;
}

reg_status reg_dense_map_export(reg_dense_map* m, int on_device, double* xyz, double* normals, double* colors, int32_t* keys,
                                int32_t* counts, int64_t capacity_rows, int64_t* n_out) {
    if (!m) return REG_BAD_ARGUMENT;
    reg_handle* h = m->h;
    if (n_out) *n_out = 0;
    if (capacity_rows < m->n) {
        h->err = "reg_dense_map_export: capacity_rows is below the number of voxels";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_out) *n_out = m->n;
    if (m->n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    StagedOut so(h, h->dm_out, on_device);   // normals / colours only when the map has met the field
    const int s_xyz = so.add(xyz, 3), s_nrm = so.add(m->has_nrm ? normals : nullptr, 3),
              s_col = so.add(m->has_col ? colors : nullptr, 3), s_keys = so.add(keys, 3), s_cnt = so.add(counts, 1);
    HIPCHK(h, so.reserve((size_t)m->n));
    k_dm_export<<<grid_for(m->n), 256, 0, h->stream>>>(dm_cols(m, m->cur, m->has_nrm, m->has_col), m->n, so.at<double>(s_xyz),
                                                       so.at<double>(s_nrm), so.at<double>(s_col), so.at<int32_t>(s_keys),
                                                       so.at<int32_t>(s_cnt));
    HIPCHK(h, so.copy_back((size_t)m->n));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return REG_OK;
}

reg_status reg_dedup_voxels(reg_handle* h, const double* xyz, int64_t n, int on_device, double voxel_size, int32_t* kept_idx,
                            int64_t* n_kept) {
    if (!h) return REG_BAD_ARGUMENT;
    if (n_kept) *n_kept = 0;
    if (!(voxel_size > 0.0) || !std::isfinite(voxel_size) || !dm_cloud_args_ok(xyz, n) || (n > 0 && !kept_idx)) {
        h->err = "reg_dedup_voxels: voxel_size finite and > 0, 0 <= n <= 2^31 - 1, a cloud and an index array for n > 0";
        return REG_BAD_ARGUMENT;
    }
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n == 0) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double* d_xyz = xyz;
    HIPCHK(h, staged_input(h, h->dm_in[0], d_xyz, (size_t)n * 3, on_device, &d_xyz));
    int64_t runs = 0;
    REGCHK(dm_sorted_keys(h, "reg_dedup_voxels", d_xyz, nullptr, n, nullptr, 1.0 / voxel_size, &runs));
    HIPCHK(h, h->dm_mark.reserve((size_t)n * 4));
    HIPCHK(h, h->dm_off1.reserve((size_t)n * 4));
    uint32_t *flags = h->dm_mark.as<uint32_t>(), *offs = h->dm_off1.as<uint32_t>();
    StagedOut so(h, h->dm_out, on_device);
    const int s_idx = so.add(kept_idx, 1);
    HIPCHK(h, so.reserve((size_t)runs));
    HIPCHK(h, hipMemsetAsync(flags, 0, (size_t)n * 4, h->stream));
    k_dm_dedup_mark<<<grid_for(n), 256, 0, h->stream>>>(h->dm.heads.as<uint32_t>(), h->dm.vals2.as<uint32_t>(), n, flags);
    REGCHK(scan_excl(h, h->rp_tmp, flags, offs, (size_t)n));
    k_carve_collect<<<grid_for(n), 256, 0, h->stream>>>(flags, offs, n, so.at<int32_t>(s_idx));
    HIPCHK(h, so.copy_back((size_t)runs));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_kept) *n_kept = runs;
    return REG_OK;
}

}  // extern "C"
