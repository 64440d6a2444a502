// host_overlap.hpp -- voxel-overlap selection and the submap-pair front of the constraint builders
// (computeIndicesOfOverlappingPoints + SelectByIndex, helpers.cpp:320-345, constraint_builders.cpp:51-58)
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// Words of ov_misc: [0] invalid-key flag, [1] / [2] unique voxels of the source / target layer
enum { kOvlBad = 0, kOvlRuns = 1 };

// Flags (input order, n + 1 / m + 1 words, the last one 0) and their exclusive scans for both layers, in ov_flags / ov_offs;
// the selected counts.  d_src / d_tgt: device pointers, n, m >= 1.  One synchronisation: the invalid-key word and the counts.
static reg_status ovl_select(reg_handle* h, const double* d_src, int64_t n, const double* d_tgt, int64_t m, const double* T_col,
                             double voxel_size, int32_t min_points, int64_t* n_src, int64_t* n_tgt) {
    const Xform64 T = xform_rows(T_col);   // applied to the source layer only
    const double inv = 1.0 / voxel_size;   // fromVoxelSize (VoxelHashMap.hpp:43-45)
    HIPCHK(h, h->ov_misc.reserve(64));
    HIPCHK(h, hipMemsetAsync(h->ov_misc.p, 0, 64, h->stream));
    uint32_t* misc = h->ov_misc.as<uint32_t>();
    const double* pts[2] = {d_src, d_tgt};
    const int64_t cnt[2] = {n, m};
    HIPCHK(h, h->ov_sorted.reserve((size_t)std::max(n, m) * 8));
    for (int l = 0; l < 2; ++l) {
        const int64_t c = cnt[l];
        HIPCHK(h, h->ov_keys[l].reserve((size_t)c * 8));
        HIPCHK(h, h->ov_ukeys[l].reserve((size_t)c * 8));
        HIPCHK(h, h->ov_ucnt[l].reserve((size_t)c * 4));
        HIPCHK(h, h->ov_flags[l].reserve((size_t)(c + 1) * 4));
        HIPCHK(h, h->ov_offs[l].reserve((size_t)(c + 1) * 4));
        k_ovl_keys<<<grid_for(c), 256, 0, h->stream>>>(pts[l], c, l == 0 && T_col ? 1 : 0, T, inv, h->ov_keys[l].as<uint64_t>(),
                                                       misc + kOvlBad);
        REGCHK(sort_keys(h, h->rp_tmp, h->ov_keys[l].as<uint64_t>(), h->ov_sorted.as<uint64_t>(), (size_t)c, 0, 64));
        REGCHK(with_tmp(h, h->rp_tmp, [&](void* t, size_t& b) {
            return rocprim::run_length_encode(t, b, h->ov_sorted.as<uint64_t>(), (unsigned int)c, h->ov_ukeys[l].as<uint64_t>(),
                                              h->ov_ucnt[l].as<uint32_t>(), misc + kOvlRuns + l, h->stream);
        }));
    }
    for (int l = 0; l < 2; ++l) {
        const int o = 1 - l;
        k_ovl_flags<<<grid_for(cnt[l] + 1), 256, 0, h->stream>>>(
            h->ov_keys[l].as<uint64_t>(), cnt[l], h->ov_ukeys[l].as<uint64_t>(), h->ov_ucnt[l].as<uint32_t>(), misc + kOvlRuns + l,
            h->ov_ukeys[o].as<uint64_t>(), h->ov_ucnt[o].as<uint32_t>(), misc + kOvlRuns + o, (uint32_t)min_points,
            h->ov_flags[l].as<uint32_t>());
        REGCHK(scan_excl(h, h->rp_tmp, h->ov_flags[l].as<uint32_t>(), h->ov_offs[l].as<uint32_t>(), (size_t)cnt[l] + 1));
    }
    uint32_t back[3] = {0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(&back[0], misc + kOvlBad, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&back[1], h->ov_offs[0].as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&back[2], h->ov_offs[1].as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (back[0]) {
        h->err = "overlap: a coordinate is not finite, or voxel_size is too small for the extent of a cloud (voxel index exceeds 2^20)";
        return REG_BAD_ARGUMENT;
    }
    *n_src = back[1];
    *n_tgt = back[2];
    return REG_OK;
}

static bool ovl_args_ok(reg_handle* h, int64_t n, int64_t m, double voxel_size, int32_t min_points) {
    if (n < 0 || m < 0 || n > 0x7fffffffLL || m > 0x7fffffffLL || !(voxel_size > 0.0) || !std::isfinite(voxel_size) ||
        min_points < 1) {
        h->err = "overlap: bad argument (0 <= n, m <= 2^31 - 1, finite voxel_size > 0, min_points_per_voxel >= 1)";
        return false;
    }
    return true;
}

extern "C" {

reg_status reg_overlap_indices(reg_handle* h, const double* src_xyz, int64_t n, const double* tgt_xyz, int64_t m, int on_device,
                               const double T_src_to_tgt[16], double voxel_size, int32_t min_points_per_voxel, int32_t* src_idx,
                               int64_t* n_src, int32_t* tgt_idx, int64_t* n_tgt) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_src) *n_src = 0;
    if (n_tgt) *n_tgt = 0;
    if (!ovl_args_ok(h, n, m, voxel_size, min_points_per_voxel)) return REG_BAD_ARGUMENT;
    if (n == 0 || m == 0) return REG_OK;
    if (!src_xyz || !tgt_xyz || !src_idx || !tgt_idx) {
        h->err = "overlap: null array";
        return REG_BAD_ARGUMENT;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    // host clouds are staged in the fp64 staging buffers of reg_set_source_f64 / reg_set_target_f64: those are dead once
    // their cast kernel has run (the handle keeps the fp32 copies), so the query does not disturb a reference or
    // reading that is set, and a handle used for both pays for one staging area
    const double *d_src = nullptr, *d_tgt = nullptr;
    HIPCHK(h, staged_input(h, h->r_in_xyz, src_xyz, (size_t)n * 3, on_device, &d_src));
    HIPCHK(h, staged_input(h, h->c_in_xyz, tgt_xyz, (size_t)m * 3, on_device, &d_tgt));
    int64_t ks = 0, kt = 0;
    const reg_status s = ovl_select(h, d_src, n, d_tgt, m, T_src_to_tgt, voxel_size, min_points_per_voxel, &ks, &kt);
    if (s != REG_OK) return s;
    // ascending lists; host callers get them through the sorted-key buffer, which is free again (8 bytes per point of the
    // larger layer hold both lists)
    StagedOut so(h, h->ov_sorted, on_device);
    const int s_si = so.add(src_idx, 1), s_ti = so.add(tgt_idx, 1);
    HIPCHK(h, so.reserve((size_t)std::max(ks, kt)));
    int32_t *d_si = so.at<int32_t>(s_si), *d_ti = so.at<int32_t>(s_ti);
    if (ks > 0) k_carve_collect<<<grid_for(n), 256, 0, h->stream>>>(h->ov_flags[0].as<uint32_t>(), h->ov_offs[0].as<uint32_t>(), n, d_si);
    if (kt > 0) k_carve_collect<<<grid_for(m), 256, 0, h->stream>>>(h->ov_flags[1].as<uint32_t>(), h->ov_offs[1].as<uint32_t>(), m, d_ti);
    HIPCHK(h, so.copy_back(s_si, (size_t)ks));
    HIPCHK(h, so.copy_back(s_ti, (size_t)kt));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_src) *n_src = ks;
    if (n_tgt) *n_tgt = kt;
    return REG_OK;
}

reg_status reg_set_pair_overlap_f64(reg_handle* h, const double* src_xyz, const double* src_normals, const double* src_covs,
                                    int64_t n, const double* tgt_xyz, const double* tgt_normals, const double* tgt_covs, int64_t m,
                                    int on_device, const double T_src_to_tgt[16], double voxel_size, int32_t min_points_per_voxel,
                                    int64_t* n_src_kept, int64_t* n_tgt_kept) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_src_kept) *n_src_kept = 0;
    if (n_tgt_kept) *n_tgt_kept = 0;
    // whatever happens below, the previous reference and reading are gone (their staging buffers are reused)
    h->crop_kept = 0;
    h->src_kept = 0;
    h->m = 0;
    h->n = 0;
    h->prepared = false;
    h->have_match = false;
    h->pm_have_match = false;
    if (!ovl_args_ok(h, n, m, voxel_size, min_points_per_voxel)) return REG_BAD_ARGUMENT;
    if (n == 0 || m == 0) {
        h->err = "The reference point cloud is empty (a cloud of the pair is empty)";
        return REG_EMPTY_TARGET;
    }
    if (!src_xyz || !tgt_xyz) {
        h->err = "overlap: null array";
        return REG_BAD_ARGUMENT;
    }
    if (const reg_status fs = check_target_fields(h, tgt_normals != nullptr, tgt_covs != nullptr)) return fs;
    if (const reg_status fs = check_source_fields(h, src_normals != nullptr, src_covs != nullptr)) return fs;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double *d_s[3] = {src_xyz, src_normals, src_covs}, *d_t[3] = {tgt_xyz, tgt_normals, tgt_covs};
    DevBuf* sb[3] = {&h->r_in_xyz, &h->r_in_nrm, &h->r_in_cov};
    DevBuf* tb[3] = {&h->c_in_xyz, &h->c_in_nrm, &h->c_in_cov};
    const size_t width[3] = {3, 3, 9};
    for (int k = 0; k < 3; ++k) {
        HIPCHK(h, staged_input(h, *sb[k], d_s[k], (size_t)n * width[k], on_device, &d_s[k]));
        HIPCHK(h, staged_input(h, *tb[k], d_t[k], (size_t)m * width[k], on_device, &d_t[k]));
    }
    int64_t ks = 0, kt = 0;
    reg_status s = ovl_select(h, d_s[0], n, d_t[0], m, T_src_to_tgt, voxel_size, min_points_per_voxel, &ks, &kt);
    if (s != REG_OK) return s;
    if (n_src_kept) *n_src_kept = ks;
    if (n_tgt_kept) *n_tgt_kept = kt;
    if (ks == 0 || kt == 0) {   // both or neither: a selected voxel holds points of both layers
        h->err = "The reference point cloud is empty (the clouds share no voxel)";
        return REG_EMPTY_TARGET;
    }
    // SelectByIndex + fp64 -> fp32 (open3d_conversions.cpp:57-118): the compaction of reg_set_target_f64 on both clouds
    HIPCHK(h, h->c_xyz.reserve((size_t)kt * 12));
    if (d_t[1]) HIPCHK(h, h->c_nrm.reserve((size_t)kt * 12));
    if (d_t[2]) HIPCHK(h, h->c_cov.reserve((size_t)kt * 24));
    HIPCHK(h, h->c_idx.reserve((size_t)kt * 4));
    k_crop_gather<<<grid_for(m), 256, 0, h->stream>>>(d_t[0], d_t[1], d_t[2], m, h->ov_flags[1].as<uint32_t>(),
                                                      h->ov_offs[1].as<uint32_t>(), h->c_xyz.as<float>(),
                                                      d_t[1] ? h->c_nrm.as<float>() : nullptr,
                                                      d_t[2] ? h->c_cov.as<float>() : nullptr, h->c_idx.as<int32_t>());
    HIPCHK(h, h->r_xyz.reserve((size_t)ks * 12));
    if (d_s[1]) HIPCHK(h, h->r_nrm.reserve((size_t)ks * 12));
    if (d_s[2]) HIPCHK(h, h->r_cov.reserve((size_t)ks * 24));
    HIPCHK(h, h->ov_sidx.reserve((size_t)ks * 4));
    k_crop_gather<<<grid_for(n), 256, 0, h->stream>>>(d_s[0], d_s[1], d_s[2], n, h->ov_flags[0].as<uint32_t>(),
                                                      h->ov_offs[0].as<uint32_t>(), h->r_xyz.as<float>(),
                                                      d_s[1] ? h->r_nrm.as<float>() : nullptr,
                                                      d_s[2] ? h->r_cov.as<float>() : nullptr, h->ov_sidx.as<int32_t>());
    HIPCHK(h, hipGetLastError());
    s = reg_set_target(h, h->c_xyz.as<float>(), 3, d_t[1] ? h->c_nrm.as<float>() : nullptr, 3,
                       d_t[2] ? h->c_cov.as<float>() : nullptr, kt, 1);
    if (s != REG_OK) return s;
    h->crop_kept = kt;
    s = reg_set_source(h, h->r_xyz.as<float>(), 3, d_s[1] ? h->r_nrm.as<float>() : nullptr, 3,
                       d_s[2] ? h->r_cov.as<float>() : nullptr, ks, 1);
    if (s != REG_OK) return s;
    h->src_kept = ks;
    return REG_OK;
}

reg_status reg_get_source_source_indices(reg_handle* h, int32_t* idx) {
    if (!h || !idx) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (h->src_kept <= 0 || h->src_kept != h->n) {
        h->err = "the current reading was not set through reg_set_pair_overlap_f64 or reg_process_scan";
        return REG_NOT_CONFIGURED;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, hipMemcpyAsync(idx, h->ov_sidx.p, (size_t)h->src_kept * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

}  // extern "C"
