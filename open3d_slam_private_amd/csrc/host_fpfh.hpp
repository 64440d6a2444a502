// host_fpfh.hpp -- reg_compute_fpfh and reg_match_features: Submap::computeFeatures (Submap.cpp:255-275) and the feature
// matching front of RegistrationRANSACBasedOnFeatureMatching (PlaceRecognition.cpp:71-85)
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// One nearest-neighbour search of the rows of A among the rows of B into nn (device, na words)
static reg_status mf_search(reg_handle* h, const double* d_a, int64_t na, const double* d_b, int64_t nb, int dim, int32_t* nn) {
    const int n_chunks = (int)((nb + kMfChunk - 1) / kMfChunk);
    HIPCHK(h, h->mf_part.reserve((size_t)n_chunks * (size_t)na * 12));
    double* pd = h->mf_part.as<double>();
    int32_t* pi = reinterpret_cast<int32_t*>(pd + (size_t)n_chunks * (size_t)na);
    const dim3 grid((unsigned)grid_for(na), (unsigned)n_chunks);
    if (dim == kFpfhDim)
        k_mf_search<kFpfhDim><<<grid, 256, 0, h->stream>>>(d_a, na, d_b, nb, dim, pd, pi);
    else
        k_mf_search<kMfMaxDim><<<grid, 256, 0, h->stream>>>(d_a, na, d_b, nb, dim, pd, pi);
    k_mf_merge<<<grid_for(na), 256, 0, h->stream>>>(pd, pi, na, n_chunks, nn);
    return REG_OK;
}

extern "C" {

reg_status reg_compute_fpfh(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* normals, int64_t nrm_stride,
                            int64_t n, int on_device, int max_nn, float radius, double* fpfh, double* spfh,
                            int32_t* n_neighbours, int64_t* n_rescanned) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_rescanned) *n_rescanned = 0;
    if (!xyz || xyz_stride < 3 || !normals || nrm_stride < 3 || !fpfh || max_nn < 2 || max_nn > kFpfhMaxNn ||
        !(radius > 0.f) || !std::isfinite(radius) || n > 0x7fffffffLL) {
        h->err = "reg_compute_fpfh: bad argument (2 <= max_nn <= 128, finite radius > 0, xyz, normals and fpfh != NULL)";
        return REG_BAD_ARGUMENT;
    }
    if (n <= 0) {
        h->err = "The point cloud is empty";
        return REG_EMPTY_SOURCE;
    }
    REGCHK(normals_workspace(h, "reg_compute_fpfh"));
    reg_handle* w = h->normals_ws;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const float *d_xyz = nullptr, *d_nrm = nullptr;
    HIPCHK(h, staged_input(h, h->fp_xyz, xyz, (size_t)n * xyz_stride, on_device, &d_xyz));
    HIPCHK(h, staged_input(h, h->fp_nrm, normals, (size_t)n * nrm_stride, on_device, &d_nrm));
    HIPCHK(h, h->fp_misc.reserve(64));
    uint32_t* misc = h->fp_misc.as<uint32_t>();   // [0] non-finite input, [1] rescanned points
    HIPCHK(h, hipMemsetAsync(misc, 0, 8, h->stream));
    k_fpfh_check<<<grid_for(n), 256, 0, h->stream>>>(d_xyz, xyz_stride, d_nrm, nrm_stride, n, misc);
    uint32_t back[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(&back[0], misc, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (back[0]) {
        h->err = "reg_compute_fpfh: a coordinate or a normal component is not finite";
        return REG_BAD_ARGUMENT;
    }
    w->prm.max_dist = radius;
    const reg_status st = reg_set_target(w, d_xyz, xyz_stride, nullptr, 3, nullptr, n, 1);
    if (st != REG_OK) {
        h->err = w->err;
        return st;
    }
    const int start = knn_start_level(w, n, max_nn);
    // workspace: ordered ids | counts, m; host callers get their outputs through fp_out
    HIPCHK(h, h->fp_ids.reserve((size_t)n * max_nn * 4));
    HIPCHK(h, h->fp_cnt.reserve((size_t)n * (kFpfhDim + 1) * 4));
    int32_t* d_ids = h->fp_ids.as<int32_t>();
    int32_t* d_cnt = h->fp_cnt.as<int32_t>();
    int32_t* d_m = d_cnt + (size_t)n * kFpfhDim;
    StagedOut so(h, h->fp_out, on_device);
    const int s_f = so.add(fpfh, kFpfhDim), s_s = so.add(spfh, kFpfhDim);
    HIPCHK(h, so.reserve((size_t)n));
    const unsigned blocks = (unsigned)((n + kFpfhWaves - 1) / kFpfhWaves);
    k_fpfh_spfh<<<blocks, 64 * kFpfhWaves, 0, h->stream>>>(w->grid, d_xyz, xyz_stride, d_nrm, nrm_stride, n, max_nn, start,
                                                         d_ids, d_cnt, d_m, misc + 1);
    k_fpfh_accum<<<blocks, 64 * kFpfhWaves, 0, h->stream>>>(d_xyz, xyz_stride, n, max_nn, d_ids, d_cnt, d_m,
                                                          so.at<double>(s_f), so.at<double>(s_s));
    HIPCHK(h, hipMemcpyAsync(&back[1], misc + 1, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, so.copy_back((size_t)n));
    HIPCHK(h, copy_out(h, n_neighbours, d_m, (size_t)n * 4, on_device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_rescanned) *n_rescanned = back[1];
    return REG_OK;
}

reg_status reg_match_features(reg_handle* h, const double* fa, int64_t na, const double* fb, int64_t nb, int dim, int on_device,
                              int32_t* nn_ab, int32_t* nn_ba, int32_t* mutual, int64_t* n_mutual) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_mutual) *n_mutual = 0;
    if (dim < 1 || dim > kMfMaxDim || na > 0x7fffffffLL || nb > 0x7fffffffLL || (mutual && !n_mutual)) {
        h->err = "reg_match_features: bad argument (1 <= dim <= 64, na, nb <= 2^31 - 1, n_mutual != NULL with mutual)";
        return REG_BAD_ARGUMENT;
    }
    if (na <= 0) {
        h->err = "The source feature set is empty";
        return REG_EMPTY_SOURCE;
    }
    if (nb <= 0) {
        h->err = "The target feature set is empty";
        return REG_EMPTY_TARGET;
    }
    if (!fa || !fb || !nn_ab) {
        h->err = "reg_match_features: null array";
        return REG_BAD_ARGUMENT;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    const bool backward = nn_ba != nullptr || mutual != nullptr;
    const double *d_a = nullptr, *d_b = nullptr;
    HIPCHK(h, staged_input(h, h->mf_a, fa, (size_t)na * dim, on_device, &d_a));
    HIPCHK(h, staged_input(h, h->mf_b, fb, (size_t)nb * dim, on_device, &d_b));
    // nn_ab (na rows), nn_ba (nb rows; the mutual test reads it whether the caller wants it or not), mutual pairs (<= na)
    StagedOut so(h, h->mf_nn, on_device);
    const int s_ab = so.add(nn_ab, 1), s_ba = so.add(nn_ba, 1, mutual != nullptr), s_mu = so.add(mutual, 2);
    HIPCHK(h, so.reserve((size_t)std::max(na, nb)));
    int32_t *d_ab = so.at<int32_t>(s_ab), *d_ba = so.at<int32_t>(s_ba), *d_mu = so.at<int32_t>(s_mu);
    REGCHK(mf_search(h, d_a, na, d_b, nb, dim, d_ab));
    int64_t km = 0;
    if (backward) REGCHK(mf_search(h, d_b, nb, d_a, na, dim, d_ba));
    if (mutual) {
        HIPCHK(h, h->mf_flags.reserve((size_t)(na + 1) * 8));
        uint32_t* flags = h->mf_flags.as<uint32_t>();
        uint32_t* offs = flags + (na + 1);
        k_mf_flags<<<grid_for(na + 1), 256, 0, h->stream>>>(d_ab, d_ba, na, flags);
        REGCHK(scan_excl(h, h->rp_tmp, flags, offs, (size_t)na + 1));
        uint32_t total = 0;
        HIPCHK(h, hipMemcpyAsync(&total, offs + na, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        km = total;
        if (km > 0) k_mf_collect<<<grid_for(na), 256, 0, h->stream>>>(flags, offs, na, d_ab, d_mu);
    }
    HIPCHK(h, so.copy_back(s_ab, (size_t)na));
    HIPCHK(h, so.copy_back(s_ba, (size_t)nb));
    HIPCHK(h, so.copy_back(s_mu, (size_t)km));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_mutual) *n_mutual = km;
    return REG_OK;
}

}  // extern "C"
