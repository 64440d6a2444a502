// host_filters.hpp -- C ABI of the data-point filters (reg_sampling_surface_normal, reg_filter_points)
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

namespace {

// Tree shape of SamplingSurfaceNormal: depends only on (n, knn).  Per level the open segments [begin, end) and the
// slots of their children in the next level (-1: a leaf); the leaves' begins in depth-first order (+ sentinel n).
struct SsnPlan {
    std::vector<int32_t> seg;          // per level: begins[ns], ends[ns], children[2 ns]
    std::vector<size_t> level_off;     // offset of each level's block in seg
    std::vector<int> level_ns;
    std::vector<int32_t> leaf_begin;
};

void ssn_plan(int n, int knn, SsnPlan& P) {
    std::vector<std::pair<int32_t, int32_t>> cur, nxt;
    if (n > knn) cur.push_back({0, n});
    else P.leaf_begin.push_back(0);
    while (!cur.empty()) {
        const int ns = (int)cur.size();
        const size_t off = P.seg.size();
        P.level_off.push_back(off);
        P.level_ns.push_back(ns);
        P.seg.resize(off + 4 * (size_t)ns);
        nxt.clear();
        for (int j = 0; j < ns; ++j) {
            const int32_t b = cur[j].first, c = cur[j].second, left = c - c / 2;
            P.seg[off + j] = b;
            P.seg[off + ns + j] = b + c;
            const std::pair<int32_t, int32_t> ch[2] = {{b, left}, {b + left, c - left}};
            for (int t = 0; t < 2; ++t) {
                if (ch[t].second > knn) {
                    P.seg[off + 2 * ns + 2 * j + t] = (int32_t)nxt.size();
                    nxt.push_back(ch[t]);
                } else {
                    P.seg[off + 2 * ns + 2 * j + t] = -1;
                    P.leaf_begin.push_back(ch[t].first);
                }
            }
        }
        cur.swap(nxt);
    }
    std::sort(P.leaf_begin.begin(), P.leaf_begin.end());
    P.leaf_begin.push_back(n);
}

// The checks reg_filter_points makes on one reg_point_filter (types REG_DPF_IDENTITY .. REG_DPF_FIX_STEP_SAMPLING).
bool pf_valid(const reg_point_filter& f) {
    const bool quant = f.type == REG_DPF_MAX_QUANTILE_ON_AXIS;
    bool ok = f.type >= REG_DPF_IDENTITY && f.type <= REG_DPF_FIX_STEP_SAMPLING &&
              (quant ? (f.dim >= 0 && f.dim <= 2) : (f.dim >= -1 && f.dim <= 2));
    if (quant) ok = ok && f.value > 0.f && f.value < 1.f;
    if (f.type == REG_DPF_FIX_STEP_SAMPLING) ok = ok && f.step >= 1 && f.phase >= 0 && f.phase < f.step;
    return ok;
}

// flag[j] = the filter keeps the j-th point of the index list (f_keys / f_misc are scratch; `who` prefixes errors)
reg_status pf_flags(reg_handle* h, const reg_point_filter& f, const float* px, const int32_t* idx, int m, uint32_t* flag,
                    const char* who) {
    hipStream_t s = h->stream;
    PointFilterDev d{};
    d.type = f.type;
    const bool uses_dim = f.type == REG_DPF_MAX_DIST || f.type == REG_DPF_MIN_DIST || f.type == REG_DPF_DISTANCE_LIMIT ||
                          f.type == REG_DPF_MAX_QUANTILE_ON_AXIS;
    d.dim = uses_dim ? f.dim : 0;
    d.remove_inside = f.remove_inside;
    d.step = f.step;
    d.phase = f.phase;
    d.value = (uses_dim && f.dim < 0) ? std::fabs(f.value) : f.value;   // anyabs() for the norm
    for (int a = 0; a < 6; ++a) d.box[a] = f.box[a];
    if (f.type == REG_DPF_MAX_QUANTILE_ON_AXIS) {
        const int q = (int)((float)m * f.value);   // int(float(n) * ratio), MaxQuantileOnAxis.cpp
        if (q >= m) {
            h->err = std::string(who) + ": MaxQuantileOnAxis quantile index beyond the cloud";
            return REG_BAD_ARGUMENT;
        }
        float* vals = h->f_keys.as<float>();
        float* sorted = vals + m;
        HIPCHK(h, hipMemsetAsync(h->f_misc.p, 0, 4, s));
        k_pf_axis<<<grid_for(m), 256, 0, s>>>(px, idx, m, f.dim, vals, h->f_misc.as<uint32_t>());
        REGCHK(sort_keys(h, h->rp_tmp, vals, sorted, (unsigned)m, 0, 32));
        uint32_t has_nan = 0;
        HIPCHK(h, hipMemcpyAsync(&d.limit, sorted + q, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(&has_nan, h->f_misc.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        if (has_nan) {
            h->err = std::string(who) + ": MaxQuantileOnAxis on an axis holding NaN (run RemoveNaN first)";
            return REG_BAD_ARGUMENT;
        }
    }
    k_pf_pred<<<grid_for(m), 256, 0, s>>>(px, idx, m, d, flag);
    return REG_OK;
}

// Order-preserving compaction of the index list by flag: idx <- the kept entries (idx2 is the spare list), m <- their count.
reg_status pf_compact(reg_handle* h, int32_t*& idx, int32_t*& idx2, const uint32_t* flag, uint32_t* pos, int& m) {
    hipStream_t s = h->stream;
    REGCHK(scan_excl(h, h->rp_tmp, flag, pos, (size_t)m));
    k_pf_compact<<<grid_for(m), 256, 0, s>>>(idx, m, flag, pos, idx2);
    uint32_t tail[2];
    REGCHK(flag_total_async(h, flag, pos, m, tail));
    HIPCHK(h, hipStreamSynchronize(s));
    m = (int)flag_total(tail);
    std::swap(idx, idx2);
    return REG_OK;
}

}  // namespace

extern "C" {

void reg_default_ssn_params(reg_ssn_params* p) {
    if (!p) return;
    p->struct_size = (int32_t)sizeof(reg_ssn_params);
    p->knn = 7;
    p->sampling_method = 0;
    p->ratio = 0.5f;
    p->max_box_dim = std::numeric_limits<float>::infinity();
    p->average_existing_descriptors = 1;
    p->keep_normals = 1;
    p->keep_densities = 0;
    p->keep_eigen_values = 0;
    p->keep_eigen_vectors = 0;
}

reg_status reg_sampling_surface_normal(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n, int on_device,
                                       const reg_ssn_params* p, const reg_ssn_out* out, int64_t* n_out,
                                       int64_t* n_unfit) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!p || p->struct_size != (int32_t)sizeof(reg_ssn_params) || !out || !out->xyz || !xyz || xyz_stride < 3 ||
        n < 0 || n > 0x7fffffffLL || !n_out || p->knn < 3 || (p->sampling_method != 0 && p->sampling_method != 1) ||
        !(p->ratio > 0.f) || std::isnan(p->max_box_dim)) {
        h->err = "reg_sampling_surface_normal: bad argument (struct_size, knn >= 3, samplingMethod 0 | 1, ratio > 0, "
                 "xyz / out->xyz / n_out != NULL)";
        return REG_BAD_ARGUMENT;
    }
    if (p->knn > kSsnMaxKnn) {
        h->err = "reg_sampling_surface_normal: knn above 64 is not supported by this build";
        return REG_UNSUPPORTED;
    }
    if (p->sampling_method == 0 && p->ratio < 1.f) {
        h->err = "reg_sampling_surface_normal: samplingMethod 0 with ratio < 1 draws from std::rand (not reproducible)";
        return REG_UNSUPPORTED;
    }
    if (n == 0) {
        h->err = "The point cloud is empty";
        return REG_EMPTY_SOURCE;
    }
    const int N = (int)n, knn = p->knn, method = p->sampling_method;
    const bool need_eig = p->keep_normals || p->keep_eigen_values || p->keep_eigen_vectors;
    HIPCHK(h, hipSetDevice(h->prm.device));
    hipStream_t s = h->stream;
    const float* d_in = nullptr;
    HIPCHK(h, staged_input(h, h->f_in, xyz, (size_t)(N - 1) * (size_t)xyz_stride + 3, on_device, &d_in));
    HIPCHK(h, h->f_px.reserve((size_t)N * 12));
    HIPCHK(h, h->f_misc.reserve(64));
    float* px = h->f_px.as<float>();
    uint32_t* misc = h->f_misc.as<uint32_t>();   // pack_cloud_box's words, then [8..9] n_unfit (64-bit)
    uint32_t box[7];
    REGCHK(pack_cloud_box(h, "reg_sampling_surface_normal", d_in, xyz_stride, N, px, box));
    SsnPlan P;
    ssn_plan(N, knn, P);
    const int n_leaves = (int)P.leaf_begin.size() - 1;
    int max_ns = 1;
    for (int ns : P.level_ns) max_ns = std::max(max_ns, ns);
    HIPCHK(h, h->f_segs.reserve((P.seg.size() + P.leaf_begin.size()) * 4));
    int32_t* d_segs = h->f_segs.as<int32_t>();
    if (!P.seg.empty()) HIPCHK(h, hipMemcpyAsync(d_segs, P.seg.data(), P.seg.size() * 4, hipMemcpyHostToDevice, s));
    int32_t* d_leaf_begin = d_segs + P.seg.size();
    HIPCHK(h, hipMemcpyAsync(d_leaf_begin, P.leaf_begin.data(), P.leaf_begin.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, h->f_perm.reserve((size_t)N * 4));
    HIPCHK(h, h->f_keys.reserve((size_t)N * 8));
    HIPCHK(h, h->f_keys2.reserve((size_t)N * 8));
    HIPCHK(h, h->f_boxes.reserve((size_t)max_ns * 24));
    HIPCHK(h, h->f_boxes2.reserve((size_t)max_ns * 24));
    int32_t* perm = h->f_perm.as<int32_t>();
    uint64_t* keys = h->f_keys.as<uint64_t>();
    uint64_t* keys2 = h->f_keys2.as<uint64_t>();
    float* boxes = h->f_boxes.as<float>();
    float* boxes2 = h->f_boxes2.as<float>();
    k_ssn_init<<<grid_for(std::max(N, 6)), 256, 0, s>>>(misc, N, boxes, perm);
    // levels: keys -> segmented radix sort of the open segments -> new order -> child boxes
    for (size_t L = 0; L < P.level_ns.size(); ++L) {
        const int ns = P.level_ns[L];
        const int32_t* sb = d_segs + P.level_off[L];
        const int32_t* se = sb + ns;
        const int32_t* ch = se + ns;
        k_ssn_keys<<<grid_for(N), 256, 0, s>>>(px, perm, N, sb, se, ns, boxes, keys);
        REGCHK(with_tmp(h, h->rp_tmp, [&](void* t, size_t& b) {
            return rocprim::segmented_radix_sort_keys(t, b, keys, keys2, (unsigned)N, (unsigned)ns, sb, se, 0, 64, s);
        }));
        k_ssn_extract<<<grid_for(N), 256, 0, s>>>(keys2, N, sb, se, ns, perm);
        k_ssn_children<<<grid_for(ns), 256, 0, s>>>(px, perm, sb, se, ch, ns, boxes, boxes2);
        std::swap(boxes, boxes2);
    }
    // leaves (fuseRange), then the kept rows ascending by kept index
    HIPCHK(h, h->f_mom.reserve((size_t)n_leaves * sizeof(PcaMoments)));
    HIPCHK(h, h->f_lid.reserve((size_t)N * 4));
    HIPCHK(h, h->f_keep.reserve((size_t)N * 4));
    HIPCHK(h, h->f_pos.reserve((size_t)N * 4));
    int32_t* d_lid = (on_device && out->leaf_id) ? out->leaf_id : h->f_lid.as<int32_t>();
    uint32_t* keep = h->f_keep.as<uint32_t>();
    uint32_t* pos = h->f_pos.as<uint32_t>();
    k_ssn_leaf<<<grid_for(n_leaves), 256, 0, s>>>(px, perm, d_leaf_begin, n_leaves, p->max_box_dim, need_eig ? 1 : 0,
                                                  method, h->f_mom.as<PcaMoments>(), d_lid, keep,
                                                  (unsigned long long*)(misc + 8));
    REGCHK(scan_excl(h, h->rp_tmp, keep, pos, (size_t)N));
    uint32_t tail[2];
    unsigned long long unfit = 0;
    REGCHK(flag_total_async(h, keep, pos, N, tail));
    HIPCHK(h, hipMemcpyAsync(&unfit, misc + 8, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const int M = (int)flag_total(tail);
    // outputs: k_ssn_scatter always writes src_idx, k_pca_finish always writes normals
    StagedOut so(h, h->f_out, on_device);
    const int s_xyz = so.add(out->xyz, 3), s_nrm = so.add(out->normals, 3, out->eigvals || out->eigvecs),
              s_den = so.add(out->densities, 1), s_eva = so.add(out->eigvals, 3), s_eve = so.add(out->eigvecs, 9),
              s_src = so.add(out->src_idx, 1, true);
    HIPCHK(h, so.reserve((size_t)M));
    HIPCHK(h, h->f_mom2.reserve((size_t)std::max(M, 1) * sizeof(PcaMoments)));
    if (M > 0) {
        k_ssn_scatter<<<grid_for(N), 256, 0, s>>>(px, N, method, keep, pos, d_lid, h->f_mom.as<PcaMoments>(),
                                                  so.at<float>(s_xyz), so.at<int32_t>(s_src), so.at<float>(s_den),
                                                  h->f_mom2.as<PcaMoments>());
        if (so.at<float>(s_nrm))
            k_pca_finish<<<grid_for(M), 256, 0, s>>>(h->f_mom2.as<PcaMoments>(), M, 0.f, 0.f, 0.f, 0, 0, so.at<float>(s_nrm),
                                                     so.at<float>(s_eva), nullptr, so.at<float>(s_eve), nullptr, nullptr);
    }
    HIPCHK(h, so.copy_back((size_t)M));
    HIPCHK(h, copy_out(h, out->leaf_id, d_lid, (size_t)N * 4, on_device));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    *n_out = M;
    if (n_unfit) *n_unfit = (int64_t)unfit;
    return REG_OK;
}

reg_status reg_filter_points(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm, const float* cov,
                             int64_t n, int on_device, const reg_point_filter* filters, int n_filters, float* out_xyz,
                             float* out_nrm, float* out_cov, int32_t* out_idx, int64_t* n_out) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!xyz || xyz_stride < 3 || n < 0 || n > 0x7fffffffLL || !out_xyz || !n_out || n_filters < 0 ||
        (n_filters > 0 && !filters)) {
        h->err = "reg_filter_points: bad argument";
        return REG_BAD_ARGUMENT;
    }
    for (int k = 0; k < n_filters; ++k)
        if (!pf_valid(filters[k])) {
            h->err = "reg_filter_points: bad filter " + std::to_string(k);
            return REG_BAD_ARGUMENT;
        }
    *n_out = 0;
    if (n == 0) return REG_OK;
    const int N = (int)n;
    HIPCHK(h, hipSetDevice(h->prm.device));
    hipStream_t s = h->stream;
    const float *d_in = nullptr, *d_nrm = nullptr, *d_cov = nullptr;
    HIPCHK(h, staged_input(h, h->f_in, xyz, (size_t)(N - 1) * (size_t)xyz_stride + 3, on_device, &d_in));
    HIPCHK(h, staged_input(h, h->f_in_nrm, nrm, (size_t)N * 3, on_device, &d_nrm));
    HIPCHK(h, staged_input(h, h->f_in_cov, cov, (size_t)N * 6, on_device, &d_cov));
    HIPCHK(h, h->f_px.reserve((size_t)N * 12));
    if (nrm) HIPCHK(h, h->f_pn.reserve((size_t)N * 12));
    if (cov) HIPCHK(h, h->f_pc.reserve((size_t)N * 24));
    HIPCHK(h, h->f_perm.reserve((size_t)N * 4));
    HIPCHK(h, h->f_lid.reserve((size_t)N * 4));
    HIPCHK(h, h->f_keep.reserve((size_t)N * 4));
    HIPCHK(h, h->f_pos.reserve((size_t)N * 4));
    HIPCHK(h, h->f_keys.reserve((size_t)N * 8));
    HIPCHK(h, h->f_misc.reserve(64));
    float *px = h->f_px.as<float>(), *pn = nrm ? h->f_pn.as<float>() : nullptr, *pc = cov ? h->f_pc.as<float>() : nullptr;
    int32_t* idx = h->f_perm.as<int32_t>();
    int32_t* idx2 = h->f_lid.as<int32_t>();
    uint32_t* flag = h->f_keep.as<uint32_t>();
    uint32_t* pos = h->f_pos.as<uint32_t>();
    k_pf_pack<<<grid_for(N), 256, 0, s>>>(d_in, xyz_stride, d_nrm, d_cov, N, px, pn, pc, idx);
    int m = N;
    for (int k = 0; k < n_filters && m > 0; ++k) {
        const reg_point_filter& f = filters[k];
        if (f.type == REG_DPF_IDENTITY) continue;
        reg_status st = pf_flags(h, f, px, idx, m, flag, "reg_filter_points");
        if (st != REG_OK) return st;
        st = pf_compact(h, idx, idx2, flag, pos, m);
        if (st != REG_OK) return st;
    }
    StagedOut so(h, h->f_out, on_device);   // normals / covariances go out only where they came in
    const int s_xyz = so.add(out_xyz, 3), s_nrm = so.add(nrm ? out_nrm : nullptr, 3),
              s_cov = so.add(cov ? out_cov : nullptr, 6), s_idx = so.add(out_idx, 1);
    HIPCHK(h, so.reserve((size_t)m));
    if (m > 0)
        k_pf_gather<<<grid_for(m), 256, 0, s>>>(px, pn, pc, idx, m, so.at<float>(s_xyz), so.at<float>(s_nrm),
                                                so.at<float>(s_cov), so.at<int32_t>(s_idx));
    HIPCHK(h, so.copy_back((size_t)m));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    *n_out = m;
    return REG_OK;
}

}  // extern "C"
