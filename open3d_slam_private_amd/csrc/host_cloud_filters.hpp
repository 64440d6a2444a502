// host_cloud_filters.hpp -- C ABI of the descriptor-carrying filter chain (reg_filter_cloud; kernels_filters.hpp)
// Part of the single translation unit reg_core.hip (included there after host_octree.hpp, whose glibc rand() replay
// MAX_DENSITY shares; not a standalone header).
#pragma once

namespace {

// What a descriptor filter needs of fields[]: spans of its inputs / output (0: the slot is unused).
struct FcNeeds {
    int span_a, span_b, span_out;   // span_a < 0: any span >= 1
};

bool fc_needs(int type, FcNeeds& nd) {
    switch (type) {
        case REG_DPF_OBSERVATION_DIRECTION: nd = {0, 0, 3}; return true;
        case REG_DPF_ORIENT_NORMALS: nd = {3, 3, 0}; return true;
        case REG_DPF_SHADOW: nd = {3, 0, 0}; return true;
        case REG_DPF_SIMPLE_SENSOR_NOISE: nd = {0, 0, 1}; return true;
        case REG_DPF_INCIDENCE_ANGLE: nd = {3, 3, 1}; return true;
        case REG_DPF_CUT_AT_DESCRIPTOR_THRESHOLD: nd = {-1, 0, 0}; return true;
        case REG_DPF_MAX_DENSITY: nd = {-1, 0, 0}; return true;
        default: return false;
    }
}

}  // namespace

extern "C" {

reg_status reg_host_glibc_rand(uint32_t seed, int64_t count, int32_t* out) {
    if (count < 0 || (count > 0 && !out)) return REG_BAD_ARGUMENT;
    std::vector<int32_t> rv;
    oct_glibc_rand(seed ? seed : 1u, count, rv);   // srand(0) seeds 1 (glibc srandom_r)
    for (int64_t j = 0; j < count; ++j) out[j] = rv[(size_t)j];
    return REG_OK;
}

reg_status reg_filter_cloud(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n, int on_device,
                            const reg_field* fields, int n_fields, const reg_cloud_filter* filters, int n_filters,
                            float* out_xyz, int32_t* out_idx, int64_t* n_out) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!xyz || xyz_stride < 3 || n < 0 || n > 0x7fffffffLL || !out_xyz || !n_out || n_filters < 0 ||
        (n_filters > 0 && !filters) || n_fields < 0 || n_fields > REG_MAX_FIELDS || (n_fields > 0 && !fields)) {
        h->err = "reg_filter_cloud: bad argument (at most 16 fields; xyz / out_xyz / n_out != NULL)";
        return REG_BAD_ARGUMENT;
    }
    size_t off[REG_MAX_FIELDS + 1] = {0};   // field f starts at off[f] * n floats of the workspace
    bool present[REG_MAX_FIELDS] = {false};
    for (int f = 0; f < n_fields; ++f) {
        if (fields[f].span < 1 || fields[f].span > 16 || fields[f].reserved != 0) {
            h->err = "reg_filter_cloud: field " + std::to_string(f) + ": span must lie in 1..16, reserved must be 0";
            return REG_BAD_ARGUMENT;
        }
        off[f + 1] = off[f] + (size_t)fields[f].span;
        present[f] = fields[f].in != nullptr;
    }
    // the whole chain is checked before anything runs: records, field indices and spans, and which fields exist where
    for (int k = 0; k < n_filters; ++k) {
        const reg_cloud_filter& c = filters[k];
        const std::string who = "reg_filter_cloud: filter " + std::to_string(k);
        if (c.struct_size != (int32_t)sizeof(reg_cloud_filter) || c.reserved[0] || c.reserved[1] || c.reserved[2]) {
            h->err = who + ": struct_size (and reserved must be 0)";
            return REG_BAD_ARGUMENT;
        }
        FcNeeds nd;
        if (!fc_needs(c.base.type, nd)) {
            if (!pf_valid(c.base)) {
                h->err = who + ": bad filter";
                return REG_BAD_ARGUMENT;
            }
            continue;
        }
        const int ids[3] = {c.field_a, c.field_b, c.field_out};
        const int spans[3] = {nd.span_a, nd.span_b, nd.span_out};
        for (int t = 0; t < 3; ++t) {
            if (spans[t] == 0) continue;
            if (ids[t] < -1 || ids[t] >= n_fields || (t == 2 && ids[t] < 0)) {
                h->err = who + ": field index out of range";
                return REG_BAD_ARGUMENT;
            }
            if (ids[t] < 0 || (t < 2 && !present[ids[t]])) {
                h->err = who + ": a descriptor field this filter reads does not exist";
                return REG_MISSING_FIELD;
            }
            if (spans[t] > 0 && fields[ids[t]].span != spans[t]) {
                h->err = who + ": field span";
                return REG_BAD_ARGUMENT;
            }
        }
        if (nd.span_out) present[c.field_out] = true;
        if (c.base.type == REG_DPF_SIMPLE_SENSOR_NOISE && (c.flag < 0 || c.flag > 4)) {
            h->err = who + ": SimpleSensorNoise sensorType must lie in 0..4";
            return REG_BAD_ARGUMENT;
        }
        if (c.base.type == REG_DPF_MAX_DENSITY && !(c.v[0] > 0.f)) {
            h->err = who + ": MaxDensity maxDensity must be > 0";
            return REG_BAD_ARGUMENT;
        }
        if (c.base.type == REG_DPF_ORIENT_NORMALS && c.field_a == c.field_b) {
            h->err = who + ": OrientNormals needs two different fields";
            return REG_BAD_ARGUMENT;
        }
    }
    *n_out = 0;
    if (n == 0) return REG_OK;
    const int N = (int)n;
    HIPCHK(h, hipSetDevice(h->prm.device));
    hipStream_t s = h->stream;
    const float* d_in = nullptr;
    HIPCHK(h, staged_input(h, h->f_in, xyz, (size_t)(N - 1) * (size_t)xyz_stride + 3, on_device, &d_in));
    HIPCHK(h, h->f_px.reserve((size_t)N * 12));
    HIPCHK(h, h->f_fields.reserve(std::max<size_t>(off[n_fields], 1) * (size_t)N * 4));
    HIPCHK(h, h->f_perm.reserve((size_t)N * 4));
    HIPCHK(h, h->f_lid.reserve((size_t)N * 4));
    HIPCHK(h, h->f_keep.reserve((size_t)N * 4));
    HIPCHK(h, h->f_pos.reserve((size_t)N * 4));
    HIPCHK(h, h->f_keys.reserve((size_t)N * 8));
    HIPCHK(h, h->f_misc.reserve(64));
    float* px = h->f_px.as<float>();
    float* ws = h->f_fields.as<float>();
    auto field_ws = [&](int f) { return ws + off[f] * (size_t)N; };
    int32_t* idx = h->f_perm.as<int32_t>();
    int32_t* idx2 = h->f_lid.as<int32_t>();
    uint32_t* flag = h->f_keep.as<uint32_t>();
    uint32_t* pos = h->f_pos.as<uint32_t>();
    uint32_t* misc = h->f_misc.as<uint32_t>();
    k_pf_pack<<<grid_for(N), 256, 0, s>>>(d_in, xyz_stride, nullptr, nullptr, N, px, nullptr, nullptr, idx);
    for (int f = 0; f < n_fields; ++f)   // existing fields go straight into the workspace
        if (fields[f].in)
            HIPCHK(h, hipMemcpyAsync(field_ws(f), fields[f].in, (size_t)N * fields[f].span * 4,
                                     on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    int m = N;
    for (int k = 0; k < n_filters && m > 0; ++k) {
        const reg_cloud_filter& c = filters[k];
        const int type = c.base.type;
        if (type == REG_DPF_IDENTITY) continue;
        FcNeeds nd;
        if (!fc_needs(type, nd)) {
            reg_status st = pf_flags(h, c.base, px, idx, m, flag, "reg_filter_cloud");
            if (st != REG_OK) return st;
            st = pf_compact(h, idx, idx2, flag, pos, m);
            if (st != REG_OK) return st;
            continue;
        }
        CloudFilterDev d{};
        d.type = type;
        d.flag = c.flag;
        for (int a = 0; a < 3; ++a) d.v[a] = c.v[a];
        float* fa = nd.span_a ? field_ws(c.field_a) : nullptr;
        const float* fb = nd.span_b ? field_ws(c.field_b) : nullptr;
        float* fo = nd.span_out ? field_ws(c.field_out) : nullptr;
        const int span_a = nd.span_a ? fields[c.field_a].span : 0;
        if (type == REG_DPF_OBSERVATION_DIRECTION || type == REG_DPF_ORIENT_NORMALS || type == REG_DPF_SIMPLE_SENSOR_NOISE ||
            type == REG_DPF_INCIDENCE_ANGLE) {
            k_fc_map<<<grid_for(m), 256, 0, s>>>(px, idx, m, d, fa, fb, fo);
            continue;
        }
        const uint32_t* need = nullptr;
        const uint32_t* draw_pos = nullptr;
        const float* d_draws = nullptr;
        std::vector<float> draws;
        if (type == REG_DPF_MAX_DENSITY) {
            uint32_t* need_w = h->f_keys.as<uint32_t>();
            uint32_t* dpos_w = need_w + m;
            HIPCHK(h, hipMemsetAsync(misc, 0, 8, s));
            k_fc_density_max<<<grid_for(m), 256, 0, s>>>(fa, span_a, idx, m, misc);
            k_fc_density_mask<<<grid_for(m), 256, 0, s>>>(fa, span_a, idx, m, c.v[0], misc, need_w);
            REGCHK(scan_excl(h, h->rp_tmp, need_w, dpos_w, (size_t)m));
            uint32_t rb[2] = {0u, 0u}, tail[2];
            HIPCHK(h, hipMemcpyAsync(rb, misc, 8, hipMemcpyDeviceToHost, s));
            REGCHK(flag_total_async(h, need_w, dpos_w, m, tail));
            HIPCHK(h, hipStreamSynchronize(s));
            d.last = float_from_orderable(rb[0]);
            d.sat_factor = (float)(1 - (int)rb[1] / m);   // integer division, MaxDensity.cpp:88
            const int64_t n_draws = flag_total(tail);
            std::vector<int32_t> rv;
            oct_glibc_rand(c.seed ? c.seed : 1u, n_draws, rv);   // srand(0) seeds 1 (glibc srandom_r)
            draws.resize((size_t)std::max<int64_t>(n_draws, 1));
            for (int64_t j = 0; j < n_draws; ++j) draws[(size_t)j] = (float)rv[(size_t)j] / (float)2147483647;
            HIPCHK(h, h->f_draws.reserve(draws.size() * 4));
            HIPCHK(h, hipMemcpy(h->f_draws.p, draws.data(), draws.size() * 4, hipMemcpyHostToDevice));   // done on return
            need = need_w;
            draw_pos = dpos_w;
            d_draws = h->f_draws.as<float>();
        }
        k_fc_pred<<<grid_for(m), 256, 0, s>>>(px, idx, m, d, fa, span_a, need, draw_pos, d_draws, flag);
        reg_status st = pf_compact(h, idx, idx2, flag, pos, m);
        if (st != REG_OK) return st;
    }
    // outputs: xyz, idx, then every field that exists at the end of the chain (slot s_f0 + f)
    StagedOut so(h, h->f_out, on_device);
    const int s_xyz = so.add(out_xyz, 3), s_idx = so.add(out_idx, 1), s_f0 = s_idx + 1;
    for (int f = 0; f < n_fields; ++f) so.add(present[f] ? fields[f].out : nullptr, (size_t)fields[f].span);
    HIPCHK(h, so.reserve((size_t)m));
    if (m > 0) {
        k_pf_gather<<<grid_for(m), 256, 0, s>>>(px, nullptr, nullptr, idx, m, so.at<float>(s_xyz), nullptr, nullptr,
                                                so.at<int32_t>(s_idx));
        for (int f = 0; f < n_fields; ++f)
            if (float* of = so.at<float>(s_f0 + f))
                k_fc_gather<<<grid_for((int64_t)m * fields[f].span), 256, 0, s>>>(field_ws(f), fields[f].span, idx, m, of);
    }
    HIPCHK(h, so.copy_back((size_t)m));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    *n_out = m;
    return REG_OK;
}

void reg_default_voxel_grid_params(reg_voxel_grid_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_voxel_grid_params);
    p->v_size[0] = p->v_size[1] = p->v_size[2] = 1.f;
    p->use_centroid = 1;
    p->average_existing_descriptors = 1;
}

reg_status reg_voxel_grid(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n, int on_device,
                          const reg_field* fields, int n_fields, const reg_voxel_grid_params* p, float* out_xyz,
                          int32_t* out_idx, int64_t* n_out) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    bool ok = xyz && xyz_stride >= 3 && n >= 0 && n <= 0x7fffffffLL && out_xyz && n_out && n_fields >= 0 &&
              n_fields <= REG_MAX_FIELDS && (n_fields == 0 || fields) && p &&
              p->struct_size == (int32_t)sizeof(reg_voxel_grid_params) && !p->reserved[0] && !p->reserved[1];
    for (int a = 0; ok && a < 3; ++a) ok = std::isfinite(p->v_size[a]) && p->v_size[a] > 0.f;
    size_t off[REG_MAX_FIELDS + 1] = {0};
    for (int f = 0; ok && f < n_fields; ++f) {
        ok = fields[f].in && fields[f].span >= 1 && fields[f].span <= 16 && fields[f].reserved == 0;
        off[f + 1] = off[f] + (size_t)(ok ? fields[f].span : 0);
    }
    if (!ok) {
        h->err = "reg_voxel_grid: bad argument (struct_size, vSize > 0, at most 16 fields with in != NULL and span 1..16, "
                 "xyz / out_xyz / n_out != NULL)";
        return REG_BAD_ARGUMENT;
    }
    if (!p->use_centroid) {
        h->err = "reg_voxel_grid: useCentroid 0 writes the cell centre into feature rows 1..3 in the reference "
                 "(VoxelGrid.cpp:289-304) and is not supported";
        return REG_UNSUPPORTED;
    }
    *n_out = 0;
    if (n == 0) return REG_OK;
    const int N = (int)n;
    HIPCHK(h, hipSetDevice(h->prm.device));
    hipStream_t s = h->stream;
    const float* d_in = nullptr;
    HIPCHK(h, staged_input(h, h->f_in, xyz, (size_t)(N - 1) * (size_t)xyz_stride + 3, on_device, &d_in));
    HIPCHK(h, h->f_px.reserve((size_t)N * 12));
    HIPCHK(h, h->f_misc.reserve(64));
    float* px = h->f_px.as<float>();
    uint32_t box[7];
    REGCHK(pack_cloud_box(h, "reg_voxel_grid", d_in, xyz_stride, N, px, box));
    VoxelGridDev g{};
    unsigned __int128 total = 1;
    uint64_t nd[3];
    for (int a = 0; a < 3; ++a) {
        const float lo = float_from_orderable(box[a]), hi = float_from_orderable(box[3 + a]);
        const float v = p->v_size[a];
        const float min_bound = lo / v;
        float d = hi / v;
        d = 1.0f + d;
        d = d - min_bound;
        if (!(d >= 0.f && d < 4294967296.f)) {
            h->err = "reg_voxel_grid: the grid has 2^32 or more cells along an axis";
            return REG_BAD_ARGUMENT;
        }
        nd[a] = (uint64_t)(unsigned)d;
        g.v[a] = v;
        g.min_bound[a] = min_bound;
        total *= nd[a];
    }
    if (total >= ((unsigned __int128)1 << 32)) {
        h->err = "reg_voxel_grid: nx * ny * nz >= 2^32 voxels";
        return REG_BAD_ARGUMENT;
    }
    g.nx = nd[0];
    g.nxy = nd[0] * nd[1];
    const size_t N4 = (size_t)N * 4, N8 = (size_t)N * 8;
    HIPCHK(h, h->f_keys.reserve(N8));
    HIPCHK(h, h->f_keys2.reserve(N8));
    HIPCHK(h, h->f_perm.reserve(N4));
    HIPCHK(h, h->f_lid.reserve(N4));
    HIPCHK(h, h->f_keep.reserve(N4));
    HIPCHK(h, h->f_pos.reserve(N4));
    uint64_t *keys = h->f_keys.as<uint64_t>(), *keys_s = h->f_keys2.as<uint64_t>();
    int32_t *iota = h->f_perm.as<int32_t>(), *idx = h->f_lid.as<int32_t>();
    uint32_t *is_first = h->f_keep.as<uint32_t>(), *pos = h->f_pos.as<uint32_t>();
    k_vg_keys<<<grid_for(N), 256, 0, s>>>(px, N, g, keys, iota);
    // a cell index may reach numDiv by rounding, so the ids stay below 4 * total (< 2^34)
    const int bits = std::min(64, oct_bits((uint64_t)total * 4u));
    REGCHK(sort_pairs(h, h->rp_tmp, keys, keys_s, iota, idx, (unsigned)N, 0, bits));
    k_vg_first<<<grid_for(N), 256, 0, s>>>(keys_s, idx, N, is_first);
    REGCHK(scan_excl(h, h->rp_tmp, is_first, pos, (size_t)N));
    uint32_t tail[2];
    REGCHK(flag_total_async(h, is_first, pos, N, tail));
    HIPCHK(h, hipStreamSynchronize(s));
    const int m = (int)flag_total(tail);
    // fields: device inputs are read in place, host inputs go through the workspace
    const float* fin[REG_MAX_FIELDS] = {nullptr};
    if (!on_device && n_fields > 0) HIPCHK(h, h->f_fields.reserve(off[n_fields] * (size_t)N * 4));
    for (int f = 0; f < n_fields; ++f) {
        fin[f] = fields[f].in;
        if (!on_device) {
            float* w = h->f_fields.as<float>() + off[f] * (size_t)N;
            HIPCHK(h, hipMemcpyAsync(w, fields[f].in, (size_t)N * fields[f].span * 4, hipMemcpyHostToDevice, s));
            fin[f] = w;
        }
    }
    StagedOut so(h, h->f_out, on_device);   // xyz, idx, then field f in slot s_f0 + f
    const int s_xyz = so.add(out_xyz, 3), s_idx = so.add(out_idx, 1), s_f0 = s_idx + 1;
    for (int f = 0; f < n_fields; ++f) so.add(fields[f].out, (size_t)fields[f].span);
    HIPCHK(h, so.reserve((size_t)m));
    k_vg_reduce<<<grid_for((int64_t)N * 3), 256, 0, s>>>(px, 3, 3, keys_s, idx, pos, N, 1, so.at<float>(s_xyz),
                                                         so.at<int32_t>(s_idx));
    for (int f = 0; f < n_fields; ++f)
        if (float* of = so.at<float>(s_f0 + f))
            k_vg_reduce<<<grid_for((int64_t)N * fields[f].span), 256, 0, s>>>(fin[f], fields[f].span, fields[f].span, keys_s,
                                                                             idx, pos, N,
                                                                             p->average_existing_descriptors ? 1 : 0, of,
                                                                             nullptr);
    HIPCHK(h, so.copy_back((size_t)m));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    *n_out = m;
    return REG_OK;
}

}  // extern "C"
