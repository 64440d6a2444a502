// host_octree.hpp -- C ABI of OctreeGridDataPointsFilter (reg_octree_grid; kernels_octree.hpp)
// Part of the single translation unit reg_core.hip (included there after host_filters.hpp; not a standalone header).
#pragma once

namespace {

// Octree_::build's root box (Octree.tpp): radius = float(pow(2, ceil(log(x) / log(2)))), x = double(max radii) * 0.5
void oct_root(const float lo[3], const float hi[3], int center_at_origin, float c[3], float* radius) {
    float radii[3];
    for (int a = 0; a < 3; ++a) radii[a] = hi[a] - lo[a];
    for (int a = 0; a < 3; ++a) {
        const float half = radii[a] * 0.5f;
        c[a] = center_at_origin ? 0.f : lo[a] + half;
    }
    const float rmax = std::max(radii[0], std::max(radii[1], radii[2]));
    const double x = (double)rmax * 0.5;
    *radius = (float)std::pow(2.0, std::ceil(std::log(x) / std::log(2.0)));   // x == 0: pow(2, -inf) == 0
}

// glibc random_r TYPE_3 after srand(seed): the values rand() returns, in order
void oct_glibc_rand(uint32_t seed, int64_t count, std::vector<int32_t>& out) {
    int32_t r[34];
    r[0] = (int32_t)seed;
    for (int i = 1; i < 31; ++i) {
        const int32_t hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
        int32_t w = 16807 * lo - 2836 * hi;
        if (w < 0) w += 2147483647;
        r[i] = w;
    }
    std::vector<uint32_t> st((size_t)(344 + count));
    for (int i = 0; i < 31; ++i) st[i] = (uint32_t)r[i];
    for (int i = 31; i < 34; ++i) st[i] = st[i - 31];
    for (size_t k = 34; k < st.size(); ++k) st[k] = st[k - 31] + st[k - 3];
    out.resize((size_t)count);   // the first 310 values are discarded by srandom_r
    for (int64_t j = 0; j < count; ++j) out[(size_t)j] = (int32_t)(st[(size_t)(344 + j)] >> 1);
}

// RandomPtsSampler's position inside a leaf of `size` members for the draw `rv`
int64_t oct_pick(int64_t size, int32_t rv) {
    const float ratio = (float)rv / (float)2147483647;
    const float f = (float)(size - 1) * ratio;
    return std::min<int64_t>((int64_t)f, size - 1);
}

int oct_bits(uint64_t v) {   // bits needed for the values 0..v
    int b = 1;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

}  // namespace

extern "C" {

void reg_default_octree_params(reg_octree_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_octree_params);
    p->build_parallel = 1;
    p->max_point_by_node = 1;
    p->max_size_by_node = 0.f;
    p->sampling_method = REG_OCTREE_FIRST;
    p->center_at_origin = 1;
}

void reg_host_octree_root(const float min[3], const float max[3], int center_at_origin, float center[3], float* radius) {
    if (!min || !max || !center || !radius) return;
    oct_root(min, max, center_at_origin, center, radius);
}

reg_status reg_host_octree_random_picks(const int64_t* sizes, int64_t n_leaves, int64_t* picks) {
    if (n_leaves < 0 || (n_leaves > 0 && (!sizes || !picks))) return REG_BAD_ARGUMENT;
    for (int64_t L = 0; L < n_leaves; ++L)
        if (sizes[L] < 1) return REG_BAD_ARGUMENT;
    std::vector<int32_t> rv;
    oct_glibc_rand(1u, n_leaves, rv);
    for (int64_t L = 0; L < n_leaves; ++L) picks[L] = oct_pick(sizes[L], rv[(size_t)L]);
    return REG_OK;
}

reg_status reg_octree_grid(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm, const float* cov,
                           int64_t n, int on_device, const reg_octree_params* p, const reg_octree_out* out,
                           int64_t* n_out) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!p || p->struct_size != (int32_t)sizeof(reg_octree_params) || !out || !out->xyz || !xyz || xyz_stride < 3 ||
        n < 0 || n > 0x7fffffffLL || !n_out || p->max_point_by_node < 1 || !(p->max_size_by_node >= 0.f) ||
        p->sampling_method < REG_OCTREE_FIRST || p->sampling_method > REG_OCTREE_MEDOID) {
        h->err = "reg_octree_grid: bad argument (struct_size, maxPointByNode >= 1, maxSizeByNode >= 0, samplingMethod "
                 "0..3, xyz / out->xyz / n_out != NULL)";
        return REG_BAD_ARGUMENT;
    }
    *n_out = 0;
    if (n == 0) {
        h->err = "The point cloud is empty";
        return REG_EMPTY_SOURCE;
    }
    const int N = (int)n, method = p->sampling_method;
    const int64_t max_pts = p->max_point_by_node;
    HIPCHK(h, hipSetDevice(h->prm.device));
    hipStream_t s = h->stream;
    const float *d_in = nullptr, *d_nrm = nullptr, *d_cov = nullptr;
    HIPCHK(h, staged_input(h, h->f_in, xyz, (size_t)(N - 1) * (size_t)xyz_stride + 3, on_device, &d_in));
    HIPCHK(h, staged_input(h, h->f_in_nrm, nrm, (size_t)N * 3, on_device, &d_nrm));
    HIPCHK(h, staged_input(h, h->f_in_cov, cov, (size_t)N * 6, on_device, &d_cov));
    HIPCHK(h, h->f_px.reserve((size_t)N * 12));
    HIPCHK(h, h->f_misc.reserve(64));
    float* px = h->f_px.as<float>();
    uint32_t* misc = h->f_misc.as<uint32_t>();   // pack_cloud_box's words, then [8] any node still open
    uint32_t box[7];
    REGCHK(pack_cloud_box(h, "reg_octree_grid", d_in, xyz_stride, N, px, box));
    float lo[3], hi[3], c0[4] = {0.f, 0.f, 0.f, 0.f}, r0 = 0.f;
    for (int a = 0; a < 3; ++a) {
        lo[a] = float_from_orderable(box[a]);
        hi[a] = float_from_orderable(box[3 + a]);
    }
    oct_root(lo, hi, p->center_at_origin, c0, &r0);
    if (!std::isfinite(r0) || !std::isfinite(c0[0]) || !std::isfinite(c0[1]) || !std::isfinite(c0[2])) {
        h->err = "reg_octree_grid: the cloud's extent overflows the root box";
        return REG_BAD_ARGUMENT;
    }
    // radius of every depth down to the first one whose nodes are leaves by size (double(r) * 2.0 <= maxSizeByNode)
    std::vector<float> radii(1, r0);
    while (!((double)radii.back() * 2.0 <= (double)p->max_size_by_node)) radii.push_back(radii.back() * 0.5f);
    const int d_size = (int)radii.size() - 1;
    HIPCHK(h, h->o_radii.reserve((radii.size() + 4) * 4));
    float* d_radii = h->o_radii.as<float>();
    HIPCHK(h, hipMemcpyAsync(d_radii, radii.data(), radii.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_radii + radii.size(), c0, 12, hipMemcpyHostToDevice, s));
    const float* d_root_c = d_radii + radii.size();
    const size_t N8 = (size_t)N * 8, N4 = (size_t)N * 4;
    HIPCHK(h, h->o_keys.reserve(N8));
    HIPCHK(h, h->o_keys_s.reserve(N8));
    HIPCHK(h, h->o_iota.reserve(N4));
    HIPCHK(h, h->o_idx.reserve(N4));
    HIPCHK(h, h->o_idx2.reserve(N4));
    HIPCHK(h, h->o_rank.reserve(N4));
    HIPCHK(h, h->o_rank_a.reserve(N4));
    HIPCHK(h, h->o_rank_s.reserve(N4));
    HIPCHK(h, h->o_c.reserve((size_t)N * 12));
    HIPCHK(h, h->o_kk.reserve(N4));
    HIPCHK(h, h->o_heads.reserve(N4));
    HIPCHK(h, h->o_pos.reserve(N4));
    HIPCHK(h, h->o_open.reserve(N4));
    HIPCHK(h, h->o_depth.reserve(N4));
    uint64_t *keys = h->o_keys.as<uint64_t>(), *keys_s = h->o_keys_s.as<uint64_t>();
    int32_t *iota = h->o_iota.as<int32_t>(), *idx = h->o_idx.as<int32_t>(), *idx2 = h->o_idx2.as<int32_t>();
    uint32_t *rank = h->o_rank.as<uint32_t>(), *rank_a = h->o_rank_a.as<uint32_t>(), *rank_s = h->o_rank_s.as<uint32_t>();
    uint32_t *kk = h->o_kk.as<uint32_t>(), *heads = h->o_heads.as<uint32_t>(), *pos = h->o_pos.as<uint32_t>();
    uint32_t* open = h->o_open.as<uint32_t>();
    int32_t* depth = h->o_depth.as<int32_t>();
    float* pc = h->o_c.as<float>();
    uint32_t n_leaves = 1;
    if ((int64_t)N <= max_pts || d_size == 0) {
        k_oct_root_leaf<<<grid_for(N), 256, 0, s>>>(N, rank, depth, iota);
    } else {
        uint32_t n_groups = 1;
        for (int d0 = 0;; d0 += kOctLevelsPerRound) {
            const int levels = std::min(kOctLevelsPerRound, d_size - d0);
            const bool first = d0 == 0;
            k_oct_keys<<<grid_for(N), 256, 0, s>>>(px, N, d_root_c, d_radii + d0, levels, first ? nullptr : open, pc, keys,
                                                   iota);
            REGCHK(sort_pairs(h, h->rp_tmp, keys, keys_s, iota, idx, (unsigned)N, 63 - 3 * levels, 63));
            const uint32_t* rk = nullptr;
            if (!first) {   // (rank, key) order: the key order above, then a stable sort by rank
                k_oct_gather_rank<<<grid_for(N), 256, 0, s>>>(idx, rank, N, rank_a);
                REGCHK(sort_pairs(h, h->rp_tmp, rank_a, rank_s, idx, idx2, (unsigned)N, 0, oct_bits(n_groups - 1)));
                std::swap(idx, idx2);
                k_oct_gather_keys<<<grid_for(N), 256, 0, s>>>(idx, keys, N, keys_s);
                rk = rank_s;
            }
            HIPCHK(h, hipMemsetAsync(misc + 8, 0, 4, s));
            k_oct_depth<<<grid_for(N), 256, 0, s>>>(keys_s, rk, idx, first ? nullptr : open, N, max_pts, d0, d_size, kk,
                                                    depth, misc + 8);
            k_oct_heads<<<grid_for(N), 256, 0, s>>>(keys_s, rk, kk, N, heads);
            REGCHK(scan_incl(h, h->rp_tmp, heads, pos, (size_t)N));
            k_oct_scatter<<<grid_for(N), 256, 0, s>>>(idx, pos, kk, N, rank, open);
            uint32_t tail[2] = {0u, 0u};
            HIPCHK(h, hipMemcpyAsync(&tail[0], pos + N - 1, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(&tail[1], misc + 8, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipStreamSynchronize(s));
            n_groups = tail[0];
            if (!tail[1]) break;
            if (d0 + kOctLevelsPerRound >= d_size) {   // cannot happen: depth d_size is a leaf by size
                h->err = "reg_octree_grid: internal error (open node at the size limit)";
                return REG_DEVICE_ERROR;
            }
        }
        n_leaves = n_groups;
    }
    // members by (leaf, input index): a stable sort of the leaf ids in input order (iota from the last k_oct_keys)
    HIPCHK(h, h->o_start.reserve(((size_t)n_leaves + 1) * 4));
    int32_t* start = h->o_start.as<int32_t>();
    REGCHK(sort_pairs(h, h->rp_tmp, rank, rank_s, iota, idx, (unsigned)N, 0, oct_bits(n_leaves - 1)));
    k_oct_starts<<<grid_for(N), 256, 0, s>>>(rank_s, N, (int)n_leaves, start);
    const int32_t* d_rand = nullptr;
    if (method == REG_OCTREE_RAND) {
        std::vector<int32_t> rv;
        oct_glibc_rand(1u, n_leaves, rv);
        HIPCHK(h, h->o_rand.reserve((size_t)n_leaves * 4));
        HIPCHK(h, hipMemcpyAsync(h->o_rand.p, rv.data(), (size_t)n_leaves * 4, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipStreamSynchronize(s));   // rv is released on return from this block
        d_rand = h->o_rand.as<int32_t>();
    }
    // outputs: normals / covariances go out only where they came in; k_oct_sample always writes src_idx
    StagedOut so(h, h->f_out, on_device);
    const int s_xyz = so.add(out->xyz, 3), s_nrm = so.add(d_nrm ? out->normals : nullptr, 3),
              s_cov = so.add(d_cov ? out->covs : nullptr, 6), s_src = so.add(out->src_idx, 1, true);
    HIPCHK(h, so.reserve((size_t)n_leaves));
    k_oct_sample<<<grid_for(n_leaves), 256, 0, s>>>(px, d_nrm, d_cov, idx, start, (int)n_leaves, method, d_rand,
                                                    so.at<float>(s_xyz), so.at<float>(s_nrm), so.at<float>(s_cov),
                                                    so.at<int32_t>(s_src));
    HIPCHK(h, so.copy_back((size_t)n_leaves));
    HIPCHK(h, copy_out(h, out->leaf_id, rank, N4, on_device));
    HIPCHK(h, copy_out(h, out->leaf_depth, depth, N4, on_device));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    *n_out = (int64_t)n_leaves;
    return REG_OK;
}

}  // extern "C"
