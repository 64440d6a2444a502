// host_target.hpp -- reference-side entry points (table build, target preparation rows, normals), reading upload
// Part of the single translation unit reg_core.hip (included there, after host_handle.hpp and host_prims.hpp; not a standalone header).
#pragma once

// copy (host or device) -> device buffer
static reg_status upload(reg_handle* h, DevBuf& dst, const float* src, size_t bytes, int on_device) {
    HIPCHK(h, dst.reserve(bytes));
    HIPCHK(h, hipMemcpyAsync(dst.p, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return REG_OK;
}

static reg_status device_centroid_sums(reg_handle* h, const float* d_xyz, int64_t stride, int64_t n, DevBuf& misc,
                                       long long s[3]) {
    HIPCHK(h, misc.reserve(256));
    HIPCHK(h, hipMemsetAsync(misc.p, 0, 3 * sizeof(unsigned long long), h->stream));
    const int blocks = std::min<int64_t>(1024, (n + 255) / 256);
    k_centroid_sums<<<blocks, 256, 0, h->stream>>>(d_xyz, stride, n, misc.as<unsigned long long>());
    HIPCHK(h, hipMemcpyAsync(s, misc.p, 3 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

static reg_status device_centroid(reg_handle* h, const float* d_xyz, int64_t stride, int64_t n, DevBuf& misc, float out[3]) {
    long long s[3];
    REGCHK(device_centroid_sums(h, d_xyz, stride, n, misc, s));
    for (int k = 0; k < 3; ++k) out[k] = (float)((double)s[k] / (65536.0 * (double)n));
    return REG_OK;
}

// Build the brick table for bin edge c.  Returns occupied-bin count through *occupied.
static reg_status build_grid(reg_handle* h, float c, const float bmin[3], const float bmax[3], uint32_t* occupied) {
    const int64_t m = h->m;
    Grid& g = h->grid;
    const float inv_c = 1.0f / c;
    g.ox = bmin[0];
    g.oy = bmin[1];
    g.oz = bmin[2];
    g.inv_c = inv_c;
    float dims[3];
    for (int k = 0; k < 3; ++k) {
        volatile float d = bmax[k] - bmin[k];
        volatile float s = d * inv_c;
        dims[k] = std::floor((float)s) + 1.0f;
    }
    const double max_dim = (double)(1u << (kBrickBits + kBrickLog2));
    if (dims[0] > max_dim || dims[1] > max_dim || dims[2] > max_dim) {
        h->err = "cell_size too small for the target extent (bin coordinates overflow the sort key)";
        return REG_BAD_ARGUMENT;
    }
    g.dimx = dims[0];
    g.dimy = dims[1];
    g.dimz = dims[2];
    h->info.dims[0] = (int32_t)dims[0];
    h->info.dims[1] = (int32_t)dims[1];
    h->info.dims[2] = (int32_t)dims[2];

    HIPCHK(h, h->t_keys.reserve(m * 8));
    HIPCHK(h, h->t_keys2.reserve(m * 8));
    HIPCHK(h, h->t_vals.reserve(m * 4));
    HIPCHK(h, h->t_vals2.reserve(m * 4));
    k_point_keys<<<grid_for(m), 256, 0, h->stream>>>(h->t_centred.as<float4>(), m, g.ox, g.oy, g.oz, inv_c,
                                                      h->t_keys.as<uint64_t>(), h->t_vals.as<uint32_t>());
    // significant key bits
    auto bits_for = [](double v) { int b = 1; while ((double)(1ull << b) < v) ++b; return b; };
    const int bz_bits = bits_for(std::ceil(dims[2] / kBrickDim) + 1);
    const int end_bit = std::min(64, 3 * kBrickLog2 + 2 * kBrickBits + bz_bits);
    REGCHK(sort_pairs(h, h->rp_tmp, h->t_keys.as<uint64_t>(), h->t_keys2.as<uint64_t>(), h->t_vals.as<uint32_t>(),
                      h->t_vals2.as<uint32_t>(), (size_t)m, 0, end_bit));
    // brick heads -> brick ids
    HIPCHK(h, h->t_flags.reserve(m * 4));
    HIPCHK(h, h->t_scan.reserve(m * 4));
    k_brick_heads<<<grid_for(m), 256, 0, h->stream>>>(h->t_keys2.as<uint64_t>(), m, h->t_flags.as<uint32_t>());
    REGCHK(scan_incl(h, h->rp_tmp, h->t_flags.as<uint32_t>(), h->t_scan.as<uint32_t>(), (size_t)m));
    uint32_t nb = 0;
    HIPCHK(h, hipMemcpyAsync(&nb, h->t_scan.as<uint32_t>() + (m - 1), 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // tables
    uint32_t cap = 16;
    while (cap < 2 * nb) cap <<= 1;
    HIPCHK(h, h->t_hash.reserve((size_t)cap * sizeof(HashEntry)));
    HIPCHK(h, hipMemsetAsync(h->t_hash.p, 0xff, (size_t)cap * sizeof(HashEntry), h->stream));
    const size_t n_cells = (size_t)nb * kBrickCells + 1;
    HIPCHK(h, h->t_cells.reserve(n_cells * 4));
    HIPCHK(h, hipMemsetAsync(h->t_cells.p, 0, n_cells * 4, h->stream));
    HIPCHK(h, h->t_misc.reserve(256));
    HIPCHK(h, hipMemsetAsync(h->t_misc.p, 0, 64, h->stream));
    // dense brick directory (brick id per brick coordinate) when the brick grid is small enough: one 4-byte load
    // instead of a 64-bit hash + probe per row segment
    const int bdx = (int)std::ceil(dims[0] / kBrickDim), bdy = (int)std::ceil(dims[1] / kBrickDim),
              bdz = (int)std::ceil(dims[2] / kBrickDim);
    const size_t n_dir = (size_t)bdx * bdy * bdz;
    // The group search needs the dense directory + row masks (12 bytes per brick coordinate): up to 256 M coordinates = 3 GB
    // of a 288 GB device.  Beyond that the bin edge is too small for the extent of the cloud (reg_set_target enlarges an
    // automatic edge and rejects an explicit one).
    if (n_dir > ((size_t)256 << 20)) {
        h->err = "cell_size too small for the target extent (more than 2^28 brick coordinates)";
        return REG_UNSUPPORTED;
    }
    const bool use_dir = true, use_rows = true;
    if (use_dir) {
        HIPCHK(h, h->t_dir.reserve(n_dir * 4));
        HIPCHK(h, hipMemsetAsync(h->t_dir.p, 0xff, n_dir * 4, h->stream));
        if (use_rows) {
            HIPCHK(h, h->t_rows.reserve(n_dir * 8));
            HIPCHK(h, hipMemsetAsync(h->t_rows.p, 0, n_dir * 8, h->stream));
        }
    }
    k_fill_tables<<<grid_for(m), 256, 0, h->stream>>>(h->t_keys2.as<uint64_t>(), h->t_flags.as<uint32_t>(),
                                                       h->t_scan.as<uint32_t>(), m, h->t_hash.as<HashEntry>(), cap - 1,
                                                       h->t_cells.as<uint32_t>(), h->t_misc.as<uint32_t>(),
                                                       use_dir ? h->t_dir.as<int32_t>() : nullptr, bdx, bdy,
                                                       use_rows ? h->t_rows.as<unsigned long long>() : nullptr);
    g.brick_dir = use_dir ? h->t_dir.as<int32_t>() : nullptr;
    g.brick_rows = use_rows ? h->t_rows.as<unsigned long long>() : nullptr;
    g.dyn_prune = h->env.no_dynprune ? 0 : 1;
    g.bdx = bdx;
    g.bdy = bdy;
    g.bdz = bdz;
    REGCHK(scan_excl(h, h->rp_tmp, h->t_cells.as<uint32_t>(), h->t_cells.as<uint32_t>(), n_cells));
    HIPCHK(h, hipMemcpyAsync(occupied, h->t_misc.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    g.hash_mask = cap - 1;
    g.hash = h->t_hash.as<HashEntry>();
    g.cell_start = h->t_cells.as<uint32_t>();
    h->info.n_bricks = nb;
    h->info.n_cells_occupied = *occupied;
    h->info.table_bytes = (int64_t)((size_t)cap * sizeof(HashEntry) + n_cells * 4 + (use_dir ? n_dir * 4 : 0) + (use_rows ? n_dir * 8 : 0));
    h->info.cell_size = c;
    return REG_OK;
}

static void set_levels(reg_handle* h, float c, float max_abs) {
    Grid& g = h->grid;
    const float md = h->prm.max_dist;
    g.max_d2 = std::isinf(md) ? INFINITY : md * md;
    h->shift0 = (g.max_d2 < 2.0f) ? 19 : 21;
    int n = 0;
    float rho = 0.5f * c;
    const float abs_margin = 4e-7f * (1.0f + max_abs);
    while (n < kMaxLevels - 1 && rho < md) {
        g.rho[n] = rho;
        g.rho_box[n] = rho + 1e-3f * rho + abs_margin;
        ++n;
        rho *= h->env.level_ratio;
        if (std::isinf(md) && rho > 32.f * c) break;  // unbounded search: beyond 32 bin edges fall through to a full scan
    }
    g.rho[n] = md;
    g.rho_box[n] = std::isinf(md) ? INFINITY : md + 1e-3f * md + abs_margin;
    ++n;
    g.n_levels = n;
}

// Level-0 accelerator: dense halo bins of edge c_h = 1.25 c (O3D_HALO_RATIO) with rho_h = 0.4 c_h (O3D_HALO_RHO; each point is
// listed in 1-2 bins per axis: ~4.5 copies).  Skipped when the dense grid would be too large or on request.
static reg_status build_halo(reg_handle* h, float c, const float bmin[3], const float bmax[3], float max_abs) {
    Grid& g = h->grid;
    g.use_halo = 0;
    g.level_after_halo = 0;
    if (h->dbg.disable_halo == 1) return REG_OK;  // A/B experiments
    const float ch = h->env.halo_ratio * c;
    const float abs_margin = 4e-7f * (1.0f + max_abs);
    const float rho_h = h->env.halo_rho * ch * (1.0f - 4e-3f) - 2.f * abs_margin;
    if (!(rho_h > 0.f)) return REG_OK;
    const float r_ins = rho_h + 1e-3f * rho_h + abs_margin;
    const float inv = 1.0f / ch;
    double dims[3];
    for (int k = 0; k < 3; ++k) dims[k] = std::floor((double)(bmax[k] - bmin[k]) * inv) + 1.0;
    const double nb = dims[0] * dims[1] * dims[2];
    if (nb > 512e6) return REG_OK;   // 2 GB of bin starts: nothing against 288 GB of HBM (a 20 M-point map needs ~30 M bins)
    const size_t nbins = (size_t)nb;
    HaloCfg hc;
    hc.ox = bmin[0];
    hc.oy = bmin[1];
    hc.oz = bmin[2];
    hc.inv_c = inv;
    hc.r_ins = r_ins;
    hc.dimx = (int)dims[0];
    hc.dimy = (int)dims[1];
    hc.dimz = (int)dims[2];
    // t_halo_start: counts, then bin starts, then -- once the directory is written -- the fill pass's cursors.
    // t_halo_dir: the directory {start, count | bound} the search reads; before that, scratch of the bound's passes
    // (bytes [0, 2 nbins): pass-x gaps, [4 nbins, 5 nbins): occupancy bytes).  t_halo_cursor: pass-y scratch (4 bytes per bin);
    // with witnesses, 9 bytes per bin: [4 nbins, 8 nbins) the arg-min offsets of pass y, [8 nbins, 9 nbins) those of pass x,
    // and -- once the directory is written -- [0, 4 nbins) the representatives of the runs.  Like the rest of the build's scratch
    // it stays with the handle for the next build (no allocation per set_target): 5 bytes per bin more than before.
    HIPCHK(h, h->t_halo_start.reserve((nbins + 1) * 4));
    HIPCHK(h, h->t_halo_dir.reserve(nbins * 8));
    HIPCHK(h, hipMemsetAsync(h->t_halo_start.p, 0, (nbins + 1) * 4, h->stream));
    // Empty-space bound: for the bins whose run is empty, a lower bound on the distance to any reference point,
    // carried in the directory record.  Only a finite max_dist has levels to skip and queries to reject.
    HaloBoundCfg bc;
    bc.dimx = hc.dimx;
    bc.dimy = hc.dimy;
    bc.dimz = hc.dimz;
    bc.R = 0;
    bc.ch = ch;
    bc.rho_h = rho_h;
    bc.eps_bins = (float)std::max(dims[0], std::max(dims[1], dims[2])) * (1.0f / 2097152.0f);
    bc.sub = 2.f * abs_margin;
    const bool bound = !h->env.no_empty_bound && std::isfinite(h->prm.max_dist) && h->prm.max_dist > 0.f;
    const bool witness = bound && !h->env.no_witness;   // (the arg-min rides on the bound's passes)
    uint8_t* const occ = (uint8_t*)h->t_halo_dir.p + 4 * nbins;
    if (bound) {
        bc.R = (int)std::min(64.0f, std::floor(h->prm.max_dist * inv) + 2.0f);   // (beyond 64 bins: a weaker, still valid bound)
        HIPCHK(h, h->t_halo_cursor.reserve(nbins * (witness ? 9 : 4)));
        HIPCHK(h, hipMemsetAsync(occ, 0, nbins, h->stream));
    }
    k_halo_insert<<<grid_for(h->m), 256, 0, h->stream>>>(h->t_pts.as<float4>(), h->m, hc, 0,
                                                         h->t_halo_start.as<uint32_t>(), nullptr, bound ? occ : nullptr);
    REGCHK(scan_excl(h, h->rp_tmp, h->t_halo_start.as<uint32_t>(), h->t_halo_start.as<uint32_t>(), nbins + 1));
    uint32_t total = 0;
    HIPCHK(h, hipMemcpyAsync(&total, h->t_halo_start.as<uint32_t>() + nbins, 4, hipMemcpyDeviceToHost, h->stream));
    uint8_t* const xo = witness ? (uint8_t*)h->t_halo_cursor.p + 8 * nbins : nullptr;
    uint32_t* const yo = witness ? h->t_halo_cursor.as<uint32_t>() + nbins : nullptr;
    if (bound) {
        k_halo_gap_x<<<grid_for((int64_t)nbins), 256, 0, h->stream>>>(occ, h->t_halo_start.as<uint32_t>(), bc, h->t_halo_dir.as<uchar2>(), xo);
        k_halo_gap_y<<<grid_for((int64_t)nbins), 256, 0, h->stream>>>(h->t_halo_dir.as<uchar2>(), bc, h->t_halo_cursor.as<ushort2>(), xo, yo);
    }
    k_halo_dir<<<grid_for((int64_t)nbins), 256, 0, h->stream>>>(h->t_halo_start.as<uint32_t>(),
                                                                 bound ? h->t_halo_cursor.as<ushort2>() : nullptr, bc,
                                                                 h->t_halo_dir.as<uint2>(), yo);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, h->t_halo_pts.reserve((size_t)std::max<uint32_t>(total, 1) * 16));
    k_halo_insert<<<grid_for(h->m), 256, 0, h->stream>>>(h->t_pts.as<float4>(), h->m, hc, 1,
                                                         h->t_halo_start.as<uint32_t>(), h->t_halo_pts.as<float4>(), nullptr);
    if (witness) {
        HaloRepCfg rc;
        rc.ox = hc.ox;
        rc.oy = hc.oy;
        rc.oz = hc.oz;
        rc.ch = ch;
        rc.dimx = hc.dimx;
        rc.dimy = hc.dimy;
        rc.dimz = hc.dimz;
        k_halo_rep<<<grid_for((int64_t)nbins), 256, 0, h->stream>>>(h->t_halo_dir.as<uint2>(), h->t_halo_pts.as<float4>(), rc,
                                                                     h->t_halo_cursor.as<uint32_t>());
        k_halo_witness<<<grid_for((int64_t)nbins), 256, 0, h->stream>>>(h->t_halo_dir.as<uint2>(), h->t_halo_cursor.as<uint32_t>(), nbins);
    }
    g.use_halo = 1;
    g.hox = hc.ox;
    g.hoy = hc.oy;
    g.hoz = hc.oz;
    g.hinv_c = inv;
    g.hdimx = hc.dimx;
    g.hdimy = hc.dimy;
    g.hdimz = hc.dimz;
    g.halo_dir = h->t_halo_dir.as<uint2>();
    g.hmaxx = bmax[0];
    g.hmaxy = bmax[1];
    g.hmaxz = bmax[2];
    g.lb_sub = 2.f * abs_margin;
    g.out_bound = (bound ? 1 : 0) | (witness ? 2 : 0);
    g.halo_pts = h->t_halo_pts.as<float4>();
    g.rho_h = rho_h;
    g.level_after_halo = g.n_levels - 1;
    for (int l = 0; l < g.n_levels; ++l)
        if (g.rho[l] > rho_h) {
            g.level_after_halo = l;
            break;
        }
    h->info.table_bytes += (int64_t)(nbins * 8 + (size_t)total * 16);
    return REG_OK;
}

extern "C" {

static reg_status set_target_impl(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm, int64_t nrm_stride,
                                  const float* cov, int64_t m, int on_device);

reg_status reg_set_target(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm, int64_t nrm_stride,
                          const float* cov, int64_t m, int on_device) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    // The reference re-derives everything in compute() after initReference(): a reading prepared against the previous
    // reference (centred on the old c_ref, pre-transformed with the old T0) must not be used with the new one.
    h->prepared = false;
    const reg_status s = set_target_impl(h, xyz, xyz_stride, nrm, nrm_stride, cov, m, on_device);
    if (s != REG_OK) h->m = 0;   // a failed build leaves NO reference (tables, origin and dims may be half-updated)
    return s;
}

static reg_status set_target_impl(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm, int64_t nrm_stride,
                                  const float* cov, int64_t m, int on_device) {
    h->m = 0;
    h->crop_kept = 0;
    h->have_match = false;
    h->pm_have_match = false;
    if (m <= 0) {
        h->err = "The reference point cloud is empty";
        return REG_EMPTY_TARGET;
    }
    if (!xyz || xyz_stride < 3 || (nrm && nrm_stride < 3) || m > 0x7fffffffLL) return REG_BAD_ARGUMENT;
    if (const reg_status fs = check_target_fields(h, nrm != nullptr, cov != nullptr)) return fs;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    const float* d_xyz = xyz;
    const float* d_nrm = nrm;
    const float* d_cov = cov;
    if (!on_device) {
        reg_status s = upload(h, h->t_raw, xyz, (size_t)m * xyz_stride * 4, 0);
        if (s != REG_OK) return s;
        d_xyz = h->t_raw.as<float>();
        if (nrm) {
            s = upload(h, h->t_nrm_raw, nrm, (size_t)m * nrm_stride * 4, 0);
            if (s != REG_OK) return s;
            d_nrm = h->t_nrm_raw.as<float>();
        }
        if (cov) {
            s = upload(h, h->t_cov_raw, cov, (size_t)m * 6 * 4, 0);
            if (s != REG_OK) return s;
            d_cov = h->t_cov_raw.as<float>();
        }
    }
    h->m = m;
    h->has_tnrm = nrm != nullptr;
    h->has_tcov = cov != nullptr;
    // R1: centroid (P2PL path only: GICP works in the input frame, as small_gicp does)
    float c[3] = {0, 0, 0};
    if (h->prm.cost == REG_COST_P2PL) {
        reg_status s = device_centroid(h, d_xyz, xyz_stride, m, h->t_misc, c);
        if (s != REG_OK) return s;
    }
    std::memcpy(h->c_ref, c, sizeof(c));
    std::memcpy(h->info.centroid, c, sizeof(c));
    // centred copy + bbox
    HIPCHK(h, h->t_centred.reserve((size_t)m * 16));
    HIPCHK(h, h->t_misc.reserve(256));
    int bb_init[6] = {0x7f800000, 0x7f800000, 0x7f800000, (int)0x80000000 ^ 0, 0, 0};
    // ordered-int encodings of +inf / -inf
    bb_init[0] = bb_init[1] = bb_init[2] = 0x7f800000;                    // +inf
    bb_init[3] = bb_init[4] = bb_init[5] = (int)(0xff800000u ^ 0x7fffffffu);  // -inf
    HIPCHK(h, hipMemcpyAsync(h->t_misc.p, bb_init, sizeof(bb_init), hipMemcpyHostToDevice, h->stream));
    const int blocks = (int)std::min<int64_t>(512, (m + 255) / 256);
    k_center_bbox<<<blocks, 256, 0, h->stream>>>(d_xyz, xyz_stride, m, c[0], c[1], c[2], h->t_centred.as<float4>(),
                                                 h->t_misc.as<int>());
    int bb[6];
    HIPCHK(h, hipMemcpyAsync(bb, h->t_misc.p, sizeof(bb), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float bmin[3], bmax[3], max_abs = 0.f;
    for (int k = 0; k < 3; ++k) {
        bmin[k] = ord2f(bb[k]);
        bmax[k] = ord2f(bb[3 + k]);
        if (!std::isfinite(bmin[k]) || !std::isfinite(bmax[k])) {
            h->err = "reference cloud contains non-finite coordinates";
            h->m = 0;
            return REG_BAD_ARGUMENT;
        }
        max_abs = std::max(max_abs, std::max(std::fabs(bmin[k]), std::fabs(bmax[k])));
        h->t_mid[k] = 0.5f * (bmin[k] + bmax[k]);
    }
    // bin edge: user value, or adapt to ~8 points per occupied bin (surface-like clouds: count ~ c^2)
    float cs = h->prm.cell_size;
    uint32_t occupied = 0;
    float cs_occ = 0.f;   // automatic edge before the reach floor (0: explicit cell_size)
    if (cs > 0.f) {
        reg_status s = build_grid(h, cs, bmin, bmax, &occupied);
        if (s != REG_OK) return s;
    } else {
        const float ext = std::max(bmax[0] - bmin[0], std::max(bmax[1] - bmin[1], bmax[2] - bmin[2]));
        // start from the edge that would give `occ` points per bin if the cloud were a single ext x ext sheet, then correct
        // with the measured occupancy (points per occupied bin grow with the square of the edge on surface-like clouds)
        const float occ = h->env.bin_occupancy;
        const float cs_abs = std::max(ext / (float)(1u << 20), 1e-6f);
        cs = std::max(std::max(ext * std::sqrt(occ / (float)m), 1e-4f * std::max(ext, 1e-3f)), cs_abs);
        auto build = [&](float& edge) {
            reg_status s = build_grid(h, edge, bmin, bmax, &occupied);
            for (int grow = 0; s == REG_UNSUPPORTED && grow < 8; ++grow) {   // extent / edge^3 beyond the dense directory
                edge *= 1.3f;
                s = build_grid(h, edge, bmin, bmax, &occupied);
            }
            return s;
        };
        for (int pass = 0; pass < 3; ++pass) {
            const reg_status s = build(cs);
            if (s != REG_OK) return s;
            const float per = (float)m / (float)std::max(1u, occupied);
            if ((per <= 1.15f * occ && per >= 0.85f * occ) || pass == 2) break;
            const float next = std::max(cs * std::sqrt(occ / per), cs_abs);
            if (std::fabs(next - cs) < 0.05f * cs) break;
            cs = next;
        }
        // A bin box of the largest radius should not span more than ~15 bins per axis: the early iterations of a registration
        // search with radii up to max_dist, and their cost grows with the number of rows in the box (measured at 20 M points:
        // 0.050 m bins 3.48 ms per registration, 0.069 m bins 3.27 ms).
        const float cs_reach = (std::isfinite(h->prm.max_dist) && !h->structure_only) ? h->prm.max_dist / h->env.reach_bins : 0.f;
        cs_occ = cs;
        if (cs < cs_reach) {
            cs = cs_reach;
            const reg_status s = build(cs);
            if (s != REG_OK) return s;
        }
    }
    // sorted arrays
    HIPCHK(h, h->t_pts.reserve((size_t)m * 16));
    if (d_nrm) HIPCHK(h, h->t_nrm.reserve((size_t)m * 32));   // {point, normal} pairs in sorted order
    if (d_cov) HIPCHK(h, h->t_cov.reserve((size_t)m * 32));
    k_gather_target<<<grid_for(m), 256, 0, h->stream>>>(h->t_centred.as<float4>(), h->t_vals2.as<uint32_t>(), m, d_nrm,
                                                         nrm_stride, d_cov, h->t_pts.as<float4>(),
                                                         d_nrm ? h->t_nrm.as<float4>() : nullptr,
                                                         d_cov ? h->t_cov.as<float4>() : nullptr);
    h->grid.pts = h->t_pts.as<float4>();
    set_levels(h, cs, max_abs);
    {
        // The halo bins serve the settled searches (neighbours a few centimetres away): their edge follows the DENSITY of the
        // map, not the reach floor of the level grid (20 M points: runs of ~170 points with 0.10 m halo bins, ~90 with 0.075 m)
        const float c_halo = (h->env.halo_occ && cs_occ > 0.f) ? std::min(cs, cs_occ) : cs;
        reg_status hs = build_halo(h, c_halo, bmin, bmax, max_abs);
        if (hs != REG_OK) return hs;
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    (void)hipEventElapsedTime(&h->target_build_ms, h->ev0, h->ev1);
    h->info.n_points = m;
    h->info.origin[0] = bmin[0];
    h->info.origin[1] = bmin[1];
    h->info.origin[2] = bmin[2];
    return REG_OK;
}

reg_status reg_set_target_f64(reg_handle* h, const double* xyz, const double* normals, const double* covs, int64_t m,
                              int on_device, const reg_crop* crop, int64_t* n_kept) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_kept) *n_kept = 0;
    h->crop_kept = 0;
    h->m = 0;            // whatever happens below, the previous reference is gone (its staging buffers are reused)
    h->prepared = false;
    if (m <= 0) {
        h->err = "The reference point cloud is empty";
        return REG_EMPTY_TARGET;
    }
    if (!xyz || m > 0x7fffffffLL) return REG_BAD_ARGUMENT;
    CropCfg c;
    if (!crop_cfg(crop, &c)) return REG_BAD_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double *d_xyz = nullptr, *d_nrm = nullptr, *d_cov = nullptr;
    HIPCHK(h, staged_input(h, h->c_in_xyz, xyz, (size_t)m * 3, on_device, &d_xyz));
    HIPCHK(h, staged_input(h, h->c_in_nrm, normals, (size_t)m * 3, on_device, &d_nrm));
    HIPCHK(h, staged_input(h, h->c_in_cov, covs, (size_t)m * 9, on_device, &d_cov));
    HIPCHK(h, h->c_flags.reserve((size_t)m * 4));
    HIPCHK(h, h->c_offs.reserve((size_t)m * 4));
    uint32_t *flags = h->c_flags.as<uint32_t>(), *offs = h->c_offs.as<uint32_t>();
    k_crop_flags<<<grid_for(m), 256, 0, h->stream>>>(d_xyz, m, c, flags);
    int64_t kept = 0;
    REGCHK(scan_total(h, flags, offs, m, &kept));
    if (n_kept) *n_kept = kept;
    if (kept == 0) {
        h->m = 0;
        h->err = "The reference point cloud is empty (no point inside the cropping volume)";   // ScanToMapRegistration.cpp:94
        return REG_EMPTY_TARGET;
    }
    HIPCHK(h, h->c_xyz.reserve((size_t)kept * 12));
    if (d_nrm) HIPCHK(h, h->c_nrm.reserve((size_t)kept * 12));
    if (d_cov) HIPCHK(h, h->c_cov.reserve((size_t)kept * 24));
    HIPCHK(h, h->c_idx.reserve((size_t)kept * 4));
    k_crop_gather<<<grid_for(m), 256, 0, h->stream>>>(d_xyz, d_nrm, d_cov, m, flags, offs, h->c_xyz.as<float>(),
                                                      d_nrm ? h->c_nrm.as<float>() : nullptr,
                                                      d_cov ? h->c_cov.as<float>() : nullptr, h->c_idx.as<int32_t>());
    const reg_status s = reg_set_target(h, h->c_xyz.as<float>(), 3, d_nrm ? h->c_nrm.as<float>() : nullptr, 3,
                                        d_cov ? h->c_cov.as<float>() : nullptr, kept, 1);
    if (s == REG_OK) h->crop_kept = kept;
    return s;
}

reg_status reg_get_target_source_indices(reg_handle* h, int32_t* idx) {
    if (!h || !idx) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (h->crop_kept <= 0 || h->crop_kept != h->m) {
        h->err = "the current reference was not set through reg_set_target_f64";
        return REG_NOT_CONFIGURED;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, hipMemcpyAsync(idx, h->c_idx.p, (size_t)h->crop_kept * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

// The reference's t_* buffers as the arrays of sort_runs: the table build shares them, so they stay loose fields and are
// reserved where they are used.
static RunArrays target_run_arrays(reg_handle* h) {
    return RunArrays{h->t_keys.as<uint64_t>(), h->t_keys2.as<uint64_t>(), h->t_vals.as<uint32_t>(),
                     h->t_vals2.as<uint32_t>(), h->t_flags.as<uint32_t>(), h->t_scan.as<uint32_t>()};
}

reg_status reg_voxelize_within_volume(reg_handle* h, const double* xyz, const double* normals, const double* covs, int64_t m,
                                      int on_device, const reg_crop* volume, double voxel_size, double* out_xyz,
                                      double* out_normals, double* out_covs, int64_t* n_out, int64_t* n_outside) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_out) *n_out = 0;
    if (n_outside) *n_outside = 0;
    if (m < 0 || m > 0x7fffffffLL || (m > 0 && (!xyz || !out_xyz)) || (normals && !out_normals) || (covs && !out_covs))
        return REG_BAD_ARGUMENT;
    if (m == 0) return REG_OK;
    CropCfg c;
    if (!crop_cfg(volume, &c)) return REG_BAD_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->prm.device));
    if (!(voxel_size > 0.0)) {   // helpers.cpp:121-124: nothing to do
        HIPCHK(h, hipMemcpyAsync(out_xyz, xyz, (size_t)m * 24, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost, h->stream));
        if (normals) HIPCHK(h, hipMemcpyAsync(out_normals, normals, (size_t)m * 24, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost, h->stream));
        if (covs) HIPCHK(h, hipMemcpyAsync(out_covs, covs, (size_t)m * 72, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (n_out) *n_out = m;
        if (n_outside) *n_outside = m;
        return REG_OK;
    }
    const double *d_xyz = nullptr, *d_nrm = nullptr, *d_cov = nullptr;
    HIPCHK(h, staged_input(h, h->c_in_xyz, xyz, (size_t)m * 3, on_device, &d_xyz));
    HIPCHK(h, staged_input(h, h->c_in_nrm, normals, (size_t)m * 3, on_device, &d_nrm));
    HIPCHK(h, staged_input(h, h->c_in_cov, covs, (size_t)m * 9, on_device, &d_cov));
    StagedOut so(h, h->v_out, on_device);
    const int s_xyz = so.add(out_xyz, 3), s_nrm = so.add(normals ? out_normals : nullptr, 3),
              s_cov = so.add(covs ? out_covs : nullptr, 9);
    HIPCHK(h, so.reserve((size_t)m));
    double *d_oxyz = so.at<double>(s_xyz), *d_onrm = so.at<double>(s_nrm), *d_ocov = so.at<double>(s_cov);
    const double inv = 1.0 / voxel_size;   // fromVoxelSize (VoxelHashMap.hpp:43-45)
    HIPCHK(h, h->c_flags.reserve((size_t)m * 4));
    HIPCHK(h, h->c_offs.reserve((size_t)m * 4));
    HIPCHK(h, h->v_fout.reserve((size_t)m * 4));
    HIPCHK(h, h->v_oout.reserve((size_t)m * 4));
    HIPCHK(h, h->t_misc.reserve(256));
    HIPCHK(h, hipMemsetAsync(h->t_misc.p, 0, 4, h->stream));
    uint32_t *f_in = h->c_flags.as<uint32_t>(), *o_in = h->c_offs.as<uint32_t>();     // inside the volume: flags, offsets
    uint32_t *f_out = h->v_fout.as<uint32_t>(), *o_out = h->v_oout.as<uint32_t>();    // outside
    k_vox_classify<<<grid_for(m), 256, 0, h->stream>>>(d_xyz, m, c, inv, f_in, f_out, h->t_misc.as<uint32_t>());
    REGCHK(scan_excl(h, h->rp_tmp, f_in, o_in, (size_t)m));
    REGCHK(scan_excl(h, h->rp_tmp, f_out, o_out, (size_t)m));
    uint32_t tail[2], bad = 0;
    REGCHK(flag_total_async(h, f_in, o_in, m, tail));
    HIPCHK(h, hipMemcpyAsync(&bad, h->t_misc.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad) {
        h->err = "voxel_size too small for the extent of the cloud (voxel index exceeds 2^20)";
        return REG_BAD_ARGUMENT;
    }
    const int64_t n_in = flag_total(tail), n_outs = m - n_in;
    int64_t n_vox = 0;
    HIPCHK(h, h->t_keys.reserve((size_t)std::max<int64_t>(n_in, 1) * 8));
    HIPCHK(h, h->t_keys2.reserve((size_t)std::max<int64_t>(n_in, 1) * 8));
    HIPCHK(h, h->t_vals.reserve((size_t)std::max<int64_t>(n_in, 1) * 4));
    HIPCHK(h, h->t_vals2.reserve((size_t)std::max<int64_t>(n_in, 1) * 4));
    k_vox_scatter<<<grid_for(m), 256, 0, h->stream>>>(d_xyz, d_nrm, d_cov, m, inv, f_in, o_in, o_out, h->t_keys.as<uint64_t>(),
                                                      h->t_vals.as<uint32_t>(), d_oxyz, d_onrm, d_ocov);
    if (n_in > 0) {
        HIPCHK(h, h->t_flags.reserve((size_t)n_in * 4));
        HIPCHK(h, h->t_scan.reserve((size_t)n_in * 4));
        const RunArrays a = target_run_arrays(h);
        uint32_t lv[2];
        REGCHK(sort_runs(h, a, n_in, lv));
        k_vox_reduce<true><<<grid_for(n_in), 256, 0, h->stream>>>(a.sorted, a.svals, n_in, a.heads, a.run, d_xyz, d_nrm, d_cov, n_outs,
                                                                  d_oxyz, d_onrm, d_ocov);
        HIPCHK(h, hipStreamSynchronize(h->stream));
        n_vox = flag_total(lv);
    }
    const int64_t total = n_outs + n_vox;
    HIPCHK(h, so.copy_back((size_t)total));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_out) *n_out = total;
    if (n_outside) *n_outside = n_outs;
    return REG_OK;
}

// Steps 1-4 of reg_carve_indices on device arrays (m > 0, n_scan > 0): on return h->v_fout holds the 0 / 1 marks over the
// map rows and h->v_oout their exclusive scan, *n_marked their total.  *n_candidates: map rows inside the volume; with
// none, nothing further runs and the marks are not written.
static reg_status carve_marks(reg_handle* h, const double* d_map, const double* d_nrm, int64_t m, const double* d_scan,
                              int64_t n_scan, const double sensor[3], const CropCfg& c, double voxel_size, double max_ray,
                              double truncation, double min_dot, int64_t* n_candidates, int64_t* n_marked) {
    *n_candidates = *n_marked = 0;
    const double inv = 1.0 / voxel_size;
    // 1. candidate map points (inside the subset volume), keyed by voxel, stably sorted
    HIPCHK(h, h->c_flags.reserve((size_t)m * 4));
    HIPCHK(h, h->c_offs.reserve((size_t)m * 4));
    HIPCHK(h, h->v_fout.reserve((size_t)m * 4));
    HIPCHK(h, h->v_oout.reserve((size_t)m * 4));
    HIPCHK(h, h->t_misc.reserve(256));
    HIPCHK(h, hipMemsetAsync(h->t_misc.p, 0, 4, h->stream));
    uint32_t *f_in = h->c_flags.as<uint32_t>(), *o_in = h->c_offs.as<uint32_t>();    // inside the subset volume: flags, offsets
    uint32_t *mark = h->v_fout.as<uint32_t>(), *o_mark = h->v_oout.as<uint32_t>();   // step 3's marks over the map
    k_vox_classify<<<grid_for(m), 256, 0, h->stream>>>(d_map, m, c, inv, f_in, mark, h->t_misc.as<uint32_t>());
    REGCHK(scan_excl(h, h->rp_tmp, f_in, o_in, (size_t)m));
    uint32_t tail[2], bad = 0;
    REGCHK(flag_total_async(h, f_in, o_in, m, tail));
    HIPCHK(h, hipMemcpyAsync(&bad, h->t_misc.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad) {
        h->err = "voxel_size too small for the extent of the map (voxel index exceeds 2^20)";
        return REG_BAD_ARGUMENT;
    }
    const int64_t n_in = *n_candidates = flag_total(tail);
    if (n_in == 0) return REG_OK;
    HIPCHK(h, h->t_keys.reserve((size_t)n_in * 8));
    HIPCHK(h, h->t_keys2.reserve((size_t)n_in * 8));
    HIPCHK(h, h->t_vals.reserve((size_t)n_in * 4));
    HIPCHK(h, h->t_vals2.reserve((size_t)n_in * 4));
    k_carve_keys<<<grid_for(m), 256, 0, h->stream>>>(d_map, m, inv, f_in, o_in, h->t_keys.as<uint64_t>(), h->t_vals.as<uint32_t>());
    // 2. unique voxels
    HIPCHK(h, h->t_flags.reserve((size_t)n_in * 4));
    HIPCHK(h, h->t_scan.reserve((size_t)n_in * 4));
    const RunArrays a = target_run_arrays(h);
    uint32_t lv[2];
    REGCHK(sort_runs(h, a, n_in, lv));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int64_t nu = flag_total(lv);
    HIPCHK(h, h->v_ukeys.reserve((size_t)nu * 8));
    HIPCHK(h, h->v_ustart.reserve((size_t)(nu + 1) * 4));
    k_carve_unique<<<grid_for(n_in), 256, 0, h->stream>>>(a.sorted, n_in, a.heads, a.run, h->v_ukeys.as<uint64_t>(),
                                                          h->v_ustart.as<uint32_t>());
    const uint32_t n_in32 = (uint32_t)n_in;
    HIPCHK(h, hipMemcpyAsync(h->v_ustart.as<uint32_t>() + nu, &n_in32, 4, hipMemcpyHostToDevice, h->stream));
    // 3. rays -> marks
    HIPCHK(h, hipMemsetAsync(mark, 0, (size_t)m * 4, h->stream));
    k_carve_rays<<<grid_for(n_scan), 256, 0, h->stream>>>(d_scan, n_scan, sensor[0], sensor[1], sensor[2], voxel_size, max_ray,
                                                          truncation, min_dot, inv, h->v_ukeys.as<uint64_t>(),
                                                          h->v_ustart.as<uint32_t>(), nu, a.svals, d_nrm, mark);
    // 4. ascending list of marked map indices
    return scan_total(h, mark, o_mark, m, n_marked);
}

reg_status reg_carve_indices(reg_handle* h, const double* map_xyz, const double* map_normals, int64_t m,
                             const double* scan_xyz, int64_t n_scan, int on_device, const double sensor[3],
                             const reg_crop* subset, double voxel_size, double max_ray, double truncation, double min_dot,
                             int32_t* removed, int64_t* n_removed) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (n_removed) *n_removed = 0;
    if (m < 0 || n_scan < 0 || m > 0x7fffffffLL || n_scan > 0x7fffffffLL || !sensor || !(voxel_size > 0.0) ||
        (m > 0 && (!map_xyz || !removed)) || (n_scan > 0 && !scan_xyz)) {
        if (h) h->err = "reg_carve_indices: bad argument (voxel_size > 0, sensor, arrays)";
        return REG_BAD_ARGUMENT;
    }
    if (m == 0 || n_scan == 0) return REG_OK;
    CropCfg c;
    if (!crop_cfg(subset, &c)) return REG_BAD_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double *d_map = nullptr, *d_nrm = nullptr, *d_scan = nullptr;
    HIPCHK(h, staged_input(h, h->c_in_xyz, map_xyz, (size_t)m * 3, on_device, &d_map));
    HIPCHK(h, staged_input(h, h->c_in_nrm, map_normals, (size_t)m * 3, on_device, &d_nrm));
    HIPCHK(h, staged_input(h, h->c_in_cov, scan_xyz, (size_t)n_scan * 3, on_device, &d_scan));   // (the third staging buffer)
    int64_t n_in = 0, nr = 0;
    REGCHK(carve_marks(h, d_map, d_nrm, m, d_scan, n_scan, sensor, c, voxel_size, max_ray, truncation, min_dot, &n_in, &nr));
    if (n_in == 0) return REG_OK;
    const uint32_t *mark = h->v_fout.as<uint32_t>(), *o_mark = h->v_oout.as<uint32_t>();
    StagedOut so(h, h->c_idx, on_device);
    const int s_rem = so.add(removed, 1);
    HIPCHK(h, so.reserve((size_t)nr));
    if (!on_device) h->crop_kept = 0;   // c_idx no longer holds the crop map of reg_set_target_f64
    if (nr > 0) k_carve_collect<<<grid_for(m), 256, 0, h->stream>>>(mark, o_mark, m, so.at<int32_t>(s_rem));
    HIPCHK(h, so.copy_back((size_t)nr));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_removed) *n_removed = nr;
    return REG_OK;
}

reg_status reg_smooth_normals(reg_handle* h, float* normals, const int32_t* ids, int64_t n, int k, int on_device,
                              int32_t* n_passes) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!normals || !ids || k < 1 || k > kPcaMaxK || n > 0x7fffffffLL) {
        h->err = "reg_smooth_normals: bad argument (normals, ids != NULL, 1 <= k <= 32)";
        return REG_BAD_ARGUMENT;
    }
    if (n <= 0) {
        h->err = "The point cloud is empty";
        return REG_EMPTY_SOURCE;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    float* d_n = normals;
    const int32_t* d_i = ids;
    if (!on_device) {
        HIPCHK(h, h->n_out.reserve((size_t)n * 12));
        HIPCHK(h, h->n_ids.reserve((size_t)n * k * 4));
        HIPCHK(h, hipMemcpyAsync(h->n_out.p, normals, (size_t)n * 12, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->n_ids.p, ids, (size_t)n * k * 4, hipMemcpyHostToDevice, h->stream));
        d_n = h->n_out.as<float>();
        d_i = h->n_ids.as<int32_t>();
    }
    // work arrays: the original normals, the pass in which a point was finished (-1: not yet), the finished count
    HIPCHK(h, h->n_extra.reserve((size_t)n * 12 + (size_t)n * 4 + 64));
    float* orig = h->n_extra.as<float>();
    int* level = reinterpret_cast<int*>(orig + (size_t)n * 3);
    unsigned int* n_done = reinterpret_cast<unsigned int*>(level + n);
    HIPCHK(h, hipMemcpyAsync(orig, d_n, (size_t)n * 12, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(level, 0xff, (size_t)n * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(n_done, 0, 8, h->stream));   // [0] finished points, [1] an id >= n was seen
    int pass = 0;
    unsigned int done = 0, done2[2] = {0, 0};
    const int batch = 32;   // passes between two looks at the count (finished sweeps are cheap no-ops)
    while (done < (unsigned int)n) {
        if ((int64_t)pass > n) {
            h->err = "reg_smooth_normals: the sweep did not terminate (neighbour ids out of range?)";
            return REG_BAD_ARGUMENT;
        }
        for (int b = 0; b < batch; ++b, ++pass)
            k_smooth_pass<<<grid_for(n), 256, 0, h->stream>>>(orig, d_n, d_i, n, k, pass, level, n_done);
        HIPCHK(h, hipMemcpyAsync(done2, n_done, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        done = done2[0];
        if (done2[1]) {
            h->err = "reg_smooth_normals: a neighbour id is >= n";
            return REG_BAD_ARGUMENT;
        }
    }
    if (n_passes) *n_passes = pass;
    if (!on_device) {
        HIPCHK(h, hipMemcpyAsync(normals, d_n, (size_t)n * 12, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    HIPCHK(h, hipGetLastError());
    return REG_OK;
}

// The workspace handle of the neighbourhood entry points (reg_estimate_normals, reg_compute_fpfh): a bin table over the
// caller's cloud in its own frame, no attributes; created on first use, on the caller's stream, destroyed with it.
static reg_status normals_workspace(reg_handle* h, const char* who) {
    if (!h->normals_ws) {
        reg_params p = h->prm;
        p.cost = REG_COST_GICP;   // no centring: neighbourhoods are formed in the input frame
        p.use_xicp = 0;
        reg_handle* w = nullptr;
        const reg_status cs = reg_create(&p, &w);
        if (w) w->dbg.disable_halo = 1;   // the k-NN search uses the brick table only
        if (cs != REG_OK) {
            h->err = std::string(who) + ": workspace: " + reg_last_error(w);
            reg_destroy(w);
            return cs;
        }
        w->structure_only = true;
        h->normals_ws = w;
    }
    (void)reg_set_stream(h->normals_ws, h->stream);
    return REG_OK;
}

// First radius level of the workspace's table expected to hold k neighbours on a surface-like cloud of n points (exactness
// does not depend on it)
static int knn_start_level(const reg_handle* w, int64_t n, int k) {
    const float per = (float)n / (float)std::max<int64_t>(1, w->info.n_cells_occupied);
    const float need = w->info.cell_size * std::sqrt(1.3f * (float)k / (3.14159265f * std::max(per, 1e-3f)));
    int start = 0;
    while (start < w->grid.n_levels - 1 && w->grid.rho[start] < need) ++start;
    return start;
}

reg_status reg_estimate_normals(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n, int on_device, int k,
                                float max_dist, const float* viewpoint, int regularise, const reg_normals_out* out,
                                int64_t* n_rescanned) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!out) return REG_BAD_ARGUMENT;
    float *normals = out->normals, *eigvals = out->eigvals, *covs = out->covs;
    int32_t* ids = out->ids;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!xyz || xyz_stride < 3 || !normals || k < 1 || k > kPcaMaxK || !(max_dist > 0.f) || n > 0x7fffffffLL) {
        h->err = "reg_estimate_normals: bad argument (1 <= k <= 32, max_dist > 0, normals != NULL)";
        return REG_BAD_ARGUMENT;
    }
    if (n <= 0) {
        h->err = "The point cloud is empty";
        return REG_EMPTY_SOURCE;
    }
    REGCHK(normals_workspace(h, "reg_estimate_normals"));
    reg_handle* w = h->normals_ws;
    w->prm.max_dist = max_dist;
    reg_status st = reg_set_target(w, xyz, xyz_stride, nullptr, 3, nullptr, n, on_device);
    if (st != REG_OK) {
        h->err = w->err;
        return st;
    }
    const int start = knn_start_level(w, n, k);
    const float* d_raw = on_device ? xyz : w->t_raw.as<float>();
    HIPCHK(h, hipSetDevice(h->prm.device));
    StagedOut so(h, h->n_out, on_device);
    const int s_n = so.add(normals, 3), s_e = so.add(eigvals, 3), s_c = so.add(covs, 6), s_i = so.add(ids, (size_t)k),
              s_v = so.add(out->eigvecs, 9), s_d = so.add(out->densities, 1), s_m = so.add(out->mean_dists, 1);
    HIPCHK(h, so.reserve((size_t)n));
    int32_t* d_i = so.at<int32_t>(s_i);
    HIPCHK(h, w->t_misc.reserve(256));
    HIPCHK(h, hipMemsetAsync(w->t_misc.p, 0, 4, h->stream));
    const float vp[3] = {viewpoint ? viewpoint[0] : 0.f, viewpoint ? viewpoint[1] : 0.f, viewpoint ? viewpoint[2] : 0.f};
    const int64_t blocks = (n + (256 / kPcaGroup) - 1) / (256 / kPcaGroup);
    HIPCHK(h, h->n_mom.reserve((size_t)n * sizeof(PcaMoments)));
    if (k <= 12)
        k_knn_pca<128><<<(unsigned)blocks, 256, 0, h->stream>>>(w->grid, d_raw, xyz_stride, n, k, start, d_i,
                                                                w->t_misc.as<uint32_t>(), h->n_mom.as<PcaMoments>());
    else
        k_knn_pca<256><<<(unsigned)blocks, 256, 0, h->stream>>>(w->grid, d_raw, xyz_stride, n, k, start, d_i,
                                                                w->t_misc.as<uint32_t>(), h->n_mom.as<PcaMoments>());
    k_pca_finish<<<grid_for(n), 256, 0, h->stream>>>(h->n_mom.as<PcaMoments>(), n, vp[0], vp[1], vp[2], viewpoint ? 1 : 0,
                                                     regularise, so.at<float>(s_n), so.at<float>(s_e), so.at<float>(s_c),
                                                     so.at<float>(s_v), so.at<float>(s_d), so.at<float>(s_m));
    uint32_t resc = 0;
    HIPCHK(h, hipMemcpyAsync(&resc, w->t_misc.p, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, so.copy_back((size_t)n));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (n_rescanned) *n_rescanned = resc;
    return REG_OK;
}

reg_status reg_get_target_info(const reg_handle* h, reg_target_info* info) {
    if (!h || !info) return REG_BAD_ARGUMENT;
    if (h->m == 0) return REG_NOT_CONFIGURED;
    *info = h->info;
    return REG_OK;
}

reg_status reg_set_source(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm, int64_t nrm_stride,
                          const float* cov, int64_t n, int on_device) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    h->n = 0;
    h->src_kept = 0;
    h->prepared = false;
    h->have_match = false;
    h->pm_have_match = false;
    if (n <= 0) {
        h->err = "The reading point cloud is empty.";
        return REG_EMPTY_SOURCE;
    }
    if (!xyz || xyz_stride < 3 || (nrm && nrm_stride < 3) || n > 0x7fffffffLL) return REG_BAD_ARGUMENT;
    if (const reg_status fs = check_source_fields(h, nrm != nullptr, cov != nullptr)) return fs;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, hipEventRecord(h->ev_s0, h->stream));
    // packed private copies (the reference deep-copies the reading, ICP.cpp:952)
    reg_status s = upload(h, h->s_raw, xyz, (size_t)n * xyz_stride * 4, on_device);
    if (s != REG_OK) return s;
    if (nrm) {
        s = upload(h, h->s_nrm_raw, nrm, (size_t)n * nrm_stride * 4, on_device);
        if (s != REG_OK) return s;
    }
    if (cov) {
        s = upload(h, h->s_cov_raw, cov, (size_t)n * 24, on_device);
        if (s != REG_OK) return s;
    }
    h->n = n;
    h->n_total_hint = 0;
    ++h->src_epoch;
    h->has_snrm = nrm != nullptr;
    h->has_scov = cov != nullptr;
    // iteration buffers
    HIPCHK(h, h->s_xyz.reserve((size_t)n * 16));
    if (nrm) HIPCHK(h, h->s_nrm.reserve((size_t)n * 16));
    if (cov) HIPCHK(h, h->s_cov.reserve((size_t)n * 32));
    HIPCHK(h, h->i_pos.reserve((size_t)n * 4));
    HIPCHK(h, h->i_d2.reserve((size_t)n * 4));
    HIPCHK(h, h->i_w.reserve((size_t)n * 4));
    HIPCHK(h, h->i_hist.reserve(3 * 2048 * 4));
    HIPCHK(h, h->i_state.reserve(sizeof(SelectState)));
    h->n_blocks = grid_for(n);
    HIPCHK(h, h->i_partials.reserve((size_t)(grid_for(n * 8) + 8) * kSums * 8));
    HIPCHK(h, h->i_band.reserve((size_t)kBandCap * kRec * 4));
    HIPCHK(h, h->i_acc.reserve((size_t)kAccRows * kSums * 8));
    HIPCHK(h, h->i_sums.reserve(kSums * 8));
    HIPCHK(h, h->i_hint.reserve((size_t)n));
    HIPCHK(h, h->i_cache.reserve((size_t)n * 64));   // per reading point: anchor + bound | matched point | its normal | runner-up
    HIPCHK(h, h->i_queue.reserve(((size_t)((n + 255) / 256 + 63) / 64) * 256 * 64 * 4));   // kQueues sub-queues (coherent_queue_cap)
    if (!h->i_qcount.p) {
        HIPCHK(h, h->i_qcount.reserve(64 * 16 * 4));
        HIPCHK(h, hipMemsetAsync(h->i_qcount.p, 0, 64 * 16 * 4, h->stream));
    }
    if (!h->i_stats.p) {
        HIPCHK(h, h->i_stats.reserve(256));
        HIPCHK(h, hipMemsetAsync(h->i_stats.p, 0, 256, h->stream));
    }
    h->s_stride = xyz_stride;
    h->s_nstride = nrm_stride;
    h->perm = nullptr;
    if (h->prm.sort_source) {
        // spatial (Morton) order of the reading, in its own frame: once per reading, not once per registration
        HIPCHK(h, h->s_keys.reserve((size_t)n * 4));
        HIPCHK(h, h->s_keys2.reserve((size_t)n * 4));
        HIPCHK(h, h->s_perm.reserve((size_t)n * 4));
        HIPCHK(h, h->s_perm2.reserve((size_t)n * 4));
        const float cell = h->m > 0 ? h->info.cell_size * (float)kBrickDim : 1.0f;
        k_source_keys<<<grid_for(n), 256, 0, h->stream>>>(h->s_raw.as<float>(), xyz_stride, n, 1.0f / cell,
                                                          h->s_keys.as<uint32_t>(), h->s_perm.as<uint32_t>());
        REGCHK(sort_pairs(h, h->s_tmp, h->s_keys.as<uint32_t>(), h->s_keys2.as<uint32_t>(), h->s_perm.as<uint32_t>(),
                          h->s_perm2.as<uint32_t>(), (size_t)n, 0, 30));
        h->perm = h->s_perm2.as<uint32_t>();
    }
    HIPCHK(h, hipEventRecord(h->ev_s1, h->stream));
    h->src_prep_pending = true;
    return REG_OK;
}

// R11, reading side: open3dToPointmatcher (open3d_conversions.cpp:57-118) converts every scan from Open3D's fp64 AoS
// (std::vector<Eigen::Vector3d> points_ / normals_, Matrix3d covariances_) to fp32 before icp_.compute
// (Mapper.cpp:288-289).  The cast runs on the device (round-to-nearest, as static_cast<float>), then reg_set_source.
reg_status reg_set_source_f64(reg_handle* h, const double* xyz, const double* normals, const double* covs, int64_t n,
                              int on_device) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    h->n = 0;
    h->prepared = false;
    h->have_match = false;
    h->pm_have_match = false;
    if (n <= 0) {
        h->err = "The reading point cloud is empty.";
        return REG_EMPTY_SOURCE;
    }
    if (!xyz || n > 0x7fffffffLL) return REG_BAD_ARGUMENT;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double *d_xyz = nullptr, *d_nrm = nullptr, *d_cov = nullptr;
    HIPCHK(h, staged_input(h, h->r_in_xyz, xyz, (size_t)n * 3, on_device, &d_xyz));
    HIPCHK(h, staged_input(h, h->r_in_nrm, normals, (size_t)n * 3, on_device, &d_nrm));
    HIPCHK(h, staged_input(h, h->r_in_cov, covs, (size_t)n * 9, on_device, &d_cov));
    HIPCHK(h, h->r_xyz.reserve((size_t)n * 12));
    if (d_nrm) HIPCHK(h, h->r_nrm.reserve((size_t)n * 12));
    if (d_cov) HIPCHK(h, h->r_cov.reserve((size_t)n * 24));
    k_cast_cloud_f64<<<grid_for(n), 256, 0, h->stream>>>(d_xyz, d_nrm, d_cov, n, h->r_xyz.as<float>(),
                                                          d_nrm ? h->r_nrm.as<float>() : nullptr,
                                                          d_cov ? h->r_cov.as<float>() : nullptr);
    HIPCHK(h, hipGetLastError());
    return reg_set_source(h, h->r_xyz.as<float>(), 3, d_nrm ? h->r_nrm.as<float>() : nullptr, 3,
                          d_cov ? h->r_cov.as<float>() : nullptr, n, 1);
}

}  // extern "C"
