// host_loop.hpp -- reading preparation, iteration state, one iteration's enqueue helpers (over host_launch.hpp), result writer, lookahead
// and steering of the host loop, reg_register and the other single-GPU entry points (the libpointmatcher chain: host_pm.hpp)
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// =================================================================================================
// iteration driver (host)
// =================================================================================================

static reg_status check_ready(reg_handle* h, bool need_prepared) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (h->m == 0) {
        h->err = "no reference set (reg_set_target)";
        return REG_NOT_CONFIGURED;
    }
    if (h->n == 0) {
        h->err = "no reading set (reg_set_source)";
        return REG_NOT_CONFIGURED;
    }
    if (need_prepared && !h->prepared) {
        h->err = "reg_prepare has not been called for this reading";
        return REG_NOT_CONFIGURED;
    }
    return REG_OK;
}

// R2
// n_global > 0: the centroid sums in s_misc have already been produced (reg_dist_centroid_sums) and reduced over all
// ranks by the caller; they describe n_global points.
static reg_status prepare_rowmajor(reg_handle* h, const float* T_init_row, const float* c_override = nullptr,
                                   int64_t n_global = 0, const IterState* init_state = nullptr) {
    reg_status s = check_ready(h, false);
    if (s != REG_OK) return s;
    if (!m4_is_finite(T_init_row)) {
        h->err = "initial transformation contains non-finite values";
        return REG_BAD_TRANSFORM;
    }
    const bool ptrace = h->env.trace;
    const auto pt0 = std::chrono::steady_clock::now();
    auto pmark = [&](const char* what) {
        if (ptrace) fprintf(stderr, "[o3dreg] prepare %-18s t=%.1fus\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - pt0).count());
    };
    HIPCHK(h, hipSetDevice(h->prm.device));
    std::memcpy(h->T_init, T_init_row, 64);
    const int64_t n = h->n;
    const bool p2pl = h->prm.cost == REG_COST_P2PL;
    {
        // R3: the rotation block of the pre-transform T0 is that of T_init bit for bit (the two centring matrices are
        // pure translations); the kernel applies the re-orthogonalised copy to the points, this only reports it
        float Tc[16];
        h->rotation_corrected = (p2pl && rigid_correct(T_init_row, Tc)) ? 1 : 0;
    }
    // centroid sums -> (device) centroid + T0; the host copy arrives later through the pinned staging buffer and is
    // only needed for the final composition (R10), so nothing here waits for the device
    HIPCHK(h, h->s_misc.reserve(256));   // allocated and cleared when the handle was created
    HIPCHK(h, h->s_prep.reserve(sizeof(PrepState)));
    // Centroid sums of a single-GPU registration alternate between two slots of s_misc (words 8.. and 16..): the
    // prepare kernel of THIS registration clears the slot the NEXT one accumulates into, so no memset launch is needed
    // (slot 0 belongs to reg_dist_centroid_sums, which clears it itself).
    unsigned long long* sums = h->s_misc.as<unsigned long long>();
    unsigned long long* sums_next = nullptr;
    if (p2pl && !c_override && n_global <= 0) {
        sums = h->s_misc.as<unsigned long long>() + (h->cent_slot ? 16 : 8);
        sums_next = h->s_misc.as<unsigned long long>() + (h->cent_slot ? 8 : 16);
        h->cent_slot ^= 1;
        // (one workgroup per CU: every workgroup ends in three atomics on ONE cache line, ~15 ns each, one after the other)
        const int blocks = (int)std::min<int64_t>(256, (n + 255) / 256);
        k_centroid_sums<<<blocks, 256, 0, h->stream>>>(h->s_raw.as<float>(), h->s_stride, n, sums);
    }
    pmark("centroid");
    PrepArgs pa;
    pa.sums = sums;
    pa.sums_to_clear = sums_next;
    pa.n = n_global > 0 ? n_global : n;
    pa.c_ref = make_float3(h->c_ref[0], h->c_ref[1], h->c_ref[2]);
    std::memcpy(pa.T_init.m, T_init_row, 64);
    pa.centre = p2pl ? 1 : 0;
    pa.use_override = c_override ? 1 : 0;
    pa.c_override = c_override ? make_float3(c_override[0], c_override[1], c_override[2]) : make_float3(0.f, 0.f, 0.f);
    pa.out = h->s_prep.as<PrepState>();
    pa.host_out = h->h_prep.dev;
    h->prep_pending = true;
    StateInit si;
    si.dst = nullptr;
    if (init_state) {
        si.init = *init_state;
        si.dst = h->i_iter.as<IterState>();
    } else {
        std::memset(&si.init, 0, sizeof(si.init));
    }
    k_prepare_source<<<grid_for(n), 256, 0, h->stream>>>(
        h->s_raw.as<float>(), h->s_stride, (p2pl && h->has_snrm) ? h->s_nrm_raw.as<float>() : nullptr, h->s_nstride, n, pa,
        p2pl ? 1 : 0, h->perm, h->s_xyz.as<float4>(), (p2pl && h->has_snrm) ? h->s_nrm.as<float4>() : nullptr,
        h->i_hint.as<uint8_t>(), h->i_hist.as<uint32_t>(), h->i_acc.as<double>(), kAccRows * kSums, si,
        h->i_cache.as<float4>());
    if (h->prm.cost == REG_COST_GICP)
        k_pack_cov<<<grid_for(n), 256, 0, h->stream>>>(h->s_cov_raw.as<float>(), n, h->perm, h->s_cov.as<float4>());
    pmark("prepare_source");
    HIPCHK(h, hipGetLastError());
    h->prepared = true;
    h->match_launches = 0;
    h->have_match = false;
    h->pm_have_match = false;
    return REG_OK;
}

// ---- iteration state ---------------------------------------------------------------------------------

// T_refMean_dataIn = T_refIn_refMean^-1 * T_init (ICP.cpp:1067), its first three rows: the frame change of the R8x analyses
static void xicp_frame_change(const reg_handle* h, float Trd12[12]) {
    float A[16], Trd[16];
    m4_identity(A);
    for (int k = 0; k < 3; ++k) A[4 * k + 3] = -h->c_ref[k];
    m4_mul(A, h->T_init, Trd);
    for (int k = 0; k < 12; ++k) Trd12[k] = Trd[k];
}

// (Re)initialise the device-side iteration state: pose T (row-major), mode and checker configuration.
// Host part: fills *st (plain memory).  reg_register hands the result to k_prepare_source as a kernel argument (the
// state then reaches the device with the launch that is enqueued anyway: a pinned-staging hipMemcpyAsync + event
// cost ~20 us of host time in front of the first search kernel); the other entry points copy it (init_iter_state).
static reg_status build_iter_state(reg_handle* h, const float* T_row, int update, IterState* st) {
    std::memset(st, 0, sizeof(IterState));
    for (int i = 0; i < 16; ++i) {
        st->T[i] = T_row[i];
        st->Td[i] = (double)T_row[i];
    }
    st->chk = Checkers();
    st->chk.max_iter = h->prm.max_iter;
    st->chk.min_diff_rot = h->prm.min_diff_rot;
    st->chk.min_diff_trans = h->prm.min_diff_trans;
    st->chk.smooth_len = h->prm.smooth_len;
    st->chk.init(T_row);
    st->cost = h->prm.cost;
    st->fixed_iters = h->prm.fixed_iters;
    st->max_iter = h->prm.max_iter;
    st->update = update;
    st->gicp_rot_eps = h->prm.gicp_rot_eps;
    st->gicp_trans_eps = h->prm.gicp_trans_eps;
    st->gicp_stop_rule = h->prm.gicp_stop_rule;
    st->gicp_rel_fitness = h->prm.gicp_rel_fitness;
    st->gicp_rel_rmse = h->prm.gicp_rel_rmse;
    st->n_total = (float)(h->n_total_hint > 0 ? h->n_total_hint : h->n);
    st->band_lo = st->band_hi = INFINITY;
    st->limit_last = st->limit_prev = st->limit_prev2 = INFINITY;
    st->use_trim = (h->prm.cost == REG_COST_P2PL && h->prm.use_trimmed) ? 1 : 0;
    st->trim_ratio = h->prm.trim_ratio;
    st->band_cap = kBandCap;
    st->qcount = h->i_qcount.as<unsigned int>();
    st->debug_narrow_band = ((h->dbg.debug_flags & 8) ? 1 : 0) | ((h->dbg.debug_flags & 64) ? 2 : 0);   // bit 1: no direct band ranking
    h->xicp_pending = false;
    for (int k = 0; k < 6; ++k) st->xicp_flags[k] = 1;
    if (h->prm.use_xicp && h->prm.cost == REG_COST_P2PL && update) {
        HIPCHK(h, h->i_xicp.reserve(sizeof(XicpState)));
        st->xicp_stage = 1;
        st->xicp_enough = h->prm.xicp_enough;
        st->xicp_insufficient = h->prm.xicp_insufficient;
        st->xicp_cos_min = (float)std::cos((double)h->prm.xicp_min_angle_deg * 3.14159265358979323846 / 180.0);
        st->xicp_cos_strong = (float)std::cos((double)h->prm.xicp_strong_angle_deg * 3.14159265358979323846 / 180.0);
        xicp_frame_change(h, st->xicp_Trd);
        h->xicp_pending = true;
    }
    return REG_OK;
}

static reg_status init_iter_state(reg_handle* h, const float* T_row, int update) {
    IterState* st = h->h_iter;
    // the pinned staging copy may still be in flight from the previous call: wait for THAT copy only (an event
    // recorded right behind it), not for everything else enqueued on the stream
    if (h->iter_copy_pending) HIPCHK(h, hipEventSynchronize(h->ev_iter));
    reg_status s = build_iter_state(h, T_row, update, st);
    if (s != REG_OK) return s;
    HIPCHK(h, hipMemcpyAsync(h->i_iter.p, st, sizeof(IterState), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->ev_iter, h->stream));
    h->iter_copy_pending = true;
    return REG_OK;
}

static reg_status enqueue_match(reg_handle* h, bool zero_hist = false) {
    const bool trim = h->prm.cost == REG_COST_P2PL && h->prm.use_trimmed;
    if (trim && zero_hist) HIPCHK(h, hipMemsetAsync(h->i_hist.p, 0, 3 * 2048 * 4, h->stream));
    const bool fused_hist = h->dbg.match_variant == 3;
    uint32_t* hist0 = (trim && fused_hist) ? h->i_hist.as<uint32_t>() : nullptr;
    uint32_t* hist2 = trim ? h->i_hist.as<uint32_t>() + 4096 : nullptr;
    const IterState* it = h->i_iter.as<IterState>();
    if (h->dbg.match_variant == 1) {
        prof_mark(h, 0, true);
        k_match<<<h->n_blocks, 256, 0, h->stream>>>(h->s_xyz.as<float4>(), h->n, it, h->grid, h->i_pos.as<int>(),
                                                    h->i_d2.as<float>(), hist0, hist2, h->shift0);
        prof_mark(h, 0, false);
    } else {
        uint8_t* hint = h->dbg.match_variant == 2 ? nullptr : h->i_hint.as<uint8_t>();
        const int lanes = h->dbg.lanes_per_point == 4 ? 4 : (h->dbg.lanes_per_point == 2 ? 2 : 8);
        const int blocks = grid_for(h->n * lanes);
        // first searches of a registration: tiles large enough to keep an XCD's L2 on one region of the reference; later ones (halo
        // runs): finer
        const int tile = h->match_launches < 2 ? h->env.xcd_tile_first : h->env.xcd_tile_later;
        ++h->match_launches;
        const dim3 grid(xcd_tiled_grid(blocks, tile)), block(256);
        auto go = [&](auto kernel) {
            launch_timed(h, 0, kernel, grid, block, 0, (const float4*)h->s_xyz.as<float4>(), h->n, it, h->grid,
                         h->i_pos.as<int>(), h->i_d2.as<float>(), hist0, hist2, hint, h->shift0, h->dbg.debug_flags, blocks,
                         h->i_cache.as<float4>(), tile);
        };
        if (lanes == 4)
            go(k_match_g8<4>);
        else if (lanes == 2)
            go(k_match_g8<2>);
        else
            go(k_match_g8<8>);
    }
    h->have_match = true;
    return REG_OK;
}

// exact k-th smallest finite d2: level 0 and 1 histograms here, the last level inside the linearize kernel
static void enqueue_select(reg_handle* h) {
    const float* d2 = h->i_d2.as<float>();
    uint32_t* hist = h->i_hist.as<uint32_t>();
    SelectState* st = h->i_state.as<SelectState>();
    const int hb = std::min(h->n_blocks, 128);
    if (h->dbg.match_variant != 3) launch_hist_level0(h, d2, h->n, hb, hist);   // variant 3: the match kernel built it
    launch_select_level(h, 1, d2, h->n, hb, hist, st, h->prm.trim_ratio);
    launch_select_level(h, 2, d2, h->n, hb, hist, st, h->prm.trim_ratio);
}

static reg_status enqueue_linearize(reg_handle* h, bool want_w, bool limit_from_state = false) {
    float* w = want_w ? h->i_w.as<float>() : nullptr;
    if (h->prm.cost == REG_COST_P2PL) {
        launch_linearize_p2pl(h, h->prm.use_trimmed ? (limit_from_state ? 1 : 2) : 0, w);
    } else if (cost_is_o3d(h->prm.cost)) {
        // select-free: no outlier filters, no X-ICP; the update kernel of the Open3D costs
        const IterState* it = h->i_iter.as<IterState>();
        const float3 o = make_float3(h->t_mid[0], h->t_mid[1], h->t_mid[2]);
        if (h->prm.cost == REG_COST_O3D_P2PL)
            k_linearize_o3d<REG_COST_O3D_P2PL><<<h->n_blocks, 256, 0, h->stream>>>(
                h->s_xyz.as<float4>(), h->n, it, h->i_pos.as<int>(), h->i_d2.as<float>(), h->t_nrm.as<float4>(), o, w,
                h->i_partials.as<double>());
        else
            k_linearize_o3d<REG_COST_O3D_P2P><<<h->n_blocks, 256, 0, h->stream>>>(
                h->s_xyz.as<float4>(), h->n, it, h->i_pos.as<int>(), h->i_d2.as<float>(), h->t_pts.as<float4>(), o, w,
                h->i_partials.as<double>());
        update_o3d_from_partials(h);
        return REG_OK;
    } else {
        launch_linearize_gicp(h, w);
    }
    update_from_partials(h);
    if (h->xicp_pending) {
        // R8x, first iteration: collect the information sums on the matched pairs, then decide + solve + update
        h->xicp_pending = false;
        launch_xicp_center(h, h->i_pos.as<int>(), h->i_w.as<float>());
        launch_xicp_detect(h, h->i_pos.as<int>(), h->i_w.as<float>());
        update_xicp_finish(h);
    }
    return REG_OK;
}

// Fused iteration (point-to-plane): search + weights + normal equations (launch_fused_search), band resolution + solve +
// update in the update kernel.  Two or three launches per Gauss-Newton iteration.
static reg_status enqueue_fused(reg_handle* h) {
    CohStats* stats = h->env.coh_stats ? h->i_stats.as<CohStats>() : nullptr;
    const int rows = h->dbg.lanes_per_point == 4 ? launch_fused_search<4>(h, h->i_band.as<float>(), (int)kBandCap, stats, true)
                                                 : launch_fused_search<8>(h, h->i_band.as<float>(), (int)kBandCap, stats, true);
    update_fused_from_band(h, rows);
    h->have_match = true;
    return REG_OK;
}

// ---- persistent settled tail (kernels_tail.hpp): one launch for every remaining iteration -----------------------------
// Two persistent kernels on one device could each hold a part of the CUs and wait for the other's rest forever, so at most
// ONE registration per device and process runs its tail this way at a time (try_lock at the start of reg_register: the
// others -- BASELINE config C5, one registration per HIP stream -- keep the three-launch iteration, which fills the gaps).
// Across processes every grid barrier of the kernel is bounded (TailCfg::timeout_ticks) and ends in REG_DEVICE_ERROR.
constexpr int kTailMaxDevices = 64;
static std::mutex g_tail_mutex[kTailMaxDevices];
// Registrations of this process currently inside reg_register, per device.  The persistent kernel takes every CU for the
// whole tail (512 threads x 256 VGPRs + 117 KB of LDS per CU: nothing else is resident beside it), which is what ONE
// registration wants and what a batch of concurrent ones does not: 64 C2 registrations on 8 streams run 57 k iterations/s
// on the three-launch iteration and 50 k when one of them at a time holds the chip (bench.py --mode replicas, round 3).
// So the tail is only taken when no other registration is in flight on the device.
static std::atomic<int> g_reg_active[kTailMaxDevices];
struct RegActiveGuard {
    int dev;
    explicit RegActiveGuard(int d) : dev(d >= 0 && d < kTailMaxDevices ? d : -1) {
        if (dev >= 0) g_reg_active[dev].fetch_add(1, std::memory_order_relaxed);
    }
    ~RegActiveGuard() {
        if (dev >= 0) g_reg_active[dev].fetch_sub(1, std::memory_order_relaxed);
    }
    bool alone() const { return dev >= 0 && g_reg_active[dev].load(std::memory_order_relaxed) == 1; }
};
static int g_tail_cus[kTailMaxDevices];          // 0: not probed yet, < 0: the kernel cannot be co-resident on this device
static std::mutex g_tail_probe_mutex;

struct TailPlan {
    bool ok = false;
    int grid = 0, wpc = 0, chunk8 = 0, tile = 0;
};

// CUs of the device if one k_tail workgroup fits on each (occupancy query), probed once per process and device.
static int tail_device_cus(int dev) {
    if (dev < 0 || dev >= kTailMaxDevices) return -1;
    std::lock_guard<std::mutex> lk(g_tail_probe_mutex);
    if (g_tail_cus[dev] != 0) return g_tail_cus[dev];
    int cus = 0, nb = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    int nb2 = 0;
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tail<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kTailLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tail<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kTailLdsBytes);
    if (e == hipSuccess)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(k_tail<false>), kTailThreads, kTailLdsBytes);
    if (e == hipSuccess)
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb2, reinterpret_cast<const void*>(k_tail<true>), kTailThreads, kTailLdsBytes);
    g_tail_cus[dev] = (e == hipSuccess && nb >= kTailWgsPerCu && nb2 >= kTailWgsPerCu && cus >= 8) ? cus : -1;
    (void)hipGetLastError();
    return g_tail_cus[dev];
}

static TailPlan tail_plan_for(int64_t n, int cus, int wpc_cap, int tile) {
    TailPlan pl;
    if (cus < 8 || n <= 0) return pl;
    int wpc_max = cus * kTailWgsPerCu / 8;
    if (wpc_cap > 0) wpc_max = std::min(wpc_max, wpc_cap);
    pl.wpc = (int)std::max<int64_t>(1, std::min<int64_t>(wpc_max, (n + 2047) / 2048));
    pl.tile = std::max(0, tile);
    const int64_t unit = 8 * (int64_t)std::max(1, pl.tile);   // points per XCD class: whole octets, whole tiles
    pl.chunk8 = (int)((((n + 7) / 8) + unit - 1) / unit * unit);
    const int64_t octets = pl.chunk8 / 8, per_wg = (octets + pl.wpc - 1) / pl.wpc * 8;
    pl.grid = 8 * pl.wpc;
    pl.ok = per_wg <= kTailSlots;
    return pl;
}
// The plan of this handle's tail launches; not ok where the handle may not or cannot take the tail
static TailPlan tail_plan(const reg_handle* h) {
    if (cost_is_o3d(h->prm.cost)) return TailPlan();   // the Open3D costs have no persistent-tail form
    if (h->prm.cost == REG_COST_GICP && h->env.no_gicp_tail) return TailPlan();
    if (h->dbg.disable_fused == 1 || (h->dbg.debug_flags & (16 | 64 | 128)) || h->dbg.lanes_per_point == 4 || h->env.no_tail)
        return TailPlan();
    return tail_plan_for(h->n, tail_device_cus(h->prm.device), h->env.tail_wpc, h->env.tail_tile);
}

// Size of the last pose update as the host mirror shows it: translation of (T T_prev^-1) and its rotation angle (small-angle: the
// norm of the skew part).  Row-major 4x4, rigid.
static void last_step_motion(const HostMirror* m, float* trans, float* rot) {
    const float* A = m->T;
    const float* B = m->T_prev;
    // D = A * inv(B), inv(B) = [Rb^T, -Rb^T tb]
    float R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = A[4 * i + 0] * B[4 * j + 0] + A[4 * i + 1] * B[4 * j + 1] + A[4 * i + 2] * B[4 * j + 2];
    float t[3];
    for (int i = 0; i < 3; ++i) t[i] = A[4 * i + 3] - (R[3 * i + 0] * B[3] + R[3 * i + 1] * B[7] + R[3 * i + 2] * B[11]);
    *trans = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    const float sx = 0.5f * (R[7] - R[5]), sy = 0.5f * (R[2] - R[6]), sz = 0.5f * (R[3] - R[1]);
    *rot = std::sqrt(sx * sx + sy * sy + sz * sz);
}

// Enqueue the tail for at most `max_iters` iterations; the kernel reports ONCE (sequence h->seq) when it leaves.
static reg_status enqueue_tail(reg_handle* h, const TailPlan& pl, int max_iters) {
    // Two copies of the counter / accumulator block: a launch works on one and its workgroup 0 zeroes the OTHER one when it
    // leaves (nobody uses that one then: the launch before it, in stream order, is over) -- no memset launch (5 us) in front of
    // every tail launch.  Zeroed by the host when first allocated and after any launch that ended in an error.
    if (!h->i_tail_sync.p) h->tail_sync_dirty = true;
    HIPCHK(h, h->i_tail_sync.reserve(2 * (size_t)kTailSyncBytes));
    if (h->tail_sync_dirty) {
        HIPCHK(h, hipMemsetAsync(h->i_tail_sync.p, 0, 2 * (size_t)kTailSyncBytes, h->stream));
        h->tail_sync_dirty = false;
    }
    const int sync_slot = h->tail_sync_slot;
    h->tail_sync_slot ^= 1;
    h->tail_sync_last = sync_slot;
    unsigned* const sync_cur = h->i_tail_sync.as<unsigned>() + (size_t)sync_slot * (kTailSyncBytes / 4);
    unsigned* const sync_next = h->i_tail_sync.as<unsigned>() + (size_t)(sync_slot ^ 1) * (kTailSyncBytes / 4);
    HIPCHK(h, h->i_tail_rows.reserve((size_t)2 * pl.grid * kTailHistRow * 8));
    HIPCHK(h, h->i_tail_band.reserve((size_t)2 * kTailBandCap * kTailRec * 4));
    const FilterCfg f = make_filter_cfg(h, 0);
    TailCfg cfg;
    cfg.n = h->n;
    cfg.chunk8 = pl.chunk8;
    cfg.wpc = pl.wpc;
    cfg.tile = pl.tile;
    cfg.max_iters = std::max(1, std::min(max_iters, kTailMaxIters));
    cfg.slack = coherent_slack(h);
    cfg.seq = ++h->seq;
    cfg.timeout_ticks = (unsigned long long)(h->env.tail_timeout_s * 1e8);
    uint8_t* hint = h->dbg.match_variant == 2 ? nullptr : h->i_hint.as<uint8_t>();
    const bool gicp = h->prm.cost == REG_COST_GICP;
    // GICP: the covariances of the reading / the reference travel in the two attribute arguments
    const float4* s_attr = gicp ? (const float4*)h->s_cov.as<float4>() : (const float4*)(h->has_snrm ? h->s_nrm.as<float4>() : nullptr);
    const float4* t_attr = gicp ? (const float4*)h->t_cov.as<float4>() : (const float4*)h->t_nrm.as<float4>();
    auto go = [&](auto kernel) {   // (the weights are always written: reg_get_correspondences reports them)
        launch_timed(h, 3, kernel, dim3(pl.grid), dim3(kTailThreads), kTailLdsBytes, (const float4*)h->s_xyz.as<float4>(), s_attr,
                     h->i_iter.as<IterState>(), h->grid, t_attr, f, h->i_pos.as<int>(), h->i_d2.as<float>(), h->i_w.as<float>(), hint,
                     h->i_cache.as<float4>(), sync_cur, h->i_tail_rows.as<double>(), h->i_tail_band.as<float>(), h->h_mirror.dev, cfg,
                     sync_next);
    };
    if (gicp)
        go(k_tail<true>);
    else
        go(k_tail<false>);
    HIPCHK(h, hipGetLastError());
    h->have_match = true;
    return REG_OK;
}

// One Gauss-Newton iteration worth of kernels (R3-R9), nothing waits on the host.
static reg_status enqueue_iteration(reg_handle* h, bool want_w) {
    reg_status s = enqueue_match(h);
    if (s != REG_OK) return s;
    if (h->prm.cost == REG_COST_P2PL && h->prm.use_trimmed) enqueue_select(h);
    return enqueue_linearize(h, want_w);
}

static inline unsigned long long mirror_seq(const reg_handle* h) {
    return __atomic_load_n(&h->h_mirror->seq, __ATOMIC_ACQUIRE);
}

// Wait until the update kernel with sequence number `seq` (or a later one) has published its mirror.
// Polling the mapped word is ~10 us cheaper per wait than hipStreamSynchronize; a stream query every few
// thousand spins turns a device fault (or an early `done`) into a return instead of a hang.
static reg_status wait_seq(reg_handle* h, unsigned long long seq) {
    for (unsigned spins = 0;; ++spins) {
        if (mirror_seq(h) >= seq) return REG_OK;
        __builtin_ia32_pause();          // the sibling hyper-thread may be another handle's enqueueing thread
        if ((spins & 0x3fff) == 0x3fff) {
            hipError_t e = hipStreamQuery(h->stream);
            if (e == hipSuccess) return REG_OK;  // everything enqueued has run (later iterations were no-ops)
            if (e != hipErrorNotReady) {
                h->err = std::string("device fault while waiting for the iteration: ") + hipGetErrorString(e);
                return REG_DEVICE_ERROR;
            }
        }
    }
}

// one full pass R3-R7 at T (row-major) without pose update; sums -> h->h_mirror->sums
static reg_status iterate_once(reg_handle* h, const float* T_row, bool want_w) {
    reg_status s = init_iter_state(h, T_row, 0);
    if (s != REG_OK) return s;
    s = enqueue_iteration(h, want_w);
    if (s != REG_OK) return s;
    s = wait_seq(h, h->seq);
    if (s != REG_OK) return s;
    HIPCHK(h, hipGetLastError());
    return REG_OK;
}

// H_last / b_last: the reduced system as reported.  P2PL: A, b of A x = b (b = -sums); GICP and O3D_P2PL: H, the gradient
// sums as accumulated (J^T M J / J^T M r, J^T J / J^T r); O3D_P2P has no normal equations: zero.
static void sums_to_system(const double* sums, int cost, float* H, float* b) {
    if (cost == REG_COST_O3D_P2P) {
        std::memset(H, 0, 36 * sizeof(float));
        std::memset(b, 0, 6 * sizeof(float));
        return;
    }
    const bool p2pl = cost == REG_COST_P2PL;
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) {
            const float v = (float)sums[k++];
            H[6 * a + c] = v;
            H[6 * c + a] = v;
        }
    for (int a = 0; a < 6; ++a) b[a] = p2pl ? -(float)sums[21 + a] : (float)sums[21 + a];
}

// R10: T = T_refIn_refMean * T_iter * T_refMean_readMean * T_readIn_readMean^-1 (ICP.cpp:1345); GICP: T_iter itself
static void compose_rowmajor(reg_handle* h, const float* T_iter, float* Tout_row, bool later_kernel_reported = false) {
    if (h->prep_pending) {
        // k_prepare_source wrote PrepState into mapped host memory (system-scope fence); it is visible once that kernel has
        // completed: either a later kernel of the same stream has already reported through the mirror, or wait here
        if (!later_kernel_reported) (void)hipStreamSynchronize(h->stream);
        std::memcpy(h->c_read, h->h_prep->c_read, 12);
        std::memcpy(h->T0, h->h_prep->T0, 64);
        h->prep_pending = false;
    }
    if (h->prm.cost == REG_COST_P2PL) {
        float A[16], B[16], t1[16], t2[16];
        m4_identity(A);
        m4_identity(B);
        for (int k = 0; k < 3; ++k) {
            A[4 * k + 3] = h->c_ref[k];
            B[4 * k + 3] = -h->c_read[k];
        }
        m4_mul(A, T_iter, t1);
        m4_mul(t1, h->T0, t2);
        m4_mul(t2, B, Tout_row);
    } else {
        std::memcpy(Tout_row, T_iter, 64);
    }
}

// Sequences one registration may enqueue: fixed_iters, else max_iter -- plus one under Open3D's stop rule (GICP rule 1,
// the O3D costs), whose last sequence only re-evaluates the correspondences at the final pose.  reg_register and
// reg_dist_register both take their limit from here.
static int sequence_limit(const reg_params& p) {
    if (p.fixed_iters > 0) return p.fixed_iters;
    const bool o3d_rule = cost_is_o3d(p.cost) || (p.cost == REG_COST_GICP && p.gicp_stop_rule == 1);
    return p.max_iter + (o3d_rule ? 1 : 0);
}

// reg_result from the mirror: iterations and flags, the six-direction block (xicp: the mirror's flags and constraint count are
// reported, else 1 / 0; xicp_sums: its information sums are reported, else 0.0), the sums over n_reading points (those of the whole
// reading the sums describe; NaN where the handle does not know it: fitness NaN); then, unless the loop ended in an error (returned,
// the caller words it), the poses and -- where T_out is given -- the composed pose.  (Stall and tail counters: reg_register's own.)
// mirror_seen: as compose_rowmajor's later_kernel_reported.
static reg_status write_result(reg_handle* h, bool xicp, bool xicp_sums, double n_reading, bool mirror_seen, float* T_out,
                               reg_result* res) {
    const HostMirror* mir = h->h_mirror;
    res->iterations = mir->iterations;
    for (int k = 0; k < 6; ++k) {
        res->localizable[k] = xicp ? mir->localizable[k] : 1;
        res->xicp_combined[k] = xicp_sums ? mir->xicp_comb[k] : 0.0;
        res->xicp_high[k] = xicp_sums ? mir->xicp_high[k] : 0.0;
    }
    res->n_constraints = xicp ? mir->n_constraints : 0;
    res->converged = mir->converged;
    res->max_iter_reached = mir->max_iter_reached;
    res->rank_last = mir->rank_last;
    res->n_inliers = (int64_t)llround(mir->sums[28]);
    res->n_matched = (int64_t)llround(mir->sums[29]);
    res->error = mir->sums[27];
    res->fitness = mir->sums[28] / n_reading;
    res->inlier_rmse = mir->sums[28] > 0 ? std::sqrt(mir->sums[30] / mir->sums[28]) : 0.0;
    sums_to_system(mir->sums, h->prm.cost, res->H_last, res->b_last);
    res->target_build_ms = h->target_build_ms;
    if (h->src_prep_pending && hipEventQuery(h->ev_s1) == hipSuccess) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev_s0, h->ev_s1) == hipSuccess) h->source_prep_ms = ms;
        h->src_prep_pending = false;
    }
    res->source_prep_ms = h->source_prep_ms;
    res->rotation_corrected = h->rotation_corrected;
    if (mir->status != REG_OK) return (reg_status)mir->status;
    float T_iter[16], Tout_row[16];
    std::memcpy(T_iter, mir->T, 64);
    row_to_col(T_iter, res->T_iter_last);
    row_to_col(mir->T_prev, res->T_iter_prev);
    if (T_out) {
        compose_rowmajor(h, T_iter, Tout_row, mirror_seen);
        row_to_col(Tout_row, T_out);
    }
    return REG_OK;
}

// Sequences seq0+1 .. h->seq are this loop's.  Every sequence <= acked has either reported or been a no-op.
struct Lookahead {
    reg_handle* h;
    unsigned long long seq0, acked, m_seq = 0;   // begin with {h, h->seq, h->seq}
    bool any = false;               // a sequence of this loop has reported: the mirror's fields are this loop's
    int completed = 0, inflight = 0;
    void look() {
        m_seq = std::max(mirror_seq(h), seq0);
        any = m_seq > seq0;
    }
    void acknowledge() {
        acked = std::max(acked, m_seq);
        completed = any ? h->h_mirror->iterations : 0;
        inflight = (int)(h->seq - acked);
    }
    // blocks until the next unacknowledged sequence has reported -- or can no longer report
    reg_status wait_next() {
        const reg_status s = wait_seq(h, acked + 1);
        if (s != REG_OK) return s;
        if (mirror_seq(h) <= acked) {
            // the stream drained without a report: the remaining sequences were no-ops (done or stalled earlier)
            if (hipStreamQuery(h->stream) == hipSuccess && mirror_seq(h) <= acked) acked = h->seq;
        }
        return REG_OK;
    }
};

// ---- steering of reg_register: which kind of iteration to enqueue next -------------------------------------------------
struct SteerInput {
    bool any;                                             // what the host last saw in the mirror: anything of this loop at all,
    float limit_last, limit_prev, step_trans, step_rot;   // the last two trimmed limits, the size of the last pose step
    int completed, inflight, generic_left, limit;         // the loop's counters
};
struct SteerPolicy {
    bool trimming, can_fuse, p2pl, no_burst;
    bool use_tail = false, tail_off = false;
    int tail_min_iters, fixed;
    float fused_settle_tol, tail_settle_tol, settle_trans, settle_rot;
    explicit SteerPolicy(const reg_handle* h) {
        p2pl = h->prm.cost == REG_COST_P2PL;
        can_fuse = p2pl && h->dbg.disable_fused != 1;
        trimming = p2pl && h->prm.use_trimmed && h->prm.trim_ratio != 1.0f;
        no_burst = h->env.no_burst;
        fixed = h->prm.fixed_iters;
        // The tail kernel copes with a limit that still moves (wide bands cost it a second exchange, not a stall): it takes over as
        // soon as the predicted band (at most +-60 % around the last limit) can be expected to hold the next one
        // ... but only where it can pay: with a fixed iteration count always; with the checkers deciding (the mapper's registrations:
        // 4 - 7 iterations) not before tail_min_iters iterations have run without convergence -- a launch behind the iteration that
        // converges, or for one or two early iterations, costs more than the three-launch iteration it replaces
        // (tools/tools_checker_priors.py: 60 k -> 600 k, 3.6 / 4.1 / 6.9 iterations: +8 / +6 / +13 % with an unconditional tail)
        // (GICP the same: from 3 / 4-iteration registrations a launch after one or three iterations measures 0.108 / 0.135 and
        //  0.115 / 0.139 ms against 0.100 / 0.149 without -- a speculative launch behind the converging iteration costs what it saves)
        tail_min_iters = fixed > 0 ? 0 : h->env.tail_min_iters;
        fused_settle_tol = h->env.settle_tol;
        tail_settle_tol = h->env.tail_settle_tol;
        settle_trans = h->env.settle_trans;
        settle_rot = h->env.settle_rot;
    }
};
struct SteerChoice {
    enum Kind { kGeneric, kFused, kTail } kind;
    int count;   // kFused: iterations to enqueue in one burst; kTail: the tail launch's iteration budget
};

// Pure: no handle, no HIP call, no clock.
static SteerChoice steer_choose(const SteerInput& in, const SteerPolicy& p) {
    // fuse once the trimmed limit has settled (last two limits the host has seen within settle_tol, 5 %): the first
    // fused iteration is the expensive one -- its band is as wide as the limit still moves (wide band -> histogram
    // select in the update kernel, many coherence failures) -- so starting too early costs more than another
    // select-based iteration (round-2 sweep, DESIGN.md 6.0: 25 % -> 5 %: C3 1.653 -> 1.574 ms)
    const bool tail_now = p.use_tail && !p.tail_off && in.completed + in.inflight >= p.tail_min_iters;
    const float settle_tol = tail_now ? p.tail_settle_tol : p.fused_settle_tol;
    bool settled = true;
    if (p.trimming) {
        settled = in.any && in.limit_prev < INFINITY && in.limit_last < INFINITY &&
                  std::fabs(in.limit_last - in.limit_prev) <= settle_tol * in.limit_last;
    }
    // ... and the pose must have stopped jumping: a registration from a far prior sits on a plateau of the trimmed limit (most
    // pairs at the matching radius) while it still turns by degrees per iteration, then the limit collapses 10 - 20 x within
    // one iteration -- a band predicted on the plateau stalls there, and a tail launch entered there searches every point
    // first (O3D_TRACE: 2.5e-2 rad steps at a limit moving by 1 %; the benchmark's registration enters at 6e-4 rad / 4 mm)
    if (settled && in.any && (p.p2pl || p.fixed <= 0) && (p.can_fuse || tail_now)) {
        if (in.step_trans > p.settle_trans || in.step_rot > p.settle_rot) settled = false;
    }
    if (!(p.can_fuse || tail_now) || in.generic_left > 0 || !settled) return {SteerChoice::kGeneric, 1};
    const int rest = in.limit - (in.completed + in.inflight);
    if (tail_now) return {SteerChoice::kTail, rest};
    // Fixed iteration count: nothing the host could learn changes what has to run, so the whole rest of
    // the registration is submitted in one go (a failed band prediction turns what follows into no-ops
    // and is repaired by the caller).  Submitting while the device crosses a kernel boundary costs about 6 us per
    // iteration (measured: rocprofv3 timeline, profiles/), hence no trickle-feeding here.
    return {SteerChoice::kFused, p.fixed > 0 && !p.no_burst ? rest : 1};
}

// Waits for the tail launch with sequence tail_seq, which reports ONCE, when it leaves; reads back its error word.
static reg_status wait_tail(reg_handle* h, unsigned long long tail_seq, Lookahead& la, bool* tail_off) {
    const HostMirror* mir = h->h_mirror;
    // It leaves at once, WITHOUT a report, when a sequence enqueued in front of
    // it ended the loop (checker mode: the last select-based iteration converged while the tail was already queued):
    // that sequence's own report says so, no need to wait for the stream to drain.
    for (unsigned spins = 0;; ++spins) {
        const unsigned long long m = mirror_seq(h);
        if (m >= tail_seq) break;
        if (m + 1 == tail_seq) {
            // (the RECORD of that sequence, not the mirror's loose fields: the tail's own mirror words -- done = 1 --
            //  become visible before its sequence word does)
            const HostMirror::SeqRecord* rec = &mir->ring[(tail_seq - 1) % kSeqRing];
            if (__atomic_load_n(&rec->seq, __ATOMIC_ACQUIRE) == tail_seq - 1 && (rec->done || rec->stall)) break;
        }
        __builtin_ia32_pause();
        if ((spins & 0xfff) == 0xfff) {
            const hipError_t e = hipStreamQuery(h->stream);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) {
                h->tail_sync_dirty = true;
                h->err = std::string("device fault while waiting for the tail kernel: ") + hipGetErrorString(e);
                return REG_DEVICE_ERROR;
            }
        }
    }
    const bool reported = mirror_seq(h) >= tail_seq;
    const unsigned* sync_last = h->i_tail_sync.as<unsigned>() + (size_t)h->tail_sync_last * (kTailSyncBytes / 4);
    unsigned words[4] = {0, 0, 0, 0};
    if (!reported || h->env.coh_stats || mir->status == REG_DEVICE_ERROR)
        (void)hipMemcpy(words, sync_last + kTailErrWord, sizeof(words), hipMemcpyDeviceToHost);
    if (words[0] != 0 || (reported && mir->status == REG_DEVICE_ERROR)) {
        h->tail_sync_dirty = true;
        h->err = "persistent tail kernel: a grid barrier timed out (workgroups not co-resident? another process "
                 "running a persistent kernel on this GPU?); set O3D_NO_TAIL=1 to use the three-launch iteration";
        return REG_DEVICE_ERROR;
    }
    // The stream drained without a report: the tail found the loop done -- or STALLED by a three-launch iteration in front of
    // it (checker mode runs those until tail_min_iters): that stall is still to be repaired by the caller, so it must not
    // be acknowledged here (the next tail launch would leave at once again, for ever).
    if (!reported && !(mir->stall && std::max(mirror_seq(h), la.seq0) > la.acked)) la.acked = h->seq;
    if (h->env.coh_stats)
        fprintf(stderr, "[o3dreg] tail launch: %u iterations, %u point searches (%.2f %% of the point-iterations), stall cause %u, band records of its last iteration %d\n", words[2],
                words[1], words[2] ? 100.0 * words[1] / ((double)words[2] * (double)h->n) : 0.0, words[3], reported ? mir->pad_nband : -1);
    if (reported) h->last_tail_iters += mir->pad3;
    // checker mode: a tail launch that stalled (the trimmed limit left even the +-60 % band: the registration is still in
    // its fast phase) is not tried again in this registration -- the repair and the three-launch iterations carry on
    // (far priors at C3 size: 1.15 launches and 0.53 stalls per registration otherwise, tools/tools_checker_priors.py)
    if (reported && mir->stall && h->prm.fixed_iters <= 0) *tail_off = true;
#if O3D_TAIL_STAMPS
    {
        unsigned long long st[24];
        (void)hipMemcpy(st, sync_last + kTailStampWord, sizeof(st), hipMemcpyDeviceToHost);
        const double it_n = std::max(1, reported ? mir->pad3 : 1);
        static const char* names[12] = {"check", "search", "epilogue", "bandrec+comps", "sum+publish+drain", "arrive+wait", "row sums",
                                        "band-stage", "band-scan", "band-rank", "band-add", "solve+update"};
        for (int wg = 0; wg < 2; ++wg) {
            fprintf(stderr, "[o3dreg] tail stamps (us per iteration, %s workgroup):", wg ? "last" : "first");
            for (int i = 0; i < 12; ++i) fprintf(stderr, " %s %.2f", names[i], st[12 * wg + i] * 0.01 / it_n);
            fprintf(stderr, "\n");
        }
    }
#endif
    return REG_OK;
}

// loop_ms: HIP events only when profiling (record + synchronise cost ~20 us of host time per registration);
// otherwise the host clock around the loop -- the loop ends when the last update kernel's mirror has arrived
static reg_status loop_time_end(reg_handle* h, bool event_timing, std::chrono::steady_clock::time_point t_begin, float* loop_ms) {
    if (event_timing) {
        HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        HIPCHK(h, hipEventSynchronize(h->ev1));
        (void)hipEventElapsedTime(loop_ms, h->ev0, h->ev1);
    } else {
        *loop_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    return REG_OK;
}

// Diagnostics after the loop (O3D_HINTS, O3D_COH_STATS, O3D_STAMPS) and the profile events of its launches -> res->prof_*
static void loop_end_diagnostics(reg_handle* h, reg_result* res) {
    const HostMirror* mir = h->h_mirror;
    if (h->env.hints) {
        // diagnostics: at which radius level did the searches of the LAST iteration end (0 = halo, l + 1 = level l)
        std::vector<uint8_t> hv((size_t)h->n);
        if (hipMemcpy(hv.data(), h->i_hint.p, (size_t)h->n, hipMemcpyDeviceToHost) == hipSuccess) {
            long long cnt[18] = {0};
            for (uint8_t v : hv) ++cnt[v < 17 ? v : 17];
            fprintf(stderr, "[o3dreg] terminating level of the last iteration (halo, then levels with rho =");
            for (int l = 0; l < h->grid.n_levels; ++l) fprintf(stderr, " %.3f", h->grid.rho[l]);
            fprintf(stderr, "):");
            for (int l = 0; l <= h->grid.n_levels; ++l) fprintf(stderr, " %lld", cnt[l]);
            fprintf(stderr, "\n");
        }
    }
    if (h->env.coh_stats) {
        CohStats cs;
        if (hipMemcpy(&cs, h->i_stats.p, sizeof(cs), hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "[o3dreg] coherent fused iterations: %llu point-iterations, %llu searched (%.2f %%)\n", cs.n_points,
                    cs.n_searched, cs.n_points ? 100.0 * (double)cs.n_searched / (double)cs.n_points : 0.0);
            (void)hipMemset(h->i_stats.p, 0, sizeof(cs));
        }
    }
    if (h->env.stamps) {
        fprintf(stderr, "update kernel stamps (cycles): reduce %llu [rows %llu select %llu band-add %llu] solve %llu update+check %llu mirror %llu\n", mir->stamps[0],
                mir->stamps[4], mir->stamps[5], mir->stamps[6], mir->stamps[1], mir->stamps[2], mir->stamps[3]);
        fprintf(stderr, "   select detail: verify+stage-issue %llu, zero+hist+barriers %llu, wave0 pick/rank %llu\n", mir->stamps[3], mir->stamps[7] >> 32, mir->stamps[7] & 0xffffffffull);
    }
    if (h->profiling) {
        for (size_t i = 0; i + 1 < h->prof_ev.size(); i += 2) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, h->prof_ev[i], h->prof_ev[i + 1]) == hipSuccess) {
                const int kind = h->prof_kind[i / 2];
                res->prof_ms[kind] += ms;
                res->prof_launches[kind] += 1;
            }
        }
        h->prof_ev.clear();
        h->prof_kind.clear();
        h->profiling = false;
    }
}

static reg_status register_pm(reg_handle* h, const float* Ti, float T_out[16], reg_result* res);   // host_pm.hpp

extern "C" {

void reg_host_tail_plan(int64_t n, int32_t cus, int32_t tile, int32_t plan[4]) {
    const TailPlan pl = tail_plan_for(n, cus, 0, tile);
    plan[0] = pl.ok ? 1 : 0;
    plan[1] = pl.grid;
    plan[2] = pl.wpc;
    plan[3] = pl.chunk8;
}

// The band predictor of every loop path (reg_state.hpp: predict_band) on the host, for the CPU tests and the band model:
// band[0..1] = [lo, hi) predicted for the next trimmed limit from the last three (newest first; +inf: none) and from the
// population / edges of the last band (0 / +inf: unknown).  consts[0..7] (may be null): kTailBandCap, kTailWideRel and the
// predictor's constants in the order they are declared.
REG_API void reg_host_predict_band(float limit, float prev, float prev2, uint32_t last_count, float last_lo, float last_hi,
                                   int32_t debug_narrow, float band[2], float consts[8]) {
    const Band b = predict_band(limit, prev, prev2, last_count, last_lo, last_hi, debug_narrow);
    if (band) {
        band[0] = b.lo;
        band[1] = b.hi;
    }
    if (consts) {
        const float c[8] = {(float)kTailBandCap, kTailWideRel, kBandFloor, kBandRatioMax, kBandCentreGain, kBandGeomRel, kBandGuardFrac,
                            kBandForcedWide};
        for (int i = 0; i < 8; ++i) consts[i] = c[i];
    }
}

reg_status reg_prepare(reg_handle* h, const float T_init[16]) {
    if (!h || !T_init) return REG_BAD_ARGUMENT;
    float Tr[16];
    col_to_row(T_init, Tr);
    return prepare_rowmajor(h, Tr);
}

reg_status reg_linearize(reg_handle* h, const float T_iter[16], float H[36], float b[6], double* err,
                         int64_t* n_inliers) {
    reg_status s = check_ready(h, true);
    if (s != REG_OK) return s;
    if (!T_iter) return REG_BAD_ARGUMENT;
    if (h->prm.cost == REG_COST_O3D_P2P) {
        h->err = "reg_linearize: point-to-point (Umeyama) has no normal equations";
        return REG_UNSUPPORTED;
    }
    if (h->pm_on) {
        h->err = "reg_linearize: not available with a libpointmatcher chain (reg_set_pm_chain)";
        return REG_UNSUPPORTED;
    }
    float Tr[16];
    col_to_row(T_iter, Tr);
    if (!m4_is_finite(Tr)) return REG_BAD_TRANSFORM;
    HIPCHK(h, hipSetDevice(h->prm.device));
    s = iterate_once(h, Tr, true);
    if (s != REG_OK) return s;
    const double* sums = h->h_mirror->sums;
    if (H && b) sums_to_system(sums, h->prm.cost, H, b);
    if (err) *err = sums[27];
    if (n_inliers) *n_inliers = (int64_t)llround(sums[28]);
    if (sums[28] == 0.0) {
        h->err = "ErrorMinimizer: no point to minimize";
        return REG_NO_CORRESPONDENCES;
    }
    return REG_OK;
}

// == ICP::compute on the prepared reading.  The whole while(iterate) loop (ICP.cpp:1027-1311) runs on the
// device; the host only keeps the queue fed.  fixed_iters > 0: every iteration is enqueued at once.
// Checker mode: the host stays at most kAhead iterations ahead of what it has seen complete, so at most
// kAhead enqueued iterations turn into no-ops after convergence.
reg_status reg_register(reg_handle* h, const float T_init[16], float T_out[16], reg_result* res) {
    if (!h || !T_init || !T_out) return REG_BAD_ARGUMENT;
    reg_result local;
    if (!res) res = &local;
    std::memset(res, 0, sizeof(*res));
    std::memcpy(T_out, T_init, 64);
    float Ti[16];
    col_to_row(T_init, Ti);
    const auto t_reg0 = std::chrono::steady_clock::now();
    auto rmark = [&](const char* what) {
        if (h->env.trace)
            fprintf(stderr, "[o3dreg] register %-14s t=%.1fus\n", what,
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_reg0).count());
    };
    if (h->pm_on) return register_pm(h, Ti, T_out, res);
    const bool p2pl = h->prm.cost == REG_COST_P2PL;
    float T_start[16];
    if (p2pl)
        m4_identity(T_start);
    else
        std::memcpy(T_start, Ti, 64);
    std::memcpy(h->T_init, Ti, 64);   // the R8x frame change in the state is derived from it (prepare sets it again)
    IterState st0;
    reg_status s = build_iter_state(h, T_start, 1, &st0);
    if (s != REG_OK) return s;
    rmark("iter state");
    s = prepare_rowmajor(h, Ti, nullptr, 0, &st0);   // the state travels as an argument of the prepare kernel
    if (s != REG_OK) return s;
    rmark("prepared");
    h->profiling = h->dbg.profile_loop != 0;
    h->prof_ev.clear(), h->prof_kind.clear();   // (left by a profiled registration that failed before it read them)
    const bool event_timing = h->profiling || h->env.event_timing;
    if (event_timing) HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    const auto t_loop_begin = std::chrono::steady_clock::now();
    rmark("ev0");
    Lookahead la{h, h->seq, h->seq};
    // The persistent tail (kernels_tail.hpp) replaces the burst of three-launch fused iterations when this registration
    // holds the device's tail lock (one persistent kernel per device at a time: see g_tail_mutex).
    // (GICP has no three-launch fused form: without the tail lock its iterations stay select-based)
    SteerPolicy pol(h);
    const TailPlan tail_pl = (pol.can_fuse || h->prm.cost == REG_COST_GICP) ? tail_plan(h) : TailPlan();
    const RegActiveGuard active(h->prm.device);
    std::unique_lock<std::mutex> tail_lock;
    if (tail_pl.ok && (active.alone() || h->env.tail_always)) {
        tail_lock = std::unique_lock<std::mutex>(g_tail_mutex[h->prm.device], std::try_to_lock);
    }
    pol.use_tail = tail_pl.ok && tail_lock.owns_lock();
    const int limit = sequence_limit(h->prm);
    const int kAhead = h->env.lookahead;
    const HostMirror* mir = h->h_mirror;
    // Iterations 0..generic_left-1 run on the generic (select-based) path: the trimmed limit still moves too
    // much to be predicted.  Afterwards the fused two-kernel iteration is used; if its band prediction fails the
    // device stalls the queue and the host repairs that iteration on the generic path.
    int generic_left = pol.trimming ? 2 : (h->prm.cost == REG_COST_GICP ? std::max(1, h->env.gicp_tail_after) : 1);
    unsigned long long last_traced = 0;
    const auto t_loop0 = std::chrono::steady_clock::now();
    unsigned long long tail_seq = 0;   // != 0: a tail launch is in flight; nothing is enqueued behind it
    h->last_stalls = h->last_tail_launches = h->last_tail_iters = 0;
    for (;;) {
        if (tail_seq) {
            s = wait_tail(h, tail_seq, la, &pol.tail_off);
            if (s != REG_OK) return s;
            tail_seq = 0;
            continue;
        }
        la.look();
        if (la.any && mir->done) break;
        if (la.any && mir->stall && la.m_seq > la.acked) {
            // band prediction failed at sequence m_seq: everything enqueued behind it is a no-op; drain, repair
            HIPCHK(h, hipStreamSynchronize(h->stream));
            la.acked = h->seq;
            generic_left = 2;
            ++h->last_stalls;
            continue;
        }
        if (h->env.trace && la.m_seq != last_traced) {
            last_traced = la.m_seq;
            float mt = 0.f, mr = 0.f;
            last_step_motion(mir, &mt, &mr);
            fprintf(stderr, "[o3dreg] seq %llu iter %d stall %d band_n %d limit %.6g prev %.6g band [%.6g, %.6g) step %.2e m %.2e rad\n",
                    la.m_seq - la.seq0, mir->iterations, mir->stall, mir->stall ? mir->band_count : mir->pad_nband, mir->limit_last,
                    mir->limit_prev, mir->band_lo, mir->band_hi, mt, mr);
        }
        la.acknowledge();
        if (la.completed + la.inflight < limit && la.inflight < kAhead) {
            SteerInput seen = {la.any, mir->limit_last, mir->limit_prev, 0.f, 0.f, la.completed, la.inflight, generic_left, limit};
            if (la.any) last_step_motion(mir, &seen.step_trans, &seen.step_rot);
            const SteerChoice c = steer_choose(seen, pol);
            const auto tq0 = std::chrono::steady_clock::now();
            if (c.kind == SteerChoice::kGeneric) {
                s = enqueue_iteration(h, true);   // weights are always written: reg_get_correspondences reports them
                if (generic_left > 0) --generic_left;
            } else if (c.kind == SteerChoice::kTail) {
                // the rest of the registration in ONE launch (it leaves when done, stalled, or out of its iteration budget)
                s = enqueue_tail(h, tail_pl, c.count);
                tail_seq = h->seq;
                ++h->last_tail_launches;
            } else {
                for (int burst = c.count; burst > 0 && s == REG_OK; --burst) s = enqueue_fused(h);
            }
            if (h->env.trace) {
                const auto tq1 = std::chrono::steady_clock::now();
                fprintf(stderr, "[o3dreg] t=%.1fus enqueue seq %llu (%s) took %.1fus; mirror at %llu\n",
                        std::chrono::duration<double, std::micro>(tq0 - t_loop0).count(), h->seq - la.seq0,
                        c.kind == SteerChoice::kGeneric ? "generic" : (c.kind == SteerChoice::kTail ? "tail" : "fused"),
                        std::chrono::duration<double, std::micro>(tq1 - tq0).count(), std::max(mirror_seq(h), la.seq0) - la.seq0);
            }
            if (s != REG_OK) return s;
            continue;
        }
        if (la.inflight == 0) break;  // nothing in flight and nothing left to enqueue
        s = la.wait_next();
        if (s != REG_OK) return s;
    }
    rmark("loop done");
    s = loop_time_end(h, event_timing, t_loop_begin, &res->loop_ms);
    if (s != REG_OK) return s;
    HIPCHK(h, hipGetLastError());
    rmark("loop timed");
    loop_end_diagnostics(h, res);
    s = write_result(h, h->prm.use_xicp != 0, /*xicp_sums=*/true, (double)h->n, /*mirror_seen=*/true, T_out, res);
    if (s != REG_OK) {
        h->err = mir->sums[29] == 0.0 ? "No matches available for computing distance quantiles"
                                      : "ErrorMinimizer: no point to minimize";
        return s;
    }
    res->n_band_stalls = h->last_stalls;
    res->n_tail_launches = h->last_tail_launches;
    res->n_tail_iterations = h->last_tail_iters;
    rmark("return");
    return REG_OK;
}

reg_status reg_information_matrix(reg_handle* h, const float T[16], float max_dist, double info[36], int64_t* n_pairs) {
    if (!h || !T || !info) return REG_BAD_ARGUMENT;
    if (n_pairs) *n_pairs = 0;
    if (!(max_dist > 0.f) || max_dist > h->prm.max_dist) {
        h->err = "reg_information_matrix: max_dist must be positive and within the handle's max_dist";
        return REG_BAD_ARGUMENT;
    }
    float Tr[16];
    col_to_row(T, Tr);
    reg_status s = prepare_rowmajor(h, Tr);
    if (s != REG_OK) return s;
    float T_start[16];
    if (h->prm.cost == REG_COST_P2PL)
        m4_identity(T_start);
    else
        std::memcpy(T_start, Tr, 64);
    s = init_iter_state(h, T_start, 0);
    if (s != REG_OK) return s;
    s = enqueue_match(h, /*zero_hist=*/false);
    if (s != REG_OK) return s;
    h->have_match = true;
    // one row of sums per workgroup, added up here in block order: the same clouds give the same 36 doubles on every call
    // and on every handle (a device-side atomic sum would depend on the order in which the workgroups retire)
    const int blocks = (int)std::min<int64_t>(512, (h->n + 255) / 256);
    HIPCHK(h, h->i_info.reserve((size_t)512 * 10 * sizeof(double)));
    HIPCHK(h, hipMemsetAsync(h->i_info.p, 0, (size_t)blocks * 10 * sizeof(double), h->stream));
    k_info_sums<<<blocks, 256, 0, h->stream>>>(h->i_pos.as<int>(), h->i_d2.as<float>(), h->n, h->t_pts.as<float4>(),
                                               h->c_ref[0], h->c_ref[1], h->c_ref[2], max_dist * max_dist,
                                               h->i_info.as<double>());
    std::vector<double> rows((size_t)blocks * 10);
    HIPCHK(h, hipMemcpyAsync(rows.data(), h->i_info.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    double m[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < blocks; ++b)
        for (int k = 0; k < 10; ++k) m[k] += rows[(size_t)b * 10 + k];
    // sum over pairs of G^T G with rows [0 z -y 1 0 0], [-z 0 x 0 1 0], [y -x 0 0 0 1]
    const double c = m[0], sx = m[1], sy = m[2], sz = m[3], xx = m[4], yy = m[5], zz = m[6], xy = m[7], xz = m[8], yz = m[9];
    const double I[36] = {yy + zz, -xy, -xz, 0, -sz, sy,
                          -xy, xx + zz, -yz, sz, 0, -sx,
                          -xz, -yz, xx + yy, -sy, sx, 0,
                          0, sz, -sy, c, 0, 0,
                          -sz, 0, sx, 0, c, 0,
                          sy, -sx, 0, 0, 0, c};
    std::memcpy(info, I, sizeof(I));
    if (n_pairs) *n_pairs = (int64_t)llround(c);
    return REG_OK;
}

reg_status reg_compute(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm, int64_t nrm_stride,
                       const float* cov, int64_t n, int on_device, const float T_init[16], float T_out[16],
                       reg_result* res) {
    reg_status s = reg_set_source(h, xyz, xyz_stride, nrm, nrm_stride, cov, n, on_device);
    if (s != REG_OK) return s;
    return reg_register(h, T_init, T_out, res);
}

reg_status reg_get_correspondences(reg_handle* h, int32_t* ids, float* d2, float* w) {
    reg_status s = check_ready(h, true);
    if (s != REG_OK) return s;
    if (!h->have_match) {
        h->err = "no iteration has run yet";
        return REG_NOT_CONFIGURED;
    }
    if (h->pm_on) {
        if (h->pm.knn != 1) {
            h->err = "reg_get_correspondences: the chain matches knn > 1 neighbours; use reg_get_correspondences_k";
            return REG_UNSUPPORTED;
        }
        return reg_get_correspondences_k(h, 1, ids, d2, w);
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    const int64_t n = h->n;
    if (ids) {
        HIPCHK(h, h->i_ids.reserve((size_t)n * 4));
        k_ids_from_pos<<<grid_for(n), 256, 0, h->stream>>>(h->i_pos.as<int>(), h->t_pts.as<float4>(), n, h->perm,
                                                           h->i_ids.as<int32_t>());
        HIPCHK(h, hipMemcpyAsync(ids, h->i_ids.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, h->i_tmpf.reserve((size_t)n * 8));
    if (d2) {
        k_unpermute_f32<<<grid_for(n), 256, 0, h->stream>>>(h->i_d2.as<float>(), n, h->perm, h->i_tmpf.as<float>());
        HIPCHK(h, hipMemcpyAsync(d2, h->i_tmpf.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (w) {
        k_unpermute_f32<<<grid_for(n), 256, 0, h->stream>>>(h->i_w.as<float>(), n, h->perm, h->i_tmpf.as<float>() + n);
        HIPCHK(h, hipMemcpyAsync(w, h->i_tmpf.as<float>() + n, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

}  // extern "C"
