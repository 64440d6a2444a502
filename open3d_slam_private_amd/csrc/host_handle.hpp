// host_handle.hpp -- the handle and its environment switches, HIPCHK and the small helpers of every host header, parameters,
// reg_create / reg_destroy / reg_set_stream, the debug entry points that read the handle
// Part of the single translation unit reg_core.hip (first of the host headers, after host_mem.hpp; not a standalone header).
#pragma once

// Diagnostic / tuning switches from the environment, read once when the handle is created (tools/ scripts set them;
// production code leaves them unset).
struct EnvSwitches {
    bool trace = false;         // O3D_TRACE: host-side timeline of prepare / enqueue / reports on stderr
    bool event_timing = false;  // O3D_EVENT_TIMING: loop_ms from HIP events even when not profiling
    bool halo_occ = true;       // O3D_NO_HALO_OCC: halo-bin edge from the floored bin edge instead of the density-derived one (A/B)
    bool no_dynprune = false;   // O3D_NO_DYNPRUNE: level scans keep the ball they started with (A/B)
    bool no_empty_bound = false;   // O3D_NO_EMPTY_BOUND: the halo directory carries no empty-space bound (A/B)
    bool no_witness = false;       // O3D_NO_WITNESS: the empty bins of the halo directory name no witness point (A/B)
    bool no_burst = false;      // O3D_NO_BURST: trickle-feed the fused iterations (A/B of the burst submission)
    bool hints = false;         // O3D_HINTS: histogram of the terminating search level of the last iteration
    bool stamps = false;        // O3D_STAMPS: in-kernel cycle stamps of the update kernel
    bool coh_stats = false;     // O3D_COH_STATS: share of the reading points the coherent fused kernel had to search
    bool tail_always = false;   // O3D_TAIL_ALWAYS: take the persistent tail even while other registrations are in flight on the device (A/B)
    bool update_generic = false;   // O3D_UPDATE_GENERIC=1: select-based / finish / Open3D updates launch the 1024-thread kernels that serve every path (A/B)
    bool no_tail = false;       // O3D_NO_TAIL: three-launch fused iterations instead of the persistent tail kernel (A/B, escape hatch)
    int tail_wpc = 0;           // O3D_TAIL_WPC: cap on the tail kernel's workgroups per XCD class (0: CUs / 8)
    double dist_timeout_s = 30.0; // O3D_DIST_TIMEOUT_S: deadline of every wait of the distributed path
    float tail_timeout_s = 2.f; // O3D_TAIL_TIMEOUT_S: bound of every grid barrier of the tail kernel
    int xcd_tile_first = 32;      // O3D_XCD_TILE_FIRST / _LATER: workgroups per XCD tile of the search kernel, first two launches of a
    int xcd_tile_later = 16;      //   registration / later ones (0: one contiguous eighth of the reading per XCD)
    float settle_trans = 0.02f;   // O3D_SETTLE_TRANS / O3D_SETTLE_ROT: largest last pose step [m] / [rad] at which the band-predicting iterations
    float settle_rot = 4e-3f;     //   (three-launch, tail kernel) may take over from the select-based ones
    int tail_min_iters = 8;       // O3D_TAIL_MIN_ITERS: checker mode (no fixed count): iterations that must have run before the tail kernel may take over
    int tail_tile = 0;            // O3D_TAIL_TILE: octets per XCD tile of the tail kernel's slot mapping (0: contiguous eighths)
    bool no_gicp_tail = false;    // O3D_NO_GICP_TAIL=1: GICP stays on its select-based iteration
    int gicp_tail_after = 1;      // O3D_GICP_TAIL_AFTER: select-based GICP iterations before the tail kernel takes over
    float tail_settle_tol = 1.2f; // O3D_TAIL_SETTLE: relative change of the trimmed limit below which the tail kernel takes over
    int lookahead = 2;          // O3D_KAHEAD
    float settle_tol = 0.05f;   // O3D_SETTLE: relative change of the trimmed limit below which the fused iterations start (round 2 sweep:
                                // 0.05 beats 0.25 by 5 % on C3 -- an early fused iteration has a wide band and moves every point by millimetres)
    float halo_ratio = 1.25f;   // O3D_HALO_RATIO: halo-bin edge in units of the brick-table bin edge.  Was 1.5 until the sweep of
                                // profiles/r05_fine_halo_geometry.txt: a run covers the bin's box grown by rho_h, so a smaller box is a
                                // shorter run (C3: 62 -> 42 records per settled query) and rho_h = 0.5 c still answers them; C3 +3 %,
                                // C4 +3 %, the table build no slower.  Finer bins go on paying in the search but cost the build
                                // 
    float halo_rho = 0.4f;      // O3D_HALO_RHO: exactness radius of the halo level in units of the halo-bin edge (round 2 sweep,
                                // profiles/r02_table_sweep.txt: 0.4 beats 0.25 by 2-6 % on C2 / C3 / C4 -- fewer queries fall through
                                // to the level scans, whose latency chain bounds the search kernels)
    float reach_bins = 7.25f;   // O3D_REACH_BINS: the automatic bin edge is at least max_dist / this
    float bin_occupancy = 8.f;  // O3D_BIN_OCC: points per occupied bin the automatic bin edge aims at
    float level_ratio = 2.0f;   // O3D_LEVEL_RATIO: ratio of consecutive search radii (c/2, ... up to max_dist)
    void read() {
        trace = getenv("O3D_TRACE") != nullptr;
        event_timing = getenv("O3D_EVENT_TIMING") != nullptr;
        no_burst = getenv("O3D_NO_BURST") != nullptr;
        no_dynprune = getenv("O3D_NO_DYNPRUNE") != nullptr;
        no_empty_bound = getenv("O3D_NO_EMPTY_BOUND") != nullptr;
        no_witness = getenv("O3D_NO_WITNESS") != nullptr;
        halo_occ = getenv("O3D_NO_HALO_OCC") == nullptr;
        hints = getenv("O3D_HINTS") != nullptr;
        stamps = getenv("O3D_STAMPS") != nullptr;
        coh_stats = getenv("O3D_COH_STATS") != nullptr;
        tail_always = getenv("O3D_TAIL_ALWAYS") != nullptr;
        no_tail = getenv("O3D_NO_TAIL") != nullptr;
        if (const char* v = getenv("O3D_UPDATE_GENERIC")) update_generic = atoi(v) != 0;
        if (const char* v = getenv("O3D_TAIL_WPC")) tail_wpc = std::max(0, atoi(v));
        if (const char* v = getenv("O3D_DIST_TIMEOUT_S")) dist_timeout_s = std::max(0.5, atof(v));
        if (const char* v = getenv("O3D_TAIL_SETTLE")) tail_settle_tol = (float)atof(v);
        if (const char* v = getenv("O3D_NO_GICP_TAIL")) no_gicp_tail = atoi(v) != 0;
        if (const char* v = getenv("O3D_TAIL_TILE")) tail_tile = std::max(0, atoi(v));
        if (const char* v = getenv("O3D_TAIL_MIN_ITERS")) tail_min_iters = std::max(0, atoi(v));
        if (const char* v = getenv("O3D_SETTLE_TRANS")) settle_trans = (float)atof(v);
        if (const char* v = getenv("O3D_SETTLE_ROT")) settle_rot = (float)atof(v);
        if (const char* v = getenv("O3D_XCD_TILE_FIRST")) xcd_tile_first = std::max(0, atoi(v));
        if (const char* v = getenv("O3D_XCD_TILE_LATER")) xcd_tile_later = std::max(0, atoi(v));
        if (const char* v = getenv("O3D_GICP_TAIL_AFTER")) gicp_tail_after = atoi(v);
        if (const char* v = getenv("O3D_TAIL_TIMEOUT_S")) tail_timeout_s = std::min(30.f, std::max(0.01f, (float)atof(v)));
        if (const char* v = getenv("O3D_KAHEAD")) lookahead = std::max(1, atoi(v));
        if (const char* v = getenv("O3D_SETTLE")) settle_tol = (float)atof(v);
        if (const char* v = getenv("O3D_HALO_RATIO")) halo_ratio = std::min(4.0f, std::max(0.5f, (float)atof(v)));
        if (const char* v = getenv("O3D_HALO_RHO")) halo_rho = std::min(1.0f, std::max(0.05f, (float)atof(v)));
        if (const char* v = getenv("O3D_REACH_BINS")) reach_bins = std::max(1.0f, (float)atof(v));
        if (const char* v = getenv("O3D_BIN_OCC")) bin_occupancy = std::min(64.0f, std::max(1.0f, (float)atof(v)));
        if (const char* v = getenv("O3D_LEVEL_RATIO")) level_ratio = std::min(4.0f, std::max(1.2f, (float)atof(v)));
    }
};

struct DistCtx;   // multi-GPU group state (host_rccl.hpp)

struct reg_handle {
    reg_params prm;
    reg_debug_params dbg;   // experiment switches (include/o3dslam_reg_debug.h); all zero in production
    EnvSwitches env;
    std::string err;
    // Every HIP resource is a member that frees itself (host_mem.hpp), in reverse order of declaration: stream, events and
    // pinned blocks stand ahead of every DevBuf, so the device buffers go first, then pinned blocks, events, the stream.
    Stream stream;
    Event ev0, ev1, ev_iter, ev_s0, ev_s1;
    Event ev_p0, ev_p1;   // reg_process_scan's stage time; created by its first call
    // loop profiling (params.profile_loop): HIP events around the search kernels of every iteration
    std::vector<Event> prof_ev;   // pairs (start, stop)
    Pinned<HostMirror> h_mirror;   // mapped: written by the update kernel through h_mirror.dev
    Pinned<IterState> h_iter;      // staging copy of the iteration state
    Pinned<PrepState> h_prep;      // mapped: host copy of the device-side preparation state
    bool device_ok = false;   // false: reg_create could not get a HIP device (every entry point then fails loudly)
    bool structure_only = false;   // workspace handle of reg_estimate_normals: bin table only, no attributes
    reg_handle* normals_ws = nullptr;
    DevBuf n_out, n_ids, n_extra, n_mom;
    // reg_compute_fpfh / reg_match_features (host_fpfh.hpp): staged inputs, ordered ids, counts + m, host-pointer outputs, flag
    // words; staged feature rows, per-chunk partial bests, index outputs, mutual flags + offsets
    DevBuf fp_xyz, fp_nrm, fp_ids, fp_cnt, fp_out, fp_misc, mf_a, mf_b, mf_part, mf_nn, mf_flags;
    // reg_ransac_correspondences (host_ransac.hpp): staged clouds and pairs; gathered pairs + inlier flags, offsets and output;
    // the batch's hypotheses, statuses and survivor lists; chunk partials; carried state + records, and their host copy
    DevBuf rs_src, rs_tgt, rs_cor, rs_pairs, rs_batch, rs_part, rs_rec;
    std::vector<RsRecord> rs_head;
    DevBuf i_xicp;                 // XicpState (R8x first-iteration analysis)
    DevBuf c_in_xyz, c_in_nrm, c_in_cov, c_flags, c_offs, c_xyz, c_nrm, c_cov, c_idx;   // reg_set_target_f64
    DevBuf r_in_xyz, r_in_nrm, r_in_cov, r_xyz, r_nrm, r_cov;                            // reg_set_source_f64
    int64_t crop_kept = 0;
    DevBuf v_fout, v_oout, v_out;   // reg_voxelize_within_volume
    DevBuf v_ukeys, v_ustart;                        // reg_carve_indices
    // reg_overlap_indices / reg_set_pair_overlap_f64 (host_overlap.hpp): per layer (0: source, 1: target) keys, sorted keys,
    // unique keys + counts, flags + offsets; run counts and the invalid-key word; the reading's index map
    DevBuf ov_keys[2], ov_sorted, ov_ukeys[2], ov_ucnt[2], ov_flags[2], ov_offs[2], ov_misc, ov_sidx;
    DevBuf i_info;                                   // reg_information_matrix: one row of sums per workgroup
    int64_t src_kept = 0;                            // > 0: ov_sidx maps the current reading back (reg_set_pair_overlap_f64,
                                                     // reg_process_scan)
    // the scan front end (host_scanprep.hpp): staged inputs; the cloud after the wide crop, after the voxel grid, after the
    // random selection (xyz, normals, covs each); the fp32 cast and the estimated fp32 normals / covariances; min-bound rows
    // + origin, the invalid-key word; sort keys and values, run heads and ids (heads / run double as the flags + offsets of
    // the crops and of the random selection); the events of scan_prep_ms
    DevBuf sp_in[3], sp_a[3], sp_b[3], sp_c[3], sp_f32[3], sp_part, sp_misc;
    RunBufs sp;
    // the dense maps of this handle (host_densemap.hpp) share their working set: staged inputs (points, normals, colours),
    // the cloud after the croppers, after the transform (points, normals); per run the rank, the new flag, its scan and the
    // new keys; touched / erase marks, keep flags and the scans of both; the invalid-key word + centre; host-pointer
    // outputs; sort keys and values, run heads and ids
    DevBuf dm_in[3], dm_crop[3], dm_tf[2], dm_rank, dm_new, dm_newoff, dm_newkeys, dm_mark, dm_keep, dm_off1, dm_off2, dm_misc,
        dm_out;
    RunBufs dm;
    // reg_dense_map_carve_scan: the brick keys and occupancy masks of the map being carved; the measurement switches of
    // reg_debug_dense_carve (lanes per ray: 0 the default, 8 / 16 / 64, -1 the lookups of k_dm_carve; sample counters) and
    // what the last call left: bricks, samples, samples done at the coarse level, rays
    DevBuf dm_bkeys, dm_bmask, dm_stats;
    int dm_carve_lanes = 0;
    bool dm_carve_stats = false;
    int64_t dm_last[4] = {0, 0, 0, 0};
    // the map clouds of this handle (host_mapcloud.hpp): staged inputs (scan points, normals, covariances; raw scan), the
    // transformed raw scan, and the working cloud an insert voxelises (survivors of the carve + the transformed scan)
    DevBuf mc_in[4], mc_raw, mc_cat[3];
    // reg_undistort_scan (host_odometry.hpp): staged input and host-pointer output
    DevBuf od_in, od_out;
    DevBuf d_d2all;                                  // select-by-gather (multi-GPU): all ranks' squared distances
    int64_t dist_nmax = 0;
    int dist_gather_ranks = 0;
    bool xicp_pending = false;     // the next generic iteration is followed by the analysis kernels
    bool src_prep_pending = false;   // ev_s0 / ev_s1 bracket the last reg_set_source; folded into source_prep_ms lazily
    float source_prep_ms = 0.f;
    int rotation_corrected = 0;
    bool iter_copy_pending = false;

    // target
    int64_t m = 0;
    bool has_tnrm = false, has_tcov = false;
    float c_ref[3] = {0, 0, 0};
    float t_mid[3] = {0, 0, 0};    // centre of the reference's bounding box (input frame unless P2PL): origin of the O3D_P2P sums
    DevBuf t_raw, t_nrm_raw, t_cov_raw, t_centred, t_keys, t_keys2, t_vals, t_vals2, t_pts, t_nrm, t_cov, t_flags,
        t_scan, t_hash, t_cells, t_misc, t_dir, t_rows;
    DevBuf rp_tmp;   // rocPRIM's temporary storage, live within one call (host_prims.hpp); every entry point but reg_set_source
    Grid grid;
    reg_target_info info;
    float target_build_ms = 0.f;

    // source
    int64_t n = 0;
    bool has_snrm = false, has_scov = false, prepared = false;
    int64_t s_stride = 3, s_nstride = 3;
    float c_read[3] = {0, 0, 0};
    DevBuf s_raw, s_nrm_raw, s_cov_raw, s_xyz, s_nrm, s_cov, s_misc;
    float T_init[16];              // row-major
    float T0[16];                  // T_refMean_readMean (row-major)
    // iteration buffers
    DevBuf i_pos, i_d2, i_w, i_hist, i_state, i_partials, i_sums, i_ids;
    DevBuf i_iter;                   // IterState on the device
    unsigned long long seq = 0;
    DevBuf t_halo_start, t_halo_cursor, t_halo_pts, t_halo_dir, i_band, i_acc, i_cache, i_stats, i_queue, i_qcount;
    DevBuf s_prep;
    int cent_slot = 0;                // which centroid-sum slot of s_misc the next single-GPU registration uses
    bool prep_pending = false;        // h_prep not yet folded into c_read / T0
    DevBuf i_hint, s_keys, s_keys2, s_perm, s_perm2, s_tmp, i_tmpf;
    const uint32_t* perm = nullptr;   // slot -> input index (null: identity)
    int last_stalls = 0;
    int64_t n_total_hint = 0;   // multi-GPU: points of the WHOLE reading (fitness of the GICP stop rule); 0: this handle's n
    int match_launches = 0;   // search launches since the reading was prepared (picks the XCD tile)
    int tail_sync_slot = 0, tail_sync_last = 0;   // which copy of the tail kernel's counter block the next / the last launch uses
    bool tail_sync_dirty = true;
    int last_tail_launches = 0, last_tail_iters = 0;   // persistent tail: launches / iterations of the last reg_register
    DevBuf i_tail_sync, i_tail_rows, i_tail_band;      // persistent tail: counters | per-workgroup sum rows | band records
    unsigned long long dist_seq0 = 0;
    DevBuf d_contrib, d_gathered;     // multi-GPU fused iteration: this rank's block / all ranks' blocks
    int dist_ranks = 0, dist_rank = 0;
    DistCtx* dist = nullptr;          // reg_dist_init: RCCL communicator (or custom transport) of this handle's group
    unsigned long long src_epoch = 0; // counts reg_set_source calls (the distributed path re-reads the slice sizes per reading)
    std::vector<int> prof_kind;        // of every pair of prof_ev: 0: k_match, 1: k_iter_fused
    bool profiling = false;
    int shift0 = 21;                  // low bit of the level-0 radix digit (19 when max_dist^2 < 2: bits 31,30 are 0)
    int n_blocks = 0;
    bool have_match = false;
    // libpointmatcher chain extension (reg_set_pm_chain; kernels_pmchain.hpp): pm_on = a non-default chain is set, or
    // EqualityConstraints is on (xt_on below): the handle registers on the chain loop
    bool pm_on = false;
    reg_pm_chain pm;
    // the chain's N x knn buffers hold the last iteration of a chain registration on the current reading (the plain
    // entry points -- reg_information_matrix, ... -- set have_match but never fill these)
    bool pm_have_match = false;
    DevBuf pm_pos, pm_d2, pm_w, pm_keys, pm_hist, pm_sel, pm_state, pm_partials;
    // VarTrimmedDist (kernels_pmoutliers.hpp): the sorted distances, rocPRIM's temporary storage, the per-tile records
    // {sum, offset, best value, best index, counts} + VarState; sized by register_pm, never inside the loop
    DevBuf pm_sorted, pm_sort_tmp, pm_var;
    size_t pm_sort_bytes = 0;
    // covariance / statistics / Bound / SolutionRemapping (kernels_pmextras.hpp): the device state of the modules, the rows
    // of the post-loop reductions, their totals and the covariance result block; host copies of the last registration
    DevBuf pm_xstate, pm_xrows, pm_xmeans, pm_xcov;
    PmExtraState pm_xhost;
    PmCovOut pm_cov_host;
    bool pm_x_valid = false;      // pm_xhost belongs to the last chain registration on the current reading
    bool pm_cov_valid = false;    // ... and pm_cov_host (a with_cov registration that ended with an update)
    float pm_cov_ms = 0.f;        // device time of the covariance evaluation (HIP events)
    double pm_last_error = 0.0;   // reg_result.error of the last chain registration
    // degeneracyAwareness EqualityConstraints (reg_set_ternary_xicp; kernels_xicp_ternary.hpp): with xt_on the handle
    // registers on the chain loop (pm_on) also under the default chain
    bool xt_on = false;
    reg_ternary_xicp xt;
    DevBuf xt_state, xt_rows;     // XtState; the per-workgroup rows of the three passes
    XtState xt_host;              // the state after the last registration with the method on
    bool xt_valid = false;        // ... which belongs to the current reading
    // data-point filters (host_filters.hpp): inputs, tree / index lists, leaf records, scans, host-pointer outputs
    DevBuf f_in, f_in_nrm, f_in_cov, f_px, f_pn, f_pc, f_perm, f_keys, f_keys2, f_segs, f_boxes, f_boxes2, f_leaf,
        f_mom, f_mom2, f_lid, f_keep, f_pos, f_misc, f_out;
    DevBuf f_fields, f_draws;     // reg_filter_cloud (host_cloud_filters.hpp): descriptor-field workspace, MaxDensity's draws
    // OctreeGridDataPointsFilter (host_octree.hpp): keys, sort orders, ranks, centres, per-round flags, leaf starts
    DevBuf o_keys, o_keys_s, o_iota, o_idx, o_idx2, o_rank, o_rank_a, o_rank_s, o_c, o_kk, o_heads, o_pos, o_open, o_depth,
        o_start, o_rand, o_radii;
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_constructible<reg_handle>::value, "owners are not copied");

#define HIPCHK(h, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return REG_DEVICE_ERROR;                                                           \
        }                                                                                      \
    } while (0)

static inline void col_to_row(const float* c, float* r) { m4_transpose(c, r); }
static inline void row_to_col(const float* r, float* c) { m4_transpose(r, c); }

static inline int grid_for(int64_t n, int block = 256) { return (int)((n + block - 1) / block); }

// The two Open3D RegistrationICP costs (select-free iterations, input frame, Open3D stop rule; include/o3dslam_reg.h)
static inline bool cost_is_o3d(int cost) { return cost == REG_COST_O3D_P2PL || cost == REG_COST_O3D_P2P; }

// A chain that reads reference normals: point-to-plane, the surface-normal filter or the robust point-to-plane distance
static inline bool pm_needs_tnrm(const reg_handle* h) {
    return h->pm.minimizer == REG_PM_POINT_TO_PLANE || h->prm.use_surface_normal ||
           (h->pm.use_robust && h->pm.distance_type == REG_DIST_POINT2PLANE);
}

// The fields the handle's cost needs on the reference / on the reading (reg_set_target, reg_set_source, reg_set_pair_overlap_f64)
static reg_status check_target_fields(reg_handle* h, bool has_nrm, bool has_cov) {
    if ((h->prm.cost == REG_COST_P2PL || h->prm.cost == REG_COST_O3D_P2PL) && !has_nrm && !h->structure_only &&
        !(h->pm_on && !pm_needs_tnrm(h))) {
        h->err = "InvalidField: point-to-plane needs the `normals` descriptor on the reference";
        return REG_MISSING_FIELD;
    }
    if (h->prm.cost == REG_COST_GICP && !has_cov && !h->structure_only) {
        h->err = "InvalidField: GICP needs covariances on the reference";
        return REG_MISSING_FIELD;
    }
    return REG_OK;
}
static reg_status check_source_fields(reg_handle* h, bool has_nrm, bool has_cov) {
    if (h->prm.cost == REG_COST_P2PL && h->prm.use_surface_normal && !has_nrm) {
        h->err = "InvalidField: SurfaceNormalOutlierFilter needs the `normals` descriptor on the reading";
        return REG_MISSING_FIELD;
    }
    if (h->prm.cost == REG_COST_GICP && !has_cov) {
        h->err = "InvalidField: GICP needs covariances on the reading";
        return REG_MISSING_FIELD;
    }
    return REG_OK;
}

extern "C" {

void reg_default_params(reg_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(reg_params);
    p->cost = REG_COST_P2PL;
    p->knn = 1;
    p->max_dist = std::numeric_limits<float>::infinity();
    p->epsilon = 0.f;
    p->use_trimmed = 1;
    p->trim_ratio = 0.85f;
    p->use_surface_normal = 0;
    p->max_normal_angle = 1.57f;
    p->use_max_dist_filter = 0;
    p->outlier_max_dist = 1.f;
    p->max_iter = 40;
    p->min_diff_rot = 0.001f;
    p->min_diff_trans = 0.001f;
    p->smooth_len = 3;
    p->fixed_iters = 0;
    p->gicp_rot_eps = 0.1f * 3.14159265358979f / 180.f;
    p->gicp_trans_eps = 1e-3f;
    p->cell_size = 0.f;
    p->device = 0;
    p->sort_source = 1;
    p->use_xicp = 0;            // ICPChainBase::setDefault has no degeneracy awareness
    p->xicp_enough = 250.f;             // icp.yaml:50-55
    p->xicp_insufficient = 180.f;
    p->xicp_min_angle_deg = 80.f;
    p->xicp_strong_angle_deg = 45.f;
    p->gicp_stop_rule = 0;
    p->gicp_rel_fitness = 1e-6f;        // open3d ICPConvergenceCriteria defaults
    p->gicp_rel_rmse = 1e-6f;
}

void reg_shipped_params(reg_params* p) {
    reg_default_params(p);
    p->max_dist = 0.5f;
    p->epsilon = 0.f;
    p->use_trimmed = 1;
    p->trim_ratio = 0.90f;
    p->use_surface_normal = 1;
    p->max_normal_angle = 1.57f;
    p->max_iter = 30;
    p->min_diff_rot = 0.001f;
    p->min_diff_trans = 0.008f;
    p->smooth_len = 3;
    p->use_xicp = 1;            // degeneracyAwareness: OptimizedEqualityConstraints (icp.yaml:50-55)
}

reg_status reg_create(const reg_params* p, reg_handle** out) {
    if (!p || !out) return REG_BAD_ARGUMENT;
    *out = nullptr;
    if (p->struct_size != (int32_t)sizeof(reg_params)) return REG_BAD_ARGUMENT;
    if (p->knn != 1) return REG_BAD_ARGUMENT;
    if (!(p->max_dist > 0.f)) return REG_BAD_ARGUMENT;
    if (p->cost != REG_COST_P2PL && p->cost != REG_COST_GICP && !cost_is_o3d(p->cost)) return REG_BAD_ARGUMENT;
    if (p->use_trimmed && !(p->trim_ratio >= 0.f && p->trim_ratio <= 1.f)) return REG_BAD_ARGUMENT;
    if (p->fixed_iters <= 0 && p->max_iter <= 0) return REG_BAD_ARGUMENT;
    // the device checkers keep the last kCheckerHist poses (k_tail stages them in LDS): a longer smoothing window would
    // average other steps than the reference's DifferentialTransformationChecker, so it is refused, not clamped
    if (p->smooth_len > kCheckerHist - 1) return REG_BAD_ARGUMENT;
    // the analysis expects libpointmatcher's point-to-plane (ICP.cpp:1118): GICP and the Open3D costs reject it
    if (p->use_xicp && p->cost != REG_COST_P2PL) return REG_BAD_ARGUMENT;
    if (p->gicp_stop_rule != 0 && p->gicp_stop_rule != 1) return REG_BAD_ARGUMENT;
    reg_handle* h = new reg_handle();
    *out = h;   // also on the two failure paths below: the handle is kept so that reg_last_error can explain
    h->prm = *p;
    std::memset(&h->dbg, 0, sizeof(h->dbg));
    h->env.read();
    std::memset(&h->info, 0, sizeof(h->info));
    std::memset(&h->grid, 0, sizeof(h->grid));
    if (hipSetDevice(p->device) != hipSuccess || h->stream.create() != hipSuccess) {
        h->err = "no usable HIP device (hipSetDevice/hipStreamCreate failed): the HIP path is mandatory";
        return REG_DEVICE_ERROR;   // entry points will fail loudly
    }
    h->device_ok = true;
    for (Event* e : {&h->ev0, &h->ev1, &h->ev_s0, &h->ev_s1}) (void)e->create();
    (void)h->ev_iter.create(hipEventDisableTiming);
    if (h->h_mirror.alloc(sizeof(HostMirror), hipHostMallocMapped) != hipSuccess ||
        h->h_iter.alloc(sizeof(IterState), hipHostMallocDefault) != hipSuccess ||
        h->h_prep.alloc(sizeof(PrepState), hipHostMallocMapped) != hipSuccess ||
        h->i_iter.reserve(sizeof(IterState)) != hipSuccess || h->s_misc.reserve(256) != hipSuccess ||
        hipMemset(h->s_misc.p, 0, 256) != hipSuccess) {   // centroid-sum slots start cleared (see prepare_rowmajor)
        h->err = "hipHostMalloc / hipMalloc of the iteration state failed";
        return REG_DEVICE_ERROR;
    }
    std::memset(h->h_mirror, 0, sizeof(HostMirror));
    return REG_OK;
}

void reg_destroy(reg_handle* h) {
    if (!h) return;
    (void)reg_dist_shutdown(h);
    if (h->normals_ws) reg_destroy(h->normals_ws);
    delete h;
}

const char* reg_last_error(const reg_handle* h) { return h ? h->err.c_str() : "null handle"; }

reg_status reg_debug_live_resources(int64_t out[4]) {
    if (!out) return REG_BAD_ARGUMENT;
    out[0] = g_live_bufs, out[1] = g_live_bytes, out[2] = g_live_pinned, out[3] = g_live_events;
    return REG_OK;
}

reg_status reg_debug_configure(reg_handle* h, const reg_debug_params* d) {
    if (!h || !d || d->struct_size != (int32_t)sizeof(reg_debug_params)) return REG_BAD_ARGUMENT;
    h->dbg = *d;
    return REG_OK;
}

// Diagnostic copy of the halo directory's empty-space bound, looked up on the host exactly as nearest_halo() looks it up:
// positions in the frame of reg_set_target's input; out[i] = lb of the bin of position i (0 for a bin with a run),
// -1 where the search would not consult the directory (outside the halo grid, or no halo level).
reg_status reg_debug_halo_bound(reg_handle* h, const float* xyz, int64_t n, float* out) {
    if (!h || !xyz || !out || n < 0) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    const Grid& g = h->grid;
    for (int64_t i = 0; i < n; ++i) out[i] = -1.f;
    if (h->m <= 0 || !g.use_halo) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const size_t nbins = (size_t)g.hdimx * g.hdimy * g.hdimz;
    std::vector<uint2> dir(nbins);
    HIPCHK(h, hipMemcpyAsync(dir.data(), g.halo_dir, nbins * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    auto bin = [](float v, float c, float o, float inv) {   // k_center_bbox, then bin_coord_f: one rounding per operation
        volatile float q = v - c;
        volatile float d = q - o;
        volatile float s = d * inv;
        return std::floor((float)s);
    };
    for (int64_t i = 0; i < n; ++i) {
        const float fx = bin(xyz[3 * i], h->c_ref[0], g.hox, g.hinv_c), fy = bin(xyz[3 * i + 1], h->c_ref[1], g.hoy, g.hinv_c),
                    fz = bin(xyz[3 * i + 2], h->c_ref[2], g.hoz, g.hinv_c);
        if (!(fx >= 0.f && fy >= 0.f && fz >= 0.f && fx < (float)g.hdimx && fy < (float)g.hdimy && fz < (float)g.hdimz)) continue;
        const uint2 hd = dir[((size_t)(int)fz * g.hdimy + (int)fy) * g.hdimx + (int)fx];
        float lb = 0.f;
        if ((int)hd.y < 0) {
            const uint32_t u = hd.y & 0x7fffffffu;
            std::memcpy(&lb, &u, 4);
        }
        out[i] = lb;
    }
    return REG_OK;
}

// Diagnostic copy of the halo directory's witnesses, looked up as nearest_halo() looks them up: out[i] = original index of the
// witness of position i's bin, -1 where the bin names none (or there is no halo level), -2 for a bin with a run.  A position
// outside the halo grid lies in no bin: it gets what the search takes from the border bin it clamps to -- that bin's
// witness, or the first record of its run (whichever record the fill pass put first), or -1 without witnesses.
reg_status reg_debug_halo_witness(reg_handle* h, const float* xyz, int64_t n, int32_t* out) {
    if (!h || !xyz || !out || n < 0) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    const Grid& g = h->grid;
    for (int64_t i = 0; i < n; ++i) out[i] = -1;
    if (h->m <= 0 || !g.use_halo) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    const size_t nbins = (size_t)g.hdimx * g.hdimy * g.hdimz;
    std::vector<uint2> dir(nbins);
    std::vector<float4> pts((size_t)h->m);
    const bool witness = (g.out_bound & 2) != 0;
    std::vector<float4> recs(witness ? h->t_halo_pts.cap / sizeof(float4) : 0);   // the runs' records (positions outside the grid)
    HIPCHK(h, hipMemcpyAsync(dir.data(), g.halo_dir, nbins * sizeof(uint2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(pts.data(), g.pts, (size_t)h->m * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    if (!recs.empty()) HIPCHK(h, hipMemcpyAsync(recs.data(), g.halo_pts, recs.size() * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    auto bin = [](float v, float c, float o, float inv) {   // k_center_bbox, then bin_coord_f: one rounding per operation
        volatile float q = v - c;
        volatile float d = q - o;
        volatile float s = d * inv;
        return std::floor((float)s);
    };
    auto clampi = [](float f, int dim) { return (int)std::fmin(std::fmax(f, 0.f), (float)(dim - 1)); };
    auto index_at = [&](uint32_t pos) {
        uint32_t idx = 0xffffffffu;
        if (pos < (uint32_t)h->m) std::memcpy(&idx, &pts[pos].w, 4);
        return (int32_t)idx;   // (a witness is a sorted position: always in range)
    };
    for (int64_t i = 0; i < n; ++i) {
        const float fx = bin(xyz[3 * i], h->c_ref[0], g.hox, g.hinv_c), fy = bin(xyz[3 * i + 1], h->c_ref[1], g.hoy, g.hinv_c),
                    fz = bin(xyz[3 * i + 2], h->c_ref[2], g.hoz, g.hinv_c);
        const bool inside = fx >= 0.f && fy >= 0.f && fz >= 0.f && fx < (float)g.hdimx && fy < (float)g.hdimy && fz < (float)g.hdimz;
        const uint2 hd = dir[((size_t)clampi(fz, g.hdimz) * g.hdimy + clampi(fy, g.hdimy)) * g.hdimx + clampi(fx, g.hdimx)];
        if ((int)hd.y >= 0) {
            out[i] = -2;
            if (!inside) {
                out[i] = -1;
                if (witness && hd.x < recs.size()) {
                    uint32_t pos;
                    std::memcpy(&pos, &recs[hd.x].w, 4);
                    out[i] = index_at(pos);
                }
            }
        } else if (witness && hd.x != 0xffffffffu) {
            out[i] = index_at(hd.x);
        }
    }
    return REG_OK;
}

reg_status reg_set_stream(reg_handle* h, void* hip_stream) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if ((hipStream_t)hip_stream == h->stream) return REG_OK;
    HIPCHK(h, hipSetDevice(h->prm.device));
    // Work already queued on the old stream (the D2D upload and Morton sort of reg_set_source, a table build, an
    // iteration) must have finished before anything is enqueued on the new one: the buffers are shared and there is no
    // other ordering between the two streams.  Switching streams is rare; a full wait is the simple, safe form.
    if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream.borrow((hipStream_t)hip_stream);   // destroys the old stream if the handle created it
    h->iter_copy_pending = false;   // the staging copy has completed with the old stream
    return REG_OK;
}

}  // extern "C"
