// host_pm.hpp -- host code of the libpointmatcher chain (reg_set_pm_chain): chain configuration, one chain iteration, register_pm,
// reg_*_pm_chain, reg_*_ternary_xicp and the covariance / bound / degeneracy / robust / var-trim accessors
// Part of the single translation unit reg_core.hip (included there, after host_loop.hpp; not a standalone header).
#pragma once

// ---- libpointmatcher chain extension (reg_set_pm_chain; kernels_pmchain.hpp) --------------------------------------

static bool pm_chain_is_default(const reg_pm_chain* c) {
    return c->knn == 1 && c->minimizer == REG_PM_POINT_TO_PLANE && !c->use_robust && !c->use_min_dist_filter &&
           !c->use_median_dist && !c->use_var_trimmed && !c->with_cov && !c->use_bound && c->degeneracy_method == 0;
}
static bool pm_chain_has_extras(const reg_pm_chain* c) { return c->with_cov || c->use_bound || c->degeneracy_method != 0; }

// The caller's chain in today's layout: a struct of REG_PM_CHAIN_SIZE_V1 bytes (built before MinDist / MedianDist /
// VarTrimmedDist) or REG_PM_CHAIN_SIZE_V2 bytes (before covariance / Bound / SolutionRemapping) is completed with the
// fields it does not hold off
static bool pm_chain_read(const reg_pm_chain* c, reg_pm_chain* out) {
    if (c->struct_size == (int32_t)sizeof(reg_pm_chain)) {
        *out = *c;
        return true;
    }
    if (c->struct_size != REG_PM_CHAIN_SIZE_V1 && c->struct_size != REG_PM_CHAIN_SIZE_V2) return false;
    reg_default_pm_chain(out);
    std::memcpy(out, c, (size_t)c->struct_size);
    out->struct_size = (int32_t)sizeof(reg_pm_chain);
    return true;
}

static PmCfg make_pm_cfg(const reg_handle* h) {
    const reg_pm_chain& c = h->pm;
    PmCfg f;
    f.knn = c.knn;
    f.minimizer = c.minimizer;
    f.use_robust = c.use_robust;
    f.robust_fct = c.robust_fct;
    f.scale_estimator = c.scale_estimator;
    f.nb_iter_for_scale = c.nb_iter_for_scale;
    f.distance_type = c.distance_type;
    f.use_trim = h->prm.use_trimmed;
    f.use_normal = h->prm.use_surface_normal;
    f.use_maxdist = h->prm.use_max_dist_filter;
    // berg: the configured tuning is the target scale; the function's own constant replaces it (Bergstrom 2014,
    // OutlierFiltersImpl.cpp:430-445)
    f.tuning = c.tuning;
    f.berg_target = c.tuning;
    if (c.scale_estimator == REG_SCALE_BERG) {
        if (c.robust_fct == REG_ROBUST_CAUCHY) f.tuning = 4.3040f;
        else if (c.robust_fct == REG_ROBUST_TUKEY) f.tuning = 7.0589f;
        else if (c.robust_fct == REG_ROBUST_HUBER) f.tuning = 2.0138f;
    }
    f.sq_approx = std::isinf(c.approximation) ? INFINITY : (float)((double)c.approximation * (double)c.approximation);
    f.cos_max_angle = std::cos(h->prm.max_normal_angle);
    const float md = h->prm.outlier_max_dist;
    f.outlier_max_d2 = md * md;
    f.use_mindist = c.use_min_dist_filter;
    f.use_median = c.use_median_dist;
    f.use_var = c.use_var_trimmed;
    f.outlier_min_d2 = c.outlier_min_dist * c.outlier_min_dist;
    f.median_factor = c.median_factor;
    f.var_min_ratio = c.var_min_ratio;
    f.var_max_ratio = c.var_max_ratio;
    f.var_lambda = c.var_lambda;
    return f;
}

static PmExtraCfg make_pm_extra_cfg(const reg_handle* h) {
    const reg_pm_chain& c = h->pm;
    PmExtraCfg x;
    x.use_bound = c.use_bound;
    x.bound_after_counter = c.bound_after_counter;
    x.max_rot = c.max_rotation_norm;
    x.max_trans = c.max_translation_norm;
    x.degeneracy = c.degeneracy_method;
    x.sr_use2019 = c.sr_use2019;
    x.sr_threshold = c.sr_threshold;
    x.with_cov = c.with_cov;
    return x;
}

// One exact select over nk keys (+inf keys are not counted) -> sel[slot]: the value of rank trim_rank(finite, ratio)
// (getDistsQuantile: index size * quantile in float), or with median != 0 of rank finite / 2 (getMedianAbsDeviation: the
// integer index, which differs from the float form once more than 2^24 keys are finite)
static void enqueue_pm_select(reg_handle* h, const float* keys, int64_t nk, float ratio, int slot, int median = 0) {
    uint32_t* hist = h->pm_hist.as<uint32_t>();
    SelectState* st = h->pm_sel.as<SelectState>();
    const IterState* it = h->i_iter.as<IterState>();
    const int hb = (int)std::min<int64_t>(128, grid_for(nk));
    launch_hist_level0(h, keys, nk, hb, hist);
    k_pm_select_level1<<<hb, 256, 0, h->stream>>>(keys, nk, h->shift0, ratio, median, hist, hist + 2048, st, it);
    launch_select_level(h, 2, keys, nk, hb, hist, st, ratio);
    k_pm_select_finish<<<1, 256, 0, h->stream>>>(hist, st, h->shift0, h->pm_state.as<PmState>(), slot, it);
}

// Tiles of the VarTrimmedDist kernels over nk keys, and the layout of pm_var: five 8-byte records per tile, VarState
static inline int pm_var_tiles(int64_t nk) { return (int)((nk + kVarTile - 1) / kVarTile); }
static inline size_t pm_var_bytes(int64_t nk) { return (size_t)pm_var_tiles(nk) * 40 + sizeof(VarState); }

// VarTrimmedDist limit of this iteration -> PmState (kernels_pmoutliers.hpp).  The sort runs whatever the loop state is
// and only writes scratch; the kernels after it return at once when the loop is done.
static reg_status enqueue_pm_var_trim(reg_handle* h, const PmCfg& cfg, const float* kd2, int64_t nk) {
    const IterState* it = h->i_iter.as<IterState>();
    const int nb = pm_var_tiles(nk);
    uint32_t* sorted = h->pm_sorted.as<uint32_t>();
    double* bsum = h->pm_var.as<double>();
    double* boff = bsum + nb;
    double* bval = boff + nb;
    long long* bidx = reinterpret_cast<long long*>(bval + nb);
    uint2* bcnt = reinterpret_cast<uint2*>(bidx + nb);
    VarState* vs = reinterpret_cast<VarState*>(bcnt + nb);
    size_t bytes = h->pm_sort_bytes;
    HIPCHK(h, rocprim::radix_sort_keys(h->pm_sort_tmp.p, bytes, reinterpret_cast<const uint32_t*>(kd2), sorted, (size_t)nk, 0, 32,
                                       h->stream));
    k_pm_var_block_sums<<<nb, 256, 0, h->stream>>>(sorted, nk, bsum, bcnt, it);
    k_pm_var_scan_blocks<<<1, 256, 0, h->stream>>>(bsum, bcnt, nb, boff, vs, nk, cfg.var_min_ratio, cfg.var_max_ratio, it);
    k_pm_var_objective<<<nb, 256, 0, h->stream>>>(sorted, nk, boff, vs, nk, 2.0 * (double)cfg.var_lambda, bval, bidx, it);
    k_pm_var_finish<<<1, 256, 0, h->stream>>>(sorted, bval, bidx, nb, vs, nk, h->pm_state.as<PmState>(), it);
    return REG_OK;
}

// One generic iteration of the chain; nothing waits on the host
static reg_status enqueue_pm_iteration(reg_handle* h) {
    const IterState* it = h->i_iter.as<IterState>();
    const reg_pm_chain& c = h->pm;
    const int64_t n = h->n, nk = n * (int64_t)c.knn;
    const PmCfg cfg = make_pm_cfg(h);
    int* kpos = h->pm_pos.as<int>();
    float* kd2 = h->pm_d2.as<float>();
    const unsigned blocks = (unsigned)((n + 15) / 16);
    const float4* src = h->s_xyz.as<float4>();
    if (c.knn <= 2)
        k_match_knn<2><<<blocks, 256, 0, h->stream>>>(h->grid, src, n, c.knn, it, kpos, kd2);
    else if (c.knn <= 4)
        k_match_knn<4><<<blocks, 256, 0, h->stream>>>(h->grid, src, n, c.knn, it, kpos, kd2);
    else if (c.knn <= 8)
        k_match_knn<8><<<blocks, 256, 0, h->stream>>>(h->grid, src, n, c.knn, it, kpos, kd2);
    else
        k_match_knn<16><<<blocks, 256, 0, h->stream>>>(h->grid, src, n, c.knn, it, kpos, kd2);
    if (cfg.use_trim) enqueue_pm_select(h, kd2, nk, h->prm.trim_ratio, 2);
    if (cfg.use_median) enqueue_pm_select(h, kd2, nk, 0.5f, 3);   // getDistsQuantile(0.5): the float index
    if (cfg.use_var) {
        const reg_status vs = enqueue_pm_var_trim(h, cfg, kd2, nk);
        if (vs != REG_OK) return vs;
    }
    if (c.use_robust) {
        // MAD: median(d2) at the integer index size / 2; berg: getDistsQuantile(0.5), the float index
        if (c.scale_estimator == REG_SCALE_MAD || c.scale_estimator == REG_SCALE_BERG)
            enqueue_pm_select(h, kd2, nk, 0.5f, 0, c.scale_estimator == REG_SCALE_MAD ? 1 : 0);
        if (c.scale_estimator == REG_SCALE_MAD) {
            k_pm_absdev<<<(unsigned)std::min<int64_t>(1024, grid_for(nk)), 256, 0, h->stream>>>(kd2, nk, h->pm_state.as<PmState>(),
                                                                                               h->pm_keys.as<float>(), it);
            enqueue_pm_select(h, h->pm_keys.as<float>(), nk, 0.5f, 1, 1);
        }
        k_pm_scale<<<1, 64, 0, h->stream>>>(h->pm_state.as<PmState>(), cfg, it);
    }
    const int lb = (int)std::min<int64_t>(kPmLinBlocks, grid_for(nk));
    const float4* snrm = h->has_snrm ? h->s_nrm.as<float4>() : nullptr;
    const float4* tnrm = h->has_tnrm ? h->t_nrm.as<float4>() : nullptr;
    if (c.minimizer == REG_PM_POINT_TO_POINT)
        k_pm_linearize<true><<<lb, 256, 0, h->stream>>>(src, snrm, n, it, kpos, kd2, h->t_pts.as<float4>(), tnrm, cfg,
                                                        h->pm_state.as<PmState>(), h->pm_w.as<float>(), h->pm_partials.as<double>());
    else
        k_pm_linearize<false><<<lb, 256, 0, h->stream>>>(src, snrm, n, it, kpos, kd2, h->t_pts.as<float4>(), tnrm, cfg,
                                                         h->pm_state.as<PmState>(), h->pm_w.as<float>(), h->pm_partials.as<double>());
    ++h->seq;
    const PmExtraCfg xc = make_pm_extra_cfg(h);
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(kXtBlocks, grid_for(n)));   // rows of the EqualityConstraints sums
    // the chain's update kernel, sequence h->seq, in the instantiation <extras, EqualityConstraints> the caller asks for;
    // finish = 1: the second launch of a sequence, behind the analysis kernels
    auto update = [&](bool extras, int p2p, int finish, XicpState* xicp, XtState* xt, const double* rows) {
        PmExtraState* xstate = extras ? h->pm_xstate.as<PmExtraState>() : nullptr;
        auto go = [&](auto kernel) {
            kernel<<<1, 256, 0, h->stream>>>(h->pm_partials.as<double>(), lb, h->i_iter.as<IterState>(), h->h_mirror.dev, h->seq,
                                             h->pm_state.as<PmState>(), p2p, cfg.use_trim, cfg.use_median, xc, xstate, finish, xicp,
                                             xt, rows, xt ? nb : 0);
        };
        if (xt)
            go(k_pm_update<true, true>);
        else if (extras)
            go(k_pm_update<true>);
        else
            go(k_pm_update<false>);
    };
    const int p2p = c.minimizer == REG_PM_POINT_TO_POINT ? 1 : 0;
    if (h->xt_on) {
        // EqualityConstraints: the analysis of THIS iteration between two launches of the update kernel; the partial-sums
        // kernel is always enqueued and gated on the device (kernels_xicp_ternary.hpp)
        XtState* xt = h->xt_state.as<XtState>();
        double* rows = h->xt_rows.as<double>();
        const float* kw = h->pm_w.as<float>();
        update(true, 0, 0, nullptr, xt, rows);
        k_xt_center<<<nb, 256, 0, h->stream>>>(src, n, it, kpos, kw, xt, rows);
        k_xt_detect<<<nb, 256, 0, h->stream>>>(src, n, it, kpos, kw, tnrm, xt, rows);
        k_xt_decide<<<1, 256, 0, h->stream>>>(it, xt, rows, nb);
        k_xt_partial<<<nb, 256, 0, h->stream>>>(src, n, it, kpos, kw, h->t_pts.as<float4>(), tnrm, xt, rows);
        update(true, 0, 1, nullptr, xt, rows);
    } else if (pm_chain_has_extras(&c))
        update(true, p2p, 0, h->prm.use_xicp ? h->i_xicp.as<XicpState>() : nullptr, nullptr, nullptr);
    else
        update(false, p2p, 0, nullptr, nullptr, nullptr);
    if (h->xicp_pending) {
        // R8x, first iteration (only a chain of Bound / covariance over the plain filters runs with use_xicp: knn 1, so
        // the chain's N x 1 buffers are the plain loop's): the information sums, then decide + solve + update
        h->xicp_pending = false;
        launch_xicp_center(h, kpos, h->pm_w.as<float>());
        launch_xicp_detect(h, kpos, h->pm_w.as<float>());
        update(true, 0, 1, h->i_xicp.as<XicpState>(), nullptr, nullptr);
    }
    HIPCHK(h, hipGetLastError());
    h->have_match = true;
    h->pm_have_match = true;
    return REG_OK;
}

// Workgroups of the post-loop reductions over nk pairs
static inline int pmx_blocks(int64_t nk) { return (int)std::max<int64_t>(1, std::min<int64_t>(kPmxBlocks, grid_for(nk))); }

// PointToPlaneWithCovErrorMinimizer::estimateCovariance on the buffers of the last iteration (kernels_pmextras.hpp): two
// passes over the pairs and two single-workgroup reductions; the result block is copied to the host.
static reg_status evaluate_pm_covariance(reg_handle* h) {
    const int64_t n = h->n, nk = n * (int64_t)h->pm.knn;
    const int nb = pmx_blocks(nk);
    HIPCHK(h, h->pm_xrows.reserve((size_t)kPmxBlocks * kPmxCovSums * 8));
    HIPCHK(h, h->pm_xmeans.reserve(kPmxRow * 8));
    HIPCHK(h, h->pm_xcov.reserve(sizeof(PmCovOut)));
    const IterState* it = h->i_iter.as<IterState>();
    const float4* src = h->s_xyz.as<float4>();
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    k_pmx_pair_means<<<nb, 256, 0, h->stream>>>(src, n, h->pm.knn, it, h->pm_pos.as<int>(), h->pm_w.as<float>(),
                                                h->t_pts.as<float4>(), h->pm_xrows.as<double>());
    k_pmx_reduce_rows<<<1, 256, 0, h->stream>>>(h->pm_xrows.as<double>(), nb, h->pm_xmeans.as<double>());
    k_pmx_cov_terms<<<nb, 256, 0, h->stream>>>(src, n, h->pm.knn, it, h->pm_pos.as<int>(), h->pm_w.as<float>(),
                                               h->t_pts.as<float4>(), h->t_nrm.as<float4>(), h->pm_xmeans.as<double>(),
                                               h->pm_xstate.as<PmExtraState>(), h->pm_xrows.as<double>());
    k_pmx_cov_finish<<<1, 256, 0, h->stream>>>(h->pm_xrows.as<double>(), nb, h->pm_xmeans.as<double>(), h->pm.sensor_std_dev,
                                               h->pm_xcov.as<PmCovOut>());
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipMemcpyAsync(&h->pm_cov_host, h->pm_xcov.p, sizeof(PmCovOut), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    (void)hipEventElapsedTime(&h->pm_cov_ms, h->ev0, h->ev1);
    HIPCHK(h, hipGetLastError());
    h->pm_cov_valid = true;
    return REG_OK;
}

// reg_register for a handle with a chain: prepare as the plain loop (centred frames), then generic iterations only,
// at most lookahead sequences in flight, the same sequence limit as the plain loop
static reg_status register_pm(reg_handle* h, const float* Ti, float T_out[16], reg_result* res) {
    if (pm_needs_tnrm(h) && !h->has_tnrm && h->m > 0) {
        h->err = "InvalidField: this chain needs the `normals` descriptor on the reference";
        return REG_MISSING_FIELD;
    }
    reg_status s = check_ready(h, false);
    if (s != REG_OK) return s;
    const int64_t nk = h->n * (int64_t)h->pm.knn;
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, h->pm_pos.reserve((size_t)nk * 4));
    HIPCHK(h, h->pm_d2.reserve((size_t)nk * 4));
    HIPCHK(h, h->pm_w.reserve((size_t)nk * 4));
    HIPCHK(h, h->pm_keys.reserve((size_t)nk * 4));
    HIPCHK(h, h->pm_partials.reserve((size_t)kPmLinBlocks * kSums * 8));
    HIPCHK(h, h->pm_sel.reserve(sizeof(SelectState)));
    if (!h->pm_hist.p) {
        HIPCHK(h, h->pm_hist.reserve(3 * 2048 * 4));
        HIPCHK(h, hipMemsetAsync(h->pm_hist.p, 0, 3 * 2048 * 4, h->stream));
    }
    if (h->pm.use_var_trimmed) {
        HIPCHK(h, h->pm_sorted.reserve((size_t)nk * 4));
        HIPCHK(h, h->pm_var.reserve(pm_var_bytes(nk)));
        // storage for the sort of enqueue_pm_var_trim, which runs inside the loop on these arguments
        REGCHK(tmp_reserve(h, h->pm_sort_tmp, h->pm_sort_bytes, [&](void* t, size_t& b) {
            return rocprim::radix_sort_keys(t, b, h->pm_d2.as<uint32_t>(), h->pm_sorted.as<uint32_t>(), (size_t)nk, 0, 32, h->stream);
        }));
    }
    const bool extras = pm_chain_has_extras(&h->pm) || h->xt_on;
    h->pm_x_valid = false;
    h->pm_cov_valid = false;
    h->xt_valid = false;
    if (extras) {
        // P = identity and clear flags, as the reference's per-registration local (PointMatcher.h:645)
        HIPCHK(h, h->pm_xstate.reserve(sizeof(PmExtraState)));
        std::memset(&h->pm_xhost, 0, sizeof(PmExtraState));
        for (int k = 0; k < 6; ++k) h->pm_xhost.P[7 * k] = 1.0;
        HIPCHK(h, hipMemcpyAsync(h->pm_xstate.p, &h->pm_xhost, sizeof(PmExtraState), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    float T_start[16];
    m4_identity(T_start);
    std::memcpy(h->T_init, Ti, 64);
    IterState st0;
    s = build_iter_state(h, T_start, 1, &st0);
    if (s != REG_OK) return s;
    st0.use_trim = 0;   // the chain's own selects; no band prediction
    if (h->xt_on) {
        HIPCHK(h, h->xt_state.reserve(sizeof(XtState)));
        HIPCHK(h, h->xt_rows.reserve(kXtRowsTotal * 8));
        XtState& x = h->xt_host;
        std::memset(&x, 0, sizeof(XtState));
        x.high_thr = h->xt.high_information;
        x.enough_thr = h->xt.enough_information;
        x.insufficient_thr = h->xt.insufficient_information;
        x.cos_min = (float)std::cos((double)h->xt.min_alignment_angle_deg * 3.14159265358979323846 / 180.0);
        x.cos_strong = (float)std::cos((double)h->xt.strong_alignment_angle_deg * 3.14159265358979323846 / 180.0);
        xicp_frame_change(h, x.Trd);
        x.sane = 1;
        HIPCHK(h, hipMemcpyAsync(h->xt_state.p, &x, sizeof(XtState), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    s = prepare_rowmajor(h, Ti, nullptr, 0, &st0);
    if (s != REG_OK) return s;
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    const int limit = sequence_limit(h->prm);
    const int kAhead = std::max(1, h->env.lookahead);
    const HostMirror* mir = h->h_mirror;
    Lookahead la{h, h->seq, h->seq};
    for (;;) {
        la.look();
        if (la.any && mir->done) break;
        la.acknowledge();
        if (la.completed + la.inflight < limit && la.inflight < kAhead) {
            s = enqueue_pm_iteration(h);
            if (s != REG_OK) return s;
            continue;
        }
        if (la.inflight == 0) break;
        s = la.wait_next();
        if (s != REG_OK) return s;
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    (void)hipEventElapsedTime(&res->loop_ms, h->ev0, h->ev1);
    HIPCHK(h, hipGetLastError());
    if (extras) {
        HIPCHK(h, hipMemcpy(&h->pm_xhost, h->pm_xstate.p, sizeof(PmExtraState), hipMemcpyDeviceToHost));
        h->pm_x_valid = true;
    }
    if (h->xt_on) {
        HIPCHK(h, hipMemcpy(&h->xt_host, h->xt_state.p, sizeof(XtState), hipMemcpyDeviceToHost));
        h->xt_valid = true;
    }
    // the detection failed (SolutionRemapping / EqualityConstraints): the prior is returned as it came in (reg_register copied it
    // to T_out), nothing is composed
    const bool prior = extras && h->pm_xhost.returned_prior;
    const bool xicp = h->prm.use_xicp || h->xt_on;
    const reg_status ms = write_result(h, xicp, /*xicp_sums=*/xicp, (double)h->n, /*mirror_seen=*/true, prior ? nullptr : T_out, res);
    // chain counts (kernels_pmchain.hpp: 29 finite pairs, 30 sum d2 over the inliers, 31 inliers), the minimizer's system
    const double* sums = mir->sums;
    res->n_inliers = (int64_t)llround(sums[31]);
    res->n_matched = (int64_t)llround(sums[29]);
    res->fitness = sums[31] / ((double)h->n * (double)h->pm.knn);
    res->inlier_rmse = sums[31] > 0 ? std::sqrt(sums[30] / sums[31]) : 0.0;
    sums_to_system(sums, h->pm.minimizer == REG_PM_POINT_TO_POINT ? REG_COST_O3D_P2P : REG_COST_P2PL, res->H_last, res->b_last);
    h->pm_last_error = res->error;
    if (ms == REG_OUT_OF_BOUNDS) {
        // BoundTransformationChecker threw: T_out stays T_init (set by reg_register), the offending pose is reported
        row_to_col(mir->T, res->T_iter_last);
        row_to_col(mir->T_prev, res->T_iter_prev);
        char msg[160];
        snprintf(msg, sizeof(msg), "limit out of bounds: rot: %g/%g tr: %g/%g", (double)h->pm_xhost.bound_rot,
                 (double)h->pm.max_rotation_norm, (double)h->pm_xhost.bound_trans, (double)h->pm.max_translation_norm);
        h->err = msg;
        return REG_OUT_OF_BOUNDS;
    }
    if (ms != REG_OK) {
        h->err = "ErrorMinimizer: no point to minimize (or no finite distance for a statistic of the chain)";
        return ms;
    }
    if (!prior && h->pm.with_cov && h->pm_xhost.have_dT) {
        s = evaluate_pm_covariance(h);
        if (s != REG_OK) return s;
        res->prof_ms[2] = h->pm_cov_ms;   // device time of the covariance evaluation, outside loop_ms
        res->prof_launches[2] = 4;
    }
    return REG_OK;
}

static reg_status write_pm_state(reg_handle* h) {
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, h->pm_state.reserve(sizeof(PmState)));
    PmState ps;
    std::memset(&ps, 0, sizeof(ps));
    ps.scale = 0.f;        // RobustOutlierFilter's constructor: scale(0.0), iteration(1)
    ps.iteration = 1;
    HIPCHK(h, hipMemcpyAsync(h->pm_state.p, &ps, sizeof(ps), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

extern "C" {

void reg_default_pm_chain(reg_pm_chain* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(reg_pm_chain);
    c->knn = 1;
    c->minimizer = REG_PM_POINT_TO_PLANE;
    c->use_robust = 0;
    // RobustOutlierFilter defaults (OutlierFiltersImpl.h:230-244)
    c->robust_fct = REG_ROBUST_CAUCHY;
    c->tuning = 1.0f;
    c->scale_estimator = REG_SCALE_MAD;
    c->nb_iter_for_scale = 0;
    c->distance_type = REG_DIST_POINT2POINT;
    c->approximation = std::numeric_limits<float>::infinity();
    // MinDist / MedianDist / VarTrimmedDist defaults (OutlierFiltersImpl.h:96-101,115-120,153-160)
    c->use_min_dist_filter = 0;
    c->outlier_min_dist = 1.0f;
    c->use_median_dist = 0;
    c->median_factor = 3.0f;
    c->use_var_trimmed = 0;
    c->var_min_ratio = 0.05f;
    c->var_max_ratio = 0.99f;
    c->var_lambda = 2.35f;
    // PointToPlaneWithCov.h:75, TransformationCheckersImpl.h (BoundTransformationChecker), SolutionRemapping off
    c->with_cov = 0;
    c->sensor_std_dev = 0.01f;
    c->use_bound = 0;
    c->max_rotation_norm = 1.0f;
    c->max_translation_norm = 1.0f;
    c->bound_after_counter = 0;
    c->degeneracy_method = REG_DEGENERACY_NONE;
    c->sr_threshold = 0.f;
    c->sr_use2019 = 0;
}

static bool pm_ratio_ok(float r) { return r >= 1e-7f && r <= 1.f; }

reg_status reg_check_pm_chain(const reg_params* p, const reg_pm_chain* c_in) {
    if (!p || !c_in) return REG_BAD_ARGUMENT;
    reg_pm_chain full;
    if (!pm_chain_read(c_in, &full)) return REG_BAD_ARGUMENT;
    const reg_pm_chain* c = &full;
    if (p->cost != REG_COST_P2PL) return REG_BAD_ARGUMENT;
    if (c->knn < 1 || c->knn > kPmMaxKnn) return REG_BAD_ARGUMENT;
    if (c->minimizer != REG_PM_POINT_TO_PLANE && c->minimizer != REG_PM_POINT_TO_POINT) return REG_BAD_ARGUMENT;
    if (c->use_robust) {
        if (c->robust_fct < REG_ROBUST_CAUCHY || c->robust_fct > REG_ROBUST_STUDENT) return REG_BAD_ARGUMENT;
        if (!(c->tuning >= 1e-7f)) return REG_BAD_ARGUMENT;                       // "tuning" range [1e-7, inf]
        if (c->scale_estimator == REG_SCALE_STD) return REG_UNSUPPORTED;          // see include/o3dslam_reg.h
        if (c->scale_estimator < REG_SCALE_NONE || c->scale_estimator > REG_SCALE_BERG) return REG_BAD_ARGUMENT;
        if (c->nb_iter_for_scale < 0 || c->nb_iter_for_scale > 100) return REG_BAD_ARGUMENT;
        if (c->distance_type != REG_DIST_POINT2POINT && c->distance_type != REG_DIST_POINT2PLANE) return REG_BAD_ARGUMENT;
        if (!(c->approximation >= 0.f)) return REG_BAD_ARGUMENT;                  // [0, inf]
    }
    // parameter ranges of the reference ("minDist" / "factor" [1e-7, inf), ratios [1e-7, 1]); NaN fails every test
    if (c->use_min_dist_filter && !(c->outlier_min_dist >= 1e-7f && c->outlier_min_dist < INFINITY)) return REG_BAD_ARGUMENT;
    if (c->use_median_dist && !(c->median_factor >= 1e-7f && c->median_factor < INFINITY)) return REG_BAD_ARGUMENT;
    if (c->use_var_trimmed) {
        if (!pm_ratio_ok(c->var_min_ratio) || !pm_ratio_ok(c->var_max_ratio) || !std::isfinite(c->var_lambda))
            return REG_BAD_ARGUMENT;
        if (c->var_min_ratio >= c->var_max_ratio) return REG_BAD_ARGUMENT;   // the filter's constructor throws
    }
    // covariance / Bound / SolutionRemapping: NaN fails every range test
    if (c->with_cov) {
        if (!(c->sensor_std_dev >= 0.f && c->sensor_std_dev < INFINITY)) return REG_BAD_ARGUMENT;   // [0, inf)
        if (c->minimizer == REG_PM_POINT_TO_POINT) return REG_UNSUPPORTED;   // PointToPointWithCov: see include/o3dslam_reg.h
    }
    if (c->use_bound) {
        if (!(c->max_rotation_norm >= 0.f) || !(c->max_translation_norm >= 0.f)) return REG_BAD_ARGUMENT;   // [0, inf]
    }
    if (c->degeneracy_method != REG_DEGENERACY_NONE) {
        if (c->degeneracy_method != REG_DEGENERACY_SOLUTION_REMAPPING) return REG_BAD_ARGUMENT;
        if (c->sr_threshold != c->sr_threshold) return REG_BAD_ARGUMENT;
        if (p->use_xicp) return REG_BAD_ARGUMENT;                            // two degeneracy methods at once
        if (c->minimizer == REG_PM_POINT_TO_POINT) return REG_UNSUPPORTED;   // the reference warns and skips the detection
    }
    // X-ICP runs with a chain only when the chain is the plain loop plus the Bound checker and / or the covariance
    if (p->use_xicp && !pm_chain_is_default(c)) {
        reg_pm_chain plain = *c;
        plain.with_cov = 0;
        plain.use_bound = 0;
        if (!pm_chain_is_default(&plain)) return REG_UNSUPPORTED;
    }
    return REG_OK;
}

reg_status reg_set_pm_chain(reg_handle* h, const reg_pm_chain* c) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    reg_pm_chain nc;
    if (c) {
        const reg_status s = reg_check_pm_chain(&h->prm, c);
        if (s != REG_OK) return s;
        (void)pm_chain_read(c, &nc);
    } else {
        reg_default_pm_chain(&nc);
    }
    if (h->xt_on) {
        // the pair (EqualityConstraints, chain) must stay valid: otherwise nothing changes
        const reg_status s = reg_check_ternary_xicp(&h->prm, &nc, &h->xt);
        if (s != REG_OK) {
            h->err = "reg_set_pm_chain: this chain does not run with EqualityConstraints (reg_set_ternary_xicp)";
            return s;
        }
    }
    const bool on = !pm_chain_is_default(&nc) || h->xt_on;
    const reg_pm_chain old = h->pm;
    const bool old_on = h->pm_on;
    h->pm = nc;
    h->pm_on = on;
    // a reference set without normals (allowed for a chain that reads none) cannot serve a chain that needs them
    if (h->m > 0 && !h->has_tnrm && (!on || pm_needs_tnrm(h))) {
        h->pm = old;
        h->pm_on = old_on;
        h->err = "InvalidField: the reference was set without normals; this chain needs them";
        return REG_MISSING_FIELD;
    }
    h->have_match = false;   // the buffers of the last iteration belong to the previous chain
    h->pm_have_match = false;
    return write_pm_state(h);
}

void reg_default_ternary_xicp(reg_ternary_xicp* t) {
    std::memset(t, 0, sizeof(*t));
    t->struct_size = (int32_t)sizeof(reg_ternary_xicp);
    t->enabled = 0;
    t->high_information = 250.f;           // icp.yaml:56-67
    t->enough_information = 180.f;
    t->insufficient_information = 35.f;
    t->min_alignment_angle_deg = 80.f;
    t->strong_alignment_angle_deg = 45.f;
}

static bool ternary_ranges_ok(const reg_ternary_xicp* t) {
    if (t->struct_size != (int32_t)sizeof(reg_ternary_xicp)) return false;
    const float hi = t->high_information, en = t->enough_information, in = t->insufficient_information;
    if (!std::isfinite(hi) || !std::isfinite(en) || !std::isfinite(in)) return false;
    if (!(in <= en && en <= hi)) return false;
    const float a = t->min_alignment_angle_deg, b = t->strong_alignment_angle_deg;
    return a > 0.f && a <= 90.f && b > 0.f && b <= 90.f;   // NaN fails
}

reg_status reg_check_ternary_xicp(const reg_params* p, const reg_pm_chain* c_in, const reg_ternary_xicp* t) {
    if (!p || !t) return REG_BAD_ARGUMENT;
    if (!ternary_ranges_ok(t)) return REG_BAD_ARGUMENT;
    reg_pm_chain full;
    if (c_in) {
        if (!pm_chain_read(c_in, &full)) return REG_BAD_ARGUMENT;
    } else {
        reg_default_pm_chain(&full);
    }
    if (!t->enabled) return REG_OK;
    if (p->use_xicp || full.degeneracy_method != REG_DEGENERACY_NONE) return REG_BAD_ARGUMENT;   // two methods at once
    if (p->cost != REG_COST_P2PL) return REG_UNSUPPORTED;
    if (full.knn != 1 || full.use_robust || full.minimizer != REG_PM_POINT_TO_PLANE || full.with_cov) return REG_UNSUPPORTED;
    return REG_OK;
}

reg_status reg_set_ternary_xicp(reg_handle* h, const reg_ternary_xicp* t) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    reg_ternary_xicp nt;
    reg_default_ternary_xicp(&nt);
    reg_pm_chain chain = h->pm;
    if (!h->pm_on) reg_default_pm_chain(&chain);   // no chain set: the default chain (the chain loop reads it)
    if (t) {
        const reg_status s = reg_check_ternary_xicp(&h->prm, &chain, t);
        if (s != REG_OK) {
            h->err = "reg_set_ternary_xicp: the method does not run with these parameters / this chain (include/o3dslam_reg.h)";
            return s;
        }
        nt = *t;
    }
    const bool on = nt.enabled != 0;
    if (on && h->m > 0 && !h->has_tnrm) {
        h->err = "InvalidField: the reference was set without normals; EqualityConstraints needs them";
        return REG_MISSING_FIELD;
    }
    // the robust state first: a device failure there leaves the handle as it was
    const reg_status ws = write_pm_state(h);
    if (ws != REG_OK) return ws;
    h->pm = chain;
    h->xt = nt;
    h->xt_on = on;
    h->xt_valid = false;
    h->pm_on = on || !pm_chain_is_default(&chain);
    h->have_match = false;   // the buffers of the last iteration belong to the previous configuration
    h->pm_have_match = false;
    return REG_OK;
}

reg_status reg_get_ternary_xicp(reg_handle* h, reg_ternary_xicp_result* out) {
    if (!h || !out || out->struct_size != (int32_t)sizeof(reg_ternary_xicp_result)) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!h->xt_on || !h->pm_have_match || !h->xt_valid || !h->xt_host.valid) return REG_NOT_CONFIGURED;
    const XtState& x = h->xt_host;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = (int32_t)sizeof(reg_ternary_xicp_result);
    out->iteration = x.iteration;
    out->sane = x.sane;
    out->n_pairs = (int64_t)x.n_pairs;
    for (int k = 0; k < 6; ++k) {
        out->category[k] = x.cat[k];
        out->combined[k] = x.comb[k];
        out->high[k] = x.high[k];
        out->n_combined[k] = (int64_t)x.n_comb[k];
        out->n_high[k] = (int64_t)x.n_high[k];
        out->constraint[k] = x.constraint[k];
        for (int c = 0; c < 9; ++c) out->partial_sums[k][c] = x.psums[9 * k + c];
    }
    for (int k = 0; k < 9; ++k) {
        out->eigenvectors[0][k] = x.vo[k];
        out->eigenvectors[1][k] = x.vo[9 + k];
    }
    return REG_OK;
}

reg_status reg_host_ternary_decide(const double combined[6], const double high[6], const int64_t n_combined[6],
                                   const int64_t n_high[6], int64_t n_pairs, const reg_ternary_xicp* params,
                                   int32_t category[6], int32_t* sane) {
    if (!combined || !high || !n_combined || !n_high || !params || !category) return REG_BAD_ARGUMENT;
    if (!ternary_ranges_ok(params)) return REG_BAD_ARGUMENT;
    long long nc[6], nh[6];
    int cat[6];
    for (int k = 0; k < 6; ++k) {
        nc[k] = (long long)n_combined[k];
        nh[k] = (long long)n_high[k];
    }
    const int ok = xicp_ternary_decide(combined, high, nc, nh, (long long)n_pairs, params->high_information,
                                       params->enough_information, params->insufficient_information, cat);
    for (int k = 0; k < 6; ++k) category[k] = cat[k];
    if (sane) *sane = ok;
    return REG_OK;
}

reg_status reg_host_partial_constraint(const double sums9[9], const float v[3], float* value) {
    if (!sums9 || !v || !value) return REG_BAD_ARGUMENT;
    const float val = xicp_partial_constraint(sums9, v);
    *value = val;
    return std::isfinite(val) ? REG_OK : REG_NO_CORRESPONDENCES;
}

int reg_host_solve6_xicp_rhs(const float A[36], const float b[6], const int32_t flags[6], const float rhs[6], float x[6]) {
    int f[6];
    for (int k = 0; k < 6; ++k) f[k] = flags[k];
    return solve6_xicp_rhs(A, b, f, rhs, x);
}

reg_status reg_get_robust_state(const reg_handle* h, float* scale, int32_t* iteration) {
    if (!h) return REG_BAD_ARGUMENT;
    PmState ps;
    std::memset(&ps, 0, sizeof(ps));
    ps.iteration = 1;
    if (h->pm_state.p) {
        if (!h->device_ok || hipSetDevice(h->prm.device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
            hipMemcpy(&ps, h->pm_state.p, sizeof(ps), hipMemcpyDeviceToHost) != hipSuccess)
            return REG_DEVICE_ERROR;
    }
    if (scale) *scale = ps.scale;
    if (iteration) *iteration = ps.iteration;
    return REG_OK;
}

reg_status reg_get_var_trim(const reg_handle* h, float* ratio, int64_t* index, int64_t* n_total) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!h->pm_on || !h->pm.use_var_trimmed || !h->pm_have_match || !h->pm_state.p) return REG_NOT_CONFIGURED;
    PmState ps;
    if (hipSetDevice(h->prm.device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        hipMemcpy(&ps, h->pm_state.p, sizeof(ps), hipMemcpyDeviceToHost) != hipSuccess)
        return REG_DEVICE_ERROR;
    if (!ps.var_valid) return REG_NOT_CONFIGURED;
    if (ratio) *ratio = ps.var_ratio;
    if (index) *index = (int64_t)ps.var_k;
    if (n_total) *n_total = (int64_t)ps.var_n;
    return REG_OK;
}

reg_status reg_get_covariance(const reg_handle* h, float cov[36], int32_t* rank) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!h->pm_on || !h->pm.with_cov || !h->pm_have_match || !h->pm_cov_valid) return REG_NOT_CONFIGURED;
    if (cov) std::memcpy(cov, h->pm_cov_host.cov, sizeof(float) * 36);
    if (rank) *rank = h->pm_cov_host.rank;
    return REG_OK;
}

reg_status reg_get_covariance_sums(const reg_handle* h, double H[21], double M[21]) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!h->pm_on || !h->pm.with_cov || !h->pm_have_match || !h->pm_cov_valid) return REG_NOT_CONFIGURED;
    if (H) std::memcpy(H, h->pm_cov_host.sums, sizeof(double) * 21);
    if (M) std::memcpy(M, h->pm_cov_host.sums + 21, sizeof(double) * 21);
    return REG_OK;
}

reg_status reg_host_censi_covariance(const double H[21], const double M[21], float sigma, float cov[36], int32_t* rank) {
    if (!H || !M || !cov) return REG_BAD_ARGUMENT;
    const int r = pmx_censi_covariance(H, M, (double)sigma, cov);
    if (rank) *rank = r;
    return REG_OK;
}

reg_status reg_get_minimizer_stats(reg_handle* h, reg_minimizer_stats* out) {
    if (!h || !out || out->struct_size != (int32_t)sizeof(reg_minimizer_stats)) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    // a chain registration reads the chain's N x knn weights; the plain point-to-plane loop its N weights
    const int knn = h->pm_on ? h->pm.knn : 1;
    const int64_t n = h->n, nk = n * (int64_t)knn;
    const bool chain_ok = h->pm_on && h->pm_have_match && h->pm_w.cap >= (size_t)nk * 4;
    const bool plain_ok = !h->pm_on && h->prm.cost == REG_COST_P2PL && h->have_match && h->i_w.cap >= (size_t)n * 4;
    if (nk <= 0 || (!chain_ok && !plain_ok)) {
        h->err = "no point-to-plane registration has run on this reading";
        return REG_NOT_CONFIGURED;
    }
    const float* kw = h->pm_on ? h->pm_w.as<float>() : h->i_w.as<float>();
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, h->pm_xrows.reserve((size_t)kPmxBlocks * kPmxCovSums * 8));
    HIPCHK(h, h->pm_xmeans.reserve(kPmxRow * 8));
    const int nb = pmx_blocks(n);
    k_pmx_stats<<<nb, 256, 0, h->stream>>>(kw, n, knn, h->pm_xrows.as<double>());
    k_pmx_reduce_rows<<<1, 256, 0, h->stream>>>(h->pm_xrows.as<double>(), nb, h->pm_xmeans.as<double>());
    double t[kPmxRow];
    HIPCHK(h, hipMemcpyAsync(t, h->pm_xmeans.p, sizeof(t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    out->returned_prior = (h->pm_x_valid && h->pm_xhost.returned_prior) ? 1 : 0;
    out->point_used_ratio = t[1] / (double)nk;
    out->weighted_point_used_ratio = t[0] / (double)nk;
    out->overlap = out->weighted_point_used_ratio;
    out->residual_error = h->pm_on ? h->pm_last_error : h->h_mirror->sums[27];
    out->n_rejected_matches = (int64_t)llround(t[2]);
    out->n_rejected_points = (int64_t)llround(t[3]);
    return REG_OK;
}

reg_status reg_get_degeneracy(const reg_handle* h, int32_t categories[6], float eigenvalues[6], float* condition_number) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!h->pm_on || h->pm.degeneracy_method == REG_DEGENERACY_NONE || !h->pm_have_match || !h->pm_x_valid ||
        !h->pm_xhost.sr_valid)
        return REG_NOT_CONFIGURED;
    for (int k = 0; k < 6; ++k) {
        if (categories) categories[k] = h->pm_xhost.cat[k];
        if (eigenvalues) eigenvalues[k] = h->pm_xhost.eig[k];
    }
    if (condition_number) *condition_number = h->pm_xhost.cond;
    return REG_OK;
}

reg_status reg_get_bound(const reg_handle* h, float* rotation, float* translation) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!h->pm_on || !h->pm.use_bound || !h->pm_have_match || !h->pm_x_valid || !h->pm_xhost.bound_valid)
        return REG_NOT_CONFIGURED;
    if (rotation) *rotation = h->pm_xhost.bound_rot;
    if (translation) *translation = h->pm_xhost.bound_trans;
    return REG_OK;
}

reg_status reg_host_solution_remap(const float A[36], float threshold, int use2019, const double P_in[36], double P_out[36],
                                   int32_t categories[6], float eigenvalues[6]) {
    if (!A || !P_in || !P_out) return REG_BAD_ARGUMENT;
    int cat[6];
    float eig[6], cond;
    const int prior = pmx_solution_remap(A, threshold, use2019, P_in, P_out, cat, eig, &cond);
    for (int k = 0; k < 6; ++k) {
        if (categories) categories[k] = cat[k];
        if (eigenvalues) eigenvalues[k] = eig[k];
    }
    return prior ? REG_NO_CORRESPONDENCES : REG_OK;
}

reg_status reg_host_var_trim(const float* d2, int64_t n, float minRatio, float maxRatio, float lambda, int64_t* index,
                             float* ratio, float* limit) {
    if (n < 0 || (n > 0 && !d2)) return REG_BAD_ARGUMENT;
    if (!pm_ratio_ok(minRatio) || !pm_ratio_ok(maxRatio) || minRatio >= maxRatio || !std::isfinite(lambda)) return REG_BAD_ARGUMENT;
    std::vector<float> fin;   // the finite distances, zeros included (getDistsQuantile)
    fin.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        if (d2[i] != INFINITY) fin.push_back(d2[i]);
    std::sort(fin.begin(), fin.end());
    const int64_t nz = std::upper_bound(fin.begin(), fin.end(), 0.f) - fin.begin();
    const int64_t m = (int64_t)fin.size() - nz;   // v = fin[nz ...]
    if (m <= 0) return REG_NO_CORRESPONDENCES;
    int64_t lo, hi;
    pm_var_range(n, m, minRatio, maxRatio, &lo, &hi);
    const double two_lambda = 2.0 * (double)lambda;
    int64_t k = m - 1;
    if (lo < hi) {
        double S = 0.0, best = 0.0;
        k = -1;
        for (int64_t j = 0; j < hi; ++j) {
            S += (double)fin[(size_t)(nz + j)];
            if (j < lo) continue;
            const double f = pm_var_frms(S, j, n, two_lambda);
            if (k < 0 || f < best) {
                best = f;
                k = j;
            }
        }
    }
    const float r = (float)k / (float)n;
    if (index) *index = k;
    if (ratio) *ratio = r;
    if (limit) *limit = fin[pm_quantile_rank((uint32_t)fin.size(), r)];
    return REG_OK;
}

reg_status reg_get_correspondences_k(reg_handle* h, int32_t knn, int32_t* ids, float* d2, float* w) {
    reg_status s = check_ready(h, true);
    if (s != REG_OK) return s;
    if (!h->pm_on) {
        if (knn != 1) return REG_BAD_ARGUMENT;
        return reg_get_correspondences(h, ids, d2, w);
    }
    if (knn != h->pm.knn) {
        h->err = "reg_get_correspondences_k: knn differs from the chain's";
        return REG_BAD_ARGUMENT;
    }
    const int64_t nk = h->n * (int64_t)knn;
    if (!h->pm_have_match || h->pm_pos.cap < (size_t)nk * 4 || h->pm_d2.cap < (size_t)nk * 4 || h->pm_w.cap < (size_t)nk * 4) {
        h->err = "no chain registration has run on this reading";
        return REG_NOT_CONFIGURED;
    }
    HIPCHK(h, hipSetDevice(h->prm.device));
    HIPCHK(h, h->i_ids.reserve((size_t)nk * 4));
    HIPCHK(h, h->i_tmpf.reserve((size_t)nk * 8));
    int32_t* d_ids = h->i_ids.as<int32_t>();
    float* d_d2 = h->i_tmpf.as<float>();
    float* d_w = h->i_tmpf.as<float>() + nk;
    k_pm_unpermute<<<grid_for(nk), 256, 0, h->stream>>>(h->pm_pos.as<int>(), h->pm_d2.as<float>(), h->pm_w.as<float>(),
                                                        h->t_pts.as<float4>(), h->n, knn, h->perm, ids ? d_ids : nullptr,
                                                        d2 ? d_d2 : nullptr, w ? d_w : nullptr);
    if (ids) HIPCHK(h, hipMemcpyAsync(ids, d_ids, (size_t)nk * 4, hipMemcpyDeviceToHost, h->stream));
    if (d2) HIPCHK(h, hipMemcpyAsync(d2, d_d2, (size_t)nk * 4, hipMemcpyDeviceToHost, h->stream));
    if (w) HIPCHK(h, hipMemcpyAsync(w, d_w, (size_t)nk * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return REG_OK;
}

reg_status reg_host_robust_weights(int32_t fct, float tuning, float scale, float approximation, const float* d2_or_e,
                                   int64_t n, float* w) {
    if (fct < REG_ROBUST_CAUCHY || fct > REG_ROBUST_STUDENT || n < 0 || (n > 0 && (!d2_or_e || !w))) return REG_BAD_ARGUMENT;
    const float sq = std::isinf(approximation) ? INFINITY : (float)((double)approximation * (double)approximation);
    for (int64_t i = 0; i < n; ++i) w[i] = pm_robust_weight(fct, tuning, scale, sq, d2_or_e[i]);
    return REG_OK;
}

reg_status reg_host_pm_p2p_update(const double sums[32], double T_update[16], int32_t* rank) {
    if (!sums || !T_update) return REG_BAD_ARGUMENT;
    if (!(sums[28] > 0.0)) return REG_NO_CORRESPONDENCES;
    double U[16];
    const int r = o3d_update_p2p(sums, U);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) T_update[4 * j + i] = U[4 * i + j];   // row-major -> column-major
    if (rank) *rank = r;
    return REG_OK;
}

}  // extern "C"
