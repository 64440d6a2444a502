// host_launch.hpp -- the ONE launch site of every kernel of the registration loop: what a call site passes is what varies
// between the callers (the plain loop, the chain, the phases of reg_dist_phase); the rest is taken from the handle here.
// Part of the single translation unit reg_core.hip (included there, before host_loop.hpp; not a standalone header).
#pragma once

static void prof_mark(reg_handle* h, int kind, bool start) {
    if (!h->profiling) return;
    Event e;
    if (e.create() != hipSuccess) return;
    (void)hipEventRecord(e, h->stream);
    h->prof_ev.push_back(std::move(e));
    if (start) h->prof_kind.push_back(kind);
}

// Launch with the kernel's own begin / end timestamps when the loop is being profiled (hipExtLaunchKernelGGL attaches
// the two events to the dispatch packet itself: the same interval rocprofv3 --kernel-trace reports, without the
// gaps that events recorded around a launch include).  kind < 0: a plain launch whatever the handle profiles.
template <class K, class... A>
static void launch_timed(reg_handle* h, int kind, K kernel, dim3 grid, dim3 block, size_t lds, A... args) {
    Event e0, e1;
    if (kind < 0 || !h->profiling || e0.create() != hipSuccess || e1.create() != hipSuccess) {
        hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, args...);
        return;
    }
    hipExtLaunchKernelGGL(kernel, grid, block, lds, h->stream, e0, e1, 0, args...);
    h->prof_ev.push_back(std::move(e0));
    h->prof_ev.push_back(std::move(e1));
    h->prof_kind.push_back(kind);
}

static FilterCfg make_filter_cfg(const reg_handle* h, int trim_mode) {
    FilterCfg f;
    f.use_trim = trim_mode;
    f.use_normal = h->prm.use_surface_normal;
    f.use_maxdist = h->prm.use_max_dist_filter;
    f.debug = h->dbg.debug_flags;
    f.cos_max_angle = std::cos(h->prm.max_normal_angle);  // cosf in T=float (OutlierFiltersImpl.cpp:229)
    const float md = h->prm.outlier_max_dist;
    f.outlier_max_d2 = md * md;
    return f;
}

// ---- exact k-th smallest finite key: three histogram levels over one 3 x 2048-bin block `hist` ----------------------
// R3+R4.  Buffer hygiene of the trimmed-quantile histograms needs no memset launches: the match kernel
// zeroes hist2, the level-2 select kernel zeroes hist0, the linearize kernel zeroes hist1.
static void launch_hist_level0(reg_handle* h, const float* keys, int64_t n, int blocks, uint32_t* hist) {
    k_hist_level0<<<blocks, 256, 0, h->stream>>>(keys, n, h->shift0, hist, h->i_iter.as<IterState>());
}
// level 1 or 2: picks level - 1 from its histogram, builds this level's; level 2 also zeroes level 0 for the next iteration
static void launch_select_level(reg_handle* h, int level, const float* keys, int64_t n, int blocks, uint32_t* hist,
                                SelectState* st, float ratio) {
    k_select_level<<<blocks, 256, 0, h->stream>>>(keys, n, level, h->shift0, ratio, hist + 2048 * (level - 1), hist + 2048 * level,
                                                  level == 2 ? hist : nullptr, st, h->i_iter.as<IterState>());
}

// ---- linearisation of the matched pairs into one row of sums per workgroup (i_partials) ----------------------------
// trim_mode: 0 no TrimmedDist, 1 the limit is in the select state, 2 the kernel finishes the select's last level itself
static void launch_linearize_p2pl(reg_handle* h, int trim_mode, float* w) {
    k_linearize_p2pl<<<h->n_blocks, 256, 0, h->stream>>>(
        h->s_xyz.as<float4>(), h->has_snrm ? h->s_nrm.as<float4>() : nullptr, h->n, h->i_iter.as<IterState>(), h->i_pos.as<int>(),
        h->i_d2.as<float>(), h->t_pts.as<float4>(), h->t_nrm.as<float4>(), make_filter_cfg(h, trim_mode),
        h->i_state.as<SelectState>(), h->i_hist.as<uint32_t>() + 4096, h->i_hist.as<uint32_t>() + 2048, h->shift0, w,
        h->i_partials.as<double>(), h->i_cache.as<float4>());
}
static void launch_linearize_gicp(reg_handle* h, float* w) {
    k_linearize_gicp<<<h->n_blocks, 256, 0, h->stream>>>(h->s_xyz.as<float4>(), h->s_cov.as<float4>(), h->n, h->i_iter.as<IterState>(),
                                                         h->i_pos.as<int>(), h->i_d2.as<float>(), h->t_pts.as<float4>(),
                                                         h->t_cov.as<float4>(), w, h->i_partials.as<double>());
}

// ---- fused iteration (point-to-plane): search + weights + normal equations in one pass over the reading -------------
// slack of the candidate-bounded boxes in the coherent kernel's fallback searches: a quarter bin (see nearest_group)
static inline float coherent_slack(const reg_handle* h) { return 0.25f * h->info.cell_size; }
// capacity of one of the kQueues sub-queues: workgroup lb (256 points) appends to sub-queue lb % kQueues
static inline int coherent_queue_cap(int64_t n) { return (int)(((n + 255) / 256 + kQueues - 1) / kQueues) * 256; }

// k_coh_check + k_coh_search<G> (or, under debug flag 16, k_iter_fused<G>: the A/B switch without the temporal-coherence
// shortcut).  Band records go to `band` (capacity band_cap), the rows of sums to i_acc; returns how many rows there are.
template <int G>
static int launch_fused_search(reg_handle* h, float* band, int band_cap, CohStats* stats, bool timed) {
    const FilterCfg f = make_filter_cfg(h, 0);
    const float4* src = h->s_xyz.as<float4>();
    const float4* snrm = h->has_snrm ? h->s_nrm.as<float4>() : nullptr;
    const float4* tnrm = h->t_nrm.as<float4>();
    IterState* it = h->i_iter.as<IterState>();
    uint8_t* hint = h->dbg.match_variant == 2 ? nullptr : h->i_hint.as<uint8_t>();
    float* w = h->i_w.as<float>();   // the weights are always written: reg_get_correspondences reports them
    if (h->dbg.debug_flags & 16) {
        const int blocks = grid_for(h->n * G);
        launch_timed(h, timed ? 1 : -1, k_iter_fused<G>, dim3(8 * ((blocks + 7) / 8)), dim3(256), 0, src, snrm, h->n, it, h->grid, tnrm,
                     f, h->i_pos.as<int>(), h->i_d2.as<float>(), w, hint, band, band_cap, h->i_acc.as<double>(), blocks);
        return blocks;
    }
    const int blocks = grid_for(h->n);
    launch_timed(h, timed ? 1 : -1, k_coh_check, dim3(8 * ((blocks + 7) / 8)), dim3(256), 0, src, snrm, h->n, it, h->grid, tnrm, f,
                 h->i_pos.as<int>(), h->i_d2.as<float>(), w, (const float4*)h->i_cache.as<float4>(), h->i_queue.as<uint32_t>(),
                 coherent_queue_cap(h->n), band, band_cap, h->i_acc.as<double>(), blocks);
    // k_coh_search: a fixed grid that strides over the queue (32 points per workgroup and pass): enough workgroups for the
    // usual few per cent of the reading in one pass, never more than the reading needs
    const int search_grid = (int)std::min<int64_t>(1024, (h->n + 31) / 32);
    launch_timed(h, timed ? 2 : -1, k_coh_search<G>, dim3(search_grid), dim3(256), 0, src, snrm, h->n, it, h->grid, tnrm, f,
                 h->i_pos.as<int>(), h->i_d2.as<float>(), w, hint, h->i_cache.as<float4>(), (const uint32_t*)h->i_queue.as<uint32_t>(),
                 coherent_queue_cap(h->n), band, band_cap, h->i_acc.as<double>(), coherent_slack(h), stats);
    return blocks;
}

// ---- the update kernel: reduce, solve, update the pose, run the checkers, publish the mirror -------------------------
enum UpdateMode { kUpdateSelect = 0, kUpdateFused = 1, kUpdateXicpFinish = 2 };
static void launch_reduce_update(reg_handle* h, UpdateMode mode, const double* rows, int n_rows, XicpState* xs,
                                 const SelectState* sel = nullptr, const float* band = nullptr, float* w = nullptr,
                                 const float* gathered = nullptr, int n_ranks = 0, int rank = 0) {
    // one kernel per path (kernels_update.hpp: UpdPath); O3D_UPDATE_GENERIC=1 keeps the select-based iteration and the finish
    // pass on the kernel that serves every path behind run-time values (A/B, tests/test_gpu_update_paths.py)
    IterState* it = h->i_iter.as<IterState>();
    if ((mode == kUpdateSelect || mode == kUpdateXicpFinish) && h->env.update_generic)
        k_reduce_update_generic<<<1, upd_threads(kUpdGeneric), 0, h->stream>>>(rows, n_rows, it, h->h_mirror.dev, h->seq, (int)mode, band, w,
                                                                               sel, gathered, n_ranks, rank, xs);
    else if (mode == kUpdateSelect)
        k_reduce_update<<<1, upd_threads(kUpdSelect), 0, h->stream>>>(rows, n_rows, it, h->h_mirror.dev, h->seq, sel, xs);
    else if (mode == kUpdateXicpFinish)
        k_reduce_update_finish<<<1, upd_threads(kUpdFinish), 0, h->stream>>>(it, h->h_mirror.dev, h->seq, xs);
    else if (gathered)
        k_reduce_update_gathered<<<1, upd_threads(kUpdGathered), 0, h->stream>>>(it, h->h_mirror.dev, h->seq, w, gathered, n_ranks, rank);
    else
        k_reduce_update_fused<<<1, upd_threads(kUpdFused), 0, h->stream>>>(rows, n_rows, it, h->h_mirror.dev, h->seq, band, w);
}
// select-free iteration of the Open3D costs: a new sequence from this GPU's rows of k_linearize_o3d
static void update_o3d_from_partials(reg_handle* h) {
    ++h->seq;
    if (h->env.update_generic)
        k_reduce_update_o3d_generic<<<1, upd_threads(kUpdGeneric), 0, h->stream>>>(h->i_partials.as<double>(), h->n_blocks,
                                                                                   h->i_iter.as<IterState>(), h->h_mirror.dev, h->seq);
    else
        k_reduce_update_o3d<<<1, kUpdO3dThreads, 0, h->stream>>>(h->i_partials.as<double>(), h->n_blocks, h->i_iter.as<IterState>(),
                                                                 h->h_mirror.dev, h->seq);
}
// a new sequence from this GPU's rows of k_linearize_* (single GPU)
static void update_from_partials(reg_handle* h) {
    ++h->seq;
    launch_reduce_update(h, kUpdateSelect, h->i_partials.as<double>(), h->n_blocks, h->i_xicp.as<XicpState>(),
                         h->prm.cost == REG_COST_P2PL ? h->i_state.as<SelectState>() : nullptr);
}
// a new sequence from the 32 sums the caller has all-reduced over the ranks (reg_dist_phase 4)
static void update_from_allreduced_sums(reg_handle* h) {
    ++h->seq;
    launch_reduce_update(h, kUpdateSelect, h->i_sums.as<double>(), 1, h->prm.use_xicp ? h->i_xicp.as<XicpState>() : nullptr,
                         h->prm.cost == REG_COST_P2PL ? h->i_state.as<SelectState>() : nullptr);
}
// a new sequence from the rows and band records of launch_fused_search (single GPU)
static void update_fused_from_band(reg_handle* h, int n_rows) {
    ++h->seq;
    launch_reduce_update(h, kUpdateFused, h->i_acc.as<double>(), n_rows, nullptr, nullptr, h->i_band.as<float>(), h->i_w.as<float>());
}
// a new sequence from the gathered contribution blocks of all ranks (reg_dist_phase 6)
static void update_fused_from_gathered(reg_handle* h) {
    ++h->seq;
    launch_reduce_update(h, kUpdateFused, nullptr, 0, nullptr, nullptr, nullptr, h->i_w.as<float>(), h->d_gathered.as<float>(),
                         h->dist_ranks, h->dist_rank);
}
// R8x finish of the CURRENT sequence: the sums are in the state, the analysis in XicpState; decide, solve, update, report
static void update_xicp_finish(reg_handle* h) { launch_reduce_update(h, kUpdateXicpFinish, nullptr, 0, h->i_xicp.as<XicpState>()); }

// ---- R8x, first iteration: the information sums on the matched pairs (pos, w) -> XicpState, centre first ------------------
static inline int xicp_blocks(const reg_handle* h) { return (int)std::min<int64_t>(512, (h->n + 255) / 256); }
static void launch_xicp_center(reg_handle* h, const int* pos, const float* w) {
    k_xicp_center<<<xicp_blocks(h), 256, 0, h->stream>>>(h->s_xyz.as<float4>(), h->n, h->i_iter.as<IterState>(), pos, w,
                                                         h->i_xicp.as<XicpState>());
}
static void launch_xicp_detect(reg_handle* h, const int* pos, const float* w) {
    k_xicp_detect<<<xicp_blocks(h), 256, 0, h->stream>>>(h->s_xyz.as<float4>(), h->n, h->i_iter.as<IterState>(), pos, w,
                                                         h->t_nrm.as<float4>(), h->i_xicp.as<XicpState>());
}
