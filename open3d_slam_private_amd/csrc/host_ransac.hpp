// host_ransac.hpp -- reg_ransac_correspondences: RegistrationRANSACBasedOnCorrespondence, the hypothesis loop of place
// recognition (PlaceRecognition.cpp:78-91) between reg_match_features and reg_set_pair_overlap_f64
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// Iterations per batch when reg_ransac_params.batch == 0: a batch costs 0.09 - 0.16 ms of launches and one synchronisation
// whatever its size up to here, so the largest batch measured; lowered, not below 4 096, where the chunk
// partials of k_rs_eval (12 bytes per batch position and chunk) would pass 48 MB
constexpr int kRsDefaultBatch = 1 << 18;
constexpr int64_t kRsDefaultPartials = 1 << 22;
constexpr int kRsMaxBatch = 1 << 20;

template <int N>
static void rs_launch_hypo(reg_handle* h, const double* P, const RsCfg& cfg, int64_t b0, int nb, int32_t* status, double* hyp,
                           uint32_t* flags) {
    k_rs_hypo<N><<<grid_for(nb + 1), 256, 0, h->stream>>>(P, cfg, b0, nb, status, hyp, flags);
}

extern "C" {

double reg_host_ransac_est_k(double est_k, double confidence, int64_t count, int64_t k, int32_t ransac_n) {
    const double ratio = (double)count / (double)k;
    const double x = std::log(1.0 - confidence) / std::log(1.0 - std::pow(ratio, (double)ransac_n));
    if (!(x >= 0.0)) return est_k;   // NaN (-inf / -inf) or -inf (the denominator rounded to log(1) = 0): no information
    const double t = std::trunc(x);
    return t < est_k ? t : est_k;
}

reg_status reg_ransac_correspondences(reg_handle* h, const double* src_xyz, int64_t n, const double* tgt_xyz, int64_t m,
                                      const int32_t* corres, int64_t k, int on_device, const reg_ransac_params* params,
                                      reg_ransac_result* result, int32_t* inliers, int32_t* iter_status) {
    if (!h) return REG_BAD_ARGUMENT;
    if (!h->device_ok) return REG_DEVICE_ERROR;
    if (!params || !result || params->struct_size != (int32_t)sizeof(reg_ransac_params) ||
        result->struct_size != (int32_t)sizeof(reg_ransac_result)) {
        h->err = "reg_ransac_correspondences: params / result NULL or a wrong struct_size";
        return REG_BAD_ARGUMENT;
    }
    const reg_ransac_params& p = *params;
    std::memset(result->T, 0, sizeof(result->T));
    result->T[0] = result->T[5] = result->T[10] = result->T[15] = 1.0;
    result->fitness = result->inlier_rmse = 0.0;
    result->n_inliers = result->n_iterations = result->n_validated = 0;
    result->batch = 0;
    result->best_iteration = -1;
    if (p.ransac_n < kRsMinN || p.ransac_n > kRsMaxN || p.max_iteration < 1 || !(p.confidence >= 0.0 && p.confidence <= 1.0) ||
        !(p.max_correspondence_distance > 0.0) || !std::isfinite(p.max_correspondence_distance) ||
        std::isnan(p.distance_threshold) || std::isnan(p.edge_similarity) || p.batch < 0 || p.batch > kRsMaxBatch ||
        k > 0x7fffffffLL || n > 0x7fffffffLL || m > 0x7fffffffLL) {
        h->err = "reg_ransac_correspondences: bad argument (3 <= ransac_n <= 8, max_iteration >= 1, 0 <= confidence <= 1, finite "
                 "max_correspondence_distance > 0, thresholds not NaN, 0 <= batch <= 2^20, n, m, k <= 2^31 - 1)";
        return REG_BAD_ARGUMENT;
    }
    if (k <= 0) {
        h->err = "The correspondence set is empty";
        return REG_EMPTY_SOURCE;
    }
    if (!src_xyz || !tgt_xyz || !corres || !inliers || n <= 0 || m <= 0) {
        h->err = "reg_ransac_correspondences: null array or empty cloud";
        return REG_BAD_ARGUMENT;
    }
    if (k < p.ransac_n) return REG_OK;   // as Open3D: the default result
    HIPCHK(h, hipSetDevice(h->prm.device));
    const double *d_src = nullptr, *d_tgt = nullptr;
    const int32_t* d_cor = nullptr;
    HIPCHK(h, staged_input(h, h->rs_src, src_xyz, (size_t)n * 3, on_device, &d_src));
    HIPCHK(h, staged_input(h, h->rs_tgt, tgt_xyz, (size_t)m * 3, on_device, &d_tgt));
    HIPCHK(h, staged_input(h, h->rs_cor, corres, (size_t)k * 2, on_device, &d_cor));
    const int n_chunks = (int)((k + kRsChunk - 1) / kRsChunk);
    const int64_t by_default = std::max<int64_t>(4096, std::min<int64_t>(kRsDefaultBatch, (kRsDefaultPartials / n_chunks) & ~63LL));
    const int batch = (int)std::min<int64_t>(p.batch > 0 ? p.batch : by_default, p.max_iteration);
    result->batch = batch;
    // rs_pairs: P | the flags and offsets of the final inlier pass | the inlier pairs of a host caller
    HIPCHK(h, h->rs_pairs.reserve((size_t)k * 48 + (size_t)(k + 1) * 8 + (size_t)k * 8));
    double* P = h->rs_pairs.as<double>();
    uint32_t* in_flags = reinterpret_cast<uint32_t*>(P + (size_t)k * 6);
    uint32_t* in_offs = in_flags + (k + 1);
    int32_t* d_inl = on_device ? inliers : reinterpret_cast<int32_t*>(in_offs + (k + 1));
    // rs_batch: hyp | survivor err2 | status, flags, offsets, survivor positions, survivor counts; rs_part: chunk partials
    HIPCHK(h, h->rs_batch.reserve((size_t)batch * (96 + 8 + 4 + 4 + 4) + (size_t)(batch + 1) * 8));
    double* hyp = h->rs_batch.as<double>();
    double* s_err = hyp + (size_t)batch * 12;
    int32_t* status = reinterpret_cast<int32_t*>(s_err + batch);
    int32_t* surv = status + batch;
    int32_t* s_cnt = surv + batch;
    uint32_t* flags = reinterpret_cast<uint32_t*>(s_cnt + batch);
    uint32_t* offs = flags + (batch + 1);
    HIPCHK(h, h->rs_part.reserve((size_t)n_chunks * batch * 12));
    double* part_err = h->rs_part.as<double>();
    int32_t* part_cnt = reinterpret_cast<int32_t*>(part_err + (size_t)n_chunks * batch);
    // rs_rec: RsState (its first word doubles as the bad-index flag of the gather) | one record per batch position, and at
    // least what the host reads in its one copy
    HIPCHK(h, h->rs_rec.reserve(sizeof(RsState) + (size_t)std::max(batch, kRsHeadRecords) * sizeof(RsRecord)));
    RsState* d_state = h->rs_rec.as<RsState>();
    RsRecord* d_rec = reinterpret_cast<RsRecord*>(d_state + 1);
    HIPCHK(h, hipMemsetAsync(d_state, 0, sizeof(RsState), h->stream));
    k_rs_gather<<<grid_for(k), 256, 0, h->stream>>>(d_src, n, d_tgt, m, d_cor, k, P, &d_state->n_rec);
    uint32_t bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, &d_state->n_rec, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    if (bad) {
        h->err = "reg_ransac_correspondences: a correspondence index lies outside its cloud";
        return REG_BAD_ARGUMENT;
    }
    const double maxd2 = p.max_correspondence_distance * p.max_correspondence_distance;
    RsCfg cfg;
    cfg.seed = p.seed;
    cfg.K = k;
    cfg.sim = p.edge_similarity;
    cfg.thr2 = p.distance_threshold > 0.0 ? p.distance_threshold * p.distance_threshold : -1.0;
    std::vector<RsRecord>& head = h->rs_head;   // RsState + the first records of a batch, one copy
    head.resize(1 + kRsHeadRecords);
    double est_k = (double)p.max_iteration;
    RsRecord best;
    best.iter = -1;
    best.count = 0;
    int64_t n_validated = 0, stop = -1;
    for (int64_t b0 = 0; stop < 0; b0 += batch) {
        const int nb = (int)std::min<int64_t>(batch, p.max_iteration - b0);
        switch (p.ransac_n) {
            case 3: rs_launch_hypo<3>(h, P, cfg, b0, nb, status, hyp, flags); break;
            case 4: rs_launch_hypo<4>(h, P, cfg, b0, nb, status, hyp, flags); break;
            case 5: rs_launch_hypo<5>(h, P, cfg, b0, nb, status, hyp, flags); break;
            case 6: rs_launch_hypo<6>(h, P, cfg, b0, nb, status, hyp, flags); break;
            case 7: rs_launch_hypo<7>(h, P, cfg, b0, nb, status, hyp, flags); break;
            default: rs_launch_hypo<8>(h, P, cfg, b0, nb, status, hyp, flags); break;
        }
        REGCHK(scan_excl(h, h->rp_tmp, flags, offs, (size_t)nb + 1));
        k_rs_compact<<<grid_for(nb), 256, 0, h->stream>>>(flags, offs, nb, surv);
        const dim3 grid((unsigned)grid_for(nb, kRsEvalLanes), (unsigned)n_chunks);
        k_rs_eval<<<grid, kRsEvalLanes, 0, h->stream>>>(P, k, maxd2, hyp, surv, offs, nb, batch, part_cnt, part_err);
        k_rs_merge<<<grid_for(nb), 256, 0, h->stream>>>(part_cnt, part_err, offs, nb, batch, n_chunks, surv, s_cnt, s_err, status);
        k_rs_records<<<1, 64, 0, h->stream>>>(s_cnt, s_err, surv, hyp, offs, nb, b0, d_state, d_rec);
        HIPCHK(h, hipMemcpyAsync(head.data(), d_state, head.size() * sizeof(RsRecord), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
        RsState hs;
        std::memcpy(&hs, head.data(), sizeof(hs));
        if (hs.n_rec > (uint32_t)kRsHeadRecords) {   // more record setters than one copy holds
            head.resize(1 + hs.n_rec);
            HIPCHK(h, hipMemcpy(head.data() + 1 + kRsHeadRecords, d_rec + kRsHeadRecords,
                                (size_t)(hs.n_rec - kRsHeadRecords) * sizeof(RsRecord), hipMemcpyDeviceToHost));
        }
        // the sequential rule on the batch's record setters: the loop ends at the first i >= est_k
        for (uint32_t r = 0; r < hs.n_rec; ++r) {
            const RsRecord& rec = head[1 + r];
            if ((double)rec.iter >= est_k) break;
            best = rec;
            est_k = reg_host_ransac_est_k(est_k, p.confidence, rec.count, k, p.ransac_n);
        }
        const int64_t b1 = b0 + nb;
        if (est_k <= (double)b1) stop = std::max<int64_t>((int64_t)est_k, best.iter + 1);
        const int64_t upto = stop >= 0 ? stop : b1;   // iterations of this batch that count
        if (upto == b1) {
            n_validated += hs.n_surv;
        } else {
            uint32_t before = 0;                      // survivors in front of the stop index
            HIPCHK(h, hipMemcpy(&before, offs + (upto - b0), 4, hipMemcpyDeviceToHost));
            n_validated += before;
        }
        if (iter_status && upto > b0)
            HIPCHK(h, hipMemcpy(iter_status + b0, status, (size_t)(upto - b0) * 4,
                                on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        head.resize(1 + kRsHeadRecords);
    }
    result->n_iterations = stop;
    result->n_validated = n_validated;
    if (best.iter < 0) return REG_OK;
    // the inlier pairs of the winning transform, ascending k
    RsPose pose;
    std::memcpy(pose.rt, best.rt, sizeof(pose.rt));
    k_rs_inlier_flags<<<grid_for(k + 1), 256, 0, h->stream>>>(P, k, pose, maxd2, in_flags);
    REGCHK(scan_excl(h, h->rp_tmp, in_flags, in_offs, (size_t)k + 1));
    uint32_t total = 0;
    HIPCHK(h, hipMemcpyAsync(&total, in_offs + k, 4, hipMemcpyDeviceToHost, h->stream));
    k_rs_collect<<<grid_for(k), 256, 0, h->stream>>>(in_flags, in_offs, k, d_cor, d_inl);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!on_device && total > 0) HIPCHK(h, hipMemcpy(inliers, d_inl, (size_t)total * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipGetLastError());
    if ((int64_t)total != (int64_t)best.count) {
        h->err = "reg_ransac_correspondences: the inlier pass disagrees with the evaluation";
        return REG_DEVICE_ERROR;
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) result->T[4 * c + r] = best.rt[3 * r + c];
        result->T[12 + r] = best.rt[9 + r];
    }
    result->fitness = (double)best.count / (double)k;
    result->inlier_rmse = std::sqrt(best.err2 / (double)best.count);
    result->n_inliers = best.count;
    result->best_iteration = best.iter;
    return REG_OK;
}

}  // extern "C"
