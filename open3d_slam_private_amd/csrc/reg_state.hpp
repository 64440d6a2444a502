// reg_state.hpp -- device-resident iteration state, host mirror, small shared helpers
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// The 32-double record every linearize kernel reduces (IterState::sums, HostMirror::sums, the distributed halves):
//   P2PL / GICP / O3D_P2PL   0-20 H (packed upper triangle), 21-26 b, 27 error, 28 inliers, 29 matched, 30 sum d^2 (inliers),
//                            31 below-band count (fused path)
//   O3D_P2P                  0-2 sum (p - o), 3-5 sum (q - o), 6-14 sum (q - o)(p - o)^T (row-major, row = q component),
//                            15-17 sum o, 27 sum |p - q|^2, 28 / 29 pairs, 30 sum d^2; o = centre of the reference's
//                            bounding box (k_linearize_o3d)
// Iteration state living in device memory: the pose the kernels read, the checker history and the
// termination flags.  The update kernel (last kernel of an iteration) is its only writer, so a whole
// registration can be enqueued without a host round trip per Gauss-Newton iteration.
struct IterState {
    float T[16];          // T_iter, row-major (P2PL: centred frames; GICP: reading -> reference)
    float T_prev[16];     // the pose the last completed iteration RAN at (its matches, weights and sums belong to it)
    double Td[16];        // GICP / O3D costs: the same in double
    Checkers chk;         // DifferentialTransformationChecker / CounterTransformationChecker state
    int iterations;
    int done;             // 1: the remaining enqueued kernels return immediately
    int status;           // reg_status of the loop (REG_OK / REG_NO_CORRESPONDENCES)
    int rank_last;
    int cost;
    int fixed_iters;
    int max_iter;
    int update;           // 0: reduce only (reg_linearize / distributed halves), 1: solve + update + check
    float gicp_rot_eps, gicp_trans_eps;
    int gicp_stop_rule;       // 1: Open3D ICPConvergenceCriteria (relative fitness / rmse between consecutive evaluations)
    float gicp_rel_fitness, gicp_rel_rmse;
    float n_total;            // reading points (all ranks): fitness = matched / n_total
    double fit_prev, rmse_prev;
    double sums[kSums];
    // fused path (k_iter_fused): predicted band [band_lo, band_hi) around the trimmed-quantile limit
    float band_lo, band_hi;   // +inf / +inf: no trimming (every finite match is inside)
    float trim_ratio;
    int use_trim;             // 1: TrimmedDistOutlierFilter active
    int stall;                // 1: the band prediction failed; enqueued fused kernels return until the host repairs
    float limit_last;         // trimmed limit of the last completed iteration (+inf: none)
    float limit_prev;         // ... and of the one before
    unsigned int band_count;  // records appended to the band buffer in this iteration
    // coherent fused iteration: kQueues counters (one per 64 bytes: same-address returning atomics serialise at ~11 ns
    // each, 800 workgroups on ONE word cost ~9 us) of the reading points whose shortcut failed, queued for k_coh_search;
    // the update kernel clears them
    unsigned int* qcount;
    unsigned int band_cap;
    int debug_narrow_band;    // test hooks: bit 0 forces band mispredictions, bit 1 disables the direct band ranking
    float limit_prev2;        // the trimmed limit before limit_prev (+inf: none): the band predictor extrapolates from three
    // R8x (X-ICP localizability, OptimizedEqualityConstraints)
    int xicp_stage;           // 0: off / analysed, 1: analysis pending (first iteration), 2: sums being collected
    int xicp_nc;              // number of non-localizable directions (constraints)
    int xicp_flags[6];        // 1 = localizable; rotation eigen-directions 0-2, translation 3-5
    float xicp_enough, xicp_insufficient, xicp_cos_min, xicp_cos_strong;
    float xicp_Trd[12];       // T_refMean_dataIn (row-major 3x4): its inverse takes the matched data to the frame it came from
    double xicp_comb[6], xicp_high[6];   // the information sums of the analysis (reported with every mirror)
};

// Scratch of the first-iteration localizability analysis.
struct XicpState {
    float vr[9], vt[9];       // eigenvectors in the data frame, [k*3 + r]
    int pad[2];
    double center[4];         // sum of the matched reading points (data frame) + their count
    double comb[6], high[6];  // information sums: rotation 0-2, translation 3-5
};

// What the update kernel mirrors into mapped host memory (the host polls `seq`).
struct HostMirror {
    double sums[kSums];
    float T[16];
    float T_prev[16];
    int iterations, done, status, rank_last, converged, max_iter_reached, stall, band_count;
    float limit_last, limit_prev, band_lo, band_hi;
    int pad_nband, pad2;
    int localizable[6];
    int n_constraints, pad3;
    double xicp_comb[6], xicp_high[6];
    unsigned long long stamps[8];   // s_memtime stamps of the update kernel (diagnostics only; nothing reads them)
    unsigned long long seq;
    // Per-sequence records (ring of kSeqRing): what the update kernel with sequence number s reported.  The multi-GPU
    // drivers steer ONLY by the record of a specific sequence -- identical on every rank -- never by "whatever has
    // arrived so far", which depends on timing and would let ranks enqueue different collectives.
    struct SeqRecord {
        unsigned long long seq;
        int iterations, done, stall, pad;
        float limit_last, limit_prev;
    } ring[16];
};
constexpr int kSeqRing = 16;

// ---- the band predicted for the next iteration's trimmed limit (every loop path: k_reduce_update and k_tail call this)
constexpr int kTailBandCap = 1024;       // band records one tail iteration may hold in all (more: stall, select-based repair)
constexpr float kTailWideRel = 0.02f;    // a band wider than this fraction of its lower edge takes the tail's two-exchange form
constexpr float kBandFloor = 0.003f;     // margin (fraction of the limit) beyond every edge: the limit's jitter once it has settled
constexpr float kBandRatioMax = 0.6f;    // a settling limit's successive changes shrink by 0.15 - 0.55: the reach covers 0.6,
constexpr float kBandCentreGain = 1.5f;  // ... or 1.5 x the last observed ratio where that is larger
constexpr float kBandGeomRel = 0.25f;    // the ratio of two changes means something only once both are small against the limit
constexpr float kBandGuardFrac = 0.75f;  // a narrow band whose estimated population exceeds this share of kTailBandCap is widened
constexpr float kBandForcedWide = 0.0205f;   // ... to this fraction of the limit: past kTailWideRel, the two-exchange form on purpose
struct Band {
    float lo, hi;
};
// limit / prev / prev2: the last three trimmed limits, newest first (+inf: none).  last_count points lay in the band
// [last_lo, last_hi) of the iteration that produced `limit` (0 / +inf: unknown).
//   * Fewer than three limits, changes of different sign, a change that did not shrink, or a change before it that was not small
//     against the limit (the collapse after a far prior's plateau says nothing about the ratio of the settled regime): the
//     symmetric band around the last limit, m = clamp(2 |L - P| / L + 0.003, 0.003, 0.6).
//   * Otherwise the limit converges geometrically and keeps its direction: the band reaches from the last limit (ratio 0) to
//     L + max(1.5 q, 0.6) (L - P), q = (L - P) / (P - PP) the last observed ratio, plus the floor margin on both sides.
//   * Count guard: the population scales with the width (the density of d^2 around the limit changes by ~1 % per iteration); a
//     narrow band expected to hold more than kBandGuardFrac * kTailBandCap points would overflow the record list and stall.
__host__ __device__ inline Band predict_band(float limit, float prev, float prev2, unsigned last_count, float last_lo, float last_hi,
                                             int debug_narrow) {
    Band b = {INFINITY, INFINITY};
    if (!(limit < INFINITY)) return b;   // nothing to predict from: every finite match is "certainly kept"
    float m = 0.3f;
    if (prev < INFINITY && prev > 0.f) m = fminf(fmaxf(2.0f * fabsf(limit - prev) / limit + kBandFloor, kBandFloor), 0.6f);
    if (debug_narrow) m = 1e-7f;   // test hook: forces band mispredictions (stall + repair path)
    b.lo = limit * (1.0f - m);
    b.hi = limit * (1.0f + m);
    if (debug_narrow) return b;
    if (prev < INFINITY && prev > 0.f && prev2 < INFINITY && prev2 > 0.f) {
        const float d = limit - prev, dp = prev - prev2;
        if (d * dp > 0.f && fabsf(d) < fabsf(dp) && fabsf(dp) <= kBandGeomRel * limit) {
            const float q = d / dp;
            const float far_edge = limit + fmaxf(kBandCentreGain * q, kBandRatioMax) * d, pad = kBandFloor * limit;
            b.lo = d < 0.f ? far_edge - pad : limit - pad;
            b.hi = d < 0.f ? limit + pad : far_edge + pad;
        }
    }
    if (last_count > 0u && last_hi < INFINITY && last_hi > last_lo) {
        const float est = (float)last_count * (b.hi - b.lo) / (last_hi - last_lo);
        if (est > kBandGuardFrac * (float)kTailBandCap && !(b.hi - b.lo > kTailWideRel * b.lo)) {
            const float grow = 0.5f * (kBandForcedWide * limit - (b.hi - b.lo));
            if (grow > 0.f) {
                b.lo -= grow;
                b.hi += grow;
            }
        }
    }
    return b;
}
constexpr int kQueues = 64;        // sub-queues of the coherent iteration's search queue (workgroup lb appends to lb % kQueues)
constexpr int kQueueStride = 16;   // counters are 16 words (64 bytes) apart

// XCD-aware workgroup order: the dispatcher deals workgroups round-robin over the 8 XCDs (blockIdx % 8
// shares an XCD).  With a Morton-ordered reading, giving each XCD ONE contiguous eighth of the reading means
// its private 4 MB L2 only has to hold that region's slice of the reference cloud and tables.
// Launch with gridDim.x = 8 * ceil(n_blocks / 8); returns the logical block (>= n_blocks: nothing to do).
__device__ __forceinline__ int xcd_block(int n_blocks) {
    const int chunk = (n_blocks + 7) >> 3;
    return (int)(blockIdx.x & 7) * chunk + (int)(blockIdx.x >> 3);
}

// ... in tiles: XCD x takes tiles x, x + 8, x + 16, ... of `tile` consecutive workgroups each.  One contiguous eighth per XCD
// ties the time of a launch to its slowest eighth: the first searches of a registration cost most where the initial guess is
// farthest off (rotation error x range), and that is ONE corner of the Morton-ordered reading (C3, second search launch:
// 160 us with eighths, 117 us in tiles of 16).  Launch with xcd_tiled_grid(n_blocks, tile) workgroups; tile <= 0: eighths.
__host__ __device__ __forceinline__ int xcd_tiled_grid(int n_blocks, int tile) {
    if (tile <= 0) return 8 * ((n_blocks + 7) / 8);
    const int per = 8 * tile;
    return per * ((n_blocks + per - 1) / per);
}
__device__ __forceinline__ int xcd_block_tiled(int n_blocks, int tile) {
    if (tile <= 0) return xcd_block(n_blocks);
    const int xcd = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
    const int t = j / tile, r = j - t * tile;
    return (t * 8 + xcd) * tile + r;
}

struct Xf4 {
    float m[16];
};

__device__ __forceinline__ Xf load_xf(const IterState* it) {
    Xf x;
#pragma unroll
    for (int k = 0; k < 12; ++k) x.m[k] = it->T[k];
    return x;
}
