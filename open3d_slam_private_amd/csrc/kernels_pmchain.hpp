// kernels_pmchain.hpp -- libpointmatcher chain extension (reg_set_pm_chain): k-NN matching, exact selects over the N*knn
// distances, RobustOutlierFilter weights, point-to-plane / point-to-point reduction and update
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
//
// One iteration of a handle with a chain (host_loop.hpp: enqueue_pm_iteration):
//   k_match_knn<K>                              N x knn {sorted position, d2} at T_iter
//   [k_hist_level0, k_pm_select_level1, k_select_level (level 2), k_pm_select_finish]  per exact select: TrimmedDist quantile, median(d2),
//                                               median(|d2 - median|) (k_pm_absdev in between) -- no host round trip
//   k_pm_scale                                  RobustOutlierFilter scale / iteration (state persists across registrations)
//   [sort + k_pm_var_*]                         VarTrimmedDist limit (kernels_pmoutliers.hpp); one more select for MedianDist
//   k_pm_linearize<kP2P>                        weights of the whole chain + per-workgroup fp64 partial sums
//   k_pm_update<kX>                             reduce, solve / Kabsch, T_iter <- dT T_iter, checkers, host mirror; kX: with
//                                               SolutionRemapping / BoundTransformationChecker (kernels_pmextras.hpp)
//   [k_pm_update<true, true>, k_xt_*, k_pm_update<true, true>]  instead, with EqualityConstraints on: the ternary X-ICP
//                                               analysis of every iteration between two launches (kernels_xicp_ternary.hpp)
// Every kernel returns at once when the loop is done (enqueued iterations past convergence are no-ops).
#pragma once

constexpr int kPmMaxKnn = 16;
constexpr int kPmCap = 128;          // candidates per point and level held in LDS; more: every extraction round rescans
constexpr int kPmLinBlocks = 1024;   // workgroups of the reduction (grid-stride over the pairs)

// Chain configuration as the kernels see it (host: make_pm_cfg)
struct PmCfg {
    int knn, minimizer, use_robust, robust_fct, scale_estimator, nb_iter_for_scale, distance_type;
    int use_trim, use_normal, use_maxdist;
    float tuning;           // effective tuning (berg: the Bergstrom constant of the function)
    float berg_target;      // berg: the configured tuning (target scale)
    float sq_approx;        // (float)(approximation^2), +inf = off
    float cos_max_angle, outlier_max_d2;
    // MinDist / MedianDist / VarTrimmedDist (kernels_pmoutliers.hpp)
    int use_mindist, use_median, use_var;
    float outlier_min_d2;   // minDist^2 (fp32 product)
    float median_factor;
    float var_min_ratio, var_max_ratio, var_lambda;
};

// Device-resident state of the chain, one per handle.  scale / iteration are the filter's members and persist across
// registrations (reset by reg_set_pm_chain); sel[] are the results of this iteration's selects.
struct PmState {
    float scale;
    int iteration;     // the filter's counter: 1 before its first call
    float sel[4];      // 0: median of d2, 1: median of |d2 - sel[0]|, 2: TrimmedDist limit (+inf: no finite distance),
                       // 3: MedianDist's getDistsQuantile(0.5)
    int fail;          // a statistic this iteration needed had no finite distance (ConvergenceError)
    int var_valid;     // var_* below belong to an iteration that ran
    // VarTrimmedDist of the last iteration that ran (k_pm_var_finish)
    float var_limit, var_ratio;
    long long var_k, var_n;
};

// Exact k nearest reference points of every transformed reading point, within max_dist.  16 lanes per point, level
// by level as k_knn_pca: the level's bin box is gathered into an LDS list (pca_scan_box, kernels_neighbours.hpp), the knn
// smallest (d2, original index) are extracted one by one, and the search ends once the knn-th distance is within the
// level's radius (every closer point was in the box).  d2 is the NC5 value of every other search of the table.
template <int K>
__global__ void __launch_bounds__(256)
k_match_knn(Grid g, const float4* __restrict__ src, int64_t n, int knn, const IterState* __restrict__ it,
            int* __restrict__ kpos, float* __restrict__ kd2) {
    constexpr int GP = 256 / kPcaGroup;   // points per workgroup
    __shared__ float l_d2[GP][kPmCap];
    __shared__ uint32_t l_idx[GP][kPmCap];
    __shared__ uint32_t l_pos[GP][kPmCap];
    __shared__ uint32_t l_cnt[GP];
    __shared__ int nb_pos[GP][K];
    __shared__ float nb_d2[GP][K];
    const int grp = threadIdx.x / kPcaGroup, sub = threadIdx.x & (kPcaGroup - 1);
    const int gbase = (int)(threadIdx.x & 63) & ~(kPcaGroup - 1);
    const int64_t q = blockIdx.x * (int64_t)GP + grp;
    if (it->done) return;
    if (q >= n) return;   // whole groups leave together; nothing below synchronises across groups
    const Xf T = load_xf(it);
    const float4 s = src[q];
    const float3 p = xf_point(T, s.x, s.y, s.z);
    const int kk = knn < K ? knn : K;
    int m = 0;
    for (int l = 0; l < g.n_levels; ++l) {
        if (sub == 0) l_cnt[grp] = 0;
        group_sync();
        pca_scan_box(g, p, l, sub, gbase, [&](uint32_t j, const float4& tpt, float d2) {
            const uint32_t slot = atomicAdd(&l_cnt[grp], 1u);
            if (slot < (uint32_t)kPmCap) {
                l_d2[grp][slot] = d2;
                l_idx[grp][slot] = __float_as_uint(tpt.w);
                l_pos[grp][slot] = j;
            }
        });
        group_sync();
        const uint32_t cnt = l_cnt[grp];
        const bool listed = cnt <= (uint32_t)kPmCap;
        float last_d2 = -1.f;
        uint32_t last_idx = 0;
        m = 0;
        for (int r = 0; r < kk; ++r) {
            float bd = INFINITY;
            uint32_t bi = 0xffffffffu, bp = 0xffffffffu;
            auto take = [&](float d, uint32_t ix, uint32_t jp) {
                const bool after = r == 0 || d > last_d2 || (d == last_d2 && ix > last_idx);
                if (after && (d < bd || (d == bd && ix < bi))) {
                    bd = d;
                    bi = ix;
                    bp = jp;
                }
            };
            if (listed) {
                for (uint32_t t2 = sub; t2 < cnt; t2 += kPcaGroup) take(l_d2[grp][t2], l_idx[grp][t2], l_pos[grp][t2]);
            } else {
                pca_scan_box(g, p, l, sub, gbase,
                             [&](uint32_t j, const float4& tpt, float d) { take(d, __float_as_uint(tpt.w), j); });
            }
#pragma unroll
            for (int x = 1; x < kPcaGroup; x <<= 1) {
                const float od = __shfl_xor(bd, x);
                const uint32_t oi = (uint32_t)__shfl_xor((int)bi, x);
                const uint32_t op = (uint32_t)__shfl_xor((int)bp, x);
                if (od < bd || (od == bd && oi < bi)) {
                    bd = od;
                    bi = oi;
                    bp = op;
                }
            }
            if (bi == 0xffffffffu) break;
            if (sub == 0) {
                nb_pos[grp][r] = (int)bp;
                nb_d2[grp][r] = bd;
            }
            last_d2 = bd;
            last_idx = bi;
            ++m;
        }
        const float r2 = g.rho[l] * g.rho[l];
        if ((m == kk && last_d2 <= r2) || l == g.n_levels - 1) break;
    }
    group_sync();
    for (int r = sub; r < kk; r += kPcaGroup) {
        const size_t o = (size_t)q * (size_t)kk + (size_t)r;
        kpos[o] = r < m ? nb_pos[grp][r] : -1;
        kd2[o] = r < m ? nb_d2[grp][r] : INFINITY;
    }
}

// First radix level of an exact select over the chain's keys (the level-1 branch of k_select_level, with the rank either
// trim_rank(total, ratio) or, median != 0, the integer median index total / 2): picks the level-0 bin, histograms bits
// [shift0-1 : shift0-11] of the keys inside it into hist1 and publishes prefix / rank / count for the next level.
__global__ void __launch_bounds__(256)
k_pm_select_level1(const float* __restrict__ keys, int64_t n, int shift0, float ratio, int median,
                   const uint32_t* __restrict__ hist0, uint32_t* __restrict__ hist1, SelectState* st,
                   const IterState* __restrict__ it) {
    __shared__ uint32_t sh[2048];
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t pick[3];
    if (it->done) return;
    uint32_t loc[8];
    load_hist8(hist0, loc);
    for (int k = threadIdx.x; k < 2048; k += blockDim.x) sh[k] = 0;
    block_pick256_regs(loc, 0xffffffffu, wave_tot, pick);
    const uint32_t total = pick[2];
    __syncthreads();
    const uint32_t rank = median ? total / 2u : trim_rank(total, ratio);
    block_pick256_regs(loc, rank, wave_tot, pick);
    const uint32_t prefix = pick[0] << shift0, rank_in = pick[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->n_finite = total;
        st->prefix = prefix;
        st->rank = rank_in;
        if (total == 0) st->limit = INFINITY;
    }
    __syncthreads();
    const int s1 = shift0 - 11;
    const uint32_t mask = ~((1u << shift0) - 1u);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t u = __float_as_uint(keys[i]);
        if (u != 0x7f800000u && (u & mask) == prefix) atomicAdd(&sh[(u >> s1) & 2047u], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2048; k += blockDim.x)
        if (sh[k]) atomicAdd(&hist1[k], sh[k]);
}

// Last radix level of an exact select (k_hist_level0 / k_select_level ran on the same keys): the value goes to
// ps->sel[slot] (+inf when no key is finite); levels 1 and 2 of the histogram are cleared for the next select
// (level 0 is cleared by the level-2 pass).  One workgroup of 256.
__global__ void __launch_bounds__(256)
k_pm_select_finish(uint32_t* __restrict__ hist /* 3 x 2048 */, const SelectState* __restrict__ st, int shift0,
                   PmState* __restrict__ ps, int slot, const IterState* __restrict__ it) {
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t pick[3];
    if (it->done) return;
    uint32_t loc[8];
    load_hist8(hist + 4096, loc);
    const uint32_t nfin = st->n_finite, pre = st->pad[0], rank = st->pad[1];
    const int nb = 1 << (shift0 - 11);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((int)threadIdx.x * 8 + k >= nb) loc[k] = 0u;
    block_pick256_regs(loc, rank, wave_tot, pick);
    if (threadIdx.x == 0) ps->sel[slot] = nfin != 0 ? __uint_as_float(pre | pick[0]) : INFINITY;
    __syncthreads();
    for (int k = threadIdx.x; k < 4096; k += blockDim.x) hist[2048 + k] = 0u;
}

// Matches::getMedianAbsDeviation, second pass: |d2 - median| in fp32 for the finite distances (+inf: not counted)
__global__ void __launch_bounds__(256)
k_pm_absdev(const float* __restrict__ d2, int64_t nk, const PmState* __restrict__ ps, float* __restrict__ keys,
            const IterState* __restrict__ it) {
    if (it->done) return;
    const float med = ps->sel[0];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nk; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = d2[i];
        keys[i] = d != INFINITY ? fabsf(d - med) : INFINITY;
    }
}

// RobustOutlierFilter::robustFiltering, scale part (OutlierFiltersImpl.cpp:510-543): one lane.
__global__ void k_pm_scale(PmState* __restrict__ ps, PmCfg c, const IterState* __restrict__ it) {
    if (it->done || threadIdx.x != 0) return;
    const int iter = ps->iteration;
    float scale = ps->scale;
    const bool upd = iter <= c.nb_iter_for_scale || c.nb_iter_for_scale == 0;
    if (c.scale_estimator == REG_SCALE_MAD) {
        if (upd) {
            if (!(ps->sel[1] < INFINITY)) ps->fail = 1;
            scale = sqrtf(ps->sel[1]);
        }
    } else if (c.scale_estimator == REG_SCALE_BERG) {
        if (upd) {
            if (iter == 1) {
                if (!(ps->sel[0] < INFINITY)) ps->fail = 1;
                scale = (float)(1.9 * (double)sqrtf(ps->sel[0]));
            } else {
                const float rate = 0.85f;
                scale = rate * (scale - c.berg_target) + c.berg_target;
            }
        }
    } else {
        scale = 1.f;
    }
    ps->scale = scale;
    ps->iteration = iter + 1;
}

// Weights of the chain (TrimmedDist, SurfaceNormal, MaxDist, Robust: a product) and the reduction, one pair per
// iteration of a grid-stride loop; per-workgroup fp64 partial records (reg_state.hpp layout, plus):
//   point-to-plane: 0-20 H, 21-26 b (sum w F r), 27 sum w r^2, 28 inliers
//   point-to-point: 0-2 sum w p, 3-5 sum w q, 6-14 sum w q p^T (row-major, row = q component), 15-17 0 (the centred
//                   frames' origin), 27 sum w |p - q|^2, 28 sum w        (the slots o3d_update_p2p reads)
//   both:           29 pairs with a finite d2, 30 sum d2 over the inliers, 31 inliers (w != 0)
// tgt: sorted reference points; tgt_nrm: {point, normal} pairs (null when the chain reads no reference normal).
template <bool kP2P>
__global__ void __launch_bounds__(256)
k_pm_linearize(const float4* __restrict__ src, const float4* __restrict__ src_nrm, int64_t n, const IterState* __restrict__ it,
               const int* __restrict__ kpos, const float* __restrict__ kd2, const float4* __restrict__ tgt,
               const float4* __restrict__ tgt_nrm, PmCfg c, const PmState* __restrict__ ps, float* __restrict__ w_out,
               double* __restrict__ partials) {
    if (it->done) return;
    const Xf T = load_xf(it);
    const float trim_limit = ps->sel[2], scale = ps->scale;
    const float median_limit = c.median_factor * ps->sel[3], var_limit = ps->var_limit;
    const int64_t nk = n * (int64_t)c.knn;
    double v[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] = 0.0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nk; e += (int64_t)gridDim.x * blockDim.x) {
        const int pos = kpos[e];
        float w = 0.f;
        if (pos >= 0) {
            const float dd = kd2[e];
            const int64_t i = e / c.knn;
            const float4 s = src[i];
            v[29] += 1.0;
            w = 1.f;
            if (c.use_trim && !(dd <= trim_limit)) w = 0.f;
            const float3 p = xf_point(T, s.x, s.y, s.z);
            const float4 q = tgt[pos];
            const float4 nn = tgt_nrm ? tgt_nrm[2 * (size_t)pos + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (c.use_normal) {
                const float4 sn = src_nrm[i];
                const float3 nr = normalize3(xf_rot(T, sn.x, sn.y, sn.z));
                const float3 nt = normalize3(make_float3(nn.x, nn.y, nn.z));
                float a = nr.x * nt.x;
                float b = nr.y * nt.y;
                float val = a + b;
                a = nr.z * nt.z;
                val = val + a;
                if (val < c.cos_max_angle) w = 0.f;
            }
            if (c.use_maxdist && !(dd <= c.outlier_max_d2)) w = 0.f;
            if (c.use_mindist && !(dd >= c.outlier_min_d2)) w = 0.f;
            if (c.use_median && !(dd <= median_limit)) w = 0.f;
            if (c.use_var && !(dd <= var_limit)) w = 0.f;
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            if (c.use_robust) {
                float dist = dd;
                if (c.distance_type == REG_DIST_POINT2PLANE) {
                    const float3 nh = normalize3(make_float3(nn.x, nn.y, nn.z));
                    float a = nh.x * dx;
                    float b = nh.y * dy;
                    float t = a + b;
                    a = nh.z * dz;
                    t = t + a;
                    dist = t * t;
                }
                w = w * pm_robust_weight(c.robust_fct, c.tuning, scale, c.sq_approx, dist);
            }
            if (w != 0.f) {
                if constexpr (kP2P) {
                    const double wd = (double)w;
                    const double pd[3] = {(double)p.x, (double)p.y, (double)p.z};
                    const double qd[3] = {(double)q.x, (double)q.y, (double)q.z};
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        v[a] += wd * pd[a];
                        v[3 + a] += wd * qd[a];
#pragma unroll
                        for (int b = 0; b < 3; ++b) v[6 + 3 * a + b] += wd * qd[a] * pd[b];
                    }
                    const double ex = pd[0] - qd[0], ey = pd[1] - qd[1], ez = pd[2] - qd[2];
                    v[27] += wd * (ex * ex + ey * ey + ez * ez);
                    v[28] += wd;
                } else {
                    float F[6];
                    float a = p.y * nn.z, b = p.z * nn.y;
                    F[0] = a - b;
                    a = p.z * nn.x; b = p.x * nn.z;
                    F[1] = a - b;
                    a = p.x * nn.y; b = p.y * nn.x;
                    F[2] = a - b;
                    F[3] = nn.x; F[4] = nn.y; F[5] = nn.z;
                    float r = dx * nn.x;
                    float t2 = dy * nn.y;
                    r = r + t2;
                    t2 = dz * nn.z;
                    r = r + t2;
                    int k = 0;
#pragma unroll
                    for (int a6 = 0; a6 < 6; ++a6) {
                        const float wf = w * F[a6];
#pragma unroll
                        for (int c6 = a6; c6 < 6; ++c6) {
                            const float pr = wf * F[c6];
                            v[k++] += (double)pr;
                        }
                    }
#pragma unroll
                    for (int a6 = 0; a6 < 6; ++a6) {
                        const float wf = w * F[a6];
                        const float pr = wf * r;
                        v[21 + a6] += (double)pr;
                    }
                    const float rr = r * r;
                    v[27] += (double)(w * rr);
                    v[28] += 1.0;
                }
                v[30] += (double)dd;
                v[31] += 1.0;
            }
        }
        if (w_out) w_out[e] = w;
    }
    block_reduce_store(v, partials);
}

// Reduce the partial records (fixed order: deterministic), then on one lane: solve (point-to-plane: the fp32 system in
// the fp64 solver, as the plain loop's fallback) or weighted Kabsch (o3d_update_p2p), T_iter <- dT T_iter, checkers,
// host mirror.  A statistic without a finite distance, or no inlier, ends the loop with REG_NO_CORRESPONDENCES.
__device__ __noinline__ int pm_solve(const double* tot, bool p2p, float* dT) {
    if (p2p) {
        double U[16];
        const int rank = o3d_update_p2p(tot, U);
        for (int i = 0; i < 16; ++i) dT[i] = (float)U[i];
        return rank;
    }
    float H[36], b6[6], x[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            const float v = (float)tot[k++];
            H[6 * i + j] = v;
            H[6 * j + i] = v;
        }
    for (int i = 0; i < 6; ++i) b6[i] = -(float)tot[21 + i];
    const int rank = solve6_p2pl(H, b6, x);
    x_to_T(x, dT);
    return rank;
}

// kT (with kX): the ternary X-ICP analysis runs EVERY iteration between a first launch (finish = 0: reduce, eigenvectors)
// and a second one (finish = 1: constraint values, KKT solve with its right-hand side, update); kernels_xicp_ternary.hpp
template <bool kX, bool kT = false>
__global__ void __launch_bounds__(256)
k_pm_update(const double* __restrict__ partials, int n_blocks, IterState* it, HostMirror* host, unsigned long long seq,
            PmState* __restrict__ ps, int p2p, int use_trim, int use_median, PmExtraCfg xc, PmExtraState* __restrict__ xs,
            int finish, XicpState* __restrict__ xq, XtState* __restrict__ xt = nullptr, const double* __restrict__ xt_rows = nullptr,
            int xt_n_rows = 0) {
    __shared__ double sh[8][kSums];
    __shared__ double tot[kSums];
    __shared__ double xt_tot[kT ? kXtPart : 1];
    if (it->done) return;
    if constexpr (kT) {
        if (finish) {
            if (xt->stage != 1) return;
            if (threadIdx.x < kSums) tot[threadIdx.x] = it->sums[threadIdx.x];
            __syncthreads();
            if (xt->mask != 0) pmx_sum_rows<kXtPart>(xt_rows + kXtRowsPart, xt_n_rows, xt_tot);
            n_blocks = 0;
        }
    }
    if constexpr (kX) {
        // R8x with a chain, second launch of the first iteration (after k_xicp_center / k_xicp_detect): the sums are the
        // ones this kernel reduced before the analysis
        if (finish && !kT) {
            if (it->xicp_stage != 2) return;
            if (threadIdx.x < kSums) tot[threadIdx.x] = it->sums[threadIdx.x];
            __syncthreads();
            n_blocks = 0;
        }
    }
    const int comp = threadIdx.x & (kSums - 1), part = threadIdx.x / kSums;   // 8 parts x 32 comps
    double t = 0;
    for (int b0 = part; b0 < n_blocks; b0 += 8 * 8) {
        double v8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int b = b0 + 8 * u;
            v8[u] = partials[(size_t)(b < n_blocks ? b : part) * kSums + comp];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) t += (b0 + 8 * u < n_blocks) ? v8[u] : 0.0;
    }
    sh[part][comp] = t;
    __syncthreads();
    if (threadIdx.x < kSums && !(kX && finish)) {   // (finish: tot holds the sums of the first launch)
        double s = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) s += sh[p][threadIdx.x];
        tot[threadIdx.x] = s;
        it->sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float Tc[16];
    for (int i = 0; i < 16; ++i) Tc[i] = it->T[i];
    bool xt_prior = false;
    float xt_rhs[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (kT) {
        if (!finish && ps->fail == 0 && tot[31] != 0.0 && tot[28] > 0.0 && !(use_trim && !(ps->sel[2] < INFINITY)) &&
            !(use_median && !(ps->sel[3] < INFINITY))) {
            // the system of this iteration is known: its eigen-directions, then the analysis kernels, then this kernel again
            xt_stage_a(tot, xt->Trd, xt->vr, xt->vo, 0);
            xt_stage_a(tot, xt->Trd, xt->vt, xt->vo + 9, 3);
            xt->mask = 0;
            xt->stage = 1;
            return;
        }
        if (finish) xt_prior = xt_finish(xt, xt_tot, it, xt_rhs) != 0;
    }
    if constexpr (kX) {
        if (!finish && it->xicp_stage == 1 && xq != nullptr && ps->fail == 0 && tot[31] != 0.0 && tot[28] > 0.0 &&
            !(use_trim && !(ps->sel[2] < INFINITY))) {
            // R8x stage A as the plain loop's update kernel: eigen-directions of the two blocks of A in the frame the data
            // came from; the analysis kernels collect the sums, then this kernel runs again (finish).  Nothing is reported.
            upd_xicp_stage_a(tot, it->xicp_Trd, xq->vr, 0);
            upd_xicp_stage_a(tot, it->xicp_Trd, xq->vt, 3);
            for (int i = 0; i < 4; ++i) xq->center[i] = 0.0;
            for (int i = 0; i < 6; ++i) {
                xq->comb[i] = 0.0;
                xq->high[i] = 0.0;
            }
            it->xicp_stage = 2;
            return;
        }
        if (finish && !kT) {
            int nc = 0;
            for (int i = 0; i < 6; ++i) {
                const int ok = (xq->comb[i] >= (double)it->xicp_enough || xq->high[i] >= (double)it->xicp_insufficient) ? 1 : 0;
                it->xicp_flags[i] = ok;
                it->xicp_comb[i] = xq->comb[i];
                it->xicp_high[i] = xq->high[i];
                nc += ok ? 0 : 1;
            }
            it->xicp_nc = nc;
            it->xicp_stage = 0;
        }
    }
    const bool fail = ps->fail != 0 || (use_trim && !(ps->sel[2] < INFINITY)) || (use_median && !(ps->sel[3] < INFINITY));
    ps->fail = 0;
    for (int i = 0; i < 16; ++i) it->T_prev[i] = Tc[i];
    if (fail || tot[31] == 0.0 || !(tot[28] > 0.0)) {
        it->status = REG_NO_CORRESPONDENCES;
        it->done = 1;
    } else {
        float dT[16], Tn[16];
        bool prior = false;
        if constexpr (kX) {
            if (kT && xt_prior) {
                prior = true;
            } else if (kT && it->xicp_nc > 0) {
                float x[6];
                it->rank_last = upd_solve6_xicp_rhs(tot, it->xicp_flags, xt_rhs, x);
                x_to_T(x, dT);
            } else if (xc.degeneracy != 0) {
                int rank = it->rank_last;
                prior = pmx_solve_remap(tot, xc, xs, dT, &rank) != 0;
                it->rank_last = rank;
            } else if (it->xicp_nc > 0) {
                // R8x: no update along the non-localizable eigen-directions of the CURRENT A (PointToPlane.cpp:459-505)
                float x[6];
                it->rank_last = upd_solve6_xicp(tot, it->xicp_flags, x);
                x_to_T(x, dT);
            } else {
                it->rank_last = pm_solve(tot, p2p != 0, dT);
            }
        } else {
            it->rank_last = pm_solve(tot, p2p != 0, dT);
        }
        if (prior) {
            // the detection failed: the reference leaves the loop before the update and returns the prior
            xs->returned_prior = 1;
            it->done = 1;
        } else {
            m4_mul(dT, Tc, Tn);   // T_iter = real * T_iter (ICP.cpp:1213-1215)
            for (int i = 0; i < 16; ++i) it->T[i] = Tn[i];
            const int iters = it->iterations + 1;
            it->iterations = iters;
            const bool iterate = it->fixed_iters > 0 ? iters < it->fixed_iters : it->chk.check(Tn);
            if (!iterate) it->done = 1;
            if constexpr (kX) {
                for (int i = 0; i < 16; ++i) xs->dT[i] = dT[i];
                xs->have_dT = 1;
                // checkers run in YAML order and an exception ends the pass: a Counter listed first that fires hides the bound
                if (xc.use_bound && it->fixed_iters <= 0 && !(xc.bound_after_counter && it->chk.max_iter_reached)) {
                    if (pmx_bound_check(Tn, xc, xs)) {
                        it->status = REG_OUT_OF_BOUNDS;
                        it->done = 1;
                    }
                }
            }
        }
    }
    for (int i = 0; i < kSums; ++i) host->sums[i] = tot[i];
    for (int i = 0; i < 16; ++i) {
        host->T[i] = it->T[i];
        host->T_prev[i] = it->T_prev[i];
    }
    host->iterations = it->iterations;
    host->done = it->done;
    host->status = it->status;
    host->rank_last = it->rank_last;
    host->converged = it->chk.converged ? 1 : 0;
    host->max_iter_reached = it->chk.max_iter_reached ? 1 : 0;
    host->stall = 0;
    host->band_count = 0;
    if constexpr (kX) {
        for (int i = 0; i < 6; ++i) {
            host->localizable[i] = it->xicp_flags[i];
            host->xicp_comb[i] = it->xicp_comb[i];
            host->xicp_high[i] = it->xicp_high[i];
        }
        host->n_constraints = it->xicp_nc;
    }
    HostMirror::SeqRecord* rec = &host->ring[seq % kSeqRing];
    rec->iterations = it->iterations;
    rec->done = it->done;
    rec->stall = 0;
    rec->pad = 0;
    rec->limit_last = INFINITY;
    rec->limit_prev = INFINITY;
    __threadfence_system();
    __hip_atomic_store(&rec->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Rows of the chain's N x knn buffers back into the caller's order: ids (original reference index), d2, w
__global__ void k_pm_unpermute(const int* __restrict__ kpos, const float* __restrict__ kd2, const float* __restrict__ kw,
                               const float4* __restrict__ tgt, int64_t n, int knn, const uint32_t* __restrict__ perm,
                               int32_t* __restrict__ ids, float* __restrict__ d2, float* __restrict__ w) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= n * (int64_t)knn) return;
    const int64_t i = e / knn, r = e - i * knn;
    const int64_t o = (perm ? (int64_t)perm[i] : i) * knn + r;
    const int p = kpos[e];
    if (ids) ids[o] = p >= 0 ? (int32_t)__float_as_uint(tgt[p].w) : -1;
    if (d2) d2[o] = kd2[e];
    if (w) w[o] = kw[e];
}
