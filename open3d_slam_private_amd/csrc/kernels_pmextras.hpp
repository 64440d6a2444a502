// kernels_pmextras.hpp -- libpointmatcher chain extension, part 3: the pose covariance of PointToPlaneWithCovErrorMinimizer,
// the ErrorMinimizer statistics, BoundTransformationChecker and degeneracyAwareness SolutionRemapping
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
//
// Inside the loop (k_pm_update<true>, kernels_pmchain.hpp; one lane, no extra launch, no host round trip):
//   pmx_solve_remap     solve + SolutionRemapping projection of the update          (ICP.cpp:2446-2501, 1621-1666)
//   pmx_bound_check     BoundTransformationChecker after the update                 (TransformationCheckersImpl.cpp:198-225)
// After the loop (host_loop.hpp: evaluate_pm_covariance, reg_get_minimizer_stats), on the buffers of the last iteration:
//   k_pmx_pair_means    sum p, sum q, count over the kept pairs  -> per-workgroup rows of 8 doubles
//   k_pmx_reduce_rows   fixed-order sum of the rows
//   k_pmx_cov_terms     the 21 + 21 sums of Censi's estimate     -> per-workgroup rows of 42 doubles
//   k_pmx_cov_finish    fixed-order sum of the rows, then cov = sigma^2 H^-1 M H^-1 on one lane (pmx_censi_covariance)
//   k_pmx_stats         sum w, pairs and points without weight   -> rows of 8 doubles (then k_pmx_reduce_rows)
// No float atomics anywhere: two evaluations of the same state return identical bits.
#pragma once

constexpr int kPmxRow = 8;          // doubles per row of the small reductions
constexpr int kPmxCovSums = 42;     // packed upper triangles of H and M
constexpr int kPmxBlocks = 1024;    // workgroups of the post-loop reductions (grid-stride over the pairs)

// What k_pm_update<true> needs of the chain (host: make_pm_extra_cfg)
struct PmExtraCfg {
    int use_bound, bound_after_counter;
    float max_rot, max_trans;
    int degeneracy, sr_use2019;
    float sr_threshold;
    int with_cov;
};

// Device-resident state of these modules, one per handle; reset at the start of every registration (P = identity, as
// the reference's struct is a local of computeWithTransformedReference, PointMatcher.h:645)
struct PmExtraState {
    double P[36];           // SolutionRemapping projector in force (row-major)
    float dT[16];           // the last update (row-major): `transformation` of estimateCovariance
    float eig[6];           // eigenvalues of the last iteration's A, descending
    float cond;             // eig[0] / eig[5]
    int cat[6];             // 1 = kept, 0 = degenerate
    int sr_valid;           // eig / cat / cond belong to an iteration that ran
    int returned_prior;     // the detection failed: the loop stopped before the update
    int have_dT;            // an update has been applied in this registration
    int bound_valid, oob;   // bound_* were evaluated / violated
    float bound_rot, bound_trans;
};

// Result block of the covariance evaluation (device -> host copy)
struct PmCovOut {
    double sums[kPmxCovSums];   // 0-20 H, 21-41 M (packed upper triangles, row by row)
    double n_pairs;
    float mean_p[3], mean_q[3];
    float cov[36];
    int rank, pad;
};

// cov = sigma^2 H^-1 M H^-1 in fp64 from the packed sums; rank of H by the rank rule of solve_sym6 (eigenvalues above
// 6 eps_fp32 of the largest).  rank < 6 (or a NaN sum): cov is all NaN.
O3D_HD inline int pmx_censi_covariance(const double* Hp, const double* Mp, double sigma, float* cov) {
    double H[36], M[36], A[36], V[36], lam[6], Hi[36], Tm[36];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            H[6 * i + j] = H[6 * j + i] = Hp[k];
            M[6 * i + j] = M[6 * j + i] = Mp[k];
            ++k;
        }
    for (int i = 0; i < 36; ++i) A[i] = H[i];
    jacobi_eig_sym(6, A, V, lam);
    double lmax = 0;
    for (int i = 0; i < 6; ++i) lmax = fmax(lmax, fabs(lam[i]));
    int rank = 0;
    for (int i = 0; i < 6; ++i)
        if (fabs(lam[i]) > lmax * (6.0 * 1.1920929e-07)) ++rank;
    if (rank < 6) {
        for (int i = 0; i < 36; ++i) cov[i] = NAN;
        return rank;
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double t = 0;
            for (int e = 0; e < 6; ++e) t += V[6 * i + e] * V[6 * j + e] / lam[e];
            Hi[6 * i + j] = t;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double t = 0;
            for (int e = 0; e < 6; ++e) t += Hi[6 * i + e] * M[6 * e + j];
            Tm[6 * i + j] = t;
        }
    const double s2 = sigma * sigma;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double t = 0;
            for (int e = 0; e < 6; ++e) t += Tm[6 * i + e] * Hi[6 * e + j];
            cov[6 * i + j] = (float)(s2 * t);
        }
    return rank;
}

// SolutionRemapping from an eigen-decomposition of the symmetrised A (V[6 r + k] = component r of eigenvector k, lam in
// the order the Jacobi routine left them): solutionRemappingProjectionCalculation + the checks of
// detectLocalizabilityWithSolutionRemappingMethod.  The singular values of the reference's JacobiSVD are the |eigenvalues|,
// descending.  Returns 1 when the reference returns the prior (the projector all zero).
O3D_HD inline int pmx_remap_from_eig(const double* V, const double* lam_in, float threshold, int use2019, const double* Pin,
                                     double* Pout, int* cat, float* eig, float* cond) {
    double lam[6];
    int ord[6] = {0, 1, 2, 3, 4, 5};
    for (int i = 0; i < 6; ++i) lam[i] = fabs(lam_in[i]);
    for (int i = 1; i < 6; ++i)   // insertion sort, descending, stable
        for (int j = i; j > 0 && lam[ord[j]] > lam[ord[j - 1]]; --j) {
            const int t = ord[j];
            ord[j] = ord[j - 1];
            ord[j - 1] = t;
        }
    for (int j = 0; j < 6; ++j) eig[j] = (float)lam[ord[j]];
    *cond = eig[0] / eig[5];
    const float thr = use2019 ? *cond : threshold;
    bool any = false;
    for (int j = 0; j < 6; ++j) {
        cat[j] = eig[j] < thr ? 0 : 1;
        any = any || cat[j] == 0;
    }
    for (int i = 0; i < 36; ++i) Pout[i] = Pin[i];
    if (any) {
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                double t = 0;
                for (int j = 0; j < 6; ++j)
                    if (cat[j]) t += V[6 * r + ord[j]] * V[6 * c + ord[j]];
                Pout[6 * r + c] = t;
            }
    }
    bool zero = true;
    for (int i = 0; i < 36; ++i) zero = zero && (Pout[i] == 0.0);
    return zero ? 1 : 0;
}

// The prior is also returned for an empty system (A all zero): nothing is decomposed then
O3D_HD inline int pmx_remap_empty(const float* A, const double* Pin, double* Pout, int* cat, float* eig, float* cond) {
    bool zero = true;
    for (int i = 0; i < 36; ++i) zero = zero && (A[i] == 0.f);
    if (!zero) return 0;
    for (int i = 0; i < 36; ++i) Pout[i] = Pin[i];
    for (int j = 0; j < 6; ++j) {
        cat[j] = 0;
        eig[j] = 0.f;
    }
    *cond = NAN;
    return 1;
}

// One SolutionRemapping step on the fp32 normal matrix A (row-major).  Returns 1 when the reference returns the prior.
O3D_HD inline int pmx_solution_remap(const float* A, float threshold, int use2019, const double* Pin, double* Pout, int* cat,
                                     float* eig, float* cond) {
    if (pmx_remap_empty(A, Pin, Pout, cat, eig, cond)) return 1;
    double M[36], V[36], lam[6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) M[6 * i + j] = 0.5 * ((double)A[6 * i + j] + (double)A[6 * j + i]);
    jacobi_eig_sym(6, M, V, lam);
    return pmx_remap_from_eig(V, lam, threshold, use2019, Pin, Pout, cat, eig, cond);
}

// Point-to-plane solve of the chain with SolutionRemapping: x = P solve(A, b), the product in fp64 rounded to fp32 (exact
// for P = I).  ONE eigen-decomposition serves the detection and the solve: the solve is solve_sym6's, operation for
// operation, on the decomposition it would compute itself (the routine indexes at run time, its arrays live in scratch,
// and a second decomposition on this one lane cost 0.49 ms per iteration).  Returns 1 when the prior is to be returned.
__device__ __noinline__ int pmx_solve_remap(const double* tot, const PmExtraCfg& xc, PmExtraState* xs, float* dT, int* rank) {
    float H[36], b6[6], xp[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            const float v = (float)tot[k++];
            H[6 * i + j] = v;
            H[6 * j + i] = v;
        }
    for (int i = 0; i < 6; ++i) b6[i] = -(float)tot[21 + i];
    double Pn[36], M[36], V[36], lam[6], g[6], x[6];
    int cat[6];
    float eig[6], cond;
    int prior = pmx_remap_empty(H, xs->P, Pn, cat, eig, &cond);
    if (!prior) {
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) M[6 * i + j] = 0.5 * ((double)H[6 * i + j] + (double)H[6 * j + i]);
        jacobi_eig_sym(6, M, V, lam);
        prior = pmx_remap_from_eig(V, lam, xc.sr_threshold, xc.sr_use2019, xs->P, Pn, cat, eig, &cond);
    }
    for (int i = 0; i < 36; ++i) xs->P[i] = Pn[i];
    for (int j = 0; j < 6; ++j) {
        xs->cat[j] = cat[j];
        xs->eig[j] = eig[j];
    }
    xs->cond = cond;
    xs->sr_valid = 1;
    if (prior) return 1;
    // solve_sym6(H, b, x, 6 eps_fp32) as solve6_p2pl calls it
    for (int i = 0; i < 6; ++i) g[i] = b6[i];
    double lmax = 0;
    for (int e = 0; e < 6; ++e) lmax = fmax(lmax, fabs(lam[e]));
    int r = 0;
    for (int i = 0; i < 6; ++i) x[i] = 0;
    for (int e = 0; e < 6; ++e) {
        if (!(fabs(lam[e]) > lmax * (6.0 * 1.1920929e-07))) continue;
        ++r;
        double vb = 0;
        for (int i = 0; i < 6; ++i) vb += V[6 * i + e] * g[i];
        vb /= lam[e];
        for (int i = 0; i < 6; ++i) x[i] += V[6 * i + e] * vb;
    }
    *rank = r;
    for (int i = 0; i < 6; ++i) {
        double t = 0;
        for (int j = 0; j < 6; ++j) t += Pn[6 * i + j] * (double)(float)x[j];
        xp[i] = (float)t;
    }
    x_to_T(xp, dT);
    return 0;
}

// BoundTransformationChecker::check on the pose after the update (fp32, strict >); the checkers were initialised with
// the identity (ICP.cpp:993-997), so the reference rotation is the unit quaternion and the reference translation zero.
__device__ __noinline__ bool pmx_bound_check(const float* Tn, const PmExtraCfg& xc, PmExtraState* xs) {
    float q[4];
    const float qi[4] = {1.f, 0.f, 0.f, 0.f};
    rot_to_quat(Tn, q);
    const float rot = quat_angular_distance(q, qi);
    const float tx = Tn[3], ty = Tn[7], tz = Tn[11];
    const float tr = sqrtf(tx * tx + ty * ty + tz * tz);
    xs->bound_rot = rot;
    xs->bound_trans = tr;
    xs->bound_valid = 1;
    const bool out = rot > xc.max_rot || tr > xc.max_trans;
    xs->oob = out ? 1 : 0;
    return out;
}

// ---- post-loop reductions ------------------------------------------------------------------------------------------

// Fixed-order sum of n_rows rows of NV doubles: P parts of the rows side by side, the parts added in order.
// One workgroup of 256 lanes.  Returns the total of component threadIdx.x in tot[] (LDS) after a barrier.
template <int NV>
__device__ __forceinline__ void pmx_sum_rows(const double* __restrict__ rows, int n_rows, double* tot /* LDS, NV */) {
    constexpr int P = 256 / NV;
    __shared__ double sh[P][NV];
    const int comp = threadIdx.x % NV, part = threadIdx.x / NV;
    if (part < P) {
        double t = 0;
        for (int b = part; b < n_rows; b += P) t += rows[(size_t)b * NV + comp];
        sh[part][comp] = t;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0;
        for (int p = 0; p < P; ++p) s += sh[p][threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) k_pmx_reduce_rows(const double* __restrict__ rows, int n_rows, double* __restrict__ out) {
    __shared__ double tot[kPmxRow];
    pmx_sum_rows<kPmxRow>(rows, n_rows, tot);
    if (threadIdx.x < kPmxRow) out[threadIdx.x] = tot[threadIdx.x];
}

__device__ __forceinline__ Xf pmx_load_xf_prev(const IterState* it) {
    Xf x;
#pragma unroll
    for (int k = 0; k < 12; ++k) x.m[k] = it->T_prev[k];
    return x;
}

// Kept pairs of the last iteration (w != 0 and a match): sums of p = T_iter_prev s and of q in fp64, and their count
// rows: {px, py, pz, qx, qy, qz, count, 0}
__global__ void __launch_bounds__(256)
k_pmx_pair_means(const float4* __restrict__ src, int64_t n, int knn, const IterState* __restrict__ it, const int* __restrict__ kpos,
                 const float* __restrict__ kw, const float4* __restrict__ tgt, double* __restrict__ rows) {
    const Xf T = pmx_load_xf_prev(it);
    const int64_t nk = n * (int64_t)knn;
    double v[kPmxRow];
#pragma unroll
    for (int k = 0; k < kPmxRow; ++k) v[k] = 0.0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nk; e += (int64_t)gridDim.x * blockDim.x) {
        const int pos = kpos[e];
        if (pos < 0 || kw[e] == 0.f) continue;
        const float4 s = src[e / knn];
        const float3 p = xf_point(T, s.x, s.y, s.z);
        const float4 q = tgt[pos];
        v[0] += (double)p.x;
        v[1] += (double)p.y;
        v[2] += (double)p.z;
        v[3] += (double)q.x;
        v[4] += (double)q.y;
        v[5] += (double)q.z;
        v[6] += 1.0;
    }
    block_sum_store<kPmxRow>(v, rows + (size_t)blockIdx.x * kPmxRow);
}

// The per-pair terms of PointToPlaneWithCovErrorMinimizer::estimateCovariance (PointToPlaneWithCov.cpp:110-146) in fp32,
// one rounding per operation in the reference's expression order; products of the 6-vectors in fp32, sums in fp64.
// ang: {alpha, beta, gamma, tx, ty, tz} of the last update.
__device__ __forceinline__ void pmx_cov_pair(const float3 p, const float3 q, const float3 nn, const float* ang, float* v, float* a,
                                             float* b) {
    const float alpha = ang[0], beta = ang[1], gamma = ang[2], t_x = ang[3], t_y = ang[4], t_z = ang[5];
    float s = p.x * p.x, u = p.y * p.y;
    s = s + u;
    u = p.z * p.z;
    s = s + u;
    const float rr = sqrtf(s);                                   // reading_range
    const float rd0 = p.x / rr, rd1 = p.y / rr, rd2 = p.z / rr;  // reading_direction
    s = q.x * q.x;
    u = q.y * q.y;
    s = s + u;
    u = q.z * q.z;
    s = s + u;
    const float fr = sqrtf(s);                                   // reference_range
    const float fd0 = q.x / fr, fd1 = q.y / fr, fd2 = q.z / fr;
    float x1, x2;
    x1 = nn.z * rd1; x2 = nn.y * rd2;
    const float n_alpha = x1 - x2;
    x1 = nn.x * rd2; x2 = nn.z * rd0;
    const float n_beta = x1 - x2;
    x1 = nn.y * rd0; x2 = nn.x * rd1;
    const float n_gamma = x1 - x2;
    // E
    float t = gamma * p.y;
    float e0 = p.x - t;
    t = beta * p.z;
    e0 = e0 + t;
    e0 = e0 + t_x;
    e0 = e0 - q.x;
    float E = nn.x * e0;
    t = gamma * p.x;
    float e1 = t + p.y;
    t = alpha * p.z;
    e1 = e1 - t;
    e1 = e1 + t_y;
    e1 = e1 - q.y;
    t = nn.y * e1;
    E = E + t;
    t = (-beta) * p.x;
    float e2 = alpha * p.y;
    e2 = t + e2;
    e2 = e2 + p.z;
    e2 = e2 + t_z;
    e2 = e2 - q.z;
    t = nn.z * e2;
    E = E + t;
    // N_reading
    t = gamma * rd1;
    float m0 = rd0 - t;
    t = beta * rd2;
    m0 = m0 + t;
    float Nr = nn.x * m0;
    t = gamma * rd0;
    float m1 = t + rd1;
    t = alpha * rd2;
    m1 = m1 - t;
    t = nn.y * m1;
    Nr = Nr + t;
    t = (-beta) * rd0;
    float m2 = alpha * rd1;
    m2 = t + m2;
    m2 = m2 + rd2;
    t = nn.z * m2;
    Nr = Nr + t;
    // N_reference
    float Nf = nn.x * fd0;
    t = nn.y * fd1;
    Nf = Nf + t;
    t = nn.z * fd2;
    Nf = Nf + t;
    Nf = -Nf;
    v[0] = nn.x; v[1] = nn.y; v[2] = nn.z;
    v[3] = rr * n_alpha; v[4] = rr * n_beta; v[5] = rr * n_gamma;
    t = rr * Nr;
    const float g = E + t;
    a[0] = nn.x * Nr; a[1] = nn.y * Nr; a[2] = nn.z * Nr;
    a[3] = n_alpha * g; a[4] = n_beta * g; a[5] = n_gamma * g;
    b[0] = nn.x * Nf; b[1] = nn.y * Nf; b[2] = nn.z * Nf;
    t = fr * n_alpha; b[3] = t * Nf;
    t = fr * n_beta; b[4] = t * Nf;
    t = fr * n_gamma; b[5] = t * Nf;
}

// Euler angles and translation of the last update as estimateCovariance reads them (lines 94-99); the angles are
// evaluated in fp64 from the fp32 matrix and rounded to fp32 (fp32 asin / atan2 differ between libraries by an ulp)
O3D_HD inline void pmx_update_angles(const float* dT /* row-major */, float* ang) {
    const double beta = -asin((double)dT[8]);
    const double alpha = atan2((double)dT[9], (double)dT[10]);
    const double cb = cos((double)(float)beta);
    const double gamma = atan2((double)(float)((double)dT[4] / cb), (double)(float)((double)dT[0] / cb));
    ang[0] = (float)alpha;
    ang[1] = (float)beta;
    ang[2] = (float)gamma;
    ang[3] = dT[3];
    ang[4] = dT[7];
    ang[5] = dT[11];
}

__global__ void __launch_bounds__(256)
k_pmx_cov_terms(const float4* __restrict__ src, int64_t n, int knn, const IterState* __restrict__ it, const int* __restrict__ kpos,
                const float* __restrict__ kw, const float4* __restrict__ tgt, const float4* __restrict__ tgt_nrm,
                const double* __restrict__ means /* k_pmx_reduce_rows of k_pmx_pair_means */, const PmExtraState* __restrict__ xs,
                double* __restrict__ rows) {
    const Xf T = pmx_load_xf_prev(it);
    const int64_t nk = n * (int64_t)knn;
    const double cnt = means[6];
    float mp[3], mq[3], ang[6], dT[16];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mp[k] = (float)(means[k] / cnt);
        mq[k] = (float)(means[3 + k] / cnt);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) dT[k] = xs->dT[k];
    pmx_update_angles(dT, ang);
    double acc[kPmxCovSums];
#pragma unroll
    for (int k = 0; k < kPmxCovSums; ++k) acc[k] = 0.0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nk; e += (int64_t)gridDim.x * blockDim.x) {
        const int pos = kpos[e];
        if (pos < 0 || kw[e] == 0.f) continue;
        const float4 s = src[e / knn];
        float3 p = xf_point(T, s.x, s.y, s.z);
        const float4 q4 = tgt[pos];
        const float4 n4 = tgt_nrm[2 * (size_t)pos + 1];
        p.x = p.x - mp[0]; p.y = p.y - mp[1]; p.z = p.z - mp[2];
        const float3 q = make_float3(q4.x - mq[0], q4.y - mq[1], q4.z - mq[2]);
        float v[6], a[6], b[6];
        pmx_cov_pair(p, q, make_float3(n4.x, n4.y, n4.z), ang, v, a, b);
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                const float hv = v[i] * v[j];
                const float ma = a[i] * a[j];
                const float mb = b[i] * b[j];
                acc[k] += (double)hv;
                acc[21 + k] += (double)ma;
                acc[21 + k] += (double)mb;
                ++k;
            }
    }
    block_sum_store<kPmxCovSums>(acc, rows + (size_t)blockIdx.x * kPmxCovSums);
}

__global__ void __launch_bounds__(256)
k_pmx_cov_finish(const double* __restrict__ rows, int n_rows, const double* __restrict__ means, float sigma,
                 PmCovOut* __restrict__ out) {
    __shared__ double tot[kPmxCovSums];
    pmx_sum_rows<kPmxCovSums>(rows, n_rows, tot);
    if (threadIdx.x < kPmxCovSums) out->sums[threadIdx.x] = tot[threadIdx.x];
    if (threadIdx.x != 0) return;
    const double cnt = means[6];
    out->n_pairs = cnt;
    for (int k = 0; k < 3; ++k) {
        out->mean_p[k] = (float)(means[k] / cnt);
        out->mean_q[k] = (float)(means[3 + k] / cnt);
    }
    double Hs[21], Ms[21];
    for (int k = 0; k < 21; ++k) {
        Hs[k] = tot[k];
        Ms[k] = tot[21 + k];
    }
    float cov[36];
    out->rank = pmx_censi_covariance(Hs, Ms, (double)sigma, cov);
    for (int k = 0; k < 36; ++k) out->cov[k] = cov[k];
}

// ErrorMinimizer statistics over the weights of the last iteration, one reading point per lane:
// rows: {sum w, pairs with w != 0, pairs with w == 0, points whose pairs all have w == 0, 0...}
__global__ void __launch_bounds__(256)
k_pmx_stats(const float* __restrict__ kw, int64_t n, int knn, double* __restrict__ rows) {
    double v[kPmxRow];
#pragma unroll
    for (int k = 0; k < kPmxRow; ++k) v[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int used = 0;
        for (int r = 0; r < knn; ++r) {
            const float w = kw[i * knn + r];
            v[0] += (double)w;
            if (w != 0.f) ++used;
        }
        v[1] += (double)used;
        v[2] += (double)(knn - used);
        if (used == 0) v[3] += 1.0;
    }
    block_sum_store<kPmxRow>(v, rows + (size_t)blockIdx.x * kPmxRow);
}
