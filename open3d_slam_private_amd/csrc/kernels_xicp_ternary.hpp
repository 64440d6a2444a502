// kernels_xicp_ternary.hpp -- degeneracyAwareness EqualityConstraints (X-ICP, ternary) on the chain's generic iteration
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
//
// Every iteration of a handle with the method on (host_loop.hpp: enqueue_pm_iteration), after k_pm_linearize:
//   k_pm_update<true, true> (finish = 0)   reduce A, b; eigenvectors of both 3x3 blocks (data and optimisation frame)
//   k_xt_center                            matched pairs -> data frame, per-workgroup rows {sum x, y, z, count}
//   k_xt_detect                            centre (fixed-order sum of those rows), both alignment vectors, the 24 sums
//                                          combined[6], high[6], n_combined[6], n_high[6] -> per-workgroup rows
//   k_xt_decide                            fixed-order sum of the rows; one lane decides the six categories and writes the
//                                          6-bit mask of partial directions and their sampling predicates
//   k_xt_partial                           returns at once when the mask is empty; otherwise recomputes the alignments
//                                          (no N x 6 buffer) and sums the nine terms of each masked direction over its sample
//   k_pm_update<true, true> (finish = 1)   constraint values, sanity rule, KKT solve with its right-hand side, update,
//                                          checkers, mirror
// Stream-ordered, no host round trip.  No floating-point atomics: the rows are added in a fixed order, so two registrations
// of the same inputs return identical bits.  Arithmetic of the alignments: kernels_xicp.hpp (fp32, one rounding per
// operation); sums in fp64.
#pragma once

constexpr int kXtBlocks = 256;   // workgroups of the three passes over the pairs (grid-stride)
constexpr int kXtDet = 24;       // combined[6], high[6], n_combined[6], n_high[6] (counts as doubles: exact)
constexpr int kXtPart = 54;      // nine sums for each of the six directions
// layout of the rows buffer (doubles)
constexpr size_t kXtRowsCenter = 0, kXtRowsDet = (size_t)kXtBlocks * 4, kXtRowsPart = kXtRowsDet + (size_t)kXtBlocks * kXtDet;
constexpr size_t kXtRowsTotal = kXtRowsPart + (size_t)kXtBlocks * kXtPart;

// Device-resident state of the method, one per handle; written by the host at the start of every registration
struct XtState {
    // configuration
    float high_thr, enough_thr, insufficient_thr, cos_min, cos_strong;
    float Trd[12];            // T_refMean_dataIn (row-major 3x4), as IterState::xicp_Trd
    // this iteration
    int stage;                // 1: the analysis kernels of this iteration run
    int mask;                 // bit k: direction k is partial
    int pred[6];              // sampling predicate of a partial direction: 1: a >= cos_min, 2: a > cos_strong
    float vr[9], vt[9];       // eigenvectors in the data frame, [k * 3 + r]
    float vo[18];             // ... in the optimisation frame: rotation 0-8, translation 9-17
    double center[4];         // sum of the matched reading points (data frame) and their count
    // results of the last analysed iteration (reg_get_ternary_xicp)
    int valid, iteration, sane, pad;
    int cat[6];
    double comb[6], high[6];
    long long n_comb[6], n_high[6];
    long long n_pairs;
    float constraint[6];
    double psums[kXtPart];
};

// Eigenvectors of one 3x3 block (o = 0: rotation, 3: translation) of the system: upd_xicp_stage_a, which also keeps the
// optimisation-frame vectors (the fp32 rounding of the decomposition, before the rotation into the data frame)
__device__ __noinline__ void xt_stage_a(const double* tot, const float* Trd, float* dst_data, float* dst_opt, int o) {
    double S[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int lo = (i < j ? i : j) + o, hi = (i < j ? j : i) + o;
            S[3 * i + j] = (double)(float)tot[lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];
        }
    eig3_desc(S, V);
    for (int kk = 0; kk < 3; ++kk)
        for (int rr = 0; rr < 3; ++rr) {
            const float a0 = Trd[rr] * (float)V[kk], a1 = Trd[4 + rr] * (float)V[3 + kk];
            const float a2 = Trd[8 + rr] * (float)V[6 + kk];
            const float sacc = a0 + a1;
            dst_data[3 * kk + rr] = sacc + a2;
            dst_opt[3 * kk + rr] = (float)V[3 * rr + kk];
        }
}

__global__ void __launch_bounds__(256)
k_xt_center(const float4* __restrict__ src, int64_t n, const IterState* __restrict__ it, const int* __restrict__ pos,
            const float* __restrict__ w, const XtState* __restrict__ xt, double* __restrict__ rows) {
    if (it->done || xt->stage != 1) return;
    const Xf T = load_xf(it);
    float Trd[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Trd[k] = xt->Trd[k];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (pos[i] < 0 || w[i] == 0.f) continue;
        const float4 s = src[i];
        const float3 ps = xicp_to_data_frame_point(Trd, xf_point(T, s.x, s.y, s.z));
        v[0] += (double)ps.x;
        v[1] += (double)ps.y;
        v[2] += (double)ps.z;
        v[3] += 1.0;
    }
    block_sum_store<4>(v, rows + kXtRowsCenter + (size_t)blockIdx.x * 4);
}

// Both alignment vectors of one pair against the six eigenvectors: ar[k] rotation, at[k] translation (k_xicp_detect)
struct XtFrame {
    float Trd[12], vr[9], vt[9], c[3];
};
__device__ __forceinline__ void xt_alignments(const XtFrame& f, const float3 p, const float4 nr, float* ar, float* at) {
    float3 ps = xicp_to_data_frame_point(f.Trd, p);
    ps.x = ps.x - f.c[0];
    ps.y = ps.y - f.c[1];
    ps.z = ps.z - f.c[2];
    const float3 nn = xicp_to_data_frame_vec(f.Trd, nr.x, nr.y, nr.z);
    float cr[3];
    float u, q;
    u = ps.y * nn.z; q = ps.z * nn.y; cr[0] = u - q;
    u = ps.z * nn.x; q = ps.x * nn.z; cr[1] = u - q;
    u = ps.x * nn.y; q = ps.y * nn.x; cr[2] = u - q;
    const float nrm = sqrtf(sum_sq3(cr[0], cr[1], cr[2]));
    if (!(nrm < 1.0f)) {
        cr[0] = cr[0] / nrm;
        cr[1] = cr[1] / nrm;
        cr[2] = cr[2] / nrm;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float a0 = cr[0] * f.vr[3 * k], a1 = cr[1] * f.vr[3 * k + 1], a2 = cr[2] * f.vr[3 * k + 2];
        float sacc = a0 + a1;
        ar[k] = fabsf(sacc + a2);
        a0 = nn.x * f.vt[3 * k];
        a1 = nn.y * f.vt[3 * k + 1];
        a2 = nn.z * f.vt[3 * k + 2];
        sacc = a0 + a1;
        at[k] = fabsf(sacc + a2);
    }
}

// The centre of the matched pairs from the rows of k_xt_center (every workgroup adds them in the same fixed order), and
// the frame of the analysis
__device__ __forceinline__ void xt_load_frame(const XtState* __restrict__ xt, const double* __restrict__ rows, int n_rows,
                                              XtFrame& f, double* cen /* LDS, 4 */) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if ((int)threadIdx.x < n_rows) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = rows[kXtRowsCenter + (size_t)threadIdx.x * 4 + k];
    }
    block_sum_store<4>(v, cen);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; ++k) f.Trd[k] = xt->Trd[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        f.vr[k] = xt->vr[k];
        f.vt[k] = xt->vt[k];
    }
    const double cnt = cen[3];
    f.c[0] = f.c[1] = f.c[2] = 0.f;
    if (cnt > 0.0) {
        f.c[0] = (float)(cen[0] / cnt);
        f.c[1] = (float)(cen[1] / cnt);
        f.c[2] = (float)(cen[2] / cnt);
    }
}

// n_rows = workgroups of this launch and of k_xt_center (<= kXtBlocks = 256 = the lanes that load one row each)
__global__ void __launch_bounds__(256)
k_xt_detect(const float4* __restrict__ src, int64_t n, const IterState* __restrict__ it, const int* __restrict__ pos,
            const float* __restrict__ w, const float4* __restrict__ tgt_nrm, XtState* __restrict__ xt, double* __restrict__ rows) {
    __shared__ double cen[4];
    if (it->done || xt->stage != 1) return;
    XtFrame f;
    xt_load_frame(xt, rows, (int)gridDim.x, f, cen);
    if (blockIdx.x == 0 && threadIdx.x < 4) xt->center[threadIdx.x] = cen[threadIdx.x];
    const Xf T = load_xf(it);
    const float cos_min = xt->cos_min, cos_strong = xt->cos_strong;
    double v[kXtDet];
#pragma unroll
    for (int k = 0; k < kXtDet; ++k) v[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = pos[i];
        if (j < 0 || w[i] == 0.f) continue;
        const float4 s = src[i];
        const float4 nr = tgt_nrm[2 * (size_t)j + 1];   // {point, normal} pairs
        float ar[3], at[3];
        xt_alignments(f, xf_point(T, s.x, s.y, s.z), nr, ar, at);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (ar[k] >= cos_min) { v[k] += (double)ar[k]; v[12 + k] += 1.0; }
            if (ar[k] > cos_strong) { v[6 + k] += (double)ar[k]; v[18 + k] += 1.0; }
            if (at[k] >= cos_min) { v[3 + k] += (double)at[k]; v[15 + k] += 1.0; }
            if (at[k] > cos_strong) { v[9 + k] += (double)at[k]; v[21 + k] += 1.0; }
        }
    }
    block_sum_store<kXtDet>(v, rows + kXtRowsDet + (size_t)blockIdx.x * kXtDet);
}

// One workgroup: the 24 totals in a fixed order, then the decision on one lane
__global__ void __launch_bounds__(256)
k_xt_decide(const IterState* __restrict__ it, XtState* __restrict__ xt, const double* __restrict__ rows, int n_rows) {
    __shared__ double tot[kXtDet];
    if (it->done || xt->stage != 1) return;
    pmx_sum_rows<kXtDet>(rows + kXtRowsDet, n_rows, tot);
    if (threadIdx.x != 0) return;
    double comb[6], high[6];
    long long nc[6], nh[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        comb[k] = tot[k];
        high[k] = tot[6 + k];
        nc[k] = (long long)tot[12 + k];
        nh[k] = (long long)tot[18 + k];
    }
    const long long n_pairs = (long long)xt->center[3];
    int cat[6];
    const int sane = xicp_ternary_decide(comb, high, nc, nh, n_pairs, xt->high_thr, xt->enough_thr, xt->insufficient_thr, cat);
    int mask = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int pr = cat[k] == kXtPartialMixed ? 1 : (cat[k] == kXtPartialHigh ? 2 : 0);
        xt->pred[k] = pr;
        if (pr != 0) mask |= 1 << k;
        xt->cat[k] = cat[k];
        xt->comb[k] = comb[k];
        xt->high[k] = high[k];
        xt->n_comb[k] = nc[k];
        xt->n_high[k] = nh[k];
    }
    xt->n_pairs = n_pairs;
    xt->sane = sane;
    xt->mask = sane ? mask : 0;   // a failed sanity rule returns the prior: no partial problem is needed
}

// The nine sums of every masked direction over its sample, in the optimisation frame: f = p x n (rotation) or n
// (translation), r = n . (p - q) as k_pm_linearize forms them; fp32 products, fp64 sums, no weights
__global__ void __launch_bounds__(256)
k_xt_partial(const float4* __restrict__ src, int64_t n, const IterState* __restrict__ it, const int* __restrict__ pos,
             const float* __restrict__ w, const float4* __restrict__ tgt, const float4* __restrict__ tgt_nrm,
             const XtState* __restrict__ xt, double* __restrict__ rows) {
    __shared__ double cen[4];
    if (it->done || xt->stage != 1) return;
    const int mask = xt->mask;
    if (mask == 0) return;
    XtFrame f;
    xt_load_frame(xt, rows, (int)gridDim.x, f, cen);
    const Xf T = load_xf(it);
    const float cos_min = xt->cos_min, cos_strong = xt->cos_strong;
    int pred[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pred[k] = xt->pred[k];
    double v[kXtPart];
#pragma unroll
    for (int k = 0; k < kXtPart; ++k) v[k] = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = pos[i];
        if (j < 0 || w[i] == 0.f) continue;
        const float4 s = src[i];
        const float3 p = xf_point(T, s.x, s.y, s.z);
        const float4 nn = tgt_nrm[2 * (size_t)j + 1];
        float al[6];
        xt_alignments(f, p, nn, al, al + 3);
        bool any = false;
        bool in[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            in[k] = (pred[k] == 1 && al[k] >= cos_min) || (pred[k] == 2 && al[k] > cos_strong);
            any = any || in[k];
        }
        if (!any) continue;
        const float4 q = tgt[j];
        const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
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
        float pr[18];   // products of the rotation block (0-8) and of the translation block (9-17)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const float* e = F + 3 * g;
            pr[9 * g + 0] = e[0] * e[0];
            pr[9 * g + 1] = e[0] * e[1];
            pr[9 * g + 2] = e[0] * e[2];
            pr[9 * g + 3] = e[1] * e[1];
            pr[9 * g + 4] = e[1] * e[2];
            pr[9 * g + 5] = e[2] * e[2];
            pr[9 * g + 6] = e[0] * r;
            pr[9 * g + 7] = e[1] * r;
            pr[9 * g + 8] = e[2] * r;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (in[k]) {
#pragma unroll
                for (int c = 0; c < 9; ++c) v[9 * k + c] += (double)pr[9 * (k / 3) + c];
            }
    }
    block_sum_store<kXtPart>(v, rows + kXtRowsPart + (size_t)blockIdx.x * kXtPart);
}

// Finish of the analysis on the lane of k_pm_update that solves: constraint values of the partial directions, flags and
// sums into the iteration state, the right-hand side of the KKT system.  Returns 1 when the prior is to be returned
// (sanity rule, or a constraint value that is not finite).
__device__ __noinline__ int xt_finish(XtState* xt, const double* ptot /* kXtPart totals; read only for masked directions */,
                                      IterState* it, float* rhs) {
    const int mask = xt->mask;
    int prior = xt->sane ? 0 : 1;
    int nc = 0;
    for (int k = 0; k < 6; ++k) {
        float val = 0.f;
        double s9[9];
        for (int c = 0; c < 9; ++c) s9[c] = 0.0;
        if ((mask >> k) & 1) {
            for (int c = 0; c < 9; ++c) s9[c] = ptot[9 * k + c];
            val = xicp_partial_constraint(s9, xt->vo + 3 * k);
            if (!(val - val == 0.f)) prior = 1;
        }
        for (int c = 0; c < 9; ++c) xt->psums[9 * k + c] = s9[c];
        xt->constraint[k] = val;
        rhs[k] = val;
        const int ok = xt->cat[k] == kXtLocalizable ? 1 : 0;
        it->xicp_flags[k] = ok;
        it->xicp_comb[k] = xt->comb[k];
        it->xicp_high[k] = xt->high[k];
        nc += ok ? 0 : 1;
    }
    it->xicp_nc = nc;
    xt->iteration = it->iterations + 1;
    xt->valid = 1;
    xt->stage = 0;
    return prior;
}

__device__ __noinline__ int upd_solve6_xicp_rhs(const double* tot, const int* flags, const float* rhs, float* x_out) {
    float H[36], b6[6], x[6], d[6];
    int fl[6];
    upd_load_sym6(tot, H, b6);
    for (int i = 0; i < 6; ++i) {
        d[i] = rhs[i];
        fl[i] = flags[i];
    }
    const int rank = solve6_xicp_rhs(H, b6, fl, d, x);
    for (int i = 0; i < 6; ++i) x_out[i] = x[i];
    return rank;
}
