// kernels_ransac.hpp -- RANSAC on feature correspondences (Open3D RegistrationRANSACBasedOnCorrespondence; the hypothesis
// loop of PlaceRecognition.cpp:78-91).  Numeric contract: include/o3dslam_reg.h.
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

constexpr int kRsMinN = 3, kRsMaxN = 8;   // ransac_n
constexpr int kRsTile = 256;              // correspondences staged in LDS at a time (12 KB)
constexpr int kRsChunk = REG_RANSAC_CHUNK;   // correspondences per partial sum of err2 (second grid dimension): part of the contract
constexpr int kRsEvalLanes = 64;          // hypotheses per workgroup of k_rs_eval: one wave
constexpr int kRsHeadRecords = 31;        // records the host reads with the header in one copy

// What the hypothesis kernel needs of reg_ransac_params
struct RsCfg {
    uint64_t seed;
    int64_t K;
    double sim;     // <= 0: no edge-length checker
    double thr2;    // fl(distance_threshold^2); < 0: no distance checker
};

// One record setter of a batch: 128 bytes, read by the host
struct RsRecord {
    int64_t iter;
    int32_t count, pad;
    double err2;
    double rt[12];   // R row-major, t
    double pad2;
};
static_assert(sizeof(RsRecord) == 128, "RsRecord is copied to the host in 128-byte units");

// Carried from batch to batch on the device: the best so far, and this batch's header
struct RsState {
    uint32_t n_rec, n_surv;   // header of the batch: records emitted, survivors
    int32_t best_count, pad;
    double best_err2;
    double pad2[13];
};
static_assert(sizeof(RsState) == 128, "the records start one unit after the state");

// The counter-based mixer of the contract (splitmix64's output for counter ctr of the stream `seed`), all mod 2^64; shared
// with the keys of reg_random_down_sample (kernels_scanprep.hpp) and with the host (reg_host_scan_key)
__host__ __device__ __forceinline__ uint64_t splitmix_key(uint64_t seed, uint64_t ctr) {
    uint64_t z = seed + (ctr + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__device__ __forceinline__ int64_t rs_draw(uint64_t seed, uint64_t ctr, int64_t K) {
    const uint64_t z = splitmix_key(seed, ctr);
    return (int64_t)(((z >> 32) * (uint64_t)K) >> 32);
}

// p = R s + t and the squared distance to q, in the contract's order
__device__ __forceinline__ double rs_d2(const double rt[12], double sx, double sy, double sz, double qx, double qy, double qz) {
    const double dx = (((rt[0] * sx + rt[1] * sy) + rt[2] * sz) + rt[9]) - qx;
    const double dy = (((rt[3] * sx + rt[4] * sy) + rt[5] * sz) + rt[10]) - qy;
    const double dz = (((rt[6] * sx + rt[7] * sy) + rt[8] * sz) + rt[11]) - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// One thread per correspondence: P[k] = (s_a, t_b); an index outside its cloud raises *bad (and leaves zeros).
__global__ void k_rs_gather(const double* __restrict__ src, int64_t n, const double* __restrict__ tgt, int64_t m,
                            const int32_t* __restrict__ corres, int64_t K, double* __restrict__ P, uint32_t* __restrict__ bad) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int64_t a = corres[2 * k], b = corres[2 * k + 1];
    const bool ok = a >= 0 && a < n && b >= 0 && b < m;
    if (!ok) atomicOr(bad, 1u);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        P[6 * k + c] = ok ? src[3 * a + c] : 0.0;
        P[6 * k + 3 + c] = ok ? tgt[3 * b + c] : 0.0;
    }
}

// Exchanges columns P and Q of A and V (and their singular values) when the later one is larger: branches, not selects,
// so that the matrices stay in registers
template <int P, int Q>
__device__ __forceinline__ void rs_order(double A[3][3], double V[3][3], double sg[3]) {
    if (sg[P] < sg[Q]) {
        double x = sg[P];
        sg[P] = sg[Q];
        sg[Q] = x;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            x = A[r][P], A[r][P] = A[r][Q], A[r][Q] = x;
            x = V[r][P], V[r][P] = V[r][Q], V[r][Q] = x;
        }
    }
}

// One Hestenes rotation: makes columns P and Q of A orthogonal (and carries V along); false: they already are, to 4e-16.
template <int P, int Q>
__device__ __forceinline__ bool rs_rotate(double A[3][3], double V[3][3]) {
    const double al = (A[0][P] * A[0][P] + A[1][P] * A[1][P]) + A[2][P] * A[2][P];
    const double be = (A[0][Q] * A[0][Q] + A[1][Q] * A[1][Q]) + A[2][Q] * A[2][Q];
    const double ga = (A[0][P] * A[0][Q] + A[1][P] * A[1][Q]) + A[2][P] * A[2][Q];
    if (ga == 0.0 || !(fabs(ga) > 4e-16 * sqrt(al * be))) return false;
    const double zeta = (be - al) / (2.0 * ga);
    const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double ap = A[r][P], aq = A[r][Q], vp = V[r][P], vq = V[r][Q];
        A[r][P] = cs * ap - sn * aq;
        A[r][Q] = sn * ap + cs * aq;
        V[r][P] = cs * vp - sn * vq;
        V[r][Q] = sn * vp + cs * vq;
    }
    return true;
}

// Rigid fit of N pairs (include/o3dslam_reg.h): H = sum (s - sm)(t - tm)^T = U S V^T by one-sided Jacobi (Hestenes) on H,
// which keeps small singular values relatively accurate; R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T over the two largest
// singular values, which is V diag(1, 1, det(V U^T)) U^T.  false: sigma_2 <= 1e-12 sigma_1.
template <int N>
__device__ __forceinline__ bool rs_fit(const double s[N][3], const double t[N][3], double rt[12]) {
    double sm[3], tm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double a = s[0][c], b = t[0][c];
#pragma unroll
        for (int j = 1; j < N; ++j) {
            a = a + s[j][c];
            b = b + t[j][c];
        }
        sm[c] = a / (double)N;
        tm[c] = b / (double)N;
    }
    double A[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double h = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) h = h + (s[j][r] - sm[r]) * (t[j][c] - tm[c]);
            A[r][c] = h;
            V[r][c] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 16; ++sweep) {
        bool rotated = rs_rotate<0, 1>(A, V);
        rotated |= rs_rotate<0, 2>(A, V);
        rotated |= rs_rotate<1, 2>(A, V);
        if (!rotated) break;
    }
    double sg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sg[c] = sqrt((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
    // the two largest singular values into columns 0 and 1 (a tie keeps the lower column first); exchanging columns of A
    // and V alike changes the sign of both cross products below, not their product
    rs_order<0, 1>(A, V, sg);
    rs_order<0, 2>(A, V, sg);
    rs_order<1, 2>(A, V, sg);
    if (sg[1] <= 1e-12 * sg[0]) return false;
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u1[r] = A[r][0] / sg[0];
        u2[r] = A[r][1] / sg[1];
        v1[r] = V[r][0];
        v2[r] = V[r][1];
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
    v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
    v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) rt[3 * r + c] = (v1[r] * u1[c] + v2[r] * u2[c]) + v3[r] * u3[c];
#pragma unroll
    for (int r = 0; r < 3; ++r) rt[9 + r] = tm[r] - ((rt[3 * r] * sm[0] + rt[3 * r + 1] * sm[1]) + rt[3 * r + 2] * sm[2]);
    return true;
}

// One thread per iteration b0 + x of the batch (x < nb; thread nb writes the closing flag, as k_mf_flags): sampling, the
// repeat test, the edge-length checker, the fit with its degeneracy test, the distance checker.  status[x] is the rule that
// failed (-1 .. -4) or 0 for a survivor, whose R, t go to hyp[12 x] and whose flag is 1.
template <int N>
__global__ void __launch_bounds__(256)
k_rs_hypo(const double* __restrict__ P, RsCfg cfg, int64_t b0, int nb, int32_t* __restrict__ status,
          double* __restrict__ hyp, uint32_t* __restrict__ flags) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x > nb) return;
    if (x == nb) {
        flags[x] = 0u;
        return;
    }
    const uint64_t ctr0 = (uint64_t)(b0 + x) * (uint64_t)N;
    int64_t idx[N];
#pragma unroll
    for (int j = 0; j < N; ++j) idx[j] = rs_draw(cfg.seed, ctr0 + (uint64_t)j, cfg.K);
    int st = 0;
#pragma unroll
    for (int u = 0; u < N; ++u)
#pragma unroll
        for (int v = u + 1; v < N; ++v)
            if (idx[u] == idx[v]) st = -1;
    double s[N][3], t[N][3];
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[j][c] = P[6 * idx[j] + c];
            t[j][c] = P[6 * idx[j] + 3 + c];
        }
    if (st == 0 && cfg.sim > 0.0) {
#pragma unroll
        for (int u = 0; u < N; ++u)
#pragma unroll
            for (int v = u + 1; v < N; ++v) {
                double dx = s[u][0] - s[v][0], dy = s[u][1] - s[v][1], dz = s[u][2] - s[v][2];
                const double ds = sqrt((dx * dx + dy * dy) + dz * dz);
                dx = t[u][0] - t[v][0], dy = t[u][1] - t[v][1], dz = t[u][2] - t[v][2];
                const double dt = sqrt((dx * dx + dy * dy) + dz * dz);
                if (ds < dt * cfg.sim || dt < ds * cfg.sim) st = -2;
            }
    }
    double rt[12];
    if (st == 0 && !rs_fit<N>(s, t, rt)) st = -3;
    if (st == 0 && cfg.thr2 >= 0.0) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (rs_d2(rt, s[j][0], s[j][1], s[j][2], t[j][0], t[j][1], t[j][2]) > cfg.thr2) st = -4;
    }
    status[x] = st;
    flags[x] = st == 0 ? 1u : 0u;
    if (st == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) hyp[12 * (size_t)x + e] = rt[e];
    }
}

// surv[j] = the batch position of the j-th survivor (offs: exclusive scan of flags)
__global__ void k_rs_compact(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs, int nb,
                             int32_t* __restrict__ surv) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < nb && flags[x]) surv[offs[x]] = x;
}

// Survivors x correspondences, the pattern of k_mf_search: each lane keeps one hypothesis (R, t) in registers; the
// correspondences of chunk blockIdx.y pass through LDS in tiles and are read as broadcasts.  Per lane an integer count and
// the sum of d2 over the inliers in ascending k, to part_cnt / part_err[chunk * cap + j].  The grid covers the whole batch;
// workgroups past the survivor count (offs[nb], read here) leave at once.
__global__ void __launch_bounds__(kRsEvalLanes)
k_rs_eval(const double* __restrict__ P, int64_t K, double maxd2, const double* __restrict__ hyp,
          const int32_t* __restrict__ surv, const uint32_t* __restrict__ offs, int nb, int cap, int32_t* __restrict__ part_cnt,
          double* __restrict__ part_err) {
    __shared__ double tile[kRsTile * 6];
    const int S = (int)offs[nb];
    if ((int)(blockIdx.x * kRsEvalLanes) >= S) return;   // the whole workgroup: nothing below is skipped by a part of it
    const int j = blockIdx.x * kRsEvalLanes + threadIdx.x;
    const int x = surv[j < S ? j : S - 1];
    double rt[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) rt[e] = hyp[12 * (size_t)x + e];
    const int64_t k0 = (int64_t)blockIdx.y * kRsChunk, k1 = k0 + kRsChunk < K ? k0 + kRsChunk : K;
    int32_t cnt = 0;
    double err = 0.0;
    for (int64_t tb = k0; tb < k1; tb += kRsTile) {
        const int rows = (int)(k1 - tb < kRsTile ? k1 - tb : kRsTile);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * 6; e += kRsEvalLanes) tile[e] = P[6 * (size_t)tb + e];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const double* c = tile + 6 * r;
            const double d2 = rs_d2(rt, c[0], c[1], c[2], c[3], c[4], c[5]);
            if (d2 < maxd2) {
                ++cnt;
                err = err + d2;
            }
        }
    }
    if (j < S) {
        part_cnt[(size_t)blockIdx.y * cap + j] = cnt;
        part_err[(size_t)blockIdx.y * cap + j] = err;
    }
}

// Adds the chunk partials in chunk order; the survivor's status becomes its inlier count.
__global__ void k_rs_merge(const int32_t* __restrict__ part_cnt, const double* __restrict__ part_err, const uint32_t* __restrict__ offs,
                           int nb, int cap, int n_chunks, const int32_t* __restrict__ surv, int32_t* __restrict__ cnt,
                           double* __restrict__ err, int32_t* __restrict__ status) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (int)offs[nb]) return;
    int32_t c = part_cnt[j];
    double e = part_err[j];
    for (int ch = 1; ch < n_chunks; ++ch) {
        c += part_cnt[(size_t)ch * cap + j];
        e = e + part_err[(size_t)ch * cap + j];
    }
    cnt[j] = c;
    err[j] = e;
    status[surv[j]] = c;
}

// One wave: walks the batch's survivors in iteration order against the best carried in st and emits every hypothesis
// that replaces it (count > 0, and a larger count or an equal count with a smaller err2; a tie keeps the earlier) as a
// record.  Lanes test 64 survivors at a time; the first that beats the running best becomes it, and the later lanes are
// tested again -- as many rounds as there are records.
__global__ void __launch_bounds__(64)
k_rs_records(const int32_t* __restrict__ cnt, const double* __restrict__ err, const int32_t* __restrict__ surv,
             const double* __restrict__ hyp, const uint32_t* __restrict__ offs, int nb, int64_t b0, RsState* __restrict__ st,
             RsRecord* __restrict__ rec) {
    const int lane = threadIdx.x;
    const int S = (int)offs[nb];
    int32_t best_c = st->best_count;
    double best_e = st->best_err2;
    uint32_t n_rec = 0;
    for (int base = 0; base < S; base += 64) {
        const int j = base + lane;
        const int32_t c = j < S ? cnt[j] : 0;
        const double e = j < S ? err[j] : 0.0;
        int from = 0;   // lanes below `from` have been passed
        while (true) {
            const bool better = lane >= from && c > 0 && (c > best_c || (c == best_c && e < best_e));
            const unsigned long long bal = __ballot(better);
            if (!bal) break;
            const int f = __ffsll((long long)bal) - 1;
            best_c = __shfl(c, f);
            best_e = __shfl(e, f);
            const int x = surv[base + f];
            if (lane == 0) {
                rec[n_rec].iter = b0 + x;
                rec[n_rec].count = best_c;
                rec[n_rec].pad = 0;
                rec[n_rec].err2 = best_e;
            }
            if (lane < 12) rec[n_rec].rt[lane] = hyp[12 * (size_t)x + lane];
            ++n_rec;
            from = f + 1;
        }
    }
    if (lane == 0) {
        st->n_rec = n_rec;
        st->n_surv = (uint32_t)S;
        st->best_count = best_c;
        st->best_err2 = best_e;
    }
}

// flags[k] = 1 when correspondence k is an inlier of (R, t) -- the test of k_rs_eval; thread K writes the closing 0.
struct RsPose {
    double rt[12];
};
__global__ void k_rs_inlier_flags(const double* __restrict__ P, int64_t K, RsPose pose, double maxd2, uint32_t* __restrict__ flags) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k > K) return;
    bool in = false;
    if (k < K) {
        const double* c = P + 6 * k;
        in = rs_d2(pose.rt, c[0], c[1], c[2], c[3], c[4], c[5]) < maxd2;
    }
    flags[k] = in ? 1u : 0u;
}

__global__ void k_rs_collect(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs, int64_t K,
                             const int32_t* __restrict__ corres, int32_t* __restrict__ out) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= K || !flags[k]) return;
    out[2 * (size_t)offs[k]] = corres[2 * k];
    out[2 * (size_t)offs[k] + 1] = corres[2 * k + 1];
}
