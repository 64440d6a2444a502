// kernels_pmoutliers.hpp -- VarTrimmedDistOutlierFilter of the libpointmatcher chain on the device (DESIGN.md 5i;
// contract in include/o3dslam_reg.h).  MinDist and MedianDist need no kernel of their own: a comparison in
// k_pm_linearize, and for MedianDist one more exact select (kernels_pmchain.hpp).
// Part of the single translation unit reg_core.hip (included after kernels_pmchain.hpp; not a standalone header).
//
// Per iteration (host_loop.hpp: enqueue_pm_var_trim), on the N*knn squared distances of k_match_knn:
//   rocprim::radix_sort_keys        the fp32 bit patterns ascending (d2 >= 0: monotone; +inf last) into a scratch buffer.
//                                   Not gated by the loop state: it only writes scratch.
//   k_pm_var_block_sums             per tile of kVarTile sorted keys: fp64 sum of the finite keys, zeros, finite keys
//   k_pm_var_scan_blocks            one workgroup: exclusive fp64 scan of the tile sums in tile order, the totals
//                                   (zeros, finite) and the candidate range [lo, hi) -> VarState
//   k_pm_var_objective              per tile that meets the range: S(j) for its keys, FRMS(j) (pm_var_frms), the tile's
//                                   (minimum, lowest index)
//   k_pm_var_finish                 one workgroup: argmin over the tiles (lowest index on ties), k, optRatio and
//                                   limit = sorted[pm_quantile_rank(n_finite, optRatio)] -> PmState
// The zeros sort in front of v and add exactly 0.0, so the prefix sums run over sorted POSITIONS p and j = p - n_zero.
// Summation order of S (fixed, hence deterministic): inside a thread its kVarItems consecutive keys in order; the
// threads of a wave by a shuffle scan (distances 1, 2, ... 32); the four waves in order; the tile offsets the same way
// over the tile sums (k_pm_var_scan_blocks: each thread a run of consecutive tiles).
//   S(p) = (tile offset + (offset of the thread's run inside the tile)) + running sum inside the run
// fp64 only here: the scan and the objective.  Every kernel returns at once when the loop is done.
#pragma once

constexpr int kVarItems = 8;                 // consecutive keys per thread: two 16-byte loads
constexpr int kVarTile = 256 * kVarItems;    // keys per workgroup

// What k_pm_var_scan_blocks leaves for the two kernels after it
struct VarState {
    long long n_zero, n_finite;   // v[j] = sorted[n_zero + j], m = n_finite - n_zero
    long long lo, hi;             // candidates j in [lo, hi) (pm_var_range); empty: k = m - 1
};

// This thread's kVarItems keys at `base` (a multiple of kVarItems); positions past nk read as +inf
__device__ __forceinline__ void var_load_keys(const uint32_t* __restrict__ sk, int64_t base, int64_t nk, uint32_t (&u)[kVarItems]) {
    if (base + kVarItems <= nk) {
        const uint4 a = reinterpret_cast<const uint4*>(sk + base)[0];
        const uint4 b = reinterpret_cast<const uint4*>(sk + base)[1];
        u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
        u[4] = b.x; u[5] = b.y; u[6] = b.z; u[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < kVarItems; ++k) u[k] = base + k < nk ? sk[base + k] : 0x7f800000u;
    }
}

__device__ __forceinline__ bool var_key_finite(uint32_t u) { return u < 0x7f800000u; }

// Exclusive prefix of t over the 256 threads in thread order, and the block total.  Shuffles inside a wave, the four
// wave totals through LDS (no scan lives in LDS).
__device__ __forceinline__ double var_block_scan(double t, double* wave_tot /*[4]*/, double* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double incl = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    double ex = __shfl_up(incl, 1);
    if (lane == 0) ex = 0.0;
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    double base = 0.0, tot = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const double v = wave_tot[w];
        if (w < wave) base += v;
        tot += v;
    }
    *total = tot;
    __syncthreads();
    return base + ex;
}

// (f1, j1) before (f2, j2): the smaller objective, the lower index on ties; j < 0 = no candidate
__device__ __forceinline__ bool var_better(double f1, long long j1, double f2, long long j2) {
    if (j1 < 0) return false;
    if (j2 < 0) return true;
    return f1 < f2 || (f1 == f2 && j1 < j2);
}

__device__ __forceinline__ void var_wave_argmin(double& f, long long& j) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double of = __shfl_xor(f, o);
        const long long oj = __shfl_xor(j, o);
        if (var_better(of, oj, f, j)) {
            f = of;
            j = oj;
        }
    }
}

__global__ void __launch_bounds__(256)
k_pm_var_block_sums(const uint32_t* __restrict__ sk, int64_t nk, double* __restrict__ bsum, uint2* __restrict__ bcnt,
                    const IterState* __restrict__ it) {
    __shared__ double wave_tot[4];
    __shared__ uint32_t cnt[4][2];
    if (it->done) return;
    uint32_t u[kVarItems];
    var_load_keys(sk, blockIdx.x * (int64_t)kVarTile + (int64_t)threadIdx.x * kVarItems, nk, u);
    double t = 0.0;
    uint32_t nz = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < kVarItems; ++k)
        if (var_key_finite(u[k])) {
            ++nf;
            nz += u[k] == 0u ? 1u : 0u;
            t += (double)__uint_as_float(u[k]);
        }
    double total;
    (void)var_block_scan(t, wave_tot, &total);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        nz += (uint32_t)__shfl_xor((int)nz, o);
        nf += (uint32_t)__shfl_xor((int)nf, o);
    }
    if ((threadIdx.x & 63) == 0) {
        cnt[threadIdx.x >> 6][0] = nz;
        cnt[threadIdx.x >> 6][1] = nf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = total;
        bcnt[blockIdx.x] = make_uint2(cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0], cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1]);
    }
}

// One workgroup: thread t owns the tiles [t * chunk, (t + 1) * chunk) in order
__global__ void __launch_bounds__(256)
k_pm_var_scan_blocks(const double* __restrict__ bsum, const uint2* __restrict__ bcnt, int nb, double* __restrict__ boff,
                     VarState* __restrict__ vs, int64_t n, float min_ratio, float max_ratio, const IterState* __restrict__ it) {
    __shared__ double wave_tot[4];
    __shared__ unsigned long long cnt[4][2];
    if (it->done) return;
    const int chunk = (nb + 255) / 256;
    const int b0 = (int)threadIdx.x * chunk, b1 = min(nb, b0 + chunk);
    double t = 0.0;
    unsigned long long nz = 0, nf = 0;
    for (int b = b0; b < b1; ++b) {
        t += bsum[b];
        const uint2 c = bcnt[b];
        nz += c.x;
        nf += c.y;
    }
    double total;
    double run = var_block_scan(t, wave_tot, &total);
    for (int b = b0; b < b1; ++b) {
        boff[b] = run;
        run += bsum[b];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        nz += (unsigned long long)__shfl_xor((long long)nz, o);
        nf += (unsigned long long)__shfl_xor((long long)nf, o);
    }
    if ((threadIdx.x & 63) == 0) {
        cnt[threadIdx.x >> 6][0] = nz;
        cnt[threadIdx.x >> 6][1] = nf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long z = (long long)(cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0]);
        const long long f = (long long)(cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1]);
        int64_t lo, hi;
        pm_var_range(n, f - z, min_ratio, max_ratio, &lo, &hi);
        vs->n_zero = z;
        vs->n_finite = f;
        vs->lo = lo;
        vs->hi = hi;
    }
}

__global__ void __launch_bounds__(256)
k_pm_var_objective(const uint32_t* __restrict__ sk, int64_t nk, const double* __restrict__ boff, const VarState* __restrict__ vs,
                   int64_t n, double two_lambda, double* __restrict__ bval, long long* __restrict__ bidx,
                   const IterState* __restrict__ it) {
    __shared__ double wave_tot[4];
    __shared__ double wf[4];
    __shared__ long long wj[4];
    if (it->done) return;
    const long long nz = vs->n_zero, lo = vs->lo, hi = vs->hi;
    const int64_t p0 = blockIdx.x * (int64_t)kVarTile;
    if (lo >= hi || p0 + kVarTile <= nz + lo || p0 >= nz + hi) {   // the same for the whole workgroup
        if (threadIdx.x == 0) {
            bval[blockIdx.x] = INFINITY;
            bidx[blockIdx.x] = -1;
        }
        return;
    }
    const int64_t base = p0 + (int64_t)threadIdx.x * kVarItems;
    uint32_t u[kVarItems];
    var_load_keys(sk, base, nk, u);
    double r[kVarItems];
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kVarItems; ++k) {
        if (var_key_finite(u[k])) t += (double)__uint_as_float(u[k]);
        r[k] = t;
    }
    double total;
    const double ex = var_block_scan(t, wave_tot, &total);
    const double off = boff[blockIdx.x] + ex;
    double best = INFINITY;
    long long bj = -1;
#pragma unroll
    for (int k = 0; k < kVarItems; ++k) {
        const long long j = base + k - nz;
        if (j >= lo && j < hi) {
            const double f = pm_var_frms(off + r[k], j, n, two_lambda);
            if (var_better(f, j, best, bj)) {
                best = f;
                bj = j;
            }
        }
    }
    var_wave_argmin(best, bj);
    if ((threadIdx.x & 63) == 0) {
        wf[threadIdx.x >> 6] = best;
        wj[threadIdx.x >> 6] = bj;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (var_better(wf[w], wj[w], best, bj)) {
                best = wf[w];
                bj = wj[w];
            }
        bval[blockIdx.x] = best;
        bidx[blockIdx.x] = bj;
    }
}

__global__ void __launch_bounds__(256)
k_pm_var_finish(const uint32_t* __restrict__ sk, const double* __restrict__ bval, const long long* __restrict__ bidx, int nb,
                const VarState* __restrict__ vs, int64_t n, PmState* __restrict__ ps, const IterState* __restrict__ it) {
    __shared__ double wf[4];
    __shared__ long long wj[4];
    if (it->done) return;
    double best = INFINITY;
    long long bj = -1;
    for (int b = threadIdx.x; b < nb; b += 256) {
        const double f = bval[b];
        const long long j = bidx[b];
        if (var_better(f, j, best, bj)) {
            best = f;
            bj = j;
        }
    }
    var_wave_argmin(best, bj);
    if ((threadIdx.x & 63) == 0) {
        wf[threadIdx.x >> 6] = best;
        wj[threadIdx.x >> 6] = bj;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w)
        if (var_better(wf[w], wj[w], best, bj)) {
            best = wf[w];
            bj = wj[w];
        }
    const long long m = vs->n_finite - vs->n_zero;
    ps->var_n = n;
    ps->var_valid = 1;
    if (m <= 0) {   // "Inlier ratio optimization failed due to absence of matches"
        ps->fail = 1;
        ps->var_k = -1;
        ps->var_ratio = 0.f;
        ps->var_limit = INFINITY;
        return;
    }
    const long long k = bj >= 0 ? bj : m - 1;
    const float ratio = (float)k / (float)n;
    ps->var_k = k;
    ps->var_ratio = ratio;
    ps->var_limit = __uint_as_float(sk[pm_quantile_rank((uint32_t)vs->n_finite, ratio)]);
}
