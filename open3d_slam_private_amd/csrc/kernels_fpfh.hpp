// kernels_fpfh.hpp -- FPFH features (Open3D ComputeFPFHFeature with a hybrid search) and nearest-neighbour matching of
// feature rows (the front of RegistrationRANSACBasedOnFeatureMatching).  Numeric contract: include/o3dslam_reg.h.
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

constexpr int kFpfhDim = 33;
constexpr int kFpfhMaxNn = 128;   // largest max_nn: two neighbours per lane of a wave
constexpr int kFpfhWaves = 4;     // query points per workgroup, one wave each
constexpr int kFpfhCap = 1024;    // candidate keys per query point held in LDS (8 B each: 32 KB per workgroup)

// (d2, original index) as one ascending key: d2 >= 0, so its bit pattern orders like its value
__device__ __forceinline__ uint64_t fpfh_key(float d2, uint32_t idx) {
    return ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)idx;
}

// One thread per point: a non-finite coordinate or normal component raises *bad.
__global__ void k_fpfh_check(const float* __restrict__ xyz, int64_t xs, const float* __restrict__ nrm, int64_t ns, int64_t n,
                             uint32_t* __restrict__ bad) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = xyz + (size_t)i * xs;
    const float* q = nrm + (size_t)i * ns;
    // x - x is 0 for every finite x and NaN otherwise
    const float s = ((p[0] - p[0]) + (p[1] - p[1])) + (p[2] - p[2]) + ((q[0] - q[0]) + (q[1] - q[1])) + (q[2] - q[2]);
    if (!(s == 0.f)) atomicOr(bad, 1u);
}

// Calls f(target point, d2) for every target point inside the bin box of level l around p that lies within max_dist: the
// rows of level_box, dealt to the 64 lanes of one wave (a lane walks its row_run alone, so f may not synchronise).
template <class F>
__device__ __forceinline__ void fpfh_scan_box(const Grid& g, const float3 p, int l, int lane, F&& f) {
    const LevelBox b = level_box(g, p, l);
    for (int64_t t = lane; t < b.total; t += 64) {
        uint32_t s, e;
        row_run(g, b, t, s, e);
        for (uint32_t j = s; j < e; ++j) {
            const float4 tpt = g.pts[j];
            const float d2 = nc5_d2(p, tpt);
            if (d2 <= g.max_d2) f(tpt, d2);
        }
    }
}

__device__ __forceinline__ double fpfh_dot(const double a[3], const double b[3]) {
    double s = a[0] * b[0];
    double t = a[1] * b[1];
    s = s + t;
    t = a[2] * b[2];
    return s + t;
}
__device__ __forceinline__ void fpfh_cross(const double a[3], const double b[3], double c[3]) {
    double u = a[1] * b[2], v = a[2] * b[1];
    c[0] = u - v;
    u = a[2] * b[0], v = a[0] * b[2];
    c[1] = u - v;
    u = a[0] * b[1], v = a[1] * b[0];
    c[2] = u - v;
}
__device__ __forceinline__ int fpfh_bin(double t) {
    t = floor(t);
    if (!(t >= 0.0)) t = 0.0;
    if (t > 10.0) t = 10.0;
    return (int)t;
}

// The three bins of the pair (i, j) (include/o3dslam_reg.h, "pair feature").
__device__ __forceinline__ void fpfh_pair_bins(const double pi[3], const double ni[3], const double pj[3], const double nj[3],
                                               int bins[3]) {
    const double kPi = 3.14159265358979323846;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    double d[3] = {pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]};
    const double L = sqrt(fpfh_dot(d, d));
    if (L != 0.0) {
        const double a1 = fpfh_dot(ni, d) / L, a2 = fpfh_dot(nj, d) / L;
        const bool swap = fabs(a1) < fabs(a2);
        double n1[3], n2[3];
        for (int k = 0; k < 3; ++k) {
            n1[k] = swap ? nj[k] : ni[k];
            n2[k] = swap ? ni[k] : nj[k];
            if (swap) d[k] = -d[k];
        }
        const double g2 = swap ? -a2 : a1;
        double v[3], w[3];
        fpfh_cross(d, n1, v);
        const double vn = sqrt(fpfh_dot(v, v));
        if (vn != 0.0) {
            for (int k = 0; k < 3; ++k) v[k] = v[k] / vn;
            fpfh_cross(n1, v, w);
            f2 = g2;
            f1 = fpfh_dot(v, n2);
            f0 = atan2(fpfh_dot(w, n2), fpfh_dot(n1, n2));
        }
    }
    double t = f0 + kPi;
    t = 11.0 * t;
    bins[0] = fpfh_bin(t / (2.0 * kPi));
    t = f1 + 1.0;
    t = 11.0 * t;
    bins[1] = fpfh_bin(t * 0.5);
    t = f2 + 1.0;
    t = 11.0 * t;
    bins[2] = fpfh_bin(t * 0.5);
}

// Neighbourhoods and SPFH counts, one wave per query point.  Per radius level the wave gathers every point of the bin box
// (within radius) as a (d2, index) key into its LDS list and sorts the list (bitonic); the max_nn-th key <= rho^2 of the
// level proves the list held every closer point, as in k_knn_pca.  A box with more than kFpfhCap candidates is rescanned:
// a bisection on the key finds a bound below which between max_nn and kFpfhCap candidates lie, those are listed and
// sorted -- the same keys in the same order, so the result is exact either way.  Outputs are indexed by original index:
// ids (n x max_nn, ascending (d2, index), the point itself dropped, -1 padded), the 33 integer counts, m.
__global__ void __launch_bounds__(256)
k_fpfh_spfh(Grid g, const float* __restrict__ raw_xyz, int64_t xs, const float* __restrict__ nrm, int64_t ns, int64_t n,
            int max_nn, int start_level, int32_t* __restrict__ ids, int32_t* __restrict__ counts, int32_t* __restrict__ m_out,
            uint32_t* __restrict__ n_overflow) {
    __shared__ uint64_t l_key[kFpfhWaves][kFpfhCap];
    __shared__ uint32_t l_cnt[kFpfhWaves];
    __shared__ int l_hist[kFpfhWaves][kFpfhDim];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t q = blockIdx.x * (int64_t)kFpfhWaves + wv;
    if (q >= n) return;   // whole waves leave together; nothing below synchronises across waves
    uint64_t* key = l_key[wv];
    const float4 me = g.pts[q];
    const float3 p = make_float3(me.x, me.y, me.z);
    const uint32_t my_idx = __float_as_uint(me.w);
    int m_all = 0;
    bool overflow = false;
    for (int l = min(start_level, g.n_levels - 1); l < g.n_levels; ++l) {
        if (lane == 0) l_cnt[wv] = 0;
        group_sync();
        fpfh_scan_box(g, p, l, lane, [&](const float4& tpt, float d2) {
            const uint32_t slot = atomicAdd(&l_cnt[wv], 1u);
            if (slot < (uint32_t)kFpfhCap) key[slot] = fpfh_key(d2, __float_as_uint(tpt.w));
        });
        group_sync();
        uint32_t cnt = l_cnt[wv];
        if (cnt > (uint32_t)kFpfhCap) {
            overflow = true;
            // keys are unique: once lo == hi the count is exactly max_nn, so the loop ends within 64 halvings
            uint64_t lo = 0, hi = ~0ull, bound = 0;
            for (int it = 0; it < 72; ++it) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                uint32_t c = 0;
                fpfh_scan_box(g, p, l, lane, [&](const float4& tpt, float d2) {
                    if (fpfh_key(d2, __float_as_uint(tpt.w)) <= mid) ++c;
                });
#pragma unroll
                for (int x = 32; x > 0; x >>= 1) c += (uint32_t)__shfl_xor((int)c, x);
                if (c < (uint32_t)max_nn) {
                    lo = mid + 1;
                } else if (c <= (uint32_t)kFpfhCap) {
                    bound = mid;
                    break;
                } else {
                    hi = mid;
                }
            }
            if (lane == 0) l_cnt[wv] = 0;
            group_sync();
            fpfh_scan_box(g, p, l, lane, [&](const float4& tpt, float d2) {
                const uint64_t kk = fpfh_key(d2, __float_as_uint(tpt.w));
                if (kk <= bound) {
                    const uint32_t slot = atomicAdd(&l_cnt[wv], 1u);
                    if (slot < (uint32_t)kFpfhCap) key[slot] = kk;
                }
            });
            group_sync();
            cnt = min(l_cnt[wv], (uint32_t)kFpfhCap);
        }
        // bitonic sort of the list, padded to a power of two
        uint32_t P = 1;
        while (P < cnt) P <<= 1;
        for (uint32_t t = cnt + (uint32_t)lane; t < P; t += 64) key[t] = ~0ull;
        group_sync();
        for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t t = (uint32_t)lane; t < (P >> 1); t += 64) {
                    const uint32_t i0 = ((t & ~(j - 1)) << 1) | (t & (j - 1)), i1 = i0 | j;
                    const uint64_t a = key[i0], b = key[i1];
                    if ((a > b) == ((i0 & k2) == 0)) {
                        key[i0] = b;
                        key[i1] = a;
                    }
                }
                group_sync();
            }
        }
        m_all = (int)min(cnt, (uint32_t)max_nn);
        if (l == g.n_levels - 1) break;
        if (m_all == max_nn) {
            const float kth = __uint_as_float((uint32_t)(key[max_nn - 1] >> 32));
            const float r2 = g.rho[l] * g.rho[l];
            if (kth <= r2) break;
        }
    }
    // the point itself is dropped by index (it is absent when more than max_nn twins precede it)
    int self = m_all;
    for (int base = 0; base < m_all; base += 64) {
        const int r = base + lane;
        const bool is = r < m_all && (uint32_t)key[r] == my_idx;
        const unsigned long long bal = __ballot(is);
        if (bal) self = base + __ffsll((long long)bal) - 1;
    }
    const int m = m_all - (self < m_all ? 1 : 0);
    if (lane < kFpfhDim) l_hist[wv][lane] = 0;
    group_sync();
    const float* nq = nrm + (size_t)my_idx * ns;
    const double pi[3] = {(double)p.x, (double)p.y, (double)p.z};
    const double ni[3] = {(double)nq[0], (double)nq[1], (double)nq[2]};
    for (int r = lane; r < max_nn; r += 64) {
        int32_t id = -1;
        if (r < m) {
            const uint32_t j = (uint32_t)key[r + (r >= self ? 1 : 0)];
            id = (int32_t)j;
            const float* sp = raw_xyz + (size_t)j * xs;
            const float* sn = nrm + (size_t)j * ns;
            const double pj[3] = {(double)sp[0], (double)sp[1], (double)sp[2]};
            const double nj[3] = {(double)sn[0], (double)sn[1], (double)sn[2]};
            int bins[3];
            fpfh_pair_bins(pi, ni, pj, nj, bins);
            atomicAdd(&l_hist[wv][bins[0]], 1);
            atomicAdd(&l_hist[wv][11 + bins[1]], 1);
            atomicAdd(&l_hist[wv][22 + bins[2]], 1);
        }
        ids[(size_t)my_idx * max_nn + r] = id;
    }
    group_sync();
    if (lane < kFpfhDim) counts[(size_t)my_idx * kFpfhDim + lane] = l_hist[wv][lane];
    if (lane == 0) {
        m_out[my_idx] = m;
        if (overflow) atomicAdd(n_overflow, 1u);   // statistics only: the result is still exact
    }
}

// One wave per point, lanes over the 33 bins, serial over the neighbours in their stored order: the fp64 sums are
// order-fixed.  Lane r holds the squared distance and 100 / m_j of neighbours r and r + 64, so that only the gather of the
// neighbour's count row is left in the serial loop.
__global__ void __launch_bounds__(256)
k_fpfh_accum(const float* __restrict__ xyz, int64_t xs, int64_t n, int max_nn, const int32_t* __restrict__ ids,
             const int32_t* __restrict__ counts, const int32_t* __restrict__ m_arr, double* __restrict__ fpfh,
             double* __restrict__ spfh) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * (int64_t)kFpfhWaves + wv;
    if (i >= n) return;
    const int b = lane < kFpfhDim ? lane : kFpfhDim - 1;   // the idle lanes shadow the last bin and write nothing
    const int m = m_arr[i];
    const float* pp = xyz + (size_t)i * xs;
    const double px = (double)pp[0], py = (double)pp[1], pz = (double)pp[2];
    int nid[2];
    double nd2[2], nsc[2];   // d2 == 0 marks a neighbour that adds nothing (a twin, or an empty SPFH row)
    for (int h = 0; h < 2; ++h) {
        const int r = lane + 64 * h;
        nid[h] = -1;
        nd2[h] = 0.0;
        nsc[h] = 0.0;
        if (r < m) {
            const int32_t j = ids[(size_t)i * max_nn + r];
            const float* sp = xyz + (size_t)j * xs;
            const double s = sum_sq3((double)sp[0] - px, (double)sp[1] - py, (double)sp[2] - pz);
            const int mj = m_arr[j];
            nid[h] = j;
            if (mj > 0) {
                nd2[h] = s;
                nsc[h] = 100.0 / (double)mj;
            }
        }
    }
    double acc = 0.0;
    for (int r = 0; r < m; ++r) {
        const int h = r >> 6, src = r & 63;
        const int j = __shfl(h ? nid[1] : nid[0], src);
        const double d2 = __shfl(h ? nd2[1] : nd2[0], src);
        const double sc = __shfl(h ? nsc[1] : nsc[0], src);
        if (d2 == 0.0) continue;
        const double s = (double)counts[(size_t)j * kFpfhDim + b] * sc;
        acc = acc + s / d2;
    }
    const int t0 = (b / 11) * 11;
    double st = 0.0;
    for (int c = 0; c < 11; ++c) st = st + __shfl(acc, t0 + c);
    const double scale = st != 0.0 ? 100.0 / st : 0.0;
    const double own = m > 0 ? (double)counts[(size_t)i * kFpfhDim + b] * (100.0 / (double)m) : 0.0;
    const double prod = acc * scale;
    if (lane < kFpfhDim) {
        fpfh[(size_t)i * kFpfhDim + lane] = prod + own;
        if (spfh) spfh[(size_t)i * kFpfhDim + lane] = own;
    }
}

// ---- nearest neighbours of feature rows -------------------------------------------------------------------------
constexpr int kMfMaxDim = 64;
constexpr int kMfTile = 32;      // rows of B staged in LDS at a time
constexpr int kMfChunk = 1024;   // rows of B per workgroup (second grid dimension)

// Each lane keeps one row of A in registers; the rows of chunk blockIdx.y of B pass through LDS in tiles and are read as
// broadcasts.  D = sum_j (a_j - b_j)^2, j ascending; the running best takes a later row only when it is strictly closer, so
// ties stay with the lowest index.  Writes the chunk's best (D, b) of every row of A to part_d / part_i[chunk * na + a].
template <int MAXD>
__global__ void __launch_bounds__(256)
k_mf_search(const double* __restrict__ A, int64_t na, const double* __restrict__ B, int64_t nb, int dim,
            double* __restrict__ part_d, int32_t* __restrict__ part_i) {
    __shared__ double tile[kMfTile * MAXD];
    const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t ar = a < na ? a : na - 1;
    double row[MAXD];
#pragma unroll
    for (int j = 0; j < MAXD; ++j) row[j] = j < dim ? A[(size_t)ar * dim + j] : 0.0;
    const int64_t b0 = (int64_t)blockIdx.y * kMfChunk, b1 = b0 + kMfChunk < nb ? b0 + kMfChunk : nb;
    double best_d = 0.0;
    int32_t best_i = (int32_t)b0;
    for (int64_t tb = b0; tb < b1; tb += kMfTile) {
        const int rows = (int)(b1 - tb < kMfTile ? b1 - tb : kMfTile);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * dim; e += blockDim.x) {
            const int r = e / dim, j = e - r * dim;
            tile[r * MAXD + j] = B[(size_t)(tb + r) * dim + j];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            double D = 0.0;
#pragma unroll
            for (int j = 0; j < MAXD; ++j) {
                if (j < dim) {
                    double d = row[j] - tile[r * MAXD + j];
                    d = d * d;
                    D = D + d;
                }
            }
            const int64_t bi = tb + r;
            if (bi == b0 || D < best_d) {
                best_d = D;
                best_i = (int32_t)bi;
            }
        }
    }
    if (a < na) {
        part_d[(size_t)blockIdx.y * na + a] = best_d;
        part_i[(size_t)blockIdx.y * na + a] = best_i;
    }
}

// Merges the per-chunk bests in chunk order (strict <: the lowest index wins a tie).
__global__ void k_mf_merge(const double* __restrict__ part_d, const int32_t* __restrict__ part_i, int64_t na, int n_chunks,
                           int32_t* __restrict__ nn) {
    const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (a >= na) return;
    double best_d = part_d[a];
    int32_t best_i = part_i[a];
    for (int c = 1; c < n_chunks; ++c) {
        const double d = part_d[(size_t)c * na + a];
        if (d < best_d) {
            best_d = d;
            best_i = part_i[(size_t)c * na + a];
        }
    }
    nn[a] = best_i;
}

// flags[a] = 1 when a and nn_ab[a] chose each other; thread na writes the closing 0 (as k_ovl_flags).
__global__ void k_mf_flags(const int32_t* __restrict__ nn_ab, const int32_t* __restrict__ nn_ba, int64_t na,
                           uint32_t* __restrict__ flags) {
    const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (a > na) return;
    flags[a] = (a < na && (int64_t)nn_ba[nn_ab[a]] == a) ? 1u : 0u;
}

__global__ void k_mf_collect(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs, int64_t na,
                             const int32_t* __restrict__ nn_ab, int32_t* __restrict__ mutual) {
    const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (a >= na || !flags[a]) return;
    mutual[2 * (size_t)offs[a]] = (int32_t)a;
    mutual[2 * (size_t)offs[a] + 1] = nn_ab[a];
}
