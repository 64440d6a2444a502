// kernels_neighbours.hpp -- the pieces the k-NN kernels on the voxel-bin table share (k_knn_pca, k_match_knn, k_fpfh_spfh,
// k_ssn_leaf, k_pca_finish): the row decode of a level box, its walk by a 16-lane group, the sequential fp32 PCA moments
// with their density and rank rule.  LevelBox / level_box and the NC5 distance are in reg_kernels.hpp,
// group_sync in group_dpp.hpp.
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

constexpr int kPcaGroup = 16;   // lanes per query point of the group k-NN kernels

// Row t of box b: the run [s, e) of sorted positions its bins hold; e == s where the row's brick does not exist.
__device__ __forceinline__ void row_run(const Grid& g, const LevelBox& b, int64_t t, uint32_t& s, uint32_t& e) {
    s = 0;
    e = 0;
    const int iz = (int)(t / b.nrow), rem = (int)(t - (int64_t)iz * b.nrow);
    const int iy = rem / b.nbx, ix = rem - iy * b.nbx;
    const int bx = b.bx0 + ix, cy = b.loy + iy, cz = b.loz + iz;
    const int bid = brick_lookup(g, bx, cy >> kBrickLog2, cz >> kBrickLog2);
    if (bid < 0) return;
    const int x0 = max(b.lox, bx << kBrickLog2) & (kBrickDim - 1);
    const int x1 = min(b.hix, (bx << kBrickLog2) + kBrickDim - 1) & (kBrickDim - 1);
    const uint32_t* cs = g.cell_start + (size_t)bid * kBrickCells +
                         (((cz & (kBrickDim - 1)) << (2 * kBrickLog2)) | ((cy & (kBrickDim - 1)) << kBrickLog2));
    s = cs[x0];
    e = cs[x1 + 1];
}

// Calls f(j, target point j, d2) on the lanes of one 16-lane group for every target point inside the bin box of
// level l around p that lies within max_dist: 16 rows at a time, the 16 lanes side by side along each non-empty one.
template <class F>
__device__ __forceinline__ void pca_scan_box(const Grid& g, const float3 p, int l, int sub, int gbase, F&& f) {
    const LevelBox b = level_box(g, p, l);
    for (int64_t base = 0; base < b.total; base += kPcaGroup) {
        uint32_t s = 0, e = 0;
        if (base + sub < b.total) row_run(g, b, base + sub, s, e);
        unsigned mask = (unsigned)((__ballot(e > s) >> gbase) & 0xffffull);
        while (mask) {
            const int it = __ffs((int)mask) - 1;
            mask &= mask - 1;
            const uint32_t si = (uint32_t)__shfl((int)s, gbase + it);
            const uint32_t ei = (uint32_t)__shfl((int)e, gbase + it);
            for (uint32_t j = si + (uint32_t)sub; j < ei; j += kPcaGroup) {
                const float4 tpt = g.pts[j];
                const float d2 = nc5_d2(p, tpt);
                if (d2 <= g.max_d2) f(j, tpt, d2);
            }
        }
    }
}

// PCA of m points point(0) .. point(m - 1) (float3 each), fp32 sequential sums in that order (numeric contract): the
// mean (sum / (float)m), the scatter sums about it in the order xx xy xz yy yz zz, and the largest squared distance
// from it.
template <class P>
__device__ __forceinline__ void pca_moments(int m, P&& point, float mean[3], float C[6], float& max_d2) {
    mean[0] = mean[1] = mean[2] = 0.f;
    for (int r = 0; r < m; ++r) {
        const float3 v = point(r);
        mean[0] = mean[0] + v.x;
        mean[1] = mean[1] + v.y;
        mean[2] = mean[2] + v.z;
    }
    const float fm = (float)m;
    if (m > 0) {
        mean[0] = mean[0] / fm;
        mean[1] = mean[1] / fm;
        mean[2] = mean[2] / fm;
    }
    for (int a = 0; a < 6; ++a) C[a] = 0.f;
    max_d2 = 0.f;
    for (int r = 0; r < m; ++r) {
        const float3 v = point(r);
        const float dx = v.x - mean[0], dy = v.y - mean[1], dz = v.z - mean[2];
        float u;
        u = dx * dx; C[0] = C[0] + u;
        u = dx * dy; C[1] = C[1] + u;
        u = dx * dz; C[2] = C[2] + u;
        u = dy * dy; C[3] = C[3] + u;
        u = dy * dz; C[4] = C[4] + u;
        u = dz * dz; C[5] = C[5] + u;
        max_d2 = fmaxf(max_d2, sum_sq3(dx, dy, dz));
    }
}

// utils.h:106-128 computeDensity: m / (4/3 pi r^3), r^2 = max_d2, in fp32 with one rounding per operation.
__device__ __forceinline__ float pca_density(int m, float max_d2) {
    const float tq = (float)(4. / 3.), pi = (float)3.14159265358979323846;
    const float c0 = tq * pi;
    const float r3 = max_d2 * sqrtf(max_d2);
    const float volume = c0 * r3;
    return volume > 0.f ? (float)m / volume : 0.f;
}

// Ascending order o[] of the eigenvalues lam[] and their rank: |lambda| > 3 eps_f32 |largest lambda|.
__device__ __forceinline__ int pca_rank(const double lam[3], int o[3]) {
    int o0 = 0, o1 = 1, o2 = 2;
    if (lam[o1] < lam[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (lam[o2] < lam[o0]) { const int t = o0; o0 = o2; o2 = t; }
    if (lam[o2] < lam[o1]) { const int t = o1; o1 = o2; o2 = t; }
    o[0] = o0; o[1] = o1; o[2] = o2;
    const double lmax = fabs(lam[o2]);
    int rank = 0;
    for (int a = 0; a < 3; ++a)
        if (lmax > 0 && fabs(lam[a]) > lmax * 3.0 * 1.1920929e-07) ++rank;
    return rank;
}
