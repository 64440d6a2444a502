// kernels_overlap.hpp -- voxel-overlap selection between two clouds (computeIndicesOfOverlappingPoints, helpers.cpp:320-345)
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// sourceToTarget, row-major, by value; on == 0: identity, the points are keyed as they are
struct OvlT {
    double m[16];
    int on;
};

constexpr uint64_t kOvlBadKey = ~0ull;   // a valid key has bit 63 clear

// One thread per point: optional transform (helpers.cpp:302-303: T * (x, y, z, 1), divided by w), then the voxel key of
// VoxelHashMap.hpp:43-51 in the packing of k_carve_keys.  A non-finite coordinate or an index outside +-2^20 raises *bad.
__global__ void k_ovl_keys(const double* __restrict__ xyz, int64_t n, OvlT T, double inv, uint64_t* __restrict__ keys,
                           uint32_t* __restrict__ bad) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (T.on) {
        double r[4];
        for (int k = 0; k < 4; ++k) {
            double a = T.m[4 * k] * x;
            double b = T.m[4 * k + 1] * y;
            double s = a + b;
            a = T.m[4 * k + 2] * z;
            s = s + a;
            r[k] = s + T.m[4 * k + 3];
        }
        x = r[0] / r[3];
        y = r[1] / r[3];
        z = r[2] / r[3];
    }
    const double vx = floor(x * inv), vy = floor(y * inv), vz = floor(z * inv);
    if (!(fabs(vx) < (double)kVoxOff && fabs(vy) < (double)kVoxOff && fabs(vz) < (double)kVoxOff)) {
        atomicOr(bad, 1u);
        keys[i] = kOvlBadKey;
        return;
    }
    keys[i] = ((uint64_t)((long long)vz + kVoxOff) << (2 * kVoxBits)) | ((uint64_t)((long long)vy + kVoxOff) << kVoxBits) |
              (uint64_t)((long long)vx + kVoxOff);
}

// points of a layer in the voxel `key`: binary search in the layer's ascending unique keys (0: the layer has none there)
__device__ __forceinline__ uint32_t ovl_count(const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ucnt,
                                              int64_t nu, uint64_t key) {
    int64_t lo = 0, hi = nu;   // first ukeys[lo] >= key
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ukeys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < nu && ukeys[lo] == key) ? ucnt[lo] : 0u;
}

// One thread per point of one layer (`own`), flag at the point's own index: both layers hold >= k points in its voxel.
// Thread n writes the closing 0, so that the exclusive scan over n + 1 flags ends in the number of selected points.
// nu_own / nu_other: the run counts rocPRIM left on the device.
__global__ void k_ovl_flags(const uint64_t* __restrict__ keys, int64_t n, const uint64_t* __restrict__ uk_own,
                            const uint32_t* __restrict__ uc_own, const uint32_t* __restrict__ nu_own,
                            const uint64_t* __restrict__ uk_other, const uint32_t* __restrict__ uc_other,
                            const uint32_t* __restrict__ nu_other, uint32_t k, uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        flags[n] = 0u;
        return;
    }
    const uint64_t key = keys[i];
    bool sel = ovl_count(uk_other, uc_other, (int64_t)*nu_other, key) >= k;
    if (sel && k > 1u) sel = ovl_count(uk_own, uc_own, (int64_t)*nu_own, key) >= k;   // k == 1: the point itself is there
    flags[i] = sel ? 1u : 0u;
}
