// kernels_overlap.hpp -- voxel-overlap selection between two clouds (computeIndicesOfOverlappingPoints, helpers.cpp:320-345)
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

constexpr uint64_t kOvlBadKey = ~0ull;   // a valid key has bit 63 clear

// One thread per point: with use_T the point goes through sourceToTarget first (helpers.cpp:302-303; xform_point), then the
// map voxel key (vox_index, vox_pack).  A non-finite coordinate or an index outside +-2^20 raises *bad.
__global__ void k_ovl_keys(const double* __restrict__ xyz, int64_t n, int use_T, Xform64 T, double inv,
                           uint64_t* __restrict__ keys, uint32_t* __restrict__ bad) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if (use_T) xform_point(T, p[0], p[1], p[2], p);
    const double vx = vox_index(p[0], inv), vy = vox_index(p[1], inv), vz = vox_index(p[2], inv);
    if (!vox_fits(vx, vy, vz)) {
        atomicOr(bad, 1u);
        keys[i] = kOvlBadKey;
        return;
    }
    keys[i] = vox_pack(vx, vy, vz);
}

// points of a layer in the voxel `key`: its place in the layer's ascending unique keys (0: the layer has none there)
__device__ __forceinline__ uint32_t ovl_count(const uint64_t* __restrict__ ukeys, const uint32_t* __restrict__ ucnt,
                                              int64_t nu, uint64_t key) {
    const int64_t lo = key_lower_bound(ukeys, nu, key);
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
