// kernels_submaps.hpp -- the occupancy set of a submap and the revisiting fitness (Submap::voxelMap_, Submap.cpp:239-240,
// 260-264; SubmapCollection::isSwitchingSubmapsConsistant, SubmapCollection.cpp:390-402): the voxel keys of a
// map cloud, the unique keys after sort_runs, and the count of scan points that fall into an occupied voxel.  The key, its
// bounds, the lower bound and the transform rows are those of kernels_cloud64.hpp.  fp64, one rounding per operation.
// Part of the single translation unit reg_core.hip (included there after kernels_mapcloud.hpp; not a standalone header).
#pragma once

// The key of floor(p * inv) per axis (VoxelHashMap.hpp:48-51; inv = 1 / (factor * mapVoxelSize), a multiplication, not a
// division).  A row with a NaN / infinite coordinate or an index that does not fit the packing gets kOccNoKey.  No voxel
// that fits packs to 0 (it would be index -2^20 on every axis, which vox_fits refuses), so 0 is free to mean "no key".
constexpr uint64_t kOccNoKey = 0;
__device__ __forceinline__ uint64_t occ_key(double x, double y, double z, double inv) {
    const double fx = vox_index(x, inv), fy = vox_index(y, inv), fz = vox_index(z, inv);
    return vox_fits(fx, fy, fz) ? vox_pack(fx, fy, fz) : kOccNoKey;
}

// one thread per map row: keys[i] (kOccNoKey: the row is refused), vals[i] = i for sort_runs
__global__ void k_occ_keys(const double* __restrict__ xyz, int64_t n, double inv, uint64_t* __restrict__ keys,
                           uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = occ_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], inv);
    vals[i] = (uint32_t)i;
}

// After sort_runs: the head of every run of equal keys goes to out[run id], ascending and unique.  The refused rows sort to
// the front as one run (kOccNoKey is the smallest key); that run is skipped and the others move down by one.
__global__ void k_occ_unique(const uint64_t* __restrict__ sorted, int64_t n, const uint32_t* __restrict__ heads,
                             const uint32_t* __restrict__ run, uint64_t* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    const uint64_t key = sorted[i];
    if (key == kOccNoKey) return;
    out[run[i] - (sorted[0] == kOccNoKey ? 1u : 0u)] = key;
}

// one thread per scan point: p' = R p + t in the operation order of xform_row<true> (Eigen's Isometry * point: no division
// by w), its key, a binary search in the candidate's ascending keys.  The 0 / 1 hits of a wave are counted by one ballot
// (no lane exchange, no LDS) and its first lane adds the count to *count: integer sums are order-free, so the result is the
// same on every run.  A point without a key is not contained.
__global__ void __launch_bounds__(256) k_occ_count(const double* __restrict__ xyz, int64_t n, Xform64 T, double inv,
                                                   const uint64_t* __restrict__ keys, int64_t n_keys,
                                                   uint32_t* __restrict__ count) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const uint64_t key = occ_key(xform_row<true>(T, 0, x, y, z), xform_row<true>(T, 1, x, y, z),
                                     xform_row<true>(T, 2, x, y, z), inv);
        if (key != kOccNoKey) {
            const int64_t lb = key_lower_bound(keys, n_keys, key);
            hit = lb < n_keys && keys[lb] == key;
        }
    }
    const uint32_t hits = (uint32_t)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(count, hits);
}

// Submap::transform of a stored sparse cloud (Submap.cpp:117), in place, one thread per row: the fp64 point by
// xform_point, the fp32 point as its cast, the fp32 normal widened, turned by xform_dir and cast back.  A thread reads its
// whole row before it writes any of it and touches no other row, so the update needs no second buffer.
__global__ void __launch_bounds__(256) k_sm_transform_sparse(double* __restrict__ xyz64, float* __restrict__ xyz,
                                                             float* __restrict__ nrm, int64_t n, Xform64 T) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = xyz64[3 * i], y = xyz64[3 * i + 1], z = xyz64[3 * i + 2];
    const double nx = (double)nrm[3 * i], ny = (double)nrm[3 * i + 1], nz = (double)nrm[3 * i + 2];
    double p[3], d[3];
    xform_point(T, x, y, z, p);
    xform_dir(T, nx, ny, nz, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        xyz64[3 * i + k] = p[k];
        xyz[3 * i + k] = (float)p[k];
        nrm[3 * i + k] = (float)d[k];
    }
}
