// kernels_scanprep.hpp -- the scan front end (ScanToMapRegistration.cpp:36-69): Open3D's VoxelDownSample and
// RandomDownSample restated, the widening of estimated normals.  The fp64 gather of the random selection and
// of the wide crop is k_gather_rows of kernels_cloud64.hpp.
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// ---- VoxelDownSample: origin = min_bound - voxel / 2, index = floor((p - origin) / voxel), 21 bits per axis ----
constexpr int kSpMinRows = 512;   // partial rows of the min-bound reduction at most

// pass 1: per axis, the minimum over a grid-stride slice.  fmin is exact, so the order does not matter; a NaN never wins
// here and is caught by k_sp_vox_keys.
__global__ void __launch_bounds__(256) k_sp_min_partial(const double* __restrict__ xyz, int64_t n, double* __restrict__ part) {
    __shared__ double sm[3][256];
    const int t = threadIdx.x;
    double m0 = INFINITY, m1 = INFINITY, m2 = INFINITY;
    for (int64_t i = blockIdx.x * (int64_t)256 + t; i < n; i += (int64_t)gridDim.x * 256) {
        m0 = fmin(m0, xyz[3 * i]);
        m1 = fmin(m1, xyz[3 * i + 1]);
        m2 = fmin(m2, xyz[3 * i + 2]);
    }
    sm[0][t] = m0;
    sm[1][t] = m1;
    sm[2][t] = m2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < 3; ++k) sm[k][t] = fmin(sm[k][t], sm[k][t + s]);
        __syncthreads();
    }
    if (t < 3) part[3 * (size_t)blockIdx.x + t] = sm[t][0];
}
// pass 2, one workgroup: the minimum over the partial rows -> out[0..2] = min_bound, out[3..5] = origin
__global__ void __launch_bounds__(256) k_sp_min_final(const double* __restrict__ part, int rows, double voxel,
                                                      double* __restrict__ out) {
    __shared__ double sm[3][256];
    const int t = threadIdx.x;
    double m[3] = {INFINITY, INFINITY, INFINITY};
    for (int r = t; r < rows; r += 256)
        for (int k = 0; k < 3; ++k) m[k] = fmin(m[k], part[3 * (size_t)r + k]);
    for (int k = 0; k < 3; ++k) sm[k][t] = m[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < 3; ++k) sm[k][t] = fmin(sm[k][t], sm[k][t + s]);
        __syncthreads();
    }
    if (t < 3) {
        const double half = 0.5 * voxel;
        out[t] = sm[t][0];
        out[3 + t] = sm[t][0] - half;
    }
}
// keys in (z, y, x) significance, value = input index.  *bad: bit 0 a non-finite coordinate, bit 1 an index >= 2^21.
// Open3D's index rule (origin subtraction, a division, the unsigned range [0, 2^21)), not the map's vox_index / vox_pack
// of kernels_cloud64.hpp: the formula and the packing below are this kernel's own on purpose.
__global__ void k_sp_vox_keys(const double* __restrict__ xyz, int64_t n, const double* __restrict__ origin, double voxel,
                              uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ bad) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v[3];
    bool finite = true, fits = true;
    for (int k = 0; k < 3; ++k) {
        const double p = xyz[3 * i + k];
        const double d = p - origin[k];
        v[k] = floor(d / voxel);
        finite = finite && fabs(p) < INFINITY;   // false for NaN too
        fits = fits && v[k] >= 0.0 && v[k] < (double)(1ll << kVoxBits);
    }
    vals[i] = (uint32_t)i;
    if (!finite || !fits) {
        atomicOr(bad, finite ? 2u : 1u);
        keys[i] = 0;
        return;
    }
    keys[i] = ((uint64_t)(long long)v[2] << (2 * kVoxBits)) | ((uint64_t)(long long)v[1] << kVoxBits) | (uint64_t)(long long)v[0];
}

// ---- RandomDownSample under the determinism contract: key(i) = splitmix_key(seed, i) ----
__global__ void k_sp_rand_keys(uint64_t seed, int64_t n, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = splitmix_key(seed, (uint64_t)i);
    vals[i] = (uint32_t)i;
}
// the first `count` values of the stable sort are the count smallest (key, index) pairs; flags start cleared
__global__ void k_sp_rand_mark(const uint32_t* __restrict__ sorted_vals, int64_t count, uint32_t* __restrict__ flags) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= count) return;
    flags[sorted_vals[j]] = 1u;
}

// estimated fp32 normals (and the six covariance entries xx xy xz yy yz zz) -> Open3D's fp64 rows (exact)
__global__ void k_sp_widen(const float* __restrict__ nrm, const float* __restrict__ cov6, int64_t n, double* __restrict__ onrm,
                           double* __restrict__ ocov) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 3; ++k) onrm[3 * i + k] = (double)nrm[3 * i + k];
    if (cov6) {
        const float* c = cov6 + 6 * i;
        double* o = ocov + 9 * i;
        o[0] = c[0], o[1] = c[1], o[2] = c[2];
        o[3] = c[1], o[4] = c[3], o[5] = c[4];
        o[6] = c[2], o[7] = c[4], o[8] = c[5];
    }
}
