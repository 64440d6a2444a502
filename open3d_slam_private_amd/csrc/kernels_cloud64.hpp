// kernels_cloud64.hpp -- the pieces every operator on the fp64 map-side clouds shares (Open3D layout: points n x 3, normals
// n x 3, covariances n x 9 or colours n x 3): the 4x4 transform of a point, a direction and a covariance, the
// map voxel key and its inverse, the lower bound in an ascending key array, the row copy and the gather built on it, the
// fp64 -> fp32 row cast.  fp64, one rounding per operation (the build forbids contraction): the only copy of each formula.
// The by-value structs are indexed with compile-time indices only (unrolled constant-trip loops), so they stay in SGPRs.
// Part of the single translation unit reg_core.hip (included there ahead of kernels_mapprep.hpp; not a standalone header).
#pragma once

// ---- the 4x4 transform (o3d_slam::transform, helpers.cpp:283-318; Eigen's T * (x, y, z, 1)) ----
struct Xform64 {   // row-major: m[4 * r + c]
    double m[16];
};
static inline Xform64 xform_rows(const double* T_col) {   // the API's column-major double[16]; null: all zero (not applied)
    Xform64 t;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) t.m[4 * r + c] = T_col ? T_col[4 * c + r] : 0.0;
    return t;
}
// row r of T applied to (x, y, z): ((m0 x + m1 y) + m2 z), then + m3 with kTranslate
template <bool kTranslate>
__device__ __forceinline__ double xform_row(const Xform64& T, int r, double x, double y, double z) {
    double a = T.m[4 * r] * x;
    double b = T.m[4 * r + 1] * y;
    double s = a + b;
    a = T.m[4 * r + 2] * z;
    s = s + a;
    return kTranslate ? s + T.m[4 * r + 3] : s;
}
// a point: the rows 0..2 divided by w = row 3
__device__ __forceinline__ void xform_point(const Xform64& T, double x, double y, double z, double* out) {
    const double w = xform_row<true>(T, 3, x, y, z);
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = xform_row<true>(T, r, x, y, z) / w;
}
// a direction (normals): (T (n, 0)).head<3>(), the rotation rows without translation or division
__device__ __forceinline__ void xform_dir(const Xform64& T, double x, double y, double z, double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = xform_row<false>(T, r, x, y, z);
}
// a covariance (Matrix3d: (r, c) at 3 c + r): R C R^T as M = R C, C' = M R^T, each element ((a0 b0 + a1 b1) + a2 b2)
__device__ __forceinline__ void xform_cov(const Xform64& T, const double* C, double* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double M[3];   // row r of R C
#pragma unroll
        for (int c = 0; c < 3; ++c) M[c] = xform_row<false>(T, r, C[3 * c], C[3 * c + 1], C[3 * c + 2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * c + r] = xform_row<false>(T, c, M[0], M[1], M[2]);
    }
}

// ---- the map voxel key (VoxelHashMap.hpp:43-51): index floor(p * (1 / voxel)) per axis, |index| < 2^20, packed offset
// binary in (z, y, x) significance so that the ascending key order is the map's order ----
constexpr int kVoxBits = 21;                       // voxel index bits per axis in the sort key (offset binary)
constexpr long long kVoxOff = 1ll << (kVoxBits - 1);
__device__ __forceinline__ double vox_index(double p, double inv) { return floor(p * inv); }
__device__ __forceinline__ bool vox_fits(double fx, double fy, double fz) {   // false for NaN too
    return fabs(fx) < (double)kVoxOff && fabs(fy) < (double)kVoxOff && fabs(fz) < (double)kVoxOff;
}
__device__ __forceinline__ uint64_t vox_pack(double fx, double fy, double fz) {   // of indices that fit
    return ((uint64_t)((long long)fz + kVoxOff) << (2 * kVoxBits)) | ((uint64_t)((long long)fy + kVoxOff) << kVoxBits) |
           (uint64_t)((long long)fx + kVoxOff);
}
__device__ __forceinline__ void vox_unpack(uint64_t key, int32_t* __restrict__ out) {
    const uint64_t mask = (1ull << kVoxBits) - 1;
    out[0] = (int32_t)((long long)(key & mask) - kVoxOff);
    out[1] = (int32_t)((long long)((key >> kVoxBits) & mask) - kVoxOff);
    out[2] = (int32_t)((long long)((key >> (2 * kVoxBits)) & mask) - kVoxOff);
}

// first position of the ascending keys[0, n) that is >= key
__device__ __forceinline__ int64_t key_lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ---- rows of a cloud ----
struct Cols64 {   // one cloud: n x 3 points, n x 3 normals or null, aux = n x 9 covariances / n x 3 colours or null
    double *xyz, *nrm, *aux;
};
__host__ __device__ static inline Cols64 cols64_in(const double* xyz, const double* nrm, const double* aux) {   // a cloud that is only read
    return Cols64{(double*)xyz, (double*)nrm, (double*)aux};
}
// kW doubles from src to dst through registers: all loads are issued before the first store, whatever the compiler may
// assume about the two pointers (the struct members below cannot carry __restrict__)
template <int kW>
__device__ __forceinline__ void copy_doubles(const double* src, double* dst) {
    double v[kW];
#pragma unroll
    for (int k = 0; k < kW; ++k) v[k] = src[k];
#pragma unroll
    for (int k = 0; k < kW; ++k) dst[k] = v[k];
}
// row i of `in` to row o of `out`; the columns `in` lacks are skipped (wave-uniform tests).  kAux: doubles per aux row
template <int kAux>
__device__ __forceinline__ void copy_row(const Cols64& in, int64_t i, const Cols64& out, int64_t o) {
    if (in.xyz) copy_doubles<3>(in.xyz + 3 * i, out.xyz + 3 * o);
    if (in.nrm) copy_doubles<3>(in.nrm + 3 * i, out.nrm + 3 * o);
    if (in.aux) copy_doubles<kAux>(in.aux + kAux * i, out.aux + kAux * o);
}
// Order-preserving compaction by 0 / 1 flags and their exclusive scan offs.  kFlagKeeps: the flagged rows stay, row i lands
// at offs[i].  Otherwise the flagged rows leave, row i lands at i - offs[i], and flags == null keeps every row (a plain
// copy).  oidx (or null) receives the input index of every output row.
template <int kAux, bool kFlagKeeps>
__global__ void k_gather_rows(Cols64 in, int64_t n, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                              Cols64 out, int32_t* __restrict__ oidx) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t o = i;
    if (kFlagKeeps || flags) {
        if ((flags[i] != 0u) != kFlagKeeps) return;
        o = kFlagKeeps ? (int64_t)offs[i] : i - (int64_t)offs[i];
    }
    copy_row<kAux>(in, i, out, o);
    if (oidx) oidx[o] = (int32_t)i;
}

// fp64 -> fp32 of one row (open3d_conversions.cpp:57-118); of the symmetric Matrix3d the six entries xx xy xz yy yz zz
__device__ __forceinline__ void cast_row_f32(const double* __restrict__ xyz, const double* __restrict__ nrm,
                                             const double* __restrict__ cov, int64_t i, float* __restrict__ oxyz,
                                             float* __restrict__ onrm, float* __restrict__ ocov, size_t o) {
    for (int k = 0; k < 3; ++k) oxyz[3 * o + k] = (float)xyz[3 * i + k];
    if (nrm)
        for (int k = 0; k < 3; ++k) onrm[3 * o + k] = (float)nrm[3 * i + k];
    if (cov) {
        const double* c = cov + 9 * i;
        ocov[6 * o + 0] = (float)c[0];
        ocov[6 * o + 1] = (float)c[1];
        ocov[6 * o + 2] = (float)c[2];
        ocov[6 * o + 3] = (float)c[4];
        ocov[6 * o + 4] = (float)c[5];
        ocov[6 * o + 5] = (float)c[8];
    }
}
