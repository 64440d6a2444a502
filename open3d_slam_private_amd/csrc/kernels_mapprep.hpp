// kernels_mapprep.hpp -- target-side preparation rows: cropping volume, fp64 -> fp32, voxelize-within-volume, space carving.
// The voxel key, the row copy and the fp32 row cast are those of kernels_cloud64.hpp.
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// ---- target-side preparation: crop (croppers.cpp:76-170) + fp64 -> fp32 (open3d_conversions.cpp:57-118)
struct CropCfg {
    int type;
    double cx, cy, cz, rmin, rmax, zmin, zmax;
};
__device__ __forceinline__ bool crop_inside(const CropCfg& c, double x, double y, double z) {
    if (c.type == REG_CROP_NONE) return true;
    const double dx = x - c.cx, dy = y - c.cy, dz = z - c.cz;
    if (c.type == REG_CROP_CYLINDER) {
        double a = dx * dx;
        double b = dy * dy;
        const double d = sqrt(a + b);
        return z >= c.zmin && z <= c.zmax && d <= c.rmax;
    }
    const double d = sqrt(sum_sq3(dx, dy, dz));
    if (c.type == REG_CROP_MAX_RADIUS) return d <= c.rmax;
    if (c.type == REG_CROP_MIN_RADIUS) return d >= c.rmin;
    return d <= c.rmax && d >= c.rmin;
}
__global__ void k_crop_flags(const double* __restrict__ xyz, int64_t m, CropCfg c, uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= m) return;
    flags[i] = crop_inside(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) ? 1u : 0u;
}
// offs = exclusive scan of flags: order-preserving compaction + conversion
__global__ void k_crop_gather(const double* __restrict__ xyz, const double* __restrict__ nrm, const double* __restrict__ cov,
                              int64_t m, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                              float* __restrict__ oxyz, float* __restrict__ onrm, float* __restrict__ ocov,
                              int32_t* __restrict__ oidx) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= m || !flags[i]) return;
    const size_t o = offs[i];
    cast_row_f32(xyz, nrm, cov, i, oxyz, onrm, ocov, o);
    oidx[o] = (int32_t)i;
}

// R11, reading side (open3d_conversions.cpp:57-118): fp64 AoS -> fp32, same order, nothing dropped
__global__ void k_cast_cloud_f64(const double* __restrict__ xyz, const double* __restrict__ nrm, const double* __restrict__ cov,
                                 int64_t n, float* __restrict__ oxyz, float* __restrict__ onrm, float* __restrict__ ocov) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    cast_row_f32(xyz, nrm, cov, i, oxyz, onrm, ocov, (size_t)i);
}

// ---- voxelizeWithinCroppingVolume (helpers.cpp:117-192) ----
__global__ void k_vox_classify(const double* __restrict__ xyz, int64_t m, CropCfg c, double inv, uint32_t* __restrict__ f_in,
                               uint32_t* __restrict__ f_out, uint32_t* __restrict__ overflow) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const bool in = crop_inside(c, x, y, z);
    f_in[i] = in ? 1u : 0u;
    f_out[i] = in ? 0u : 1u;
    if (in && !vox_fits(vox_index(x, inv), vox_index(y, inv), vox_index(z, inv))) atomicOr(overflow, 1u);
}
__global__ void k_vox_scatter(const double* __restrict__ xyz, const double* __restrict__ nrm, const double* __restrict__ cov,
                              int64_t m, double inv, const uint32_t* __restrict__ f_in, const uint32_t* __restrict__ o_in,
                              const uint32_t* __restrict__ o_out, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                              double* __restrict__ oxyz, double* __restrict__ onrm, double* __restrict__ ocov) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (f_in[i]) {
        keys[o_in[i]] = vox_pack(vox_index(xyz[3 * i], inv), vox_index(xyz[3 * i + 1], inv), vox_index(xyz[3 * i + 2], inv));
        vals[o_in[i]] = (uint32_t)i;
    } else {
        copy_row<9>(cols64_in(xyz, nrm, cov), i, Cols64{oxyz, onrm, ocov}, (int64_t)o_out[i]);
    }
}
__global__ void k_vox_heads(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
// one thread per voxel head: sequential sums in double over the voxel's points, which the stable sort left in
// ascending index order (= the insertion order of the reference's accumulator).  kRenormalise: the averaged normal is
// re-normalised (voxelizeWithinCroppingVolume, helpers.cpp:56-63) or left as sum / count (Open3D's GetAverageNormal,
// reg_voxel_down_sample); a compile-time switch, so that each form is the straight-line code it would be alone
template <bool kRenormalise>
__global__ void k_vox_reduce(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n,
                             const uint32_t* __restrict__ heads, const uint32_t* __restrict__ vox_id,
                             const double* __restrict__ xyz, const double* __restrict__ nrm, const double* __restrict__ cov,
                             int64_t base, double* __restrict__ oxyz, double* __restrict__ onrm, double* __restrict__ ocov) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    const uint64_t key = keys[i];
    double p[3] = {0, 0, 0}, nn[3] = {0, 0, 0}, cc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int cnt = 0;
    for (int64_t j = i; j < n && keys[j] == key; ++j) {
        const size_t s = vals[j];
        p[0] += xyz[3 * s];
        p[1] += xyz[3 * s + 1];
        p[2] += xyz[3 * s + 2];
        if (nrm) {
            const double a = nrm[3 * s], b = nrm[3 * s + 1], c = nrm[3 * s + 2];
            if (!(a != a) && !(b != b) && !(c != c)) {
                nn[0] += a;
                nn[1] += b;
                nn[2] += c;
            }
        }
        if (cov)
            for (int k = 0; k < 9; ++k) cc[k] += cov[9 * s + k];
        ++cnt;
    }
    const size_t o = (size_t)base + vox_id[i];
    const double dc = (double)cnt;
    for (int k = 0; k < 3; ++k) oxyz[3 * o + k] = p[k] / dc;
    if (nrm) {
        double a[3] = {nn[0] / dc, nn[1] / dc, nn[2] / dc};
        double u = a[0] * a[0];
        double v = a[1] * a[1];
        double z2 = u + v;
        u = a[2] * a[2];
        z2 = z2 + u;
        if (kRenormalise && z2 > 0.0) {   // Eigen normalized(): the zero vector stays zero
            const double r = sqrt(z2);
            a[0] = a[0] / r;
            a[1] = a[1] / r;
            a[2] = a[2] / r;
        }
        for (int k = 0; k < 3; ++k) onrm[3 * o + k] = a[k];
    }
    if (cov)
        for (int k = 0; k < 9; ++k) ocov[9 * o + k] = cc[k] / dc;
}

// ---- space carving (helpers.cpp:238-283) ----
// keys of the map points inside the subset volume (compacted by o_in), value = map index
__global__ void k_carve_keys(const double* __restrict__ xyz, int64_t m, double inv, const uint32_t* __restrict__ f_in,
                             const uint32_t* __restrict__ o_in, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= m || !f_in[i]) return;
    keys[o_in[i]] = vox_pack(vox_index(xyz[3 * i], inv), vox_index(xyz[3 * i + 1], inv), vox_index(xyz[3 * i + 2], inv));
    vals[o_in[i]] = (uint32_t)i;
}
// unique voxel keys and the first sorted position of each (ustart[nu] = n is written by the host)
__global__ void k_carve_unique(const uint64_t* __restrict__ keys, int64_t n, const uint32_t* __restrict__ heads,
                               const uint32_t* __restrict__ uid, uint64_t* __restrict__ ukeys, uint32_t* __restrict__ ustart) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    ukeys[uid[i]] = keys[i];
    ustart[uid[i]] = (uint32_t)i;
}
__global__ void k_carve_rays(const double* __restrict__ scan, int64_t n_scan, double sx, double sy, double sz, double step,
                             double max_ray, double trunc, double min_dot, double inv, const uint64_t* __restrict__ ukeys,
                             const uint32_t* __restrict__ ustart, int64_t nu, const uint32_t* __restrict__ vals,
                             const double* __restrict__ nrm, uint32_t* __restrict__ mark) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_scan) return;
    const double dx = scan[3 * i] - sx, dy = scan[3 * i + 1] - sy, dz = scan[3 * i + 2] - sz;
    const double length = sqrt(sum_sq3(dx, dy, dz));
    if (!(length > 0.0) || !(length < INFINITY)) return;
    const double ux = dx / length, uy = dy / length, uz = dz / length;
    const double reach = fmax(step, fmin(length - trunc, max_ray));
    double distance = 0.0;
    while (distance < reach) {
        double t = distance * ux;
        const double px = t + sx;
        t = distance * uy;
        const double py = t + sy;
        t = distance * uz;
        const double pz = t + sz;
        const double fx = vox_index(px, inv), fy = vox_index(py, inv), fz = vox_index(pz, inv);
        if (vox_fits(fx, fy, fz)) {
            const uint64_t key = vox_pack(fx, fy, fz);
            const int64_t lo = key_lower_bound(ukeys, nu, key);
            if (lo < nu && ukeys[lo] == key) {
                for (uint32_t j = ustart[lo]; j < ustart[lo + 1]; ++j) {
                    const uint32_t id = vals[j];
                    bool rm = true;
                    if (nrm) {
                        double n0 = nrm[3 * (size_t)id], n1 = nrm[3 * (size_t)id + 1], n2 = nrm[3 * (size_t)id + 2];
                        double u = n0 * n0;
                        double v = n1 * n1;
                        double z2 = u + v;
                        u = n2 * n2;
                        z2 = z2 + u;
                        if (z2 > 0.0) {
                            const double r = sqrt(z2);
                            n0 = n0 / r;
                            n1 = n1 / r;
                            n2 = n2 / r;
                        }
                        u = ux * n0;
                        v = uy * n1;
                        double d = u + v;
                        u = uz * n2;
                        d = d + u;
                        rm = fabs(d) > min_dot;
                    }
                    if (rm) mark[id] = 1u;   // idempotent: no atomic needed
                }
            }
        }
        distance += step;
    }
}
__global__ void k_carve_collect(const uint32_t* __restrict__ mark, const uint32_t* __restrict__ offs, int64_t m,
                                int32_t* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= m || !mark[i]) return;
    out[offs[i]] = (int32_t)i;
}
