// kernels_densemap.hpp -- the dense map (o3d_slam::VoxelizedPointCloud, Voxel.cpp:38-114): a resident table of
// per-voxel running sums, sorted by ascending 64-bit key; merge of a cloud into it, neighbourhood carve, export, transform,
// centre, first-wins de-duplication.  fp64, one rounding per operation (the build forbids contraction).  The transform, the
// voxel key, the lower bound and the gather of insert_scan are those of kernels_cloud64.hpp.
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

constexpr int kDmMaxOffsets = 16;   // neighbourhood offsets per axis at most (reg_dense_map_carve)
struct DmOffsets {
    double d[kDmMaxOffsets];   // the running sum -r, +v, +v, ... while <= r, built on the host
    int n;
};

// ---- insert, stage 1: optional transform (xform_point, xform_dir) and the map key (vox_index, vox_pack) ----
// use_T: the transformed points go to oxyz (the normals to onrm) and the later stages read those.
// *bad: bit 0 a non-finite coordinate, bit 1 an index outside +-2^20
__global__ void k_dm_keys(const double* __restrict__ xyz, const double* __restrict__ nrm, int64_t n, int use_T, Xform64 T,
                          double inv, double* __restrict__ oxyz, double* __restrict__ onrm, uint64_t* __restrict__ keys,
                          uint32_t* __restrict__ vals, uint32_t* __restrict__ bad) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if (use_T) {
        xform_point(T, p[0], p[1], p[2], p);
        for (int r = 0; r < 3; ++r) oxyz[3 * i + r] = p[r];
        if (nrm) {
            double d[3];
            xform_dir(T, nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], d);
            for (int r = 0; r < 3; ++r) onrm[3 * i + r] = d[r];
        }
    }
    vals[i] = (uint32_t)i;
    const bool finite = fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY;   // false for NaN too
    const double fx = vox_index(p[0], inv), fy = vox_index(p[1], inv), fz = vox_index(p[2], inv);
    if (!finite || !vox_fits(fx, fy, fz)) {
        atomicOr(bad, finite ? 2u : 1u);
        keys[i] = 0;
        return;
    }
    keys[i] = vox_pack(fx, fy, fz);
}

// ---- insert, stage 4: one thread per run head of the sorted cloud keys.  rank[run] = position of the run's key among the
// resident keys (found: its index; new: the number of resident keys below it); a found resident voxel is flagged touched.
__global__ void k_dm_rank(const uint64_t* __restrict__ skeys, int64_t n, const uint32_t* __restrict__ heads,
                          const uint32_t* __restrict__ run, const uint64_t* __restrict__ rkeys, int64_t n_res,
                          uint32_t* __restrict__ rank, uint32_t* __restrict__ is_new, uint32_t* __restrict__ touched) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    const uint64_t key = skeys[i];
    const int64_t lb = key_lower_bound(rkeys, n_res, key);
    const bool found = lb < n_res && rkeys[lb] == key;
    const uint32_t r = run[i];
    rank[r] = (uint32_t)lb;
    is_new[r] = found ? 0u : 1u;
    if (found) touched[lb] = 1u;
}
// the keys of the new runs, ascending (new_off = exclusive scan of is_new)
__global__ void k_dm_new_keys(const uint64_t* __restrict__ skeys, int64_t n, const uint32_t* __restrict__ heads,
                              const uint32_t* __restrict__ run, const uint32_t* __restrict__ is_new,
                              const uint32_t* __restrict__ new_off, uint64_t* __restrict__ new_keys) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    const uint32_t r = run[i];
    if (is_new[r]) new_keys[new_off[r]] = skeys[i];
}

// One side of the double-buffered columns (kernel argument)
struct DmCols {
    uint64_t* key;
    int32_t* cnt;
    double *pos, *nrm, *col;   // nrm / col: null while the map has not met the field
};

// ---- insert, stage 5: every untouched resident voxel moves to own index + number of new keys below it.  A column that
// the output has and the resident side lacks (the field arrives with this cloud) is zero.
__global__ void k_dm_copy(DmCols in, int64_t n_res, const uint32_t* __restrict__ touched, const uint64_t* __restrict__ new_keys,
                          int64_t n_new, DmCols out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_res || touched[i]) return;
    const uint64_t key = in.key[i];
    const size_t o = (size_t)(i + key_lower_bound(new_keys, n_new, key));
    out.key[o] = key;
    out.cnt[o] = in.cnt[i];
    for (int k = 0; k < 3; ++k) out.pos[3 * o + k] = in.pos[3 * i + k];
    if (out.nrm)
        for (int k = 0; k < 3; ++k) out.nrm[3 * o + k] = in.nrm ? in.nrm[3 * i + k] : 0.0;
    if (out.col)
        for (int k = 0; k < 3; ++k) out.col[3 * o + k] = in.col ? in.col[3 * i + k] : 0.0;
}
// ---- insert, stage 6: one thread per run.  Starts from the resident record (or zero), adds the run's points one by one in
// index order -- ((S + p1) + p2) ..., the order the stable sort left them in -- and writes the record at its merged position.
// NaN normals are added as they are (Voxel.cpp:78-85 does not filter).
__global__ void k_dm_accumulate(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ vals, int64_t n,
                                const uint32_t* __restrict__ heads, const uint32_t* __restrict__ run,
                                const uint32_t* __restrict__ rank, const uint32_t* __restrict__ is_new,
                                const uint32_t* __restrict__ new_off, const uint64_t* __restrict__ new_keys, int64_t n_new,
                                const double* __restrict__ xyz, const double* __restrict__ nrm, const double* __restrict__ col,
                                DmCols in, DmCols out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    const uint64_t key = skeys[i];
    const uint32_t r = run[i];
    const size_t lb = rank[r];
    double p[3] = {0, 0, 0}, nn[3] = {0, 0, 0}, cc[3] = {0, 0, 0};
    int32_t cnt = 0;
    size_t o;
    if (is_new[r]) {
        o = lb + new_off[r];
    } else {
        o = lb + (size_t)key_lower_bound(new_keys, n_new, key);
        cnt = in.cnt[lb];
        for (int k = 0; k < 3; ++k) {
            p[k] = in.pos[3 * lb + k];
            if (in.nrm) nn[k] = in.nrm[3 * lb + k];
            if (in.col) cc[k] = in.col[3 * lb + k];
        }
    }
    for (int64_t j = i; j < n && skeys[j] == key; ++j) {
        const size_t s = vals[j];
        p[0] += xyz[3 * s];
        p[1] += xyz[3 * s + 1];
        p[2] += xyz[3 * s + 2];
        if (nrm) {
            nn[0] += nrm[3 * s];
            nn[1] += nrm[3 * s + 1];
            nn[2] += nrm[3 * s + 2];
        }
        if (col) {
            cc[0] += col[3 * s];
            cc[1] += col[3 * s + 1];
            cc[2] += col[3 * s + 2];
        }
        ++cnt;
    }
    out.key[o] = key;
    out.cnt[o] = cnt;
    for (int k = 0; k < 3; ++k) out.pos[3 * o + k] = p[k];
    if (out.nrm)
        for (int k = 0; k < 3; ++k) out.nrm[3 * o + k] = nn[k];
    if (out.col)
        for (int k = 0; k < 3; ++k) out.col[3 * o + k] = cc[k];
}

// ---- insert_scan: the dense-map cropper and ColorRangeCropper (croppers.cpp:178-239) as one flag; the compaction of the
// three fp64 x 3 arrays is k_gather_rows<3, true>
__global__ void k_dm_scan_flags(const double* __restrict__ xyz, const double* __restrict__ col, int64_t n, CropCfg c, double lo0,
                                double lo1, double lo2, double hi0, double hi1, double hi2, uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool keep = crop_inside(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    if (col) {
        const double r = col[3 * i], g = col[3 * i + 1], b = col[3 * i + 2];
        keep = keep && lo0 <= r && lo1 <= g && lo2 <= b && r <= hi0 && g <= hi1 && b <= hi2;
    }
    flags[i] = keep ? 1u : 0u;
}

// ---- carve (getKeysOfCarvedPoints, helpers.cpp:360-390; getVoxelsWithinPointNeighborhood, VoxelHashMap.cpp:13-45) ----
// One wave per ray, four rays per workgroup.  The sample loop is wave-uniform (every lane of a wave reads the same scan
// point, so `distance` is the reference's running sum in every lane); the 64 lanes share the off.n^3 test points of a sample
// and the sample's own key (slot off.n^3).  Lookup key: floor(t / v) -- a division, unlike the map key; centre k v + v/2;
// accepted when sqrt((d0^2 + d1^2) + d2^2) <= r.  Marks are idempotent plain stores.
__global__ void __launch_bounds__(256) k_dm_carve(const double* __restrict__ scan, int64_t n_scan, double sx, double sy, double sz,
                                                  double step, double max_ray, double trunc, double radius, double voxel,
                                                  double half_voxel, DmOffsets off, const uint64_t* __restrict__ rkeys,
                                                  int64_t n_res, uint32_t* __restrict__ mark) {
    __shared__ double s_off[kDmMaxOffsets];   // lane-indexed below: LDS, not a runtime-indexed kernel argument
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kDmMaxOffsets; ++k) s_off[k] = off.d[k];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
    if (i >= n_scan) return;   // wave-uniform, after the only barrier
    const double dx = scan[3 * i] - sx, dy = scan[3 * i + 1] - sy, dz = scan[3 * i + 2] - sz;
    const double length = sqrt(sum_sq3(dx, dy, dz));
    if (!(length > 0.0) || !(length < INFINITY)) return;   // as k_carve_rays: zero-length and non-finite rays are skipped
    const double ux = dx / length, uy = dy / length, uz = dz / length;
    const double reach = fmax(step, fmin(length - trunc, max_ray));
    const int no = off.n, cube = no * no * no;
    double distance = 0.0;
    while (distance < reach) {
        double t = distance * ux;
        const double px = t + sx;
        t = distance * uy;
        const double py = t + sy;
        t = distance * uz;
        const double pz = t + sz;
        for (int c = lane; c <= cube; c += 64) {
            double tx = px, ty = py, tz = pz;
            if (c < cube) {
                const int ix = c / (no * no), iy = (c / no) % no, iz = c % no;
                tx = px + s_off[ix];
                ty = py + s_off[iy];
                tz = pz + s_off[iz];
            }
            const double kx = floor(tx / voxel), ky = floor(ty / voxel), kz = floor(tz / voxel);
            if (!vox_fits(kx, ky, kz)) continue;   // cannot be in the map (NaN included)
            if (c < cube) {
                double cx = kx * voxel;
                cx = cx + half_voxel;
                double cy = ky * voxel;
                cy = cy + half_voxel;
                double cz = kz * voxel;
                cz = cz + half_voxel;
                const double d0 = tx - cx, d1 = ty - cy, d2 = tz - cz;
                double u = d0 * d0;
                double v = d1 * d1;
                double q = u + v;
                u = d2 * d2;
                q = q + u;
                if (!(sqrt(q) <= radius)) continue;
            }
            const uint64_t key = vox_pack(kx, ky, kz);
            const int64_t lb = key_lower_bound(rkeys, n_res, key);
            if (lb < n_res && rkeys[lb] == key) mark[lb] = 1u;
        }
        distance += step;
    }
}
// the marked voxels leave: keep[i] = !mark[i] and its exclusive scan give the positions of the rest; the erased keys go out
// as int32 triples in ascending key order (rem_off = exclusive scan of mark; removed may be null)
__global__ void k_dm_keep_flags(const uint32_t* __restrict__ mark, int64_t n, uint32_t* __restrict__ keep) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    keep[i] = mark[i] ? 0u : 1u;
}
__global__ void k_dm_erase(DmCols in, int64_t n, const uint32_t* __restrict__ mark, const uint32_t* __restrict__ keep_off,
                           const uint32_t* __restrict__ rem_off, DmCols out, int32_t* __restrict__ removed) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mark[i]) {
        if (removed) vox_unpack(in.key[i], removed + 3 * (size_t)rem_off[i]);
        return;
    }
    const size_t o = keep_off[i];
    out.key[o] = in.key[i];
    out.cnt[o] = in.cnt[i];
    for (int k = 0; k < 3; ++k) out.pos[3 * o + k] = in.pos[3 * i + k];
    if (out.nrm)
        for (int k = 0; k < 3; ++k) out.nrm[3 * o + k] = in.nrm[3 * i + k];
    if (out.col)
        for (int k = 0; k < 3; ++k) out.col[3 * o + k] = in.col[3 * i + k];
}

// ---- export (toPointCloud, Voxel.cpp:90-114): sum / count, normals not re-normalised; any output may be null ----
__global__ void k_dm_export(DmCols in, int64_t n, double* __restrict__ oxyz, double* __restrict__ onrm, double* __restrict__ ocol,
                            int32_t* __restrict__ okeys, int32_t* __restrict__ ocnt) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double dc = (double)in.cnt[i];
    if (oxyz)
        for (int k = 0; k < 3; ++k) oxyz[3 * i + k] = in.pos[3 * i + k] / dc;
    if (onrm)
        for (int k = 0; k < 3; ++k) onrm[3 * i + k] = in.nrm[3 * i + k] / dc;
    if (ocol)
        for (int k = 0; k < 3; ++k) ocol[3 * i + k] = in.col[3 * i + k] / dc;
    if (okeys) vox_unpack(in.key[i], okeys + 3 * i);
    if (ocnt) ocnt[i] = in.cnt[i];
}

// ---- VoxelizedPointCloud::transform (Voxel.cpp:49-64), literally: position sum and normal sum each become R S + t
// (xform_row with the translation, and no division by w: this kernel's own rule); keys, colour sums and counts stay.
// Written into the spare side.
__global__ void k_dm_transform(DmCols in, int64_t n, Xform64 T, DmCols out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    out.key[i] = in.key[i];
    out.cnt[i] = in.cnt[i];
    for (int f = 0; f < 2; ++f) {
        const double* s = f ? in.nrm : in.pos;
        double* d = f ? out.nrm : out.pos;
        if (!s) continue;
        const double x = s[3 * i], y = s[3 * i + 1], z = s[3 * i + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[3 * i + r] = xform_row<true>(T, r, x, y, z);
    }
    if (out.col)
        for (int k = 0; k < 3; ++k) out.col[3 * i + k] = in.col[3 * i + k];
}

// ---- computeCenter (helpers.cpp:392-402): the sum of the averaged positions in key order, divided by (n + 1e-6).  An
// order-fixed sum: one thread.
__global__ void k_dm_center(DmCols in, int64_t n, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double c[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const double dc = (double)in.cnt[i];
        for (int k = 0; k < 3; ++k) {
            const double a = in.pos[3 * i + k] / dc;
            c[k] = c[k] + a;
        }
    }
    const double d = (double)n + 1e-6;
    for (int k = 0; k < 3; ++k) out[k] = c[k] / d;
}

// ---- removeDuplicatePointsWithinSameVoxels (Voxel.cpp:162-191): the stable sort leaves the lowest index at every run head
__global__ void k_dm_dedup_mark(const uint32_t* __restrict__ heads, const uint32_t* __restrict__ vals, int64_t n,
                                uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    flags[vals[i]] = 1u;   // flags start cleared
}
