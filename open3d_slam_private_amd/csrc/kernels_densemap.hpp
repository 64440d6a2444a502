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

// ---- carve by bricks (reg_dense_map_carve_scan).  The coarse level of a map, built per call from its
// ascending keys: a brick is 8 x 8 x 8 voxels; its key is the voxel key with every 21-bit offset-binary field shifted right
// by 3, packed as vox_pack packs.  The brick keys are sorted and run-length encoded (sort_runs); per brick a 512-bit
// occupancy mask: word = z & 7, bit = (y & 7) << 3 | (x & 7).
constexpr int kDmBrickShift = 3;
constexpr int kDmBrickSlots = 64;   // bricks a sample's box may touch: 4 per axis (16 offsets span at most 17 voxels: 3)
constexpr uint64_t kDmFieldMask = (1ull << kVoxBits) - 1;
__device__ __forceinline__ uint64_t dm_brick_pack(uint64_t bx, uint64_t by, uint64_t bz) {
    return (bz << (2 * kVoxBits)) | (by << kVoxBits) | bx;
}
__global__ void k_dm_brick_keys(const uint64_t* __restrict__ rkeys, int64_t n, uint64_t* __restrict__ keys,
                                uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = rkeys[i];
    keys[i] = dm_brick_pack((k & kDmFieldMask) >> kDmBrickShift, ((k >> kVoxBits) & kDmFieldMask) >> kDmBrickShift,
                            ((k >> (2 * kVoxBits)) & kDmFieldMask) >> kDmBrickShift);
    vals[i] = (uint32_t)i;
}
// one thread per run head of the sorted brick keys: the brick's key and the OR of its voxels' bits (a run holds at most 512)
__global__ void k_dm_brick_masks(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ svals, int64_t n,
                                 const uint32_t* __restrict__ heads, const uint32_t* __restrict__ run,
                                 const uint64_t* __restrict__ rkeys, uint64_t* __restrict__ bkeys, uint64_t* __restrict__ bmask) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n || !heads[i]) return;
    const uint64_t key = sorted[i];
    uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t j = i; j < n && sorted[j] == key; ++j) {
        const uint64_t k = rkeys[svals[j]];
        const uint64_t bit = 1ull << ((((k >> kVoxBits) & 7ull) << 3) | (k & 7ull));
        const int z = (int)((k >> (2 * kVoxBits)) & 7ull);
#pragma unroll
        for (int q = 0; q < 8; ++q) w[q] |= z == q ? bit : 0ull;   // compile-time indices: w stays in registers
    }
    const size_t r = run[i];
    bkeys[r] = key;
#pragma unroll
    for (int q = 0; q < 8; ++q) bmask[8 * r + q] = w[q];
}

// The carve with the coarse level in front of the lookups.  kLanes lanes per ray (a lane group never straddles a wave);
// the sample loop is uniform in the group, so `distance` is the reference's running sum in each of its lanes.  The
// arithmetic per sample and per test point is that of k_dm_carve, operation for operation; only the way a lookup key is
// found in the map differs:
//   A. the box of a sample: per axis the keys floor((p + first offset) / v) and floor((p + last offset) / v) -- the
//      operations of a test point, and x -> floor((p + x) / v) is monotonic in fp64, so every test point's key lies between
//      them -- widened by the sample's own key and cut to the packable range.  The lanes of the group look the box's bricks
//      up in the brick keys (one binary search each) and leave their positions in the group's LDS slots.  No brick: the
//      sample is done.
//   B. a test point whose brick is absent, or whose bit in the brick's mask is clear, is not in the map; the others go on
//      to key_lower_bound and the mark.  A box of more than kDmBrickSlots bricks (not reachable with 16 offsets) and a
//      key outside its sample's box are looked up directly: the coarse level only ever skips keys it has proven absent.
// stats (null in production): [0] samples, [1] samples that ended at A, added once per ray.
template <int kLanes>
__global__ void __launch_bounds__(256)
    k_dm_carve_bricks(const double* __restrict__ scan, int64_t n_scan, double sx, double sy, double sz, double step, double max_ray,
                      double trunc, double radius, double voxel, double half_voxel, DmOffsets off,
                      const uint64_t* __restrict__ rkeys, int64_t n_res, const uint64_t* __restrict__ bkeys,
                      const uint64_t* __restrict__ bmask, int64_t n_bricks, uint32_t* __restrict__ mark,
                      unsigned long long* __restrict__ stats) {
    static_assert(kLanes == 8 || kLanes == 16 || kLanes == 32 || kLanes == 64, "a lane group divides a wave");
    constexpr int kRays = 256 / kLanes;
    __shared__ double s_off[kDmMaxOffsets];   // lane-indexed below: LDS, not a runtime-indexed kernel argument
    __shared__ int32_t s_slot[kRays][kDmBrickSlots];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kDmMaxOffsets; ++k) s_off[k] = off.d[k];
    }
    __syncthreads();
    const int lane = threadIdx.x % kLanes, g = threadIdx.x / kLanes;
    const int gbase = (threadIdx.x & 63) - lane;
    const unsigned long long gmask = kLanes == 64 ? ~0ull : ((1ull << kLanes) - 1ull);
    const int64_t i = blockIdx.x * (int64_t)kRays + g;
    if (i >= n_scan) return;   // group-uniform, after the only barrier
    const double dx = scan[3 * i] - sx, dy = scan[3 * i + 1] - sy, dz = scan[3 * i + 2] - sz;
    const double length = sqrt(sum_sq3(dx, dy, dz));
    if (!(length > 0.0) || !(length < INFINITY)) return;   // as k_dm_carve
    const double ux = dx / length, uy = dy / length, uz = dz / length;
    const double reach = fmax(step, fmin(length - trunc, max_ray));
    const int no = off.n, cube = no * no * no;
    const double off_lo = s_off[0], off_hi = s_off[no - 1];
    const double kmax = (double)(kVoxOff - 1);
    unsigned long long n_samples = 0, n_done = 0;
    double distance = 0.0;
    while (distance < reach) {
        double t = distance * ux;
        const double px = t + sx;
        t = distance * uy;
        const double py = t + sy;
        t = distance * uz;
        const double pz = t + sz;
        ++n_samples;
        // A. the box and its bricks
        const double p3[3] = {px, py, pz};
        long long b0[3];
        int nb[3];
        bool empty = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double t0 = p3[a] + off_lo, t1 = p3[a] + off_hi;
            const double own = floor(p3[a] / voxel);
            const double lo = fmax(fmin(floor(t0 / voxel), own), -kmax), hi = fmin(fmax(floor(t1 / voxel), own), kmax);
            empty = empty || !(lo <= hi);   // no key of this axis fits (NaN included)
            b0[a] = ((long long)lo + kVoxOff) >> kDmBrickShift;
            nb[a] = empty ? 1 : (int)((((long long)hi + kVoxOff) >> kDmBrickShift) - b0[a]) + 1;
        }
        if (empty) {   // every lookup of the sample is skipped by vox_fits
            ++n_done;
            distance += step;
            continue;
        }
        const int nbricks = nb[0] * nb[1] * nb[2];
        const bool coarse = nbricks <= kDmBrickSlots;
        if (coarse) {
            group_sync();   // the slots of the previous sample have been read
            bool any = false;
            for (int c0 = 0; c0 < nbricks; c0 += kLanes) {
                const int c = c0 + lane;
                int32_t slot = -1;
                if (c < nbricks) {
                    const int ix = c % nb[0], iy = (c / nb[0]) % nb[1], iz = c / (nb[0] * nb[1]);
                    const uint64_t bk = dm_brick_pack((uint64_t)(b0[0] + ix), (uint64_t)(b0[1] + iy), (uint64_t)(b0[2] + iz));
                    const int64_t lb = key_lower_bound(bkeys, n_bricks, bk);
                    if (lb < n_bricks && bkeys[lb] == bk) slot = (int32_t)lb;
                    s_slot[g][c] = slot;
                }
                any = any || ((__ballot(slot >= 0) >> gbase) & gmask) != 0ull;
            }
            if (!any) {
                ++n_done;
                distance += step;
                continue;
            }
            group_sync();   // the slots are visible to every lane of the group
        }
        // B. the test points
        for (int c = lane; c <= cube; c += kLanes) {
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
            if (coarse) {
                const long long fx = (long long)kx + kVoxOff, fy = (long long)ky + kVoxOff, fz = (long long)kz + kVoxOff;
                const long long jx = (fx >> kDmBrickShift) - b0[0], jy = (fy >> kDmBrickShift) - b0[1],
                                jz = (fz >> kDmBrickShift) - b0[2];
                if (jx >= 0 && jx < nb[0] && jy >= 0 && jy < nb[1] && jz >= 0 && jz < nb[2]) {
                    const int32_t slot = s_slot[g][((int)jz * nb[1] + (int)jy) * nb[0] + (int)jx];
                    if (slot < 0) continue;
                    const uint64_t w = bmask[8 * (size_t)slot + (size_t)(fz & 7)];
                    if (!((w >> (((fy & 7) << 3) | (fx & 7))) & 1ull)) continue;
                }
            }
            const uint64_t key = vox_pack(kx, ky, kz);
            const int64_t lb = key_lower_bound(rkeys, n_res, key);
            if (lb < n_res && rkeys[lb] == key) mark[lb] = 1u;
        }
        distance += step;
    }
    if (stats && lane == 0) {
        atomicAdd(stats, n_samples);
        atomicAdd(stats + 1, n_done);
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
