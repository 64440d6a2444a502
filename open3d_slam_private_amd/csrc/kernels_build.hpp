// kernels_build.hpp -- target preparation (R1): centroid, centring + bbox, sort keys, brick table, halo bins
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// =================================================================================================
// kernels: target preparation (R1)
// =================================================================================================

// Order-independent centroid: integer sum of llrint(x * 2^16) (numeric contract NC1).
__global__ void k_centroid_sums(const float* __restrict__ xyz, int64_t stride, int64_t n, unsigned long long* sums) {
    __shared__ long long sh[3][4];
    long long s0 = 0, s1 = 0, s2 = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float* p = xyz + i * stride;
        s0 += llrint((double)p[0] * 65536.0);
        s1 += llrint((double)p[1] * 65536.0);
        s2 += llrint((double)p[2] * 65536.0);
    }
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_down(s0, o);
        s1 += __shfl_down(s1, o);
        s2 += __shfl_down(s2, o);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        sh[0][wave] = s0;
        sh[1][wave] = s1;
        sh[2][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long t = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[threadIdx.x][w];
        atomicAdd(&sums[threadIdx.x], (unsigned long long)t);
    }
}

__device__ __forceinline__ int f2ord(float f) {
    int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float ord2f(int i) {
    int j = i >= 0 ? i : i ^ 0x7fffffff;
    float f;
    memcpy(&f, &j, 4);
    return f;
}

// centred = fl(x - c); bounding box of the centred cloud (ordered-int atomics).
__global__ void k_center_bbox(const float* __restrict__ xyz, int64_t stride, int64_t n, float cx, float cy, float cz,
                              float4* __restrict__ out, int* bbox /* min xyz, max xyz as ordered ints */) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float* p = xyz + i * stride;
        float4 q;
        q.x = p[0] - cx;
        q.y = p[1] - cy;
        q.z = p[2] - cz;
        q.w = __uint_as_float((uint32_t)i);
        out[i] = q;
        mn[0] = fminf(mn[0], q.x); mx[0] = fmaxf(mx[0], q.x);
        mn[1] = fminf(mn[1], q.y); mx[1] = fmaxf(mx[1], q.y);
        mn[2] = fminf(mn[2], q.z); mx[2] = fmaxf(mx[2], q.z);
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], __shfl_down(mn[k], o));
            mx[k] = fmaxf(mx[k], __shfl_down(mx[k], o));
        }
    // same-address atomics serialise (measured: 49 k of them on 6 words cost 0.5 ms): one set per workgroup only
    __shared__ float red[6][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) {
            red[k][wave] = mn[k];
            red[3 + k][wave] = mx[k];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        const int nw = (int)(blockDim.x >> 6);
        float v = red[k][0];
        for (int w = 1; w < nw; ++w) v = k < 3 ? fminf(v, red[k][w]) : fmaxf(v, red[k][w]);
        if (k < 3)
            atomicMin(&bbox[k], f2ord(v));
        else
            atomicMax(&bbox[k], f2ord(v));
    }
}

// sort key = (brick z,y,x | bin-in-brick z,y,x)
__global__ void k_point_keys(const float4* __restrict__ pts, int64_t n, float ox, float oy, float oz, float inv_c,
                             uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const int cx = (int)bin_coord_f(p.x, ox, inv_c);
    const int cy = (int)bin_coord_f(p.y, oy, inv_c);
    const int cz = (int)bin_coord_f(p.z, oz, inv_c);
    const uint64_t bk = brick_key((uint32_t)(cx >> kBrickLog2), (uint32_t)(cy >> kBrickLog2), (uint32_t)(cz >> kBrickLog2));
    const uint32_t local = ((cz & (kBrickDim - 1)) << (2 * kBrickLog2)) | ((cy & (kBrickDim - 1)) << kBrickLog2) |
                           (cx & (kBrickDim - 1));
    keys[i] = (bk << (3 * kBrickLog2)) | local;
    vals[i] = (uint32_t)i;
}

__global__ void k_gather_target(const float4* __restrict__ centred, const uint32_t* __restrict__ order, int64_t n,
                                const float* __restrict__ nrm, int64_t nrm_stride, const float* __restrict__ cov,
                                float4* __restrict__ pts_sorted, float4* __restrict__ nrm_sorted,
                                float4* __restrict__ cov_sorted /* 2 float4 per point */) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = order[i];
    const float4 pt = centred[src];
    pts_sorted[i] = pt;
    if (nrm_sorted) {
        // point and normal INTERLEAVED (32 bytes, one 128-byte line holds four pairs): whoever needs the matched point's
        // normal needs the point too, and a random 16-byte gather costs a whole line -- two arrays meant two lines per match
        const float* q = nrm + (int64_t)src * nrm_stride;
        nrm_sorted[2 * i] = pt;
        nrm_sorted[2 * i + 1] = make_float4(q[0], q[1], q[2], 0.f);
    }
    if (cov_sorted) {
        const float* q = cov + (int64_t)src * 6;
        cov_sorted[2 * i] = make_float4(q[0], q[1], q[2], q[3]);
        cov_sorted[2 * i + 1] = make_float4(q[4], q[5], 0.f, 0.f);
    }
}

__global__ void k_brick_heads(const uint64_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || (keys[i] >> (3 * kBrickLog2)) != (keys[i - 1] >> (3 * kBrickLog2))) ? 1u : 0u;
}

// brick_id = inclusive_scan(flags) - 1.  Inserts brick heads into the hash and counts points per bin.
__global__ void k_fill_tables(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flags,
                              const uint32_t* __restrict__ scan, int64_t n, HashEntry* hash, uint32_t mask,
                              uint32_t* __restrict__ counts, uint32_t* __restrict__ occupied,
                              int32_t* __restrict__ dir, int bdx, int bdy, unsigned long long* __restrict__ rows) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t bid = scan[i] - 1u;
    const uint64_t key = keys[i];
    const uint32_t local = (uint32_t)(key & (kBrickCells - 1));
    if (flags[i]) {
        const uint64_t bk = key >> (3 * kBrickLog2);
        uint32_t h = (uint32_t)mix64(bk) & mask;
        for (;;) {
            const unsigned long long prev =
                atomicCAS((unsigned long long*)&hash[h].key, (unsigned long long)kEmptyKey, (unsigned long long)bk);
            if (prev == kEmptyKey) {
                hash[h].val = bid;
                break;
            }
            h = (h + 1) & mask;
        }
        if (dir) {
            const uint32_t m18 = (1u << kBrickBits) - 1u;
            const uint32_t bx = (uint32_t)bk & m18, by = (uint32_t)(bk >> kBrickBits) & m18,
                           bz = (uint32_t)(bk >> (2 * kBrickBits)) & m18;
            dir[((size_t)bz * bdy + by) * bdx + bx] = (int32_t)bid;
        }
    }
    const uint32_t old = atomicAdd(&counts[(size_t)bid * kBrickCells + local], 1u);
    if (rows && old == 0) {   // first point of its bin: mark the bin's x-row (z_local * 8 + y_local) as occupied
        const uint64_t bk = key >> (3 * kBrickLog2);
        const uint32_t m18 = (1u << kBrickBits) - 1u;
        const uint32_t bx = (uint32_t)bk & m18, by = (uint32_t)(bk >> kBrickBits) & m18, bz = (uint32_t)(bk >> (2 * kBrickBits)) & m18;
        atomicOr(&rows[((size_t)bz * bdy + by) * bdx + bx], 1ull << (local >> kBrickLog2));
    }
    // one aggregated atomic per wave on the single "occupied bins" word (same-address atomics serialise)
    const unsigned long long first = __ballot(old == 0);
    if (first && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)first) - 1)) atomicAdd(occupied, (uint32_t)__popcll(first));
}

// Halo bins: every reference point is listed in each bin whose box, grown by rho_h, contains it.
struct HaloCfg {
    float ox, oy, oz, inv_c, r_ins;  // r_ins = rho_h + safety margin
    int dimx, dimy, dimz;
};
__device__ __forceinline__ void halo_range(float v, float o, float inv_c, float r, int dim, int& lo, int& hi) {
    lo = (int)fminf(fmaxf(bin_coord_f(v - r, o, inv_c), 0.f), (float)(dim - 1));
    hi = (int)fminf(fmaxf(bin_coord_f(v + r, o, inv_c), 0.f), (float)(dim - 1));
}
// pass 0: count (and mark the bin the point itself lies in: `occ`, one byte per bin, may be null -- plain stores of the
// same value: bit masks would need atomics, and same-address atomics serialise),
// pass 1: fill (cursor = running insert position per bin)
__global__ void k_halo_insert(const float4* __restrict__ pts_sorted, int64_t n, HaloCfg c, int pass,
                              uint32_t* __restrict__ counts_or_cursor, float4* __restrict__ halo_pts,
                              uint8_t* __restrict__ occ) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts_sorted[i];
    int x0, x1, y0, y1, z0, z1;
    halo_range(p.x, c.ox, c.inv_c, c.r_ins, c.dimx, x0, x1);
    halo_range(p.y, c.oy, c.inv_c, c.r_ins, c.dimy, y0, y1);
    halo_range(p.z, c.oz, c.inv_c, c.r_ins, c.dimz, z0, z1);
    if (pass == 0 && occ) {
        int bx, by, bz, unused;
        halo_range(p.x, c.ox, c.inv_c, 0.f, c.dimx, bx, unused);
        halo_range(p.y, c.oy, c.inv_c, 0.f, c.dimy, by, unused);
        halo_range(p.z, c.oz, c.inv_c, 0.f, c.dimz, bz, unused);
        occ[((size_t)bz * c.dimy + by) * c.dimx + bx] = 1;
    }
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const size_t B = ((size_t)z * c.dimy + y) * c.dimx + x;
                const uint32_t slot = atomicAdd(&counts_or_cursor[B], 1u);
                if (pass == 1) halo_pts[slot] = make_float4(p.x, p.y, p.z, __uint_as_float((uint32_t)i));
            }
}

// Empty-space bound of the halo bins.  lb(B) bounds from below the distance between ANY position that bin_coord_f maps to
// bin B and ANY reference point.  Two facts, both per bin B' = B + (dx, dy, dz) with g = max(|d| - 1, 0) whole bins between
// the two per axis:
//  (a) a reference point INSIDE B' is at least c_h * |g| away;
//  (b) every reference point p lies only in and near bins whose run is non-empty (a run lists the points within rho_h of
//      its bin's box).  Let S be the smallest |g|^2 over the bins with a run.  Walking from p towards B by s < rho_h ends in
//      a bin that lists p, hence one with |g|^2 >= S, and has shortened the distance by exactly s: p is at least
//      c_h * sqrt(S) + rho_h away.
// lb is the larger of the two.  The minimum of |g|^2 over a set of bins separates per axis: three passes over the dense
// grid, each looking R bins either way (R bins cover max_dist; "nothing within R" counts as a gap of R bins, still a lower
// bound).  .x of the intermediate pairs belongs to (a), .y to (b).
struct HaloBoundCfg {
    int dimx, dimy, dimz, R;
    float ch;        // bin edge
    float rho_h;     // exactness radius of the halo level
    float eps_bins;  // rounding of a bin coordinate fl(fl(v - o) * 1/c_h), in bins (2^-21 * largest dimension)
    float sub;       // absolute margin taken off (2 * abs_margin, as the halo radius carries)
};
// Witness of an empty bin: the passes below carry the arg-min of (b) along -- WHICH bin with a run is the nearest, as
// signed bin offsets -- so that the last pass knows that bin, L, and the directory entry of an empty bin can name one real
// reference point near it (the representative of L's run, k_halo_rep).  Tie rule, the same in every pass: the smallest
// squared whole-bin gap S1 first; among equal S1, axis by axis in the order z, y, x: the smallest |d| and, between -d and +d,
// the negative offset.  (Each pass walks d from -R to +R and replaces its choice only on a strictly smaller (S1, |d|).)  The
// offsets live in arrays of their own (`xo`, `yo`), null when no witness is wanted: the bound's intermediates stay as they
// were.  xo: offset + 128, 0 = no run in reach; yo: {dx + 128, dy + 128, 1, 0}, all 0 = none; S1 of the arg-min is kept
// uncapped in yo's upper half so that a choice made at a gap beyond R (where the bound's S1 saturates at R^2) is still by gap.
// pass x: whole bins between bin (x, y, z) and the nearest bin of its x-row that holds a point (.x: `occ` bytes) / that has a
// run (.y: `start`, after its scan); 0: that bin itself or its neighbour; R: none within R + 1
__global__ void k_halo_gap_x(const uint8_t* __restrict__ occ, const uint32_t* __restrict__ start, HaloBoundCfg c,
                             uchar2* __restrict__ gx, uint8_t* __restrict__ xo) {
    const size_t B = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t nb = (size_t)c.dimx * c.dimy * c.dimz;
    if (B >= nb) return;
    const int x = (int)(B % (size_t)c.dimx);
    int own = c.R + 1, run = c.R + 1, at = -128;
    const int lo = max(-c.R - 1, -x), hi = min(c.R + 1, c.dimx - 1 - x);
    uint32_t prev = start[(ptrdiff_t)B + lo];
    for (int d = lo; d <= hi; ++d) {
        const uint32_t next = start[(ptrdiff_t)B + d + 1];
        if (next != prev) {
            if (at == -128 || abs(d) < run) at = d;
            run = min(run, abs(d));
        }
        if (occ[(ptrdiff_t)B + d]) own = min(own, abs(d));
        prev = next;
    }
    gx[B] = make_uchar2((unsigned char)min(max(own - 1, 0), c.R), (unsigned char)min(max(run - 1, 0), c.R));
    if (xo) xo[B] = (uint8_t)(at + 128);
}
// pass y: min over the bins of the same (x, z) column of gx^2 + gy^2
__global__ void k_halo_gap_y(const uchar2* __restrict__ gx, HaloBoundCfg c, ushort2* __restrict__ sxy,
                             const uint8_t* __restrict__ xo, uint32_t* __restrict__ yo) {
    const size_t B = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t nb = (size_t)c.dimx * c.dimy * c.dimz;
    if (B >= nb) return;
    const int y = (int)((B / (size_t)c.dimx) % (size_t)c.dimy);
    int S0 = c.R * c.R, S1 = S0;
    int wS = 0x7fffffff, wdy = 0, wdx = 0;   // arg-min of S1 over the rows that have a run in reach
    const int lo = max(-c.R, -y), hi = min(c.R, c.dimy - 1 - y);
    for (int d = lo; d <= hi; ++d) {
        const uchar2 v = gx[(ptrdiff_t)B + (ptrdiff_t)d * c.dimx];
        const int g = max(abs(d) - 1, 0);
        S0 = min(S0, g * g + (int)v.x * (int)v.x);
        S1 = min(S1, g * g + (int)v.y * (int)v.y);
        if (xo) {
            const int o = (int)xo[(ptrdiff_t)B + (ptrdiff_t)d * c.dimx];
            const int s = g * g + (int)v.y * (int)v.y;
            if (o != 0 && (s < wS || (s == wS && abs(d) < abs(wdy)))) {
                wS = s;
                wdy = d;
                wdx = o - 128;
            }
        }
    }
    sxy[B] = make_ushort2((unsigned short)S0, (unsigned short)S1);
    if (yo) yo[B] = wS == 0x7fffffff ? 0u : ((uint32_t)(wdx + 128) | ((uint32_t)(wdy + 128) << 8) | ((uint32_t)(wS + 1) << 16));
}
// pass z + directory: one aligned record per bin, {first halo record, count} -- or, for a bin whose run is empty,
// {witness, 0x80000000 | bits(lb)} (lb >= 0, rounded down by the margins below): the search reads it with the ONE load
// that used to fetch the run's start.  sxy == null: no bound (lb = 0).  The witness field leaves this kernel as the linear
// index of L, the nearest bin with a run (yo == null, or no run within R bins: kNoWitness); k_halo_witness turns it into
// a reference point once the runs are filled.  (.x of an empty bin used to repeat the start of the next run; the search
// only ever read it as an empty range.)
constexpr uint32_t kNoWitness = 0xffffffffu;
__global__ void k_halo_dir(const uint32_t* __restrict__ start, const ushort2* __restrict__ sxy, HaloBoundCfg c,
                           uint2* __restrict__ dir, const uint32_t* __restrict__ yo) {
    const size_t B = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t nb = (size_t)c.dimx * c.dimy * c.dimz;
    if (B >= nb) return;
    const uint32_t s = start[B], cnt = start[B + 1] - s;
    uint32_t first = s, second = cnt;
    if (cnt == 0) {
        float lb = 0.f;
        first = kNoWitness;
        if (sxy) {
            const size_t plane = (size_t)c.dimx * c.dimy;
            const int z = (int)(B / plane);
            int S0 = c.R * c.R, S1 = S0;
            int wS = 0x7fffffff, wdz = 0;
            uint32_t wo = 0;
            const int lo = max(-c.R, -z), hi = min(c.R, c.dimz - 1 - z);
            for (int d = lo; d <= hi; ++d) {
                const ushort2 v = sxy[(ptrdiff_t)B + (ptrdiff_t)d * (ptrdiff_t)plane];
                const int g = max(abs(d) - 1, 0);
                S0 = min(S0, g * g + (int)v.x);
                S1 = min(S1, g * g + (int)v.y);
                if (yo) {
                    const uint32_t o = yo[(ptrdiff_t)B + (ptrdiff_t)d * (ptrdiff_t)plane];
                    const int sw = g * g + (int)(o >> 16) - 1;
                    if (o != 0u && (sw < wS || (sw == wS && abs(d) < abs(wdz)))) {
                        wS = sw;
                        wdz = d;
                        wo = o;
                    }
                }
            }
            if (wo != 0u)
                first = (uint32_t)((ptrdiff_t)B + (ptrdiff_t)wdz * (ptrdiff_t)plane + ((ptrdiff_t)((wo >> 8) & 255u) - 128) * c.dimx +
                                   ((ptrdiff_t)(wo & 255u) - 128));
            // bins -> metres, downward: 1e-3 relative (rounding of 1/c_h, of the distance the search computes and of its
            // comparison with rho), the rounding of the two bin coordinates per axis, the absolute margin of the radii
            const float down = 1.0f - 1e-3f;
            const float g0 = sqrtf((float)S0) * down - 3.5f * c.eps_bins;
            const float g1 = sqrtf((float)S1) * down - 3.5f * c.eps_bins;
            const float lb0 = g0 * c.ch - c.sub;
            const float lb1 = S1 > 0 ? g1 * c.ch + c.rho_h * down - c.sub : 0.f;
            lb = fmaxf(fmaxf(lb0, lb1), 0.f);
        }
        second = 0x80000000u | __float_as_uint(lb);
    }
    dir[B] = make_uint2(first, second);
}
// Representative of a bin's run: the listed point nearest the centre of the bin's box, ties by the smallest sorted position --
// a function of the run as a SET (its records arrive in atomic order).  One thread per bin with a run.
struct HaloRepCfg {
    float ox, oy, oz, ch;
    int dimx, dimy, dimz;
};
__global__ void k_halo_rep(const uint2* __restrict__ dir, const float4* __restrict__ halo_pts, HaloRepCfg c,
                           uint32_t* __restrict__ rep) {
    const size_t B = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t nb = (size_t)c.dimx * c.dimy * c.dimz;
    if (B >= nb) return;
    const uint2 hd = dir[B];
    if ((int)hd.y < 0) return;
    const int x = (int)(B % (size_t)c.dimx), y = (int)((B / (size_t)c.dimx) % (size_t)c.dimy), z = (int)(B / ((size_t)c.dimx * c.dimy));
    const float cx = c.ox + ((float)x + 0.5f) * c.ch, cy = c.oy + ((float)y + 0.5f) * c.ch, cz = c.oz + ((float)z + 0.5f) * c.ch;
    float bd = INFINITY;
    uint32_t bp = kNoWitness;
    for (uint32_t j = hd.x; j < hd.x + hd.y; ++j) {
        const float4 t = halo_pts[j];
        const float dx = t.x - cx, dy = t.y - cy, dz = t.z - cz;
        const float d2 = sum_sq3(dx, dy, dz);
        const uint32_t pos = __float_as_uint(t.w);
        if (d2 < bd || (d2 == bd && pos < bp)) {
            bd = d2;
            bp = pos;
        }
    }
    rep[B] = bp;
}
// ... and the empty bins trade the index of L for L's representative (a sorted position into Grid::pts)
__global__ void k_halo_witness(uint2* __restrict__ dir, const uint32_t* __restrict__ rep, size_t nb) {
    const size_t B = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (B >= nb) return;
    const uint2 hd = dir[B];
    if ((int)hd.y < 0 && hd.x != kNoWitness) dir[B].x = rep[hd.x];
}
