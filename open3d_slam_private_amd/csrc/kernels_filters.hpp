// kernels_filters.hpp -- data-point filters: SamplingSurfaceNormal (reference side) and the reading-side point filters
// Part of the single translation unit reg_core.hip (included there, in this order; not a standalone header).
#pragma once

// =================================================================================================
// SamplingSurfaceNormalDataPointsFilter (libpointmatcher DataPointsFilters/SamplingSurfaceNormal.cpp buildNew /
// fuseRange) under the determinism contract of reg_sampling_surface_normal (include/o3dslam_reg.h).
// The tree shape depends only on (n, knn): the host lists every level's open segments (count > knn) and every leaf.
// Per level: k_ssn_keys (cut axis from the propagated box, 64-bit key (orderable coordinate << 32) | index),
// a rocPRIM segmented radix sort over the open segments, k_ssn_extract (new order) and k_ssn_children (cut value ->
// child boxes).  Leaves: one thread per leaf (k_ssn_leaf), then a scan over the input indices and k_ssn_scatter.
// =================================================================================================
constexpr int kSsnMaxKnn = 64;

__device__ __forceinline__ uint32_t ssn_orderable(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;   // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// utils.h argMax: first strict maximum, starting from 0 (an all-zero extent gives axis 0)
__device__ __forceinline__ int ssn_axis(const float* box) {
    float best = 0.f;
    int arg = 0;
    for (int a = 0; a < 3; ++a) {
        const float e = box[3 + a] - box[a];
        if (e > best) {
            best = e;
            arg = a;
        }
    }
    return arg;
}

// last open segment whose begin <= i; -1 when i lies in no open segment (a leaf of an earlier level)
__device__ __forceinline__ int ssn_segment_of(const int32_t* __restrict__ sb, const int32_t* __restrict__ se, int ns, int i) {
    int lo = 0, hi = ns;   // first begin > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sb[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    const int j = lo - 1;
    return (j >= 0 && i < se[j]) ? j : -1;
}

// Packs the (strided) input into n x 3 floats, flags non-finite values and reduces the bounding box (orderable keys).
__global__ void __launch_bounds__(256)
k_ssn_pack(const float* __restrict__ xyz, int64_t stride, int n, float* __restrict__ px, uint32_t* __restrict__ misc) {
    __shared__ uint32_t s_lo[3][256], s_hi[3][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (i < n) {
        bool bad = false;
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[(size_t)i * stride + a];
            px[3 * (size_t)i + a] = v;
            if (!isfinite(v)) bad = true;
            lo[a] = hi[a] = ssn_orderable(v);
        }
        if (bad) misc[6] = 1u;
    }
    for (int a = 0; a < 3; ++a) {
        s_lo[a][threadIdx.x] = lo[a];
        s_hi[a][threadIdx.x] = hi[a];
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                s_lo[a][threadIdx.x] = min(s_lo[a][threadIdx.x], s_lo[a][threadIdx.x + s]);
                s_hi[a][threadIdx.x] = max(s_hi[a][threadIdx.x], s_hi[a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int a = 0; a < 3; ++a) {
            atomicMin(&misc[a], s_lo[a][0]);
            atomicMax(&misc[3 + a], s_hi[a][0]);
        }
}

// root box + identity permutation
__global__ void __launch_bounds__(256)
k_ssn_init(const uint32_t* __restrict__ misc, int n, float* __restrict__ box0, int32_t* __restrict__ perm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 6) box0[i] = float_from_orderable(misc[i]);
    if (i < n) perm[i] = i;
}

__global__ void __launch_bounds__(256)
k_ssn_keys(const float* __restrict__ px, const int32_t* __restrict__ perm, int n, const int32_t* __restrict__ sb,
           const int32_t* __restrict__ se, int ns, const float* __restrict__ boxes, uint64_t* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = ssn_segment_of(sb, se, ns, i);
    if (j < 0) return;
    const int ax = ssn_axis(boxes + 6 * (size_t)j);
    const uint32_t p = (uint32_t)perm[i];
    keys[i] = ((uint64_t)ssn_orderable(px[3 * (size_t)p + ax]) << 32) | (uint64_t)p;
}

__global__ void __launch_bounds__(256)
k_ssn_extract(const uint64_t* __restrict__ keys, int n, const int32_t* __restrict__ sb, const int32_t* __restrict__ se,
              int ns, int32_t* __restrict__ perm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (ssn_segment_of(sb, se, ns, i) < 0) return;
    perm[i] = (int32_t)(uint32_t)keys[i];
}

// child boxes: cutVal = coordinate of the first point of the right half (buildNew)
__global__ void __launch_bounds__(256)
k_ssn_children(const float* __restrict__ px, const int32_t* __restrict__ perm, const int32_t* __restrict__ sb,
               const int32_t* __restrict__ se, const int32_t* __restrict__ child, int ns, const float* __restrict__ boxes,
               float* __restrict__ next_boxes) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ns) return;
    float box[6];
    for (int a = 0; a < 6; ++a) box[a] = boxes[6 * (size_t)j + a];
    const int ax = ssn_axis(box);
    const int c = se[j] - sb[j];
    const int left = c - c / 2;
    const float cut = px[3 * (size_t)perm[sb[j] + left] + ax];
    const int cl = child[2 * j], cr = child[2 * j + 1];
    if (cl >= 0) {
        for (int a = 0; a < 6; ++a) next_boxes[6 * (size_t)cl + a] = box[a];
        next_boxes[6 * (size_t)cl + 3 + ax] = cut;
    }
    if (cr >= 0) {
        for (int a = 0; a < 6; ++a) next_boxes[6 * (size_t)cr + a] = box[a];
        next_boxes[6 * (size_t)cr + ax] = cut;
    }
}

// Rank of the scatter sums C: eigenvalues by fp64 Jacobi, the rank rule of k_pca_finish (pca_rank).
__device__ __forceinline__ int ssn_rank(const float* C) {
    double M[9] = {C[0], C[1], C[2], C[1], C[3], C[4], C[2], C[4], C[5]}, V[9], lam[3];
    jacobi_eig_sym3(M, V, lam);
    int o[3];
    return pca_rank(lam, o);
}

// One thread per leaf (fuseRange): actual extent vs maxBoxDim, fp32 sequential mean / scatter, rank test when an
// eigen output is requested.  Writes the leaf's PcaMoments (idx = its smallest original index), the per-input leaf id
// and the keep flag of the input indices that become output rows.
__global__ void __launch_bounds__(256)
k_ssn_leaf(const float* __restrict__ px, const int32_t* __restrict__ perm, const int32_t* __restrict__ leaf_begin,
           int n_leaves, float max_box_dim, int need_eig, int method, PcaMoments* __restrict__ leaf_mom,
           int32_t* __restrict__ leaf_id, uint32_t* __restrict__ keep, unsigned long long* __restrict__ n_unfit) {
    const int L = blockIdx.x * 256 + threadIdx.x;
    if (L >= n_leaves) return;
    const int b = leaf_begin[L], e = leaf_begin[L + 1];
    const int m = e - b;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int32_t min_idx = 0x7fffffff;
    for (int r = b; r < e; ++r) {
        const int32_t p = perm[r];
        min_idx = min(min_idx, p);
        for (int a = 0; a < 3; ++a) {
            const float v = px[3 * (size_t)p + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
    float dim = hi[0] - lo[0];
    for (int a = 1; a < 3; ++a) dim = fmaxf(dim, hi[a] - lo[a]);
    bool fit = !(dim > max_box_dim);
    PcaMoments rec;
    pca_moments(m, [&](int r) {
        const size_t p = (size_t)perm[b + r];
        return make_float3(px[3 * p], px[3 * p + 1], px[3 * p + 2]);
    }, rec.mean, rec.C, rec.max_d2);
    if (fit && need_eig && ssn_rank(rec.C) + 1 < 3) fit = false;
    for (int a = 0; a < 3; ++a) rec.p[a] = rec.mean[a];
    rec.m = (float)m;
    rec.idx = (uint32_t)min_idx;
    rec.pad = fit ? 1u : 0u;
    leaf_mom[L] = rec;
    for (int r = b; r < e; ++r) {
        const int32_t p = perm[r];
        leaf_id[p] = fit ? L : -1;
        if (method == 0) keep[p] = fit ? 1u : 0u;
        else keep[p] = (fit && p == min_idx) ? 1u : 0u;
    }
    if (!fit) atomicAdd(n_unfit, (unsigned long long)m);
}

// One thread per input index: kept rows go to slot pos[i] (ascending kept index).  Output moments carry idx = slot so
// k_pca_finish writes the compacted normals / eigen outputs directly.
__global__ void __launch_bounds__(256)
k_ssn_scatter(const float* __restrict__ px, int n, int method, const uint32_t* __restrict__ keep,
              const uint32_t* __restrict__ pos, const int32_t* __restrict__ leaf_id, const PcaMoments* __restrict__ leaf_mom,
              float* __restrict__ out_xyz, int32_t* __restrict__ src_idx, float* __restrict__ densities,
              PcaMoments* __restrict__ out_mom) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const uint32_t s = pos[i];
    PcaMoments rec = leaf_mom[leaf_id[i]];
    if (method == 0)
        for (int a = 0; a < 3; ++a) rec.p[a] = px[3 * (size_t)i + a];
    for (int a = 0; a < 3; ++a) out_xyz[3 * (size_t)s + a] = rec.p[a];
    src_idx[s] = i;
    if (densities) densities[s] = pca_density((int)rec.m, rec.max_d2);
    rec.idx = s;
    out_mom[s] = rec;
}

// =================================================================================================
// Reading-side point filters (reg_filter_points): a predicate per point of the current index list + order-preserving
// compaction (rocPRIM exclusive scan).  Norm: sqrtf((x*x + y*y) + z*z), no contraction.
// =================================================================================================
struct PointFilterDev {
    int type, dim, remove_inside, step, phase;
    float value, limit;
    float box[6];
};

__global__ void __launch_bounds__(256)
k_pf_pack(const float* __restrict__ xyz, int64_t stride, const float* __restrict__ nrm, const float* __restrict__ cov,
          int n, float* __restrict__ px, float* __restrict__ pn, float* __restrict__ pc, int32_t* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int a = 0; a < 3; ++a) px[3 * (size_t)i + a] = xyz[(size_t)i * stride + a];
    if (nrm)
        for (int a = 0; a < 3; ++a) pn[3 * (size_t)i + a] = nrm[3 * (size_t)i + a];
    if (cov)
        for (int a = 0; a < 6; ++a) pc[6 * (size_t)i + a] = cov[6 * (size_t)i + a];
    idx[i] = i;
}

__global__ void __launch_bounds__(256)
k_pf_axis(const float* __restrict__ px, const int32_t* __restrict__ idx, int m, int dim, float* __restrict__ vals,
          uint32_t* __restrict__ has_nan) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const float v = px[3 * (size_t)idx[j] + dim];
    if (isnan(v)) has_nan[0] = 1u;
    vals[j] = v;
}

__global__ void __launch_bounds__(256)
k_pf_pred(const float* __restrict__ px, const int32_t* __restrict__ idx, int m, PointFilterDev f,
          uint32_t* __restrict__ flag) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const float* p = px + 3 * (size_t)idx[j];
    const float x = p[0], y = p[1], z = p[2];
    float d;
    if (f.dim < 0) {
        float a = x * x;
        float b = y * y;
        float s = a + b;
        a = z * z;
        s = s + a;
        d = sqrtf(s);
    } else {
        d = p[f.dim];
    }
    bool keep = true;
    switch (f.type) {
        case REG_DPF_MAX_DIST: keep = d < f.value; break;
        case REG_DPF_MIN_DIST: keep = d > f.value; break;
        case REG_DPF_DISTANCE_LIMIT: keep = f.remove_inside ? (d > f.value) : (d < f.value); break;
        case REG_DPF_BOUNDING_BOX: {
            const bool in = x > f.box[0] && x < f.box[1] && y > f.box[2] && y < f.box[3] && z > f.box[4] && z < f.box[5];
            keep = f.remove_inside ? !in : in;
            break;
        }
        case REG_DPF_REMOVE_NAN: keep = !(isnan(x) || isnan(y) || isnan(z)); break;
        case REG_DPF_MAX_QUANTILE_ON_AXIS: keep = d < f.limit; break;
        case REG_DPF_FIX_STEP_SAMPLING: keep = j >= f.phase && (j - f.phase) % f.step == 0; break;
        default: keep = true; break;
    }
    flag[j] = keep ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
k_pf_compact(const int32_t* __restrict__ idx, int m, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
             int32_t* __restrict__ idx_out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m || !flag[j]) return;
    idx_out[pos[j]] = idx[j];
}

__global__ void __launch_bounds__(256)
k_pf_gather(const float* __restrict__ px, const float* __restrict__ pn, const float* __restrict__ pc,
            const int32_t* __restrict__ idx, int m, float* __restrict__ ox, float* __restrict__ on, float* __restrict__ oc,
            int32_t* __restrict__ oidx) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const size_t i = (size_t)idx[j];
    for (int a = 0; a < 3; ++a) ox[3 * (size_t)j + a] = px[3 * i + a];
    if (on)
        for (int a = 0; a < 3; ++a) on[3 * (size_t)j + a] = pn[3 * i + a];
    if (oc)
        for (int a = 0; a < 6; ++a) oc[6 * (size_t)j + a] = pc[6 * i + a];
    if (oidx) oidx[j] = (int32_t)i;
}

// =================================================================================================
// Descriptor-carrying filters (reg_filter_cloud): the same index list + predicate + scan + compaction, with every
// descriptor field held in a workspace of n x span floats addressed by SOURCE index.  Map filters (k_fc_map) create or
// rewrite a field for the points of the current index list; predicates (k_fc_pred) read fields the same way.
// norm = sqrtf((x*x + y*y) + z*z), dot = (a0*b0 + a1*b1) + a2*b2, no contraction (include/o3dslam_reg.h).
// =================================================================================================
struct CloudFilterDev {
    int type, flag;
    float v[3];
    float last;         // MAX_DENSITY: the largest density of the current cloud
    float sat_factor;   // MAX_DENSITY: float(1 - nSat / nPoints)
};

__device__ __forceinline__ float fc_dot(const float* a, const float* b) {
    float s = a[0] * b[0];
    float t = a[1] * b[1];
    s = s + t;
    t = a[2] * b[2];
    return s + t;
}

__device__ __forceinline__ float fc_norm(const float* a) { return sqrtf(fc_dot(a, a)); }

// Eigen's normalized(): v / norm when norm > 0, else v
__device__ __forceinline__ void fc_normalized(const float* a, float* out) {
    const float nn = fc_norm(a);
    for (int c = 0; c < 3; ++c) out[c] = nn > 0.f ? a[c] / nn : a[c];
}

__device__ __forceinline__ float fc_laser_noise(float min_radius, float beam_angle, float beam_const, float r) {
    float e = beam_angle * r;
    e = e + beam_const;
    return fmaxf(min_radius, e);
}

__global__ void __launch_bounds__(256)
k_fc_map(const float* __restrict__ px, const int32_t* __restrict__ idx, int m, CloudFilterDev f, float* fa,
         const float* fb, float* fout) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const size_t i = (size_t)idx[j];
    const float p[3] = {px[3 * i], px[3 * i + 1], px[3 * i + 2]};
    switch (f.type) {
        case REG_DPF_OBSERVATION_DIRECTION:
            for (int c = 0; c < 3; ++c) fout[3 * i + c] = f.v[c] - p[c];
            break;
        case REG_DPF_ORIENT_NORMALS: {
            const float nr[3] = {fa[3 * i], fa[3 * i + 1], fa[3 * i + 2]};
            const float ob[3] = {fb[3 * i], fb[3 * i + 1], fb[3 * i + 2]};
            const float s = fc_dot(ob, nr);
            if (f.flag ? (s < 0.f) : (s > 0.f))
                for (int c = 0; c < 3; ++c) fa[3 * i + c] = -nr[c];
            break;
        }
        case REG_DPF_SIMPLE_SENSOR_NOISE: {
            const float r = fc_norm(p);
            float v;
            switch (f.flag) {
                case 0: v = fc_laser_noise(0.012f, 0.0068f, 0.0008f, r); break;
                case 1: v = fc_laser_noise(0.028f, 0.0013f, 0.0001f, r); break;
                case 2: v = fc_laser_noise(0.018f, 0.0006f, 0.0015f, r); break;
                case 3: v = (r * r) * (float)(0.5 * 0.00285); break;
                default: v = fc_laser_noise(0.004f, 0.0053f, -0.0092f, r); break;
            }
            fout[i] = v;
            break;
        }
        case REG_DPF_INCIDENCE_ANGLE: {
            const float nr[3] = {fa[3 * i], fa[3 * i + 1], fa[3 * i + 2]};
            const float ob[3] = {fb[3 * i], fb[3 * i + 1], fb[3 * i + 2]};
            float u[3];
            fc_normalized(ob, u);
            fout[i] = acosf(fc_dot(u, nr));
            break;
        }
        default: break;
    }
}

// MAX_DENSITY, pass 1: the largest density of the current cloud as an orderable key (NaN never wins: it is skipped)
__global__ void __launch_bounds__(256)
k_fc_density_max(const float* __restrict__ den, int span, const int32_t* __restrict__ idx, int m,
                 uint32_t* __restrict__ misc) {
    __shared__ uint32_t s_hi[256];
    const int j = blockIdx.x * 256 + threadIdx.x;
    uint32_t k = 0u;
    if (j < m) {
        const float d = den[(size_t)idx[j] * span];
        if (!isnan(d)) k = ssn_orderable(d);
    }
    s_hi[threadIdx.x] = k;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_hi[threadIdx.x] = max(s_hi[threadIdx.x], s_hi[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(&misc[0], s_hi[0]);
}

// MAX_DENSITY, pass 2: flag = needs a draw (density > maxDensity); misc[1] += points equal to the largest density
__global__ void __launch_bounds__(256)
k_fc_density_mask(const float* __restrict__ den, int span, const int32_t* __restrict__ idx, int m, float max_density,
                  uint32_t* __restrict__ misc, uint32_t* __restrict__ need) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    bool sat = false;
    if (j < m) {
        const float d = den[(size_t)idx[j] * span];
        need[j] = d > max_density ? 1u : 0u;
        sat = !isnan(d) && ssn_orderable(d) == misc[0];
    }
    const int c = __syncthreads_count(sat ? 1 : 0);
    if (threadIdx.x == 0 && c) atomicAdd(&misc[1], (uint32_t)c);
}

__global__ void __launch_bounds__(256)
k_fc_pred(const float* __restrict__ px, const int32_t* __restrict__ idx, int m, CloudFilterDev f,
          const float* __restrict__ fa, int span_a, const uint32_t* __restrict__ need,
          const uint32_t* __restrict__ draw_pos, const float* __restrict__ draws, uint32_t* __restrict__ flag) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const size_t i = (size_t)idx[j];
    bool keep = true;
    switch (f.type) {
        case REG_DPF_SHADOW: {
            const float p[3] = {px[3 * i], px[3 * i + 1], px[3 * i + 2]};
            const float nr[3] = {fa[3 * i], fa[3 * i + 1], fa[3 * i + 2]};
            float un[3], up[3];
            fc_normalized(nr, un);
            fc_normalized(p, up);
            keep = fabsf(fc_dot(un, up)) > f.v[0];
            break;
        }
        case REG_DPF_CUT_AT_DESCRIPTOR_THRESHOLD: {
            const float v = fa[i * span_a];
            keep = f.flag ? (v <= f.v[0]) : (v >= f.v[0]);
            break;
        }
        case REG_DPF_MAX_DENSITY: {
            if (need[j]) {
                const float d = fa[i * span_a];
                float a = f.v[0] / d;
                if (d == f.last) a = a * f.sat_factor;
                keep = draws[draw_pos[j]] < a;
            }
            break;
        }
        default: break;
    }
    flag[j] = keep ? 1u : 0u;
}

// one thread per output element of a field: out[j, c] = ws[idx[j], c]
__global__ void __launch_bounds__(256)
k_fc_gather(const float* __restrict__ ws, int span, const int32_t* __restrict__ idx, int m, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)m * span) return;
    const size_t j = t / span, c = t % span;
    out[t] = ws[(size_t)idx[j] * span + c];
}

// =================================================================================================
// VoxelGridDataPointsFilter, useCentroid 1 (reg_voxel_grid): 64-bit linear voxel ids, a stable rocPRIM radix sort of
// (id, input index), then ordered sums -- one thread per voxel and column walks the voxel's members in input order.
// =================================================================================================
struct VoxelGridDev {
    float v[3], min_bound[3];
    uint64_t nx, nxy;
};

__global__ void __launch_bounds__(256)
k_vg_keys(const float* __restrict__ px, int n, VoxelGridDev g, uint64_t* __restrict__ keys, int32_t* __restrict__ iota) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t c[3];
    for (int a = 0; a < 3; ++a) {
        float q = px[3 * (size_t)i + a] / g.v[a];
        q = q - g.min_bound[a];
        c[a] = (uint64_t)(unsigned)floorf(q);
    }
    keys[i] = c[0] + c[1] * g.nx + c[2] * g.nxy;
    iota[i] = i;
}

// is_first[i] = input point i is the first member of its voxel (sorted position r is a segment head)
__global__ void __launch_bounds__(256)
k_vg_first(const uint64_t* __restrict__ keys_s, const int32_t* __restrict__ idx, int n, uint32_t* __restrict__ is_first) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    is_first[idx[r]] = (r == 0 || keys_s[r] != keys_s[r - 1]) ? 1u : 0u;
}

// One thread per (sorted position, column); only segment heads work.  in: n x span addressed by input index (row
// stride `stride`); out row = pos[first member].  average 0 copies the first member.
__global__ void __launch_bounds__(256)
k_vg_reduce(const float* __restrict__ in, int64_t stride, int span, const uint64_t* __restrict__ keys_s,
            const int32_t* __restrict__ idx, const uint32_t* __restrict__ pos, int n, int average,
            float* __restrict__ out, int32_t* __restrict__ src_idx) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * span) return;
    const int r = (int)(t / span), c = (int)(t % span);
    const uint64_t key = keys_s[r];
    if (r > 0 && keys_s[r - 1] == key) return;
    const int32_t first = idx[r];
    float acc = in[(size_t)first * stride + c];
    if (average) {
        int count = 1;
        for (int q = r + 1; q < n && keys_s[q] == key; ++q) {
            acc = acc + in[(size_t)idx[q] * stride + c];
            ++count;
        }
        acc = acc / (float)count;
    }
    const size_t row = pos[first];
    out[row * span + c] = acc;
    if (src_idx && c == 0) src_idx[row] = first;
}
