// kernels_octree.hpp -- OctreeGridDataPointsFilter (reg_octree_grid, include/o3dslam_reg.h)
// Part of the single translation unit reg_core.hip (included there, after kernels_filters.hpp; not a standalone header).
#pragma once

// =================================================================================================
// The octree splits at power-of-two box centres, so a point's whole path down the tree depends on the point alone:
// k_oct_keys walks the fp32 centre chain and packs 3 bits per level into a 64-bit key (21 levels per round).  One
// rocPRIM radix sort (key, index) puts every node's points next to each other in depth-first order; k_oct_depth finds a
// point's leaf depth as the first level whose node (a run of equal key prefixes) meets a stop rule, by a binary search
// over the levels and, per level, over at most max_point_by_node + 1 positions either side.  k_oct_heads + an inclusive
// scan give every node a dense depth-first rank.  Nodes still open after 21 levels (dense duplicates) take another round
// of keys relative to their level-21 centre; the round sorts by (rank, key) with two stable radix sorts.  Finally a
// stable sort of (leaf id, input index) restores the member order and k_oct_sample emits one row per leaf.
// =================================================================================================
constexpr int kOctLevelsPerRound = 21;
constexpr uint32_t kOctOpen = 0x100u;   // k_oct_depth: the node is still open after this round's 21 levels

// Per point: the key of this round's (up to 21) levels below depth d0, and the centre reached after them.  Points whose
// node is already a leaf (open[i] == 0, rounds after the first) get key 0.
__global__ void __launch_bounds__(256)
k_oct_keys(const float* __restrict__ px, int n, const float* __restrict__ root_c, const float* __restrict__ radii,
           int levels, const uint32_t* __restrict__ open, float* __restrict__ pc, uint64_t* __restrict__ keys,
           int32_t* __restrict__ iota) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    iota[i] = i;
    if (open && !open[i]) {
        keys[i] = 0ull;
        return;
    }
    const float x = px[3 * (size_t)i], y = px[3 * (size_t)i + 1], z = px[3 * (size_t)i + 2];
    float c0, c1, c2;
    if (open) {
        c0 = pc[3 * (size_t)i];
        c1 = pc[3 * (size_t)i + 1];
        c2 = pc[3 * (size_t)i + 2];
    } else {
        c0 = root_c[0];
        c1 = root_c[1];
        c2 = root_c[2];
    }
    uint64_t key = 0ull;
    for (int k = 0; k < levels; ++k) {
        const float r = radii[k];
        const uint32_t b = (uint32_t)(x > c0) | ((uint32_t)(y > c1) << 1) | ((uint32_t)(z > c2) << 2);
        key |= (uint64_t)b << (60 - 3 * k);
        // Octree.tpp: centre + offsetTable[b] * radius, offsets +-0.5f
        const float o0 = (b & 1u) ? 0.5f : -0.5f, o1 = (b & 2u) ? 0.5f : -0.5f, o2 = (b & 4u) ? 0.5f : -0.5f;
        const float t0 = o0 * r, t1 = o1 * r, t2 = o2 * r;
        c0 = c0 + t0;
        c1 = c1 + t1;
        c2 = c2 + t2;
    }
    pc[3 * (size_t)i] = c0;
    pc[3 * (size_t)i + 1] = c1;
    pc[3 * (size_t)i + 2] = c2;
    keys[i] = key;
}

// sorted positions a and b lie in the same node k levels below this round's start (same rank, same k key groups)
__device__ __forceinline__ bool oct_same(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, int a,
                                         int b, int k) {
    if (rank && rank[a] != rank[b]) return false;
    return k == 0 || ((keys[a] ^ keys[b]) >> (63 - 3 * k)) == 0ull;
}

// size of the node of sorted position i, k levels down, clipped to max_pts + 1 (enough for the count rule)
__device__ __forceinline__ int64_t oct_count(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, int n,
                                             int i, int k, int64_t max_pts) {
    int64_t a = max((int64_t)0, (int64_t)i - max_pts), b = i;   // first position of the run
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (oct_same(keys, rank, (int)mid, i, k)) b = mid;
        else a = mid + 1;
    }
    const int64_t s = a;
    a = i;
    b = min((int64_t)n - 1, (int64_t)i + max_pts);   // last position of the run
    while (a < b) {
        const int64_t mid = (a + b + 1) >> 1;
        if (oct_same(keys, rank, (int)mid, i, k)) a = mid;
        else b = mid - 1;
    }
    return a - s + 1;
}

// Per sorted position: the number of key groups (1..21) that name the point's leaf, | kOctOpen when its node is still
// open after 21 levels, 0 for a point whose leaf an earlier round settled.  Leaf depth per input point.
__global__ void __launch_bounds__(256)
k_oct_depth(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, const int32_t* __restrict__ idx,
            const uint32_t* __restrict__ open, int n, int64_t max_pts, int d0, int d_size, uint32_t* __restrict__ kk,
            int32_t* __restrict__ depth, uint32_t* __restrict__ any_open) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = idx[i];
    if (open && !open[p]) {
        kk[i] = 0u;
        return;
    }
    int a = 1, b = kOctLevelsPerRound + 1;   // smallest k with a stop rule met, kOctLevelsPerRound + 1: none
    while (a < b) {
        const int mid = (a + b) >> 1;
        const bool leaf = d0 + mid >= d_size || oct_count(keys, rank, n, i, mid, max_pts) <= max_pts;
        if (leaf) b = mid;
        else a = mid + 1;
    }
    if (a > kOctLevelsPerRound) {
        kk[i] = (uint32_t)kOctLevelsPerRound | kOctOpen;
        any_open[0] = 1u;
    } else {
        kk[i] = (uint32_t)a;
        depth[p] = d0 + a;
    }
}

__global__ void __launch_bounds__(256)
k_oct_heads(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ kk, int n,
            uint32_t* __restrict__ heads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool h = i == 0;
    if (!h) h = kk[i] != kk[i - 1] || !oct_same(keys, rank, i, i - 1, (int)(kk[i] & 0xffu));
    heads[i] = h ? 1u : 0u;
}

// new dense depth-first rank (inclusive scan of the heads - 1) and open flag, back to input-point order
__global__ void __launch_bounds__(256)
k_oct_scatter(const int32_t* __restrict__ idx, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ kk, int n,
              uint32_t* __restrict__ rank, uint32_t* __restrict__ open) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = idx[i];
    rank[p] = pos[i] - 1u;
    open[p] = (kk[i] & kOctOpen) ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
k_oct_gather_rank(const int32_t* __restrict__ idx, const uint32_t* __restrict__ rank, int n, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = rank[idx[i]];
}

__global__ void __launch_bounds__(256)
k_oct_gather_keys(const int32_t* __restrict__ idx, const uint64_t* __restrict__ keys, int n, uint64_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = keys[idx[i]];
}

// single-leaf tree (root is a leaf): rank 0, depth 0
__global__ void __launch_bounds__(256)
k_oct_root_leaf(int n, uint32_t* __restrict__ rank, int32_t* __restrict__ depth, int32_t* __restrict__ iota) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rank[i] = 0u;
    depth[i] = 0;
    iota[i] = i;
}

// leaf starts over the members sorted by (leaf id, input index); start[n_leaves] = n
__global__ void __launch_bounds__(256)
k_oct_starts(const uint32_t* __restrict__ leaf_sorted, int n, int n_leaves, int32_t* __restrict__ start) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || leaf_sorted[i] != leaf_sorted[i - 1]) start[leaf_sorted[i]] = i;
    if (i == n - 1) start[n_leaves] = n;
}

// One thread per non-empty leaf: row L of the output (OctreeSamplers.tpp under the contract of reg_octree_grid).
__global__ void __launch_bounds__(256)
k_oct_sample(const float* __restrict__ px, const float* __restrict__ nrm, const float* __restrict__ cov,
             const int32_t* __restrict__ members, const int32_t* __restrict__ start, int n_leaves, int method,
             const int32_t* __restrict__ rands, float* __restrict__ out_xyz, float* __restrict__ out_nrm,
             float* __restrict__ out_cov, int32_t* __restrict__ src_idx) {
    const int L = blockIdx.x * 256 + threadIdx.x;
    if (L >= n_leaves) return;
    const int b = start[L], e = start[L + 1];
    const int cnt = e - b;
    int s = members[b];
    if (method == REG_OCTREE_RAND) {
        const float ratio = (float)rands[L] / (float)2147483647;   // float(rand()) / float(RAND_MAX)
        const float f = (float)(cnt - 1) * ratio;
        const int pick = min((int)f, cnt - 1);
        s = members[b + pick];
    } else if (method == REG_OCTREE_CENTROID) {
        const float fc = (float)cnt;
        float acc[6];
        for (int a = 0; a < 3; ++a) acc[a] = px[3 * (size_t)s + a];
        for (int r = b + 1; r < e; ++r) {
            const size_t q = (size_t)members[r];
            for (int a = 0; a < 3; ++a) acc[a] = acc[a] + px[3 * q + a];
        }
        for (int a = 0; a < 3; ++a) out_xyz[3 * (size_t)L + a] = acc[a] / fc;
        if (out_nrm) {
            for (int a = 0; a < 3; ++a) acc[a] = nrm[3 * (size_t)s + a];
            for (int r = b + 1; r < e; ++r) {
                const size_t q = (size_t)members[r];
                for (int a = 0; a < 3; ++a) acc[a] = acc[a] + nrm[3 * q + a];
            }
            for (int a = 0; a < 3; ++a) out_nrm[3 * (size_t)L + a] = acc[a] / fc;
        }
        if (out_cov) {
            for (int a = 0; a < 6; ++a) acc[a] = cov[6 * (size_t)s + a];
            for (int r = b + 1; r < e; ++r) {
                const size_t q = (size_t)members[r];
                for (int a = 0; a < 6; ++a) acc[a] = acc[a] + cov[6 * q + a];
            }
            for (int a = 0; a < 6; ++a) out_cov[6 * (size_t)L + a] = acc[a] / fc;
        }
        src_idx[L] = s;
        return;
    } else if (method == REG_OCTREE_MEDOID) {
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
        for (int r = b; r < e; ++r) {
            const size_t q = (size_t)members[r];
            m0 = m0 + px[3 * q];
            m1 = m1 + px[3 * q + 1];
            m2 = m2 + px[3 * q + 2];
        }
        const float fc = (float)cnt;
        m0 = m0 / fc;
        m1 = m1 / fc;
        m2 = m2 / fc;
        float best = 3.40282347e+38f;   // std::numeric_limits<float>::max()
        for (int r = b; r < e; ++r) {
            const int q = members[r];
            const float d0 = px[3 * (size_t)q] - m0, d1 = px[3 * (size_t)q + 1] - m1, d2 = px[3 * (size_t)q + 2] - m2;
            const float s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2;
            const float t = s1 + s2;
            const float dist = sqrtf(s0 + t);   // Eigen's norm() of a 3-vector: x0^2 + (x1^2 + x2^2)
            if (dist < best) {
                best = dist;
                s = q;
            }
        }
    }
    for (int a = 0; a < 3; ++a) out_xyz[3 * (size_t)L + a] = px[3 * (size_t)s + a];
    if (out_nrm)
        for (int a = 0; a < 3; ++a) out_nrm[3 * (size_t)L + a] = nrm[3 * (size_t)s + a];
    if (out_cov)
        for (int a = 0; a < 6; ++a) out_cov[6 * (size_t)L + a] = cov[6 * (size_t)s + a];
    src_idx[L] = s;
}
