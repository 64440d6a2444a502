// kernels_posegraph.hpp -- pose-graph optimisation: the per-edge linearisation, the ordered assembly of the
// dense normal equations, the scalars of one Levenberg-Marquardt step, the pose step and the confidences, and the dense fp64
// solver of (H + lambda I) d = b: a blocked right-looking Cholesky (diagonal tile in LDS, panel solve, register-tiled
// trailing update) with blocked forward and back substitution.  Every sum has a fixed order and nothing is atomic: the same
// graph gives the same bytes on every run.  The per-edge and per-node formulas are those of host_math.hpp, the only copy.
// Part of the single translation unit reg_core.hip (included there, after kernels_odometry.hpp; not a standalone header).
#pragma once

constexpr int kPgNB = 48;        // panel width = edge of the diagonal tile (a multiple of 6: n = 8 nodes fill one tile)
constexpr int kPgTile = 96;      // edge of a trailing-update tile: 16 x 16 threads, 6 x 6 elements each
constexpr int kPgKC = 24;        // k rows of the A and B tiles staged in LDS at a time
constexpr int kPgTilePad = 97;   // LDS row stride of the staged tiles (odd: the transposing writes spread over the banks)
constexpr int kPgRecord = 8;     // doubles of the record read back per LM step

struct PgEdges {   // the graph's edges on the device
    const int32_t *src, *tgt, *uncertain;
    const double *X, *info;
};

// One thread per edge.  kFull: zeta, e^T L e and the record (four blocks, two vectors); otherwise zeta and e^T L e alone.
// term[e] = l e^T L e + w (sqrt(l) - 1)^2 with the confidences as they stand.
template <bool kFull>
__global__ void __launch_bounds__(64) k_pg_edge(PgEdges g, int n_edges, const double* pose, const double* conf, double w,
                                                double* zeta, double* ele, double* term, double* rec) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n_edges) return;
    double z[6];
    const double* Ts = pose + 16 * (size_t)g.src[e];
    const double* Tt = pose + 16 * (size_t)g.tgt[e];
    const double q = kFull ? pg_edge_record(Ts, Tt, g.X + 16 * (size_t)e, g.info + 36 * (size_t)e, z, rec + (size_t)kPgRec * e)
                           : pg_edge_cost(Ts, Tt, g.X + 16 * (size_t)e, g.info + 36 * (size_t)e, z);
    for (int k = 0; k < 6; ++k) zeta[6 * (size_t)e + k] = z[k];
    ele[e] = q;
    const double l = conf[e], s = sqrt(l) - 1.0;
    term[e] = l * q + w * (s * s);
}

// confidence = (w / (w + e^T L e))^2 on the uncertain edges; the others keep theirs
__global__ void k_pg_conf(PgEdges g, int n_edges, const double* ele, double w, double* conf) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges || !g.uncertain[e]) return;
    const double r = w / (w + ele[e]);
    conf[e] = r * r;
}

// H (M x M, M = 6 n) and b: one thread per element sums its list in edge order.  blk_ptr (n * n + 1) / blk_item: per 6 x 6
// block the items edge * 4 + {0: ss, 1: st, 2: ts, 3: tt}; node_ptr (n + 1) / node_item: per node edge * 2 + {0: s, 1: t}.
// A block without items is written as zero.  Threads M * M .. M * M + M - 1 write b.
__global__ void k_pg_assemble(int n_nodes, const int32_t* blk_ptr, const int32_t* blk_item, const int32_t* node_ptr,
                              const int32_t* node_item, const double* rec, const double* conf, double* H, double* b) {
    const int64_t M = 6 * (int64_t)n_nodes;
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx < M * M) {
        const int r = (int)(idx / M), c = (int)(idx % M);
        const int64_t blk = (int64_t)(r / 6) * n_nodes + c / 6;
        const int at = (r % 6) * 6 + c % 6;
        double s = 0.0;
        for (int k = blk_ptr[blk]; k < blk_ptr[blk + 1]; ++k) {
            const int it = blk_item[k], e = it >> 2;
            s = s + conf[e] * rec[(size_t)kPgRec * e + 36 * (it & 3) + at];
        }
        H[idx] = s;
    } else if (idx < M * M + M) {
        const int r = (int)(idx - M * M), node = r / 6;
        double s = 0.0;
        for (int k = node_ptr[node]; k < node_ptr[node + 1]; ++k) {
            const int it = node_item[k], e = it >> 1;
            s = s - conf[e] * rec[(size_t)kPgRec * e + 144 + 6 * (it & 1) + r % 6];
        }
        b[r] = s;
    }
}

// One workgroup of 256.  out[0] = sum of term in edge order; [1] = max diag H; [2] = max b (signed); [3] = |d|; [4] = |x|;
// [5] = d . (lambda d + b); [6] = the solver's pivot word (0: fine, else 1 + the row of the bad pivot); [7] = 0.
// Sums other than [0]: thread t adds the elements t, t + 256, ... in order, then a fixed tree over the 256 partials.
__device__ inline double pg_tree(double v, double* red, bool is_max) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = is_max ? fmax(red[t], red[t + s]) : red[t] + red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__global__ void __launch_bounds__(256) k_pg_scalars(int n_edges, int M, const double* term, const double* H, const double* b,
                                                    const double* d, const double* x, double lambda, const int32_t* pivot,
                                                    double* out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double res = 0.0;
    for (int base = 0; base < n_edges; base += 256) {   // staged through LDS, summed by one thread: edge order
        if (base + t < n_edges) red[t] = term[base + t];
        __syncthreads();
        if (t == 0)
            for (int k = 0; k < 256 && base + k < n_edges; ++k) res = res + red[k];
        __syncthreads();
    }
    double md = -INFINITY, mb = -INFINITY, nd = 0.0, nx = 0.0, dot = 0.0;
    for (int i = t; i < M; i += 256) {
        md = fmax(md, H[(size_t)i * M + i]);
        mb = fmax(mb, b[i]);
        const double di = d[i];
        nd = nd + di * di;
        nx = nx + x[i] * x[i];
        dot = dot + di * (lambda * di + b[i]);
    }
    md = pg_tree(md, red, true);
    mb = pg_tree(mb, red, true);
    nd = pg_tree(nd, red, false);
    nx = pg_tree(nx, red, false);
    dot = pg_tree(dot, red, false);
    if (t == 0) {
        out[0] = res;
        out[1] = md;
        out[2] = mb;
        out[3] = sqrt(nd);
        out[4] = sqrt(nx);
        out[5] = dot;
        out[6] = (double)pivot[0];
        out[7] = 0.0;
    }
}

// One thread per node: out_i = V(d_i) pose_i (d == null: none) and / or x_i = the pose vector of pose_i
__global__ void k_pg_nodes(int n_nodes, const double* pose, const double* d, double* out, double* x) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    if (d) pg_pose_step(d + 6 * (size_t)i, pose + 16 * (size_t)i, out + 16 * (size_t)i);
    if (x) pg_pose_vector(pose + 16 * (size_t)i, x + 6 * (size_t)i);
}

// ---- the solver.  L is Mp x Mp row-major, Mp = M rounded up to a multiple of kPgTile: the padding is the identity, so every
// tile of every kernel is whole and the first M entries of the solution are those of the M x M system. ----

// L = A + lambda I inside M x M, identity outside; rhs = b padded with zeros; the pivot word cleared
__global__ void k_pg_load(const double* A, int M, int Mp, double lambda, const double* b, double* L, double* rhs, int32_t* pivot) {
    const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (idx >= (int64_t)Mp * Mp) return;
    const int r = (int)(idx / Mp), c = (int)(idx % Mp);
    double v = (r == c) ? 1.0 : 0.0;
    if (r < M && c < M) {
        v = A[(size_t)r * M + c];
        if (r == c) v = v + lambda;
    }
    L[idx] = v;
    if (c == 0) rhs[r] = r < M ? b[r] : 0.0;
    if (idx == 0) pivot[0] = 0;
}

// The diagonal tile of panel p, factorised in LDS by one workgroup of 256 (lower triangle, right-looking: every element
// takes its updates in column order).  A pivot that is not positive and finite is reported once (the first) and the
// factorisation goes on over NaN: the host reads the word with the step's record.
__global__ void __launch_bounds__(256) k_pg_potrf(double* L, int Mp, int p, int32_t* pivot) {
    __shared__ double a[kPgNB][kPgNB + 1];
    const int t = threadIdx.x, o = p * kPgNB;
    for (int i = t; i < kPgNB * kPgNB; i += 256) a[i / kPgNB][i % kPgNB] = L[(size_t)(o + i / kPgNB) * Mp + o + i % kPgNB];
    __syncthreads();
    for (int j = 0; j < kPgNB; ++j) {
        const double djj = a[j][j];
        __syncthreads();
        if (t == 0) {
            if (!(djj > 0.0) || !(djj < INFINITY)) {
                if (pivot[0] == 0) pivot[0] = o + j + 1;
            }
            a[j][j] = sqrt(djj);
        }
        const double s = sqrt(djj);
        if (t > j && t < kPgNB) a[t][j] = a[t][j] / s;
        __syncthreads();
        // rows i > j, columns j < k <= i
        for (int q = t; q < kPgNB * kPgNB; q += 256) {
            const int i = q / kPgNB, k = q % kPgNB;
            if (i > j && k > j && k <= i) a[i][k] = a[i][k] - a[i][j] * a[k][j];
        }
        __syncthreads();
    }
    for (int i = t; i < kPgNB * kPgNB; i += 256)
        if (i % kPgNB <= i / kPgNB) L[(size_t)(o + i / kPgNB) * Mp + o + i % kPgNB] = a[i / kPgNB][i % kPgNB];
}

// The panel below the diagonal tile: rows X of L21 solve X L11^T = A21, kPgTile rows per workgroup of 256, staged in LDS,
// one thread per row: x_c = (a_c - x_0 l_c0 - ... - x_{c-1} l_{c,c-1}) / l_cc in that order.  Grid: (Mp - o - kPgNB) / kPgNB
// is not a multiple of two tiles in general, so rows at and beyond Mp are skipped.
__global__ void __launch_bounds__(256) k_pg_trsm(double* L, int Mp, int p) {
    __shared__ double l11[kPgNB][kPgNB + 1];
    __shared__ double rows[kPgTile][kPgNB + 1];
    const int t = threadIdx.x, o = p * kPgNB;
    const int r0 = o + kPgNB + blockIdx.x * kPgTile;
    for (int i = t; i < kPgNB * kPgNB; i += 256) l11[i / kPgNB][i % kPgNB] = L[(size_t)(o + i / kPgNB) * Mp + o + i % kPgNB];
    for (int i = t; i < kPgTile * kPgNB; i += 256) {
        const int r = r0 + i / kPgNB;
        if (r < Mp) rows[i / kPgNB][i % kPgNB] = L[(size_t)r * Mp + o + i % kPgNB];
    }
    __syncthreads();
    if (t < kPgTile && r0 + t < Mp) {
        for (int c = 0; c < kPgNB; ++c) {
            double v = rows[t][c];
            for (int k = 0; k < c; ++k) v = v - rows[t][k] * l11[c][k];
            rows[t][c] = v / l11[c][c];
        }
    }
    __syncthreads();
    for (int i = t; i < kPgTile * kPgNB; i += 256) {
        const int r = r0 + i / kPgNB;
        if (r < Mp) L[(size_t)r * Mp + o + i % kPgNB] = rows[i / kPgNB][i % kPgNB];
    }
}

// The trailing update C -= A B^T after panel p: A = L[rows of the tile, panel columns], B = L[columns of the tile, panel
// columns], C the kPgTile x kPgTile tile (ti, tj), tj <= ti, of the lower triangle.  256 threads as 16 x 16, a 6 x 6 register
// tile each (rows ty + 16 r, columns tx + 16 c), explicit fma in k order; A and B go through LDS kPgKC panel columns at a
// time, k-major, so that a wave reads 4 row values (broadcast over tx) and 16 consecutive column values per k.  Elements
// whose row or column lies above the trailing region (the tile that holds the panel's own rows when the region starts in
// mid-tile) are computed and not stored.  blockIdx.x enumerates the lower-triangle tiles of the region.
__global__ void __launch_bounds__(256) k_pg_trailing(double* L, int Mp, int p, int tile0) {
    __shared__ double As[kPgKC][kPgTilePad];
    __shared__ double Bs[kPgKC][kPgTilePad];
    // blockIdx.x -> (i, j), j <= i, row-major over the triangle: i = floor((sqrt(8 b + 1) - 1) / 2), fixed up in integers
    const int bid = blockIdx.x;
    int i = (int)((sqrtf(8.f * (float)bid + 1.f) - 1.f) * 0.5f);
    while ((i + 1) * (i + 2) / 2 <= bid) ++i;
    while (i * (i + 1) / 2 > bid) --i;
    const int j = bid - i * (i + 1) / 2;
    const int row0 = (tile0 + i) * kPgTile, col0 = (tile0 + j) * kPgTile;
    const int o = p * kPgNB, start = o + kPgNB;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double c[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int q = 0; q < 6; ++q) c[r][q] = L[(size_t)(row0 + ty + 16 * r) * Mp + col0 + tx + 16 * q];
    for (int k0 = 0; k0 < kPgNB; k0 += kPgKC) {
        __syncthreads();
        for (int q = t; q < kPgTile * kPgKC; q += 256) {
            const int r = q / kPgKC, k = q % kPgKC;
            As[k][r] = L[(size_t)(row0 + r) * Mp + o + k0 + k];
            Bs[k][r] = L[(size_t)(col0 + r) * Mp + o + k0 + k];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kPgKC; ++k) {
            double a[6], b[6];
#pragma unroll
            for (int r = 0; r < 6; ++r) a[r] = -As[k][ty + 16 * r];
#pragma unroll
            for (int q = 0; q < 6; ++q) b[q] = Bs[k][tx + 16 * q];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int q = 0; q < 6; ++q) c[r][q] = fma(a[r], b[q], c[r][q]);
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int gr = row0 + ty + 16 * r, gc = col0 + tx + 16 * q;
            if (gr >= start && gc >= start) L[(size_t)gr * Mp + gc] = c[r][q];
        }
}

// Forward substitution L y = b, block p: every workgroup solves the kPgNB x kPgNB triangle of block p from the working
// vector w (column order: y_j = w_j / l_jj, then w_i -= l_ij y_j for i > j), workgroup 0 writes y, and the workgroups
// together take the block's columns out of w below it: 64 rows per workgroup, 4 threads per row over 12 columns each,
// combined as ((q0 + q1) + q2) + q3.
__device__ inline void pg_tile_solve(double (*a)[kPgNB + 1], double* v, bool transposed) {
    const int t = threadIdx.x;
    for (int s = 0; s < kPgNB; ++s) {
        const int j = transposed ? kPgNB - 1 - s : s;
        if (t == 0) v[j] = v[j] / a[j][j];
        __syncthreads();
        if (t < kPgNB && (transposed ? t < j : t > j)) v[t] = v[t] - (transposed ? a[j][t] : a[t][j]) * v[j];
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) k_pg_forward(const double* L, int Mp, int p, double* w, double* y) {
    __shared__ double a[kPgNB][kPgNB + 1];
    __shared__ double v[kPgNB];
    __shared__ double part[256];
    const int t = threadIdx.x, o = p * kPgNB;
    for (int i = t; i < kPgNB * kPgNB; i += 256) a[i / kPgNB][i % kPgNB] = L[(size_t)(o + i / kPgNB) * Mp + o + i % kPgNB];
    if (t < kPgNB) v[t] = w[o + t];
    __syncthreads();
    pg_tile_solve(a, v, false);
    if (blockIdx.x == 0 && t < kPgNB) y[o + t] = v[t];
    const int r = o + kPgNB + blockIdx.x * 64 + (t >> 2), q = t & 3;
    double s = 0.0;
    if (r < Mp)
        for (int k = 12 * q; k < 12 * q + 12; ++k) s = s + L[(size_t)r * Mp + o + k] * v[k];
    part[t] = s;
    __syncthreads();
    if (q == 0 && r < Mp) w[r] = w[r] - (((part[t] + part[t + 1]) + part[t + 2]) + part[t + 3]);
}

// Back substitution L^T x = y, block p (from the last block down): every workgroup solves the transposed triangle of block
// p from the working vector y, workgroup 0 writes x, and the workgroups take the block out of y above it: one thread per
// column c < o, y_c -= l_{o,c} x_0 + ... in row order.
__global__ void __launch_bounds__(256) k_pg_backward(const double* L, int Mp, int p, double* y, double* x) {
    __shared__ double a[kPgNB][kPgNB + 1];
    __shared__ double v[kPgNB];
    const int t = threadIdx.x, o = p * kPgNB;
    for (int i = t; i < kPgNB * kPgNB; i += 256) a[i / kPgNB][i % kPgNB] = L[(size_t)(o + i / kPgNB) * Mp + o + i % kPgNB];
    if (t < kPgNB) v[t] = y[o + t];
    __syncthreads();
    pg_tile_solve(a, v, true);
    if (blockIdx.x == 0 && t < kPgNB) x[o + t] = v[t];
    const int c = blockIdx.x * 256 + t;
    if (c < o) {
        double s = 0.0;
        for (int k = 0; k < kPgNB; ++k) s = s + L[(size_t)(o + k) * Mp + c] * v[k];
        y[c] = y[c] - s;
    }
}
