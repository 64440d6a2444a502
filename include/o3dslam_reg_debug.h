/*
 * o3dslam_reg_debug.h -- experiment / measurement switches of the registration library.
 *
 * NOT part of the drop-in boundary (include/o3dslam_reg.h): nothing a maintainer of the reference binds to.  Used by
 * the parity tests (forcing the rare branches: band misprediction, histogram select, generic-only path), the A/B
 * scripts under tools/, bench.py's kernel timing and the lifetime tests (reg_debug_live_resources).  All zero in production.
 */
#ifndef O3DSLAM_REG_DEBUG_H
#define O3DSLAM_REG_DEBUG_H

#include "o3dslam_reg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t struct_size;        /* = sizeof(reg_debug_params); checked */
    int32_t profile_loop;       /* 1: every search kernel of reg_register carries begin/end HIP events (reg_result.prof_ms) */
    int32_t match_variant;      /* 0: 8 lanes per reading point + level hints (default); 1: one lane per point; 2: 8 lanes, no hints; 3: as 0 with the level-0 histogram fused into the match kernel */
    int32_t debug_flags;        /* ablation bits: 4, 8 change results (tests only: 8 forces band mispredictions); 32 = hash instead of the dense brick directory, 64 = histogram select for every trimmed band (results unchanged) */
    int32_t disable_halo;       /* 1: no halo-bin level */
    int32_t lanes_per_point;    /* 0 = default (8); 4 */
    int32_t disable_fused;      /* 1: every iteration on the generic (select-based) path */
    int32_t reserved;
} reg_debug_params;

/* Call right after reg_create, before reg_set_target (disable_halo and debug_flags & 32 act on the table build). */
REG_API reg_status reg_debug_configure(reg_handle* h, const reg_debug_params* d);

/* Empty-space bound of the halo directory (tests): out[i] = the lower bound on the distance from position i (n x 3 floats,
 * frame of reg_set_target's input) to any reference point that the search reads for the halo bin of that position; 0 for a
 * bin that lists points; -1 where the search does not consult the directory (outside the halo grid, no halo level). */
REG_API reg_status reg_debug_halo_bound(reg_handle* h, const float* xyz, int64_t n, float* out);

/* Witnesses of the halo directory (tests): out[i] = original index of the reference point that the directory names for the
 * halo bin of position i; -1 where the bin names none (or there is no halo level); -2 for a bin that lists points.  A
 * position outside the halo grid lies in no bin: it gets what the search takes from the border bin it clamps to (that
 * bin's witness, or the first record of its run), -1 without witnesses. */
REG_API reg_status reg_debug_halo_witness(reg_handle* h, const float* xyz, int64_t n, int32_t* out);

/* HIP resources the library holds in this process, all handles together (tests of the handles' lifetime): out[0] = device
 * buffers, out[1] = their bytes (as reserved), out[2] = pinned host blocks, out[3] = events + streams the library created.
 * Counted where a resource is created and where it is destroyed: a handle leaves all four as it found them. */
REG_API reg_status reg_debug_live_resources(int64_t out[4]);

/* The pose graph's dense solver on a caller's system (tests): A is n x n row-major, symmetric (the lower triangle is read),
   1 <= n <= 6 * REG_POSE_GRAPH_MAX_NODES; x solves A x = b through the blocked Cholesky of DESIGN.md 5z.  *status = 0, or
   1 + the row of the first pivot that is not positive and finite; then the return value is REG_BAD_TRANSFORM, x is not
   written and reg_last_error names the row.  Host arrays. */
REG_API reg_status reg_debug_spd_solve_f64(reg_handle* h, int64_t n, const double* A, const double* b, double* x,
                                           int32_t* status);

/* Measurement switches of reg_dense_map_carve_scan on the dense maps of this handle (tools/time_submaps_dense.py; results
   never change).  lanes_per_ray: 0 the shipped choice, 8 / 16 / 64 another instance of k_dm_carve_bricks, -1 the lookups of
   k_dm_carve without the coarse level.  collect_stats != 0: the kernel counts its samples.  last (may be NULL) receives what
   the last reg_dense_map_carve_scan on this handle left BEFORE this call takes effect: [0] bricks of the coarse level,
   [1] samples and [2] samples that ended at the coarse level (both 0 unless counted), [3] rays after de-duplication. */
REG_API reg_status reg_debug_dense_carve(reg_handle* h, int32_t lanes_per_ray, int32_t collect_stats, int64_t last[4]);

#ifdef __cplusplus
}
#endif
#endif /* O3DSLAM_REG_DEBUG_H */
