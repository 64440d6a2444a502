// group_dpp.hpp -- reductions, prefixes and broadcasts over a lane group of G <= 8 adjacent lanes without LDS.
//
// A group lies inside one DPP row (16 lanes) -- G = 8 inside a half row, G = 4 inside a quad -- so its exchanges are
// data-parallel-primitive moves (__builtin_amdgcn_update_dpp: one VALU instruction, no LDS round trip) instead of
// __shfl* (ds_bpermute_b32: ~50 cycles of dependent LDS latency plus the address arithmetic).  Results are the same
// values lane for lane.  Every lane of a group takes the same control flow, so the source lanes of a group operation are
// always that group's own active lanes; a read that can reach into a neighbouring (possibly inactive) group is given the
// operation's identity as `old` and is discarded by the caller's guard.
// O3D_GROUP_DPP=0: the shuffle forms (whole-build A/B).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef O3D_GROUP_DPP
#define O3D_GROUP_DPP 1
#endif

namespace o3dreg {

constexpr int kDppXor1 = 0xB1;         // quad_perm:[1,0,3,2]
constexpr int kDppXor2 = 0x4E;         // quad_perm:[2,3,0,1]
constexpr int kDppQuadLast = 0xFF;     // quad_perm:[3,3,3,3]
constexpr int kDppPairLast = 0xF5;     // quad_perm:[1,1,3,3]
constexpr int kDppHalfMirror = 0x141;  // row_half_mirror: lane i of a half row reads lane 7 - i
constexpr int kDppRowShr = 0x110;      // row_shr:n = 0x110 + n: lane i of a row reads lane i - n (none: keeps `old`)
constexpr int kDppRowRor = 0x120;      // row_ror:n = 0x120 + n: rotation inside the row

template <int CTRL>
__device__ __forceinline__ int dpp_mov(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false);
}

// Value of the partner lane at step M (1, 2, 4) of a group butterfly.  M = 4 is the half-row mirror, not lane ^ 4: it pairs
// every lane with one of the OTHER quad, which is all a reduction needs once steps 1 and 2 have made the quads uniform --
// so the steps must run in the order 1, 2, 4 and the combination must be symmetric (both partners end with the same value).
template <int M>
__device__ __forceinline__ int group_partner(int v) {
    static_assert(M == 1 || M == 2 || M == 4, "groups of at most 8 lanes");
#if O3D_GROUP_DPP
    if constexpr (M == 1) return dpp_mov<kDppXor1>(v, v);
    if constexpr (M == 2) return dpp_mov<kDppXor2>(v, v);
    return dpp_mov<kDppHalfMirror>(v, v);
#else
    return __shfl_xor(v, M);
#endif
}
template <int M>
__device__ __forceinline__ float group_partner(float v) {
    return __int_as_float(group_partner<M>(__float_as_int(v)));
}
template <int M>
__device__ __forceinline__ uint32_t group_partner(uint32_t v) {
    return (uint32_t)group_partner<M>((int)v);
}

// all-reduce minimum over the group
template <int G>
__device__ __forceinline__ float group_min_f32(float v) {
    if constexpr (G >= 2) v = fminf(v, group_partner<1>(v));
    if constexpr (G >= 4) v = fminf(v, group_partner<2>(v));
    if constexpr (G >= 8) v = fminf(v, group_partner<4>(v));
    return v;
}
template <int G>
__device__ __forceinline__ uint32_t group_min_u32(uint32_t v) {
    if constexpr (G >= 2) v = min(v, group_partner<1>(v));
    if constexpr (G >= 4) v = min(v, group_partner<2>(v));
    if constexpr (G >= 8) v = min(v, group_partner<4>(v));
    return v;
}

// lexicographic minimum of (d2, idx) with its payload pos: ties of both keys are the same reference point
template <int M>
__device__ __forceinline__ void group_min3_step(float& d2, uint32_t& idx, int& pos) {
    const float od2 = group_partner<M>(d2);
    const uint32_t oidx = group_partner<M>(idx);
    const int opos = group_partner<M>(pos);
    if (od2 < d2 || (od2 == d2 && oidx < idx)) {
        d2 = od2;
        idx = oidx;
        pos = opos;
    }
}
template <int G>
__device__ __forceinline__ void group_min3(float& d2, uint32_t& idx, int& pos) {
    if constexpr (G >= 2) group_min3_step<1>(d2, idx, pos);
    if constexpr (G >= 4) group_min3_step<2>(d2, idx, pos);
    if constexpr (G >= 8) group_min3_step<4>(d2, idx, pos);
}

// inclusive prefix sum over the group (sub = lane index inside the group)
template <int G>
__device__ __forceinline__ uint32_t group_scan_incl(uint32_t v, int sub) {
#if O3D_GROUP_DPP
    if constexpr (G >= 2) {
        const uint32_t o = (uint32_t)dpp_mov<kDppRowShr + 1>(0, (int)v);
        if (sub >= 1) v += o;
    }
    if constexpr (G >= 4) {
        const uint32_t o = (uint32_t)dpp_mov<kDppRowShr + 2>(0, (int)v);
        if (sub >= 2) v += o;
    }
    if constexpr (G >= 8) {
        const uint32_t o = (uint32_t)dpp_mov<kDppRowShr + 4>(0, (int)v);
        if (sub >= 4) v += o;
    }
#else
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, o);
        if (sub >= o) v += t;
    }
#endif
    return v;
}

// value of the group's last lane, in every lane (gbase = first lane of the group in the wave)
template <int G>
__device__ __forceinline__ uint32_t group_bcast_last(uint32_t v, int sub, int gbase) {
#if O3D_GROUP_DPP
    if constexpr (G == 2) return (uint32_t)dpp_mov<kDppPairLast>((int)v, (int)v);
    const int q = dpp_mov<kDppQuadLast>((int)v, (int)v);   // every lane: last lane of its quad
    if constexpr (G == 4) return (uint32_t)q;
    const int m = dpp_mov<kDppHalfMirror>(q, q);           // lower quad: the upper quad's value
    return (uint32_t)(sub < 4 ? m : q);
#else
    return (uint32_t)__shfl((int)v, gbase + G - 1);
#endif
}

// partner at lane ^ BIT of a 64-bit value, BIT = 1, 2 or 8 (inside a row); other distances keep the shuffle
template <int BIT>
__device__ __forceinline__ double wave_xor_f64(double v) {
#if O3D_GROUP_DPP
    if constexpr (BIT == 1 || BIT == 2 || BIT == 8) {
        constexpr int ctrl = BIT == 1 ? kDppXor1 : (BIT == 2 ? kDppXor2 : kDppRowRor + 8);
        const int lo = __double2loint(v), hi = __double2hiint(v);
        return __hiloint2double(dpp_mov<ctrl>(hi, hi), dpp_mov<ctrl>(lo, lo));
    } else {
        return __shfl_xor(v, BIT);
    }
#else
    return __shfl_xor(v, BIT);
#endif
}

// LDS written by some lanes of a wave becomes visible to its other lanes: the lane groups of the k-NN kernels (and whole
// waves that work alone) exchange through LDS without a workgroup barrier.
__device__ __forceinline__ void group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// Sum over a workgroup of 256 threads (4 waves) of NV doubles per lane: thread c < NV returns the total of component c,
// the waves added in the fixed order (0 + 1) + (2 + 3); the other threads return 0.  v[] is left with the wave's sums.
// A second call with the same NV in one kernel needs a __syncthreads() in between (the LDS rows are reused).
template <int NV>
__device__ __forceinline__ double block_sum(double* v) {
    __shared__ double red[4][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x >= NV) return 0.0;
    return (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// ... stored to dst[NV] (global or LDS; a reader in the same workgroup needs a barrier first)
template <int NV>
__device__ __forceinline__ void block_sum_store(double* v, double* dst) {
    const double t = block_sum<NV>(v);
    if (threadIdx.x < NV) dst[threadIdx.x] = t;
}

}  // namespace o3dreg
