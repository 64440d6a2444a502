// host_math.hpp -- host-side (CPU) pieces of the registration path: 4x4 fp32 algebra, the
// 6x6 solve, x -> SE(3), the transformation checkers.  Product code (not the oracle).
//
// Reference behaviour restated (paths relative to the reference tree):
//   solve      libpointmatcher/pointmatcher/ErrorMinimizers/PointToPlane.cpp:112-265
//   x -> T     PointToPlane.cpp:327-381   (angle = atan(|w|), axis = w/|w|, t = x[3..5])
//   checkers   TransformationCheckersImpl.cpp:57-158
//   frames     ICP.cpp:883-890, 966-984, 1345
// All 4x4 matrices in this file are ROW-major float[16]; the C ABI converts from/to column-major.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define O3D_HD __host__ __device__
#else
#define O3D_HD
#endif

// NOTE: this header relies on being compiled with -ffp-contract=off (one rounding per fp32 operation).
namespace o3dreg {

O3D_HD inline void m4_identity(float* T) {
    memset(T, 0, 16 * sizeof(float));
    T[0] = T[5] = T[10] = T[15] = 1.f;
}

// C = A*B with one rounding per operation, k = 0..3 in order (numeric contract NC3).
O3D_HD inline void m4_mul(const float* A, const float* B, float* C) {
    float R[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = A[4 * i] * B[j];
            float t = A[4 * i + 1] * B[4 + j];
            s = s + t;
            t = A[4 * i + 2] * B[8 + j];
            s = s + t;
            t = A[4 * i + 3] * B[12 + j];
            s = s + t;
            R[4 * i + j] = s;
        }
    memcpy(C, R, sizeof(R));
}

// The float behind an orderable key (k_ssn_pack: the key order is the float order; minima / maxima are taken on keys)
O3D_HD inline float float_from_orderable(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    memcpy(&v, &u, 4);
    return v;
}

O3D_HD inline void m4_transpose(const float* A, float* B) {
    float R[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) R[4 * i + j] = A[4 * j + i];
    memcpy(B, R, sizeof(R));
}

// R3: RigidTransformation::checkParameters / correctParameters (TransformationsImpl.cpp:105-166), row-major 4x4.
// |1 - det(R)| > 1e-3 in fp32 -> Tc = the re-orthogonalised copy the reference applies to the FEATURES (col1, col2
// normalised; newCol0 = col1 x col2; newCol1 = col2 x newCol0; newCol2 = col2; translation kept).  Descriptors keep
// the matrix as given (TransformationsImpl.cpp:83-101).  One rounding per operation; returns true when corrected.
O3D_HD inline bool rigid_correct(const float* T, float* Tc) {
    for (int i = 0; i < 16; ++i) Tc[i] = T[i];
    float m0 = T[5] * T[10], m1 = T[6] * T[9];
    const float c0 = m0 - m1;
    m0 = T[4] * T[10]; m1 = T[6] * T[8];
    const float c1 = m0 - m1;
    m0 = T[4] * T[9]; m1 = T[5] * T[8];
    const float c2 = m0 - m1;
    float a = T[0] * c0, b = T[1] * c1;
    float det = a - b;
    a = T[2] * c2;
    det = det + a;
    const float dev = 1.0f - det;
    if (!(fabsf(dev) > 0.001f)) return false;
    float n1[3] = {T[1], T[5], T[9]}, n2[3] = {T[2], T[6], T[10]}, n0[3], mv[3];
    for (int k = 0; k < 2; ++k) {   // Eigen 3.3 normalized(): z > 0 ? v / sqrt(z) : v
        float* v = k == 0 ? n1 : n2;
        float p = v[0] * v[0], q = v[1] * v[1];
        float z = p + q;
        p = v[2] * v[2];
        z = z + p;
        if (z > 0.f) {
            const float s = sqrtf(z);
            v[0] = v[0] / s; v[1] = v[1] / s; v[2] = v[2] / s;
        }
    }
    float u, v;
    u = n1[1] * n2[2]; v = n1[2] * n2[1]; n0[0] = u - v;
    u = n1[2] * n2[0]; v = n1[0] * n2[2]; n0[1] = u - v;
    u = n1[0] * n2[1]; v = n1[1] * n2[0]; n0[2] = u - v;
    u = n2[1] * n0[2]; v = n2[2] * n0[1]; mv[0] = u - v;
    u = n2[2] * n0[0]; v = n2[0] * n0[2]; mv[1] = u - v;
    u = n2[0] * n0[1]; v = n2[1] * n0[0]; mv[2] = u - v;
    for (int r = 0; r < 3; ++r) {
        Tc[4 * r + 0] = n0[r];
        Tc[4 * r + 1] = mv[r];
        Tc[4 * r + 2] = n2[r];
    }
    return true;
}

O3D_HD inline bool m4_is_finite(const float* T) {
    for (int i = 0; i < 16; ++i)
        if (!(T[i] - T[i] == 0.0f)) return false;  // NaN or +-inf
    return true;
}

// ---------------------------------------------------------------------------------------------
// 6x6 symmetric solve, fp64.  Full rank -> LDL^T with diagonal pivoting; rank deficient (pivot test
// with the fp32 threshold size*eps_f32 of fullPivHouseholderQr::isInvertible) -> minimum-norm
// solution through a Jacobi eigen-decomposition.  Returns the numerical rank.
// ---------------------------------------------------------------------------------------------
O3D_HD inline void jacobi_eig_sym(int n, double* A, double* V, double* lam) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
        if (off < 1e-300) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < n; ++i) lam[i] = A[i * n + i];
}

// Fixed-size 3x3 variant of the cyclic Jacobi iteration above: constant indices keep A and V in registers on the
// device (the generic routine indexes at run time, which puts its arrays into scratch memory: 40 us per call on one
// lane), and the sweep loop stops as soon as the off-diagonal mass is below fp64 resolution relative to the diagonal
// (quadratic convergence: further sweeps would not change a bit of the result).
template <int P, int Q>
O3D_HD inline void jacobi3_rotate(double* A, double* V) {
    const double apq = A[3 * P + Q];
    if (fabs(apq) < 1e-300) return;
    const double theta = (A[3 * Q + Q] - A[3 * P + P]) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double akp = A[3 * k + P], akq = A[3 * k + Q];
        A[3 * k + P] = c * akp - s * akq;
        A[3 * k + Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double apk = A[3 * P + k], aqk = A[3 * Q + k];
        A[3 * P + k] = c * apk - s * aqk;
        A[3 * Q + k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[3 * k + P], vkq = V[3 * k + Q];
        V[3 * k + P] = c * vkp - s * vkq;
        V[3 * k + Q] = s * vkp + c * vkq;
    }
}
O3D_HD inline void jacobi_eig_sym3(double* A, double* V, double* lam) {
    V[0] = 1.0; V[1] = 0.0; V[2] = 0.0;
    V[3] = 0.0; V[4] = 1.0; V[5] = 0.0;
    V[6] = 0.0; V[7] = 0.0; V[8] = 1.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
        const double dg = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
        if (off < 1e-300 || off <= 1e-34 * dg) break;
        jacobi3_rotate<0, 1>(A, V);
        jacobi3_rotate<0, 2>(A, V);
        jacobi3_rotate<1, 2>(A, V);
    }
    lam[0] = A[0];
    lam[1] = A[4];
    lam[2] = A[8];
}

// Work arrays of the eigen-solvers below.  The plain entry points keep them on the stack; the device passes a block of
// shared memory instead (jacobi_eig_sym indexes at run time, which puts stack arrays into scratch memory there).
struct Sym6Work {
    double M[36], V[36], lam[6];
};

// rel_thr: eigenvalues <= rel_thr * max are treated as zero.  n6 is 6: a caller that passes it as a value the compiler cannot
// see keeps the loops of the eigen-decomposition rolled.
O3D_HD inline int solve_sym6_in(const double* H, const double* g, double* x, double rel_thr, Sym6Work& w, int n6 = 6) {
    double* const M = w.M;
    double* const V = w.V;
    double* const lam = w.lam;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) M[6 * i + j] = 0.5 * (H[6 * i + j] + H[6 * j + i]);
    jacobi_eig_sym(n6, M, V, lam);
    double lmax = 0;
    for (int k = 0; k < 6; ++k) lmax = fmax(lmax, fabs(lam[k]));
    int rank = 0;
    for (int i = 0; i < 6; ++i) x[i] = 0;
    for (int k = 0; k < 6; ++k) {
        if (!(fabs(lam[k]) > lmax * rel_thr)) continue;
        ++rank;
        double vb = 0;
        for (int i = 0; i < 6; ++i) vb += V[6 * i + k] * g[i];
        vb /= lam[k];
        for (int i = 0; i < 6; ++i) x[i] += V[6 * i + k] * vb;
    }
    return rank;
}
O3D_HD inline int solve_sym6(const double* H, const double* g, double* x, double rel_thr) {
    Sym6Work w;
    return solve_sym6_in(H, g, x, rel_thr, w);
}

constexpr double kP2plRankThr = 6.0 * 1.1920929e-07;   // size * eps_f32: the fp32 rank threshold of the reference's solver
O3D_HD inline int solve6_p2pl(const float* A, const float* b, float* x) {
    double H[36], g[6], xd[6];
    for (int i = 0; i < 36; ++i) H[i] = A[i];
    for (int i = 0; i < 6; ++i) g[i] = b[i];
    const int rank = solve_sym6(H, g, xd, kP2plRankThr);
    for (int i = 0; i < 6; ++i) x[i] = (float)xd[i];
    return rank;
}
// ... with every array in the caller's work area (H, g, xd: 36 + 6 + 6 doubles); n6: see solve_sym6_in
O3D_HD inline int solve6_p2pl_in(const float* A, const float* b, float* x, double* H, double* g, double* xd, Sym6Work& w, int n6 = 6) {
    for (int i = 0; i < 36; ++i) H[i] = A[i];
    for (int i = 0; i < 6; ++i) g[i] = b[i];
    const int rank = solve_sym6_in(H, g, xd, kP2plRankThr, w, n6);
    for (int i = 0; i < 6; ++i) x[i] = (float)xd[i];
    return rank;
}

// ---- R8x: X-ICP localizability (ICP.cpp:1580-1591, 2187-2444; PointToPlane.cpp:459-505) --------------------
// Eigenvectors of a symmetric 3x3 block in DESCENDING eigenvalue order (the order of JacobiSVD's U for a PSD
// matrix); V[3*r+k] = component r of eigenvector k.  kSel: the columns are picked by selects instead of run-time indices
// (the same values; on the device W then stays in registers instead of scratch memory).
template <bool kSel = false>
O3D_HD inline void eig3_desc(const double* S, double* V) {
    double M[9], W[9], l[3];
    for (int i = 0; i < 9; ++i) M[i] = S[i];
    jacobi_eig_sym3(M, W, l);
    int o0 = 0, o1 = 1, o2 = 2;
    if (l[o1] > l[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (l[o2] > l[o0]) { const int t = o0; o0 = o2; o2 = t; }
    if (l[o2] > l[o1]) { const int t = o1; o1 = o2; o2 = t; }
    for (int r = 0; r < 3; ++r) {
        if (kSel) {
            const double w0 = W[3 * r], w1 = W[3 * r + 1], w2 = W[3 * r + 2];
            V[3 * r + 0] = o0 == 0 ? w0 : (o0 == 1 ? w1 : w2);
            V[3 * r + 1] = o1 == 0 ? w0 : (o1 == 1 ? w1 : w2);
            V[3 * r + 2] = o2 == 0 ? w0 : (o2 == 1 ? w1 : w2);
        } else {
            V[3 * r + 0] = W[3 * r + o0];
            V[3 * r + 1] = W[3 * r + o1];
            V[3 * r + 2] = W[3 * r + o2];
        }
    }
}

// rotation (rows/cols 0-2) and translation (3-5) eigenvectors of the fp32 system matrix (row-major 6x6)
template <bool kSel = false>
O3D_HD inline void xicp_eigvecs(const float* A, double* Vr, double* Vt) {
    double Sr[9], St[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Sr[3 * i + j] = 0.5 * ((double)A[6 * i + j] + (double)A[6 * j + i]);
            St[3 * i + j] = 0.5 * ((double)A[6 * (i + 3) + j + 3] + (double)A[6 * (j + 3) + i + 3]);
        }
    eig3_desc<kSel>(Sr, Vr);
    eig3_desc<kSel>(St, Vt);
}

// Work arrays of the constrained solve (see Sym6Work: the stack for the plain entry points, shared memory on the device),
// and where the solve finds each of them
struct XicpWork {
    double Vr[9], Vt[9], Z[36], xn[6], AZ[36], M[36], V[36], lam[6], g[6], bb[6], y[6];
};
struct XicpArrays {
    double *Vr, *Vt, *Z, *xn, *AZ, *M, *V, *lam, *g, *bb, *y;
};

// Equality-constrained solve: v_k . x = rhs[k] along the non-localizable eigen-directions (flags[k] == 0).  Null-space form
// of the reference's (6+c)x(6+c) KKT system: x = N d + Z y with N the constrained eigenvectors, d their right-hand sides,
// Z the localizable ones and Z^T A Z y = Z^T (b - A N d).  kRhs = false is the constraint value 0 of the optimised method
// (x = Z (Z^T A Z)^-1 Z^T b; rhs is not read); with kRhs = true an all-zero rhs returns the same bits: N d and A N d are
// then +0, and adding +0 changes no term (tests/test_xicp_ternary_host.py).
template <bool kRhs, bool kSel = false>
O3D_HD inline int solve6_xicp_impl(const float* A, const float* b, const int* flags, const float* rhs, float* x, const XicpArrays& w) {
    double* const Vr = w.Vr;
    double* const Vt = w.Vt;
    double* const Z = w.Z;
    double* const xn = w.xn;
    double* const AZ = w.AZ;
    double* const M = w.M;
    double* const V = w.V;
    double* const lam = w.lam;
    double* const g = w.g;
    double* const bb = w.bb;
    double* const y = w.y;
    for (int i = 0; i < 6; ++i) xn[i] = 0;
    xicp_eigvecs<kSel>(A, Vr, Vt);
    int m = 0;
    for (int k = 0; k < 3; ++k)
        if (flags[k]) {
            for (int r = 0; r < 6; ++r) Z[6 * r + m] = r < 3 ? Vr[3 * r + k] : 0.0;
            ++m;
        } else if (kRhs) {
            for (int r = 0; r < 3; ++r) xn[r] += Vr[3 * r + k] * (double)rhs[k];
        }
    for (int k = 0; k < 3; ++k)
        if (flags[3 + k]) {
            for (int r = 0; r < 6; ++r) Z[6 * r + m] = r >= 3 ? Vt[3 * (r - 3) + k] : 0.0;
            ++m;
        } else if (kRhs) {
            for (int r = 0; r < 3; ++r) xn[3 + r] += Vt[3 * r + k] * (double)rhs[3 + k];
        }
    for (int i = 0; i < 6; ++i) x[i] = kRhs ? (float)xn[i] : 0.f;
    if (m == 0) return 0;
    for (int i = 0; i < 6; ++i) {
        bb[i] = (double)b[i];
        if (kRhs) {
            double t = 0;
            for (int j = 0; j < 6; ++j) t += 0.5 * ((double)A[6 * i + j] + (double)A[6 * j + i]) * xn[j];
            bb[i] = (double)b[i] - t;
        }
    }
    for (int i = 0; i < 6; ++i)
        for (int c = 0; c < m; ++c) {
            double t = 0;
            for (int j = 0; j < 6; ++j) t += 0.5 * ((double)A[6 * i + j] + (double)A[6 * j + i]) * Z[6 * j + c];
            AZ[6 * i + c] = t;
        }
    for (int a = 0; a < m; ++a) {
        for (int c = 0; c < m; ++c) {
            double t = 0;
            for (int i = 0; i < 6; ++i) t += Z[6 * i + a] * AZ[6 * i + c];
            M[m * a + c] = t;
        }
        double t = 0;
        for (int i = 0; i < 6; ++i) t += Z[6 * i + a] * bb[i];
        g[a] = t;
    }
    for (int a = 0; a < m; ++a)
        for (int c = a + 1; c < m; ++c) {
            const double v = 0.5 * (M[m * a + c] + M[m * c + a]);
            M[m * a + c] = v;
            M[m * c + a] = v;
        }
    jacobi_eig_sym(m, M, V, lam);
    double lmax = 0;
    for (int k = 0; k < m; ++k) lmax = fmax(lmax, fabs(lam[k]));
    const double thr = lmax * (double)m * 1.1920929e-07;
    for (int i = 0; i < 6; ++i) y[i] = 0;
    int rank = 0;
    for (int k = 0; k < m; ++k) {
        if (!(fabs(lam[k]) > thr)) continue;
        ++rank;
        double vb = 0;
        for (int a = 0; a < m; ++a) vb += V[m * a + k] * g[a];
        vb /= lam[k];
        for (int a = 0; a < m; ++a) y[a] += V[m * a + k] * vb;
    }
    for (int i = 0; i < 6; ++i) {
        double t = kRhs ? xn[i] : 0.0;
        for (int c = 0; c < m; ++c) t += Z[6 * i + c] * y[c];
        x[i] = (float)t;
    }
    return rank;
}
O3D_HD inline int solve6_xicp(const float* A, const float* b, const int* flags, float* x) {
    double Vr[9], Vt[9], Z[36], xn[6], AZ[36], M[36], V[36], lam[6], g[6], bb[6], y[6];
    const XicpArrays w = {Vr, Vt, Z, xn, AZ, M, V, lam, g, bb, y};
    return solve6_xicp_impl<false>(A, b, flags, nullptr, x, w);
}
O3D_HD inline int solve6_xicp_in(const float* A, const float* b, const int* flags, float* x, XicpWork& w) {
    const XicpArrays a = {w.Vr, w.Vt, w.Z, w.xn, w.AZ, w.M, w.V, w.lam, w.g, w.bb, w.y};
    return solve6_xicp_impl<false, true>(A, b, flags, nullptr, x, a);
}
// ... with right-hand sides on the constraint rows (EqualityConstraints: the constraint values of partial directions)
O3D_HD inline int solve6_xicp_rhs(const float* A, const float* b, const int* flags, const float* rhs, float* x) {
    double Vr[9], Vt[9], Z[36], xn[6], AZ[36], M[36], V[36], lam[6], g[6], bb[6], y[6];
    const XicpArrays w = {Vr, Vt, Z, xn, AZ, M, V, lam, g, bb, y};
    return solve6_xicp_impl<true>(A, b, flags, rhs, x, w);
}

// ---- X-ICP ternary EqualityConstraints (ICP.cpp:1698-2125, 2504-2795; PointToPlane.cpp:459-505, 570-626) ----------
// Shared by the device (kernels_xicp_ternary.hpp, k_pm_update) and the reg_host_* entry points: the same code.
// Deviations from the reference, all documented in DESIGN.md 5l:
//   * the 3x3 partial problem is built from fp64 sums of fp32 products rounded once to fp32, where the reference runs
//     Eigen's fp32 GEMM over the sampled cloud;
//   * the fp64 least-squares step uses the project's Jacobi eigen-solver in place of Eigen's JacobiSVD;
//   * the eigenvector of the constraint value is taken in the optimisation frame directly, before the round trip through
//     the data frame the reference makes (two fp32 rotations that cancel up to rounding);
//   * a constraint value that is not finite (a singular U) ends the registration as a failed detection (prior returned)
//     where the reference would carry the NaN into the solve.
constexpr int kXtLocalizable = 0, kXtPartialMixed = 1, kXtPartialHigh = 2, kXtNone = 3;

// Category of the six eigen-directions from both alignment sums and their pair counts.  The order of the tests is the
// reference's (decideLocalizabilityLevel).  Returns 0 when the sanity rule (ICP.cpp:1956-1967) fails for the sample of a
// partial direction: fewer pairs than the insufficient threshold, or more than there are pairs.
O3D_HD inline int xicp_ternary_decide(const double* comb, const double* high, const long long* n_comb, const long long* n_high,
                                      long long n_pairs, float high_thr, float enough_thr, float insufficient_thr, int* cat) {
    int sane = 1;
    for (int k = 0; k < 6; ++k) {
        long long sample = -1;
        if (comb[k] >= (double)high_thr || high[k] >= (double)enough_thr) {
            cat[k] = kXtLocalizable;
        } else if (comb[k] >= (double)enough_thr) {
            cat[k] = kXtPartialMixed;
            sample = n_comb[k];
        } else if (high[k] >= (double)insufficient_thr) {
            cat[k] = kXtPartialHigh;
            sample = n_high[k];
        } else {
            cat[k] = kXtNone;
        }
        if (sample >= 0 && ((double)sample < (double)insufficient_thr || sample > n_pairs)) sane = 0;
    }
    return sane;
}

// cofactor_3x3<i, j> of Eigen's Inverse_impl.h on a row-major 3x3
O3D_HD inline float xicp_cof3(const float* m, int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    const float p = m[3 * i1 + j1] * m[3 * i2 + j2], q = m[3 * i1 + j2] * m[3 * i2 + j1];
    return p - q;
}

// Constraint value of one partial direction from the nine sums of its sample (0-5: upper triangle of A3 row by row,
// 6-8: sum of f r with f the normal (translation) or p x n (rotation); b3 = -that) and its eigenvector v in the
// optimisation frame.  solveSimpleOptimizationProblemForPartialConstraints: partial-pivot LU of A3 in fp32 (Eigen's
// unblocked order), new_A = L^T L, new_b = L^T (P b3) in fp32, y = least squares of new_A y = new_b in fp64 rounded to
// fp32, x3 = U^-1 y with the 3x3 cofactor inverse in fp32, value = v . x3.  A singular U gives a value that is not finite.
O3D_HD inline float xicp_partial_constraint(const double* s, const float* v) {
    float a00 = (float)s[0], a01 = (float)s[1], a02 = (float)s[2], a11 = (float)s[3], a12 = (float)s[4], a22 = (float)s[5];
    float m0[3] = {a00, a01, a02}, m1[3] = {a01, a11, a12}, m2[3] = {a02, a12, a22};
    float b0 = -(float)s[6], b1 = -(float)s[7], b2 = -(float)s[8];
    // column 0
    {
        int piv = 0;
        float big = fabsf(m0[0]);
        if (fabsf(m1[0]) > big) { big = fabsf(m1[0]); piv = 1; }
        if (fabsf(m2[0]) > big) { big = fabsf(m2[0]); piv = 2; }
        if (piv == 1) {
            for (int c = 0; c < 3; ++c) { const float t = m0[c]; m0[c] = m1[c]; m1[c] = t; }
            const float t = b0; b0 = b1; b1 = t;
        } else if (piv == 2) {
            for (int c = 0; c < 3; ++c) { const float t = m0[c]; m0[c] = m2[c]; m2[c] = t; }
            const float t = b0; b0 = b2; b2 = t;
        }
        if (big != 0.f) {
            m1[0] = m1[0] / m0[0];
            m2[0] = m2[0] / m0[0];
        }
        float t;
        t = m1[0] * m0[1]; m1[1] = m1[1] - t;
        t = m1[0] * m0[2]; m1[2] = m1[2] - t;
        t = m2[0] * m0[1]; m2[1] = m2[1] - t;
        t = m2[0] * m0[2]; m2[2] = m2[2] - t;
    }
    // column 1
    {
        const float big = fabsf(m2[1]) > fabsf(m1[1]) ? fabsf(m2[1]) : fabsf(m1[1]);
        if (fabsf(m2[1]) > fabsf(m1[1])) {
            for (int c = 0; c < 3; ++c) { const float t = m1[c]; m1[c] = m2[c]; m2[c] = t; }
            const float t = b1; b1 = b2; b2 = t;
        }
        if (big != 0.f) m2[1] = m2[1] / m1[1];
        const float t = m2[1] * m1[2];
        m2[2] = m2[2] - t;
    }
    const float l10 = m1[0], l20 = m2[0], l21 = m2[1];
    // new_A = L^T L (k = 0, 1, 2 in order; the products with the structural zeros and ones of L are exact)
    float n00, n01, n02, n11, n12, t;
    t = l10 * l10; n00 = 1.f + t; t = l20 * l20; n00 = n00 + t;
    t = l20 * l21; n01 = l10 + t;
    n02 = l20;
    t = l21 * l21; n11 = 1.f + t;
    n12 = l21;
    // new_b = L^T (P b3)
    float nb0, nb1;
    t = l10 * b1; nb0 = b0 + t; t = l20 * b2; nb0 = nb0 + t;
    t = l21 * b2; nb1 = b1 + t;
    const float nb2 = b2;
    // y: fp64 least squares (eigenvalues above 3 eps_fp64 of the largest, the rank rule of JacobiSVD::solve)
    double M[9] = {(double)n00, (double)n01, (double)n02, (double)n01, (double)n11, (double)n12, (double)n02, (double)n12, 1.0};
    double W[9], lam[3];
    jacobi_eig_sym3(M, W, lam);
    const double g[3] = {(double)nb0, (double)nb1, (double)nb2};
    const double lmax = fmax(fabs(lam[0]), fmax(fabs(lam[1]), fabs(lam[2])));
    double yd[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(fabs(lam[k]) > lmax * (3.0 * 2.220446049250313e-16))) continue;
        const double vb = (W[k] * g[0] + W[3 + k] * g[1] + W[6 + k] * g[2]) / lam[k];
        yd[0] += W[k] * vb;
        yd[1] += W[3 + k] * vb;
        yd[2] += W[6 + k] * vb;
    }
    const float y0 = (float)yd[0], y1 = (float)yd[1], y2 = (float)yd[2];
    // x3 = U^-1 y: Eigen's 3x3 inverse (cofactors; the determinant along column 0; inverse(r, c) = cofactor<c, r> / det)
    const float u[9] = {m0[0], m0[1], m0[2], 0.f, m1[1], m1[2], 0.f, 0.f, m2[2]};
    const float c00 = xicp_cof3(u, 0, 0), c10 = xicp_cof3(u, 1, 0), c20 = xicp_cof3(u, 2, 0);
    float det = c00 * u[0];
    t = c10 * u[3]; det = det + t;
    t = c20 * u[6]; det = det + t;
    const float invdet = 1.f / det;
    const float i00 = c00 * invdet, i01 = c10 * invdet, i02 = c20 * invdet;
    const float i10 = xicp_cof3(u, 0, 1) * invdet, i11 = xicp_cof3(u, 1, 1) * invdet, i12 = xicp_cof3(u, 2, 1) * invdet;
    const float i20 = xicp_cof3(u, 0, 2) * invdet, i21 = xicp_cof3(u, 1, 2) * invdet, i22 = xicp_cof3(u, 2, 2) * invdet;
    float x0, x1, x2;
    t = i00 * y0; x0 = t; t = i01 * y1; x0 = x0 + t; t = i02 * y2; x0 = x0 + t;
    t = i10 * y0; x1 = t; t = i11 * y1; x1 = x1 + t; t = i12 * y2; x1 = x1 + t;
    t = i20 * y0; x2 = t; t = i21 * y1; x2 = x2 + t; t = i22 * y2; x2 = x2 + t;
    float val = v[0] * x0;
    t = v[1] * x1; val = val + t;
    t = v[2] * x2; val = val + t;
    return val;
}

// x = [rx ry rz tx ty tz] -> row-major 4x4, fp32, one rounding per op (NC10).
O3D_HD inline void x_to_T(const float* x, float* T) {
    float a = x[0] * x[0], b = x[1] * x[1], c = x[2] * x[2];
    float s = a + b;
    s = s + c;
    const float nrm = sqrt((float)s);
    const float angle = atanf(nrm);
    float ax[3] = {x[0], x[1], x[2]};
    const float w = fmax(fabs(x[0]), fmax(fabs(x[1]), fabs(x[2])));
    const float y0 = x[0] / w, y1 = x[1] / w, y2 = x[2] / w;
    float z = y0 * y0, z1 = y1 * y1;
    z = z + z1;
    z1 = y2 * y2;
    z = z + z1;
    if (z > 0.f) {
        float d = sqrt((float)z);
        d = d * w;
        ax[0] = x[0] / d;
        ax[1] = x[1] / d;
        ax[2] = x[2] / d;
    }
    const float sn = sinf(angle), cs = cosf(angle);
    float sa0 = sn * ax[0], sa1 = sn * ax[1], sa2 = sn * ax[2];
    const float c1 = 1.0f - cs;
    float ca0 = c1 * ax[0], ca1 = c1 * ax[1], ca2 = c1 * ax[2];
    float R[9];
    float t;
    t = ca0 * ax[1];
    R[1] = t - sa2;
    R[3] = t + sa2;
    t = ca0 * ax[2];
    R[2] = t + sa1;
    R[6] = t - sa1;
    t = ca1 * ax[2];
    R[5] = t - sa0;
    R[7] = t + sa0;
    t = ca0 * ax[0];
    R[0] = t + cs;
    t = ca1 * ax[1];
    R[4] = t + cs;
    t = ca2 * ax[2];
    R[8] = t + cs;
    bool bad = false;
    for (int i = 0; i < 9; ++i) bad |= (R[i] != R[i]);
    for (int i = 3; i < 6; ++i) bad |= (x[i] != x[i]);
    m4_identity(T);
    if (!bad)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
    T[3] = x[3];
    T[7] = x[4];
    T[11] = x[5];
}

// SE(3) exponential (rotation first), fp64, row-major.
O3D_HD inline void se3_exp(const double* d, double* T) {
    const double w[3] = {d[0], d[1], d[2]}, v[3] = {d[3], d[4], d[5]};
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double A, B, C;
    if (th < 1e-10) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
        C = 1.0 / 6.0 - th2 / 120.0;
    } else {
        A = sin(th) / th;
        B = (1 - cos(th)) / th2;
        C = (1 - A) / th2;
    }
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double K2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += K[3 * i + k] * K[3 * k + j];
            K2[3 * i + j] = s;
        }
    memset(T, 0, 16 * sizeof(double));
    T[15] = 1;
    for (int i = 0; i < 3; ++i) {
        double t = 0;
        for (int j = 0; j < 3; ++j) {
            T[4 * i + j] = (i == j ? 1.0 : 0.0) + A * K[3 * i + j] + B * K2[3 * i + j];
            t += ((i == j ? 1.0 : 0.0) + B * K[3 * i + j] + C * K2[3 * i + j]) * v[j];
        }
        T[4 * i + 3] = t;
    }
}

// ---------------------------------------------------------------------------------------------
// Transformation checkers (TransformationCheckersImpl.cpp:57-158)
// ---------------------------------------------------------------------------------------------
O3D_HD inline void rot_to_quat(const float* T, float* q /* w x y z */) {
    const float m00 = T[0], m11 = T[5], m22 = T[10];
    const float tr = m00 + m11 + m22;
    if (tr > 0.f) {
        float t = sqrt(tr + 1.0f);
        q[0] = 0.5f * t;
        t = 0.5f / t;
        q[1] = (T[9] - T[6]) * t;
        q[2] = (T[2] - T[8]) * t;
        q[3] = (T[4] - T[1]) * t;
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > T[5 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        float t = sqrt(T[5 * i] - T[5 * j] - T[5 * k] + 1.0f);
        float v[3];
        v[i] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (T[4 * k + j] - T[4 * j + k]) * t;
        v[j] = (T[4 * j + i] + T[4 * i + j]) * t;
        v[k] = (T[4 * k + i] + T[4 * i + k]) * t;
        q[1] = v[0];
        q[2] = v[1];
        q[3] = v[2];
    }
}

O3D_HD inline float quat_angular_distance(const float* a, const float* b) {
    const float bw = b[0], bx = -b[1], by = -b[2], bz = -b[3];
    const float w = a[0] * bw - a[1] * bx - a[2] * by - a[3] * bz;
    const float x = a[0] * bx + a[1] * bw + a[2] * bz - a[3] * by;
    const float y = a[0] * by + a[2] * bw + a[3] * bx - a[1] * bz;
    const float z = a[0] * bz + a[3] * bw + a[1] * by - a[2] * bx;
    return 2.0f * atan2f(sqrt(x * x + y * y + z * z), fabs(w));
}

constexpr int kCheckerHist = 16;   // reg_create refuses smooth_len > kCheckerHist - 1 (init's clamp only guards the ring)

// DifferentialTransformationChecker + CounterTransformationChecker state (fixed-size ring so the same
// code runs inside the device-side update kernel).
struct Checkers {
    int max_iter = 40;
    float min_diff_rot = 1e-3f, min_diff_trans = 1e-3f;
    int smooth_len = 3;
    float quats[kCheckerHist][4];
    float trans[kCheckerHist][3];
    int n_hist = 0;        // total poses pushed (ring holds the last kCheckerHist)
    int count = 0;
    bool converged = false, max_iter_reached = false;

    O3D_HD void init(const float* T) {
        n_hist = 0;
        count = 0;
        converged = max_iter_reached = false;
        if (smooth_len > kCheckerHist - 1) smooth_len = kCheckerHist - 1;
        push(T);
    }
    O3D_HD void push(const float* T) {
        const int slot = n_hist % kCheckerHist;
        rot_to_quat(T, quats[slot]);
        trans[slot][0] = T[3];
        trans[slot][1] = T[7];
        trans[slot][2] = T[11];
        ++n_hist;
    }
    // returns `iterate`
    O3D_HD bool check(const float* T) {
        bool iterate = true;
        push(T);
        if (smooth_len > 0 && n_hist > smooth_len) {
            float cr = 0.f, ct = 0.f;
            for (int i = n_hist - 1; i >= n_hist - smooth_len; --i) {
                const int a = i % kCheckerHist, b = (i - 1) % kCheckerHist;
                cr += fabsf(quat_angular_distance(quats[a], quats[b]));
                const float dx = trans[a][0] - trans[b][0], dy = trans[a][1] - trans[b][1],
                            dz = trans[a][2] - trans[b][2];
                ct += sqrtf(dx * dx + dy * dy + dz * dz);
            }
            cr /= (float)smooth_len;
            ct /= (float)smooth_len;
            if (cr < min_diff_rot && ct < min_diff_trans) {
                iterate = false;
                converged = true;
            }
        }
        ++count;
        if (count >= max_iter) {
            iterate = false;
            max_iter_reached = true;
        }
        return iterate;
    }
};

// LDL^T solve of a symmetric 6x6 system in fp64 (no pivoting).  Returns false when a pivot falls below
// rel_thr * (largest diagonal entry): the caller then uses the eigen-solve (minimum-norm) path.
O3D_HD inline bool solve_ldlt6(const double* H, const double* g, double* x, double rel_thr) {
    double L[36], d[6];
    double dmax = 0;
    for (int i = 0; i < 6; ++i) dmax = fmax(dmax, fabs(H[6 * i + i]));
    if (!(dmax > 0)) return false;
    for (int j = 0; j < 6; ++j) {
        double dj = H[6 * j + j];
        for (int k = 0; k < j; ++k) dj -= L[6 * j + k] * L[6 * j + k] * d[k];
        if (!(dj > rel_thr * dmax)) return false;
        d[j] = dj;
        L[6 * j + j] = 1.0;
        for (int i = j + 1; i < 6; ++i) {
            double v = 0.5 * (H[6 * i + j] + H[6 * j + i]);
            for (int k = 0; k < j; ++k) v -= L[6 * i + k] * L[6 * j + k] * d[k];
            L[6 * i + j] = v / dj;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = g[i];
        for (int k = 0; k < i; ++k) v -= L[6 * i + k] * y[k];
        y[i] = v;
    }
    for (int i = 0; i < 6; ++i) y[i] /= d[i];
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[6 * k + i] * x[k];
        x[i] = v;
    }
    return true;
}

// Point-to-plane step (R8): A x = b.  Well-conditioned -> LDL^T; otherwise the eigen-solve with the fp32
// rank threshold (minimum-norm solution, PointToPlane.cpp:206-247).  Returns the numerical rank.
O3D_HD inline int solve6_p2pl_fast(const float* A, const float* b, float* x) {
    double H[36], g[6], xd[6];
    for (int i = 0; i < 36; ++i) H[i] = A[i];
    for (int i = 0; i < 6; ++i) g[i] = b[i];
    int rank = 6;
    if (!solve_ldlt6(H, g, xd, 1e-4)) rank = solve_sym6(H, g, xd, 6.0 * 1.1920929e-07);
    for (int i = 0; i < 6; ++i) x[i] = (float)xd[i];
    return rank;
}

// ---------------------------------------------------------------------------------------------
// Updates of Open3D's RegistrationICP (REG_COST_O3D_P2PL / REG_COST_O3D_P2P) from the reduced 32-double record of one
// iteration; fp64, row-major 4x4 U of T <- U T.  Open3D 0.15.1 is not part of the reference tree: restated from its
// published TransformationEstimationPointToPlane / PointToPoint, PARITY UNPINNED.  The update kernel and
// reg_host_o3d_update both run exactly this code.
// ---------------------------------------------------------------------------------------------

// TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x3..5
O3D_HD inline void o3d_x_to_T(const double* x, double* U) {
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    U[0] = cg * cb;
    U[1] = cg * sb * sa - sg * ca;
    U[2] = cg * sb * ca + sg * sa;
    U[3] = x[3];
    U[4] = sg * cb;
    U[5] = sg * sb * sa + cg * ca;
    U[6] = sg * sb * ca - cg * sa;
    U[7] = x[4];
    U[8] = -sb;
    U[9] = cb * sa;
    U[10] = cb * ca;
    U[11] = x[5];
    U[12] = U[13] = U[14] = 0.0;
    U[15] = 1.0;
}

// Point-to-plane: J^T J x = -J^T r (slots 0-20 packed upper triangle, 21-26).  LDL^T; a rank-deficient system takes the
// minimum-norm eigen-solve (Open3D's Eigen LDLT returns some solution there: a documented deviation).  Returns the rank.
O3D_HD inline int o3d_update_p2pl_in(const double* s, double* U, Sym6Work& w) {
    double H[36], g[6], x[6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) H[6 * i + j] = H[6 * j + i] = s[k++];
    for (int i = 0; i < 6; ++i) g[i] = -s[21 + i];
    int rank = 6;
    if (!solve_ldlt6(H, g, x, 1e-10)) rank = solve_sym6_in(H, g, x, 1e-12, w);
    o3d_x_to_T(x, U);
    return rank;
}
O3D_HD inline int o3d_update_p2pl(const double* s, double* U) {
    Sym6Work w;
    return o3d_update_p2pl_in(s, U, w);
}

// Point-to-point: Umeyama without scaling from the sums about the origin o (slots 0-2 sum (p - o), 3-5 sum (q - o),
// 6-14 sum (q - o)(p - o)^T, 15-17 sum o, 28 pairs).  S = cov(q, p) = U D V^T by the eigenvectors v_k of S^T S
// (descending), made a proper rotation by flipping v_2; then u_k = S v_k / |S v_k| for k = 0, 1 (Gram-Schmidt against
// rounding) and u_2 = u_0 x u_1, which is exactly d u_2 of U diag(1, 1, d) V^T with d = sign(det U det V): no
// determinant is needed.  Rank 1 (all pairs on a line): u_1 is the unit vector perpendicular to u_0 closest to v_1 or
// v_2; rank 0: R = I.  Returns the rank of S (singular values above 1e-10 of the largest).
O3D_HD inline int o3d_update_p2p(const double* s, double* U) {
    const double n = s[28];
    double o[3], mp[3], mq[3], S[9];
    for (int k = 0; k < 3; ++k) {
        o[k] = s[15 + k] / n;
        mp[k] = s[k] / n;
        mq[k] = s[3 + k] / n;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[3 * i + j] = s[6 + 3 * i + j] / n - mq[i] * mp[j];
    double B[9], W[9], lam[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) B[3 * i + j] = S[i] * S[j] + S[3 + i] * S[3 + j] + S[6 + i] * S[6 + j];
    jacobi_eig_sym3(B, W, lam);
    int o0 = 0, o1 = 1, o2 = 2;
    if (lam[o1] > lam[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (lam[o2] > lam[o0]) { const int t = o0; o0 = o2; o2 = t; }
    if (lam[o2] > lam[o1]) { const int t = o1; o1 = o2; o2 = t; }
    // (selects, not run-time indices: the arrays stay in registers on the device)
    double v[3][3], a[3][3], sig[3];
    for (int r = 0; r < 3; ++r) {
        const double w0 = W[3 * r], w1 = W[3 * r + 1], w2 = W[3 * r + 2];
        v[0][r] = o0 == 0 ? w0 : (o0 == 1 ? w1 : w2);
        v[1][r] = o1 == 0 ? w0 : (o1 == 1 ? w1 : w2);
        v[2][r] = o2 == 0 ? w0 : (o2 == 1 ? w1 : w2);
    }
    const double detv = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                        v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    if (detv < 0)
        for (int r = 0; r < 3; ++r) v[2][r] = -v[2][r];
    for (int k = 0; k < 3; ++k) {
        for (int r = 0; r < 3; ++r) a[k][r] = S[3 * r] * v[k][0] + S[3 * r + 1] * v[k][1] + S[3 * r + 2] * v[k][2];
        sig[k] = sqrt(a[k][0] * a[k][0] + a[k][1] * a[k][1] + a[k][2] * a[k][2]);
    }
    int rank = 0;
    if (sig[0] > 1e-300) {
        rank = 1;
        for (int k = 1; k < 3; ++k) rank += sig[k] > 1e-10 * sig[0] ? 1 : 0;
    }
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (rank >= 1) {
        double u0[3], u1[3], u2[3];
        for (int r = 0; r < 3; ++r) u0[r] = a[0][r] / sig[0];
        double c[3];
        if (rank >= 2) {
            for (int r = 0; r < 3; ++r) c[r] = a[1][r];
        } else {
            const double d1 = u0[0] * v[1][0] + u0[1] * v[1][1] + u0[2] * v[1][2];
            const double d2 = u0[0] * v[2][0] + u0[1] * v[2][1] + u0[2] * v[2][2];
            const bool use1 = fabs(d1) <= fabs(d2);
            for (int r = 0; r < 3; ++r) c[r] = use1 ? v[1][r] : v[2][r];
        }
        const double dc = u0[0] * c[0] + u0[1] * c[1] + u0[2] * c[2];
        for (int r = 0; r < 3; ++r) c[r] -= dc * u0[r];
        const double cn = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        for (int r = 0; r < 3; ++r) u1[r] = c[r] / cn;
        u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
        u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
        u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = u0[i] * v[0][j] + u1[i] * v[1][j] + u2[i] * v[2][j];
    }
    // t = mean(q) - R mean(p) with the means about o: (mq + o) - R (mp + o)
    for (int i = 0; i < 3; ++i) {
        const double pi = R[3 * i] * (mp[0] + o[0]) + R[3 * i + 1] * (mp[1] + o[1]) + R[3 * i + 2] * (mp[2] + o[2]);
        for (int j = 0; j < 3; ++j) U[4 * i + j] = R[3 * i + j];
        U[4 * i + 3] = (mq[i] + o[i]) - pi;
    }
    U[12] = U[13] = U[14] = 0.0;
    U[15] = 1.0;
    return rank;
}

O3D_HD inline int o3d_update(bool point_to_point, const double* s, double* U) {
    return point_to_point ? o3d_update_p2p(s, U) : o3d_update_p2pl(s, U);
}

// ---------------------------------------------------------------------------------------------
// RobustOutlierFilter::robustFiltering (OutlierFiltersImpl.cpp:545-598), one entry, fp32 in the reference's operation
// order: e2 = d / (scale * scale); k2 = k * k; the ARBITRARY_SMALL_VALUE clamp compares in double and stores
// (float)1e-50 == 0 (a no-op but for -0 / 0); sq_approx = (float)(approximation^2 in double), +inf = off.
// The chain's weight kernel and reg_host_robust_weights run exactly this code.
// ---------------------------------------------------------------------------------------------
O3D_HD inline float pm_robust_weight(int fct, float k, float scale, float sq_approx, float d) {
    const float s2 = scale * scale;
    const float e2 = d / s2;
    const float k2 = k * k;
    float w = 0.f;
    switch (fct) {
        case 0: {   // cauchy: 1 / (1 + e2 / k2)
            const float a = e2 / k2;
            w = 1.f / (1.f + a);
            break;
        }
        case 1: {   // welsch: exp(-e2 / k2)
            const float a = -e2 / k2;
            w = expf(a);
            break;
        }
        case 2: {   // sc: e2 >= k ? 4 k2 / (k + e2)^2 : 1
            const float a = k + e2;
            const float inv = 1.f / (a * a);
            const float c = 4.f * k2;   // (float)(4.0 * k2): a power of two, exact
            w = e2 >= k ? c * inv : 1.f;
            break;
        }
        case 3: {   // gm: k2 / (k + e2)^2
            const float a = k + e2;
            const float inv = 1.f / (a * a);
            w = k2 * inv;
            break;
        }
        case 4: {   // tukey: e2 >= k2 ? 0 : (1 - e2 / k2)^2
            const float a = 1.f - e2 / k2;
            w = e2 >= k2 ? 0.f : a * a;
            break;
        }
        case 5: {   // huber: e2 >= k2 ? k / sqrt(e2) : 1
            const float inv = 1.f / sqrtf(e2);
            w = e2 >= k2 ? k * inv : 1.f;
            break;
        }
        case 6:     // L1: 1 / sqrt(e2)
            w = 1.f / sqrtf(e2);
            break;
        case 7: {   // student, d = 3: (1 + e2 / k)^(-(k + 3) / 2) (k + 3) / (k + e2)
            const float dd = 3.f;
            const float ex = -(k + dd) / 2.f;
            const float p = powf(1.f + e2 / k, ex);
            const float inv = 1.f / (k + e2);
            w = p * (k + dd) * inv;
            break;
        }
        default:
            break;
    }
    if ((double)w <= 1e-50) w = (float)1e-50;
    if (sq_approx != INFINITY && e2 >= sq_approx) w = 0.f;
    return w;
}

// ---------------------------------------------------------------------------------------------
// VarTrimmedDistOutlierFilter (include/o3dslam_reg.h): the objective and the candidate range, shared by
// the device kernels (kernels_pmoutliers.hpp) and reg_host_var_trim.
//   FRMS(j) = S(j) / (j + 1) / ((j + 1) / n)^(2 lambda) in fp64, n = every entry of the distance matrix
//   candidates j in [minEl, min(maxEl, m)), minEl = floor(minRatio * n), maxEl = floor(maxRatio * n) as fp32 products
// ---------------------------------------------------------------------------------------------
O3D_HD inline double pm_var_frms(double S, int64_t j, int64_t n, double two_lambda) {
    const double id = (double)(j + 1);
    const double ratio = id / (double)n;
    return S / id / pow(ratio, two_lambda);
}

O3D_HD inline void pm_var_range(int64_t n, int64_t m, float min_ratio, float max_ratio, int64_t* lo, int64_t* hi) {
    const float a = min_ratio * (float)n, b = max_ratio * (float)n;
    const int64_t min_el = (int64_t)floorf(a), max_el = (int64_t)floorf(b);
    *lo = min_el;
    *hi = max_el < m ? max_el : m;
}

// Matches::getDistsQuantile's index (Matches.cpp:82-86): size * quantile evaluated in float, truncated; 1 -> the maximum
// (the host-and-device form of trim_rank, kernels_match.hpp)
O3D_HD inline uint32_t pm_quantile_rank(uint32_t total, float ratio) {
    if (total == 0) return 0;
    if (ratio == 1.0f) return total - 1;
    const float posf = (float)total * ratio;
    const uint32_t r = (uint32_t)posf;
    return r >= total ? total - 1 : r;
}

// ---------------------------------------------------------------------------------------------
// Motion compensation of the odometry worker (include/o3dslam_reg.h): the per-point undistortion, shared by
// the device kernel (kernels_odometry.hpp) and reg_host_undistort_point.  fp64, one rounding per operation; every sum of
// three products is (a0 b0 + a1 b1) + a2 b2.
// ---------------------------------------------------------------------------------------------
O3D_HD inline double dot3_ordered(double a0, double b0, double a1, double b1, double a2, double b2) {
    double p = a0 * b0;
    double q = a1 * b1;
    double s = p + q;
    p = a2 * b2;
    return s + p;
}

// Hamilton product a b of (w, x, y, z) quaternions, every component summed left to right
O3D_HD inline void quat_mul_ordered(const double* a, const double* b, double* o) {
    double w = a[0] * b[0], x = a[0] * b[1], y = a[0] * b[2], z = a[0] * b[3];
    w = w - a[1] * b[1];
    x = x + a[1] * b[0];
    y = y + a[2] * b[0];
    z = z + a[3] * b[0];
    w = w - a[2] * b[2];
    x = x + a[2] * b[3];
    y = y + a[3] * b[1];
    z = z + a[1] * b[2];
    w = w - a[3] * b[3];
    x = x - a[3] * b[2];
    y = y - a[1] * b[3];
    z = z - a[2] * b[1];
    o[0] = w;
    o[1] = x;
    o[2] = y;
    o[3] = z;
}

// ConstantVelocityMotionCompensation::computePhase (MotionCompensation.cpp:120-139)
O3D_HD inline double undistort_phase(double x, double y, int clockwise) {
    const double two_pi = 2.0 * 3.14159265358979323846;
    const double a = atan2(y, x);
    const double aw = a < 0.0 ? a + two_pi : a;
    if (aw == 0.0) return 0.0;
    const double f = aw / two_pi;
    return clockwise ? 1.0 - f : f;
}

// One point of undistortInputPointCloud (MotionCompensation.cpp:82-100) for given velocities: lin = linear velocity, rpy =
// angular velocity as roll / pitch / yaw rates.  A motion whose six components all compare equal to zero is the identity
// and copies the point (the arithmetic below would only turn a -0.0 coordinate into +0.0).
O3D_HD inline void undistort_point(const double* p, int clockwise, double scan_duration, const double* lin, const double* rpy,
                                   double* out) {
    const double s = undistort_phase(p[0], p[1], clockwise) * scan_duration;
    const double t[3] = {s * lin[0], s * lin[1], s * lin[2]};
    const double e[3] = {s * rpy[0], s * rpy[1], s * rpy[2]};
    if (t[0] == 0.0 && t[1] == 0.0 && t[2] == 0.0 && e[0] == 0.0 && e[1] == 0.0 && e[2] == 0.0) {
        out[0] = p[0];
        out[1] = p[1];
        out[2] = p[2];
        return;
    }
    const double hr = e[0] * 0.5, hp = e[1] * 0.5, hy = e[2] * 0.5;
    const double qx[4] = {cos(hr), sin(hr), 0.0, 0.0};
    const double qy[4] = {cos(hp), 0.0, sin(hp), 0.0};
    const double qz[4] = {cos(hy), 0.0, 0.0, sin(hy)};
    double qzy[4], q[4];
    quat_mul_ordered(qz, qy, qzy);   // fromRPY: yaw * pitch * roll (math.cpp:32-37)
    quat_mul_ordered(qzy, qx, q);
    double n2 = q[0] * q[0];
    n2 = n2 + q[1] * q[1];
    n2 = n2 + q[2] * q[2];
    n2 = n2 + q[3] * q[3];
    const double nn = sqrt(n2);
    const double w = q[0] / nn, x = q[1] / nn, y = q[2] / nn, z = q[3] / nn;
    // Eigen's QuaternionBase::toRotationMatrix
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz),
                         tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)};   // row-major
    for (int r = 0; r < 3; ++r) out[r] = dot3_ordered(R[3 * r], p[0], R[3 * r + 1], p[1], R[3 * r + 2], p[2]) + t[r];
}

// ---------------------------------------------------------------------------------------------
// The odometry object (include/o3dslam_reg.h): the covariance Open3D's GeneralizedICP derives from a normal
// (shared by k_cov_from_normals and reg_host_covariance_from_normal) and the pose update.  fp64, one rounding per operation.
// ---------------------------------------------------------------------------------------------

// InitializePointCloudForGeneralizedICP for one point: cov = Rx diag(eps, 1, 1) Rx^T with Rx = GetRotationFromE1ToX(x), row-major.
// x is not normalised.  Oddity reproduced: c < -0.99 returns Rx = I (Open3D's comment calls this "the same direction").
O3D_HD inline void cov_from_normal(const double* x, double eps, double* out) {
    const double v[3] = {0.0 * x[2] - 0.0 * x[1], 0.0 * x[0] - 1.0 * x[2], 1.0 * x[1] - 0.0 * x[0]};   // e1 x x, Eigen's cross
    const double c = dot3_ordered(1.0, x[0], 0.0, x[1], 0.0, x[2]);
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (!(c < -0.99)) {
        const double sv[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
        const double f = 1.0 / (1.0 + c);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double s2 = dot3_ordered(sv[3 * i], sv[j], sv[3 * i + 1], sv[3 + j], sv[3 * i + 2], sv[6 + j]);
                const double a = R[3 * i + j] + sv[3 * i + j];
                R[3 * i + j] = a + s2 * f;
            }
    }
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        M[3 * i] = R[3 * i] * eps;
        M[3 * i + 1] = R[3 * i + 1] * 1.0;
        M[3 * i + 2] = R[3 * i + 2] * 1.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            out[3 * i + j] = dot3_ordered(M[3 * i], R[3 * j], M[3 * i + 1], R[3 * j + 1], M[3 * i + 2], R[3 * j + 2]);
}

// a b - c d, each product rounded, then the difference
O3D_HD inline double det2_ordered(double a, double b, double c, double d) {
    const double p = a * b;
    const double q = c * d;
    return p - q;
}

// cum = cum * inverse(T): both column-major 4x4, fp64.  The inverse is the general cofactor inverse over the six 2x2
// minors of the upper and of the lower row pair (no rigidity assumed, as Matrix4d::inverse() assumes none); the product sums
// each entry left to right over k.  The order is written out in include/o3dslam_reg.h.
O3D_HD inline void odometry_accumulate(double* cum, const double* T) {
#define A_(r, c) T[(c) * 4 + (r)]
    const double s0 = det2_ordered(A_(0, 0), A_(1, 1), A_(1, 0), A_(0, 1)), s1 = det2_ordered(A_(0, 0), A_(1, 2), A_(1, 0), A_(0, 2));
    const double s2 = det2_ordered(A_(0, 0), A_(1, 3), A_(1, 0), A_(0, 3)), s3 = det2_ordered(A_(0, 1), A_(1, 2), A_(1, 1), A_(0, 2));
    const double s4 = det2_ordered(A_(0, 1), A_(1, 3), A_(1, 1), A_(0, 3)), s5 = det2_ordered(A_(0, 2), A_(1, 3), A_(1, 2), A_(0, 3));
    const double c5 = det2_ordered(A_(2, 2), A_(3, 3), A_(3, 2), A_(2, 3)), c4 = det2_ordered(A_(2, 1), A_(3, 3), A_(3, 1), A_(2, 3));
    const double c3 = det2_ordered(A_(2, 1), A_(3, 2), A_(3, 1), A_(2, 2)), c2 = det2_ordered(A_(2, 0), A_(3, 3), A_(3, 0), A_(2, 3));
    const double c1 = det2_ordered(A_(2, 0), A_(3, 2), A_(3, 0), A_(2, 2)), c0 = det2_ordered(A_(2, 0), A_(3, 1), A_(3, 0), A_(2, 1));
    double det = s0 * c5;
    det = det - s1 * c4;
    det = det + s2 * c3;
    det = det + s3 * c2;
    det = det - s4 * c1;
    det = det + s5 * c0;
    const double id = 1.0 / det;
    // x y0 - y y1 + z y2, left to right
    auto t3 = [](double x, double y0, double y, double y1, double z, double y2) {
        double r = x * y0;
        r = r - y * y1;
        return r + z * y2;
    };
    double B[16];   // the inverse, row-major
    B[0] = t3(A_(1, 1), c5, A_(1, 2), c4, A_(1, 3), c3) * id;
    B[1] = -t3(A_(0, 1), c5, A_(0, 2), c4, A_(0, 3), c3) * id;
    B[2] = t3(A_(3, 1), s5, A_(3, 2), s4, A_(3, 3), s3) * id;
    B[3] = -t3(A_(2, 1), s5, A_(2, 2), s4, A_(2, 3), s3) * id;
    B[4] = -t3(A_(1, 0), c5, A_(1, 2), c2, A_(1, 3), c1) * id;
    B[5] = t3(A_(0, 0), c5, A_(0, 2), c2, A_(0, 3), c1) * id;
    B[6] = -t3(A_(3, 0), s5, A_(3, 2), s2, A_(3, 3), s1) * id;
    B[7] = t3(A_(2, 0), s5, A_(2, 2), s2, A_(2, 3), s1) * id;
    B[8] = t3(A_(1, 0), c4, A_(1, 1), c2, A_(1, 3), c0) * id;
    B[9] = -t3(A_(0, 0), c4, A_(0, 1), c2, A_(0, 3), c0) * id;
    B[10] = t3(A_(3, 0), s4, A_(3, 1), s2, A_(3, 3), s0) * id;
    B[11] = -t3(A_(2, 0), s4, A_(2, 1), s2, A_(2, 3), s0) * id;
    B[12] = -t3(A_(1, 0), c3, A_(1, 1), c1, A_(1, 2), c0) * id;
    B[13] = t3(A_(0, 0), c3, A_(0, 1), c1, A_(0, 2), c0) * id;
    B[14] = -t3(A_(3, 0), s3, A_(3, 1), s1, A_(3, 2), s0) * id;
    B[15] = t3(A_(2, 0), s3, A_(2, 1), s1, A_(2, 2), s0) * id;
#undef A_
    double P[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double r = cum[i] * B[j];   // cum(i, 0) * B(0, j)
            r = r + cum[4 + i] * B[4 + j];
            r = r + cum[8 + i] * B[8 + j];
            r = r + cum[12 + i] * B[12 + j];
            P[j * 4 + i] = r;
        }
    for (int k = 0; k < 16; ++k) cum[k] = P[k];
}

// ---- pose graph (the order of every product and sum is written out in include/o3dslam_reg.h) ----
// All 4x4 matrices row-major fp64.  C = A B, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 over k; C may not alias A or B.
O3D_HD inline void pg_mul(const double* A, const double* B, double* C) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double r = A[4 * i] * B[j];
            r = r + A[4 * i + 1] * B[4 + j];
            r = r + A[4 * i + 2] * B[8 + j];
            r = r + A[4 * i + 3] * B[12 + j];
            C[4 * i + j] = r;
        }
}

// The rigid inverse (R^T, -R^T t): t'_i = -(((R0i t0) + R1i t1) + R2i t2); last row 0 0 0 1
O3D_HD inline void pg_rigid_inverse(const double* T, double* O) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) O[4 * i + j] = T[4 * j + i];
        double r = T[i] * T[3];
        r = r + T[4 + i] * T[7];
        r = r + T[8 + i] * T[11];
        O[4 * i + 3] = -r;
    }
    O[12] = O[13] = O[14] = 0.0;
    O[15] = 1.0;
}

O3D_HD inline void pg_lin6(const double* M, double* v) {
    v[0] = (M[9] - M[6]) * 0.5;
    v[1] = (M[2] - M[8]) * 0.5;
    v[2] = (M[4] - M[1]) * 0.5;
    v[3] = M[3];
    v[4] = M[7];
    v[5] = M[11];
}

// Generator k (0..2: rotation about x, y, z; 3..5: unit translation), times sign
O3D_HD inline void pg_generator(int k, double sign, double* G) {
    for (int i = 0; i < 16; ++i) G[i] = 0.0;
    if (k == 0) G[6] = -sign, G[9] = sign;
    else if (k == 1) G[2] = sign, G[8] = -sign;
    else if (k == 2) G[1] = -sign, G[4] = sign;
    else G[4 * (k - 3) + 3] = sign;
}

// One edge: A = X^-1 Tt^-1; zeta = lin6(A Ts); column k of Js = lin6((A Gk) Ts), of Jt = lin6((A (-Gk)) Ts).
// Js, Jt: 6 x 6 row-major (row = component of zeta, column = k); either may be null.
O3D_HD inline void pg_edge(const double* Ts, const double* Tt, const double* X, double* zeta, double* Js, double* Jt) {
    double Xi[16], Tti[16], A[16], M[16], G[16], AG[16], v[6];
    pg_rigid_inverse(X, Xi);
    pg_rigid_inverse(Tt, Tti);
    pg_mul(Xi, Tti, A);
    pg_mul(A, Ts, M);
    pg_lin6(M, zeta);
    for (int side = 0; side < 2; ++side) {
        double* J = side ? Jt : Js;
        if (!J) continue;
        for (int k = 0; k < 6; ++k) {
            pg_generator(k, side ? -1.0 : 1.0, G);
            pg_mul(A, G, AG);
            pg_mul(AG, Ts, M);
            pg_lin6(M, v);
            for (int i = 0; i < 6; ++i) J[6 * i + k] = v[i];
        }
    }
}

// out = A^T B over 6 x 6 row-major blocks, every entry summed left to right over the row index
O3D_HD inline void pg_atb6(const double* A, const double* B, double* out) {
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) {
            double r = A[a] * B[c];
            for (int i = 1; i < 6; ++i) r = r + A[6 * i + a] * B[6 * i + c];
            out[6 * a + c] = r;
        }
}

// The record of one edge (kPgRec doubles): Js^T L Js, Js^T L Jt, Jt^T L Js, Jt^T L Jt (36 each), Js^T L e, Jt^T L e (6 each)
// with L = info; W = L J first (rows left to right over the column of L), then J^T W.  Returns e^T L e = sum e_i (L e)_i.
constexpr int kPgRec = 4 * 36 + 12;
O3D_HD inline double pg_edge_record(const double* Ts, const double* Tt, const double* X, const double* info, double* zeta,
                                    double* rec) {
    double Js[36], Jt[36], Ws[36], Wt[36], v[6];
    pg_edge(Ts, Tt, X, zeta, Js, Jt);
    for (int i = 0; i < 6; ++i) {
        for (int c = 0; c < 6; ++c) {
            double rs = info[6 * i] * Js[c], rt = info[6 * i] * Jt[c];
            for (int j = 1; j < 6; ++j) {
                rs = rs + info[6 * i + j] * Js[6 * j + c];
                rt = rt + info[6 * i + j] * Jt[6 * j + c];
            }
            Ws[6 * i + c] = rs;
            Wt[6 * i + c] = rt;
        }
        double r = info[6 * i] * zeta[0];
        for (int j = 1; j < 6; ++j) r = r + info[6 * i + j] * zeta[j];
        v[i] = r;
    }
    if (rec) {
        pg_atb6(Js, Ws, rec);
        pg_atb6(Js, Wt, rec + 36);
        pg_atb6(Jt, Ws, rec + 72);
        pg_atb6(Jt, Wt, rec + 108);
        for (int a = 0; a < 6; ++a) {
            double rs = Js[a] * v[0], rt = Jt[a] * v[0];
            for (int i = 1; i < 6; ++i) {
                rs = rs + Js[6 * i + a] * v[i];
                rt = rt + Jt[6 * i + a] * v[i];
            }
            rec[144 + a] = rs;
            rec[150 + a] = rt;
        }
    }
    double q = zeta[0] * v[0];
    for (int i = 1; i < 6; ++i) q = q + zeta[i] * v[i];
    return q;
}

// e^T L e alone (the trial step), the same order as pg_edge_record
O3D_HD inline double pg_edge_cost(const double* Ts, const double* Tt, const double* X, const double* info, double* zeta) {
    pg_edge(Ts, Tt, X, zeta, nullptr, nullptr);
    double q = 0.0;
    for (int i = 0; i < 6; ++i) {
        double r = info[6 * i] * zeta[0];
        for (int j = 1; j < 6; ++j) r = r + info[6 * i + j] * zeta[j];
        q = i ? q + zeta[i] * r : zeta[i] * r;
    }
    return q;
}

// pose <- V(d) pose, V(al, be, ga, a, b, c) = [Rz(ga) Ry(be) Rx(al) | (a, b, c)]
O3D_HD inline void pg_pose_step(const double* d, const double* pose, double* out) {
    const double sa = sin(d[0]), ca = cos(d[0]), sb = sin(d[1]), cb = cos(d[1]), sg = sin(d[2]), cg = cos(d[2]);
    double V[16];
    V[0] = cg * cb;
    V[1] = (cg * sb) * sa - sg * ca;
    V[2] = (cg * sb) * ca + sg * sa;
    V[3] = d[3];
    V[4] = sg * cb;
    V[5] = (sg * sb) * sa + cg * ca;
    V[6] = (sg * sb) * ca - cg * sa;
    V[7] = d[4];
    V[8] = -sb;
    V[9] = cb * sa;
    V[10] = cb * ca;
    V[11] = d[5];
    V[12] = V[13] = V[14] = 0.0;
    V[15] = 1.0;
    pg_mul(V, pose, out);
}

// The pose vector (only the increment test reads it): the inverse map of V
O3D_HD inline void pg_pose_vector(const double* T, double* x) {
    const double sy = sqrt(T[0] * T[0] + T[4] * T[4]);
    if (sy >= 1e-6) {
        x[0] = atan2(T[9], T[10]);
        x[1] = atan2(-T[8], sy);
        x[2] = atan2(T[4], T[0]);
    } else {
        x[0] = atan2(-T[6], T[5]);
        x[1] = atan2(-T[8], sy);
        x[2] = 0.0;
    }
    x[3] = T[3];
    x[4] = T[7];
    x[5] = T[11];
}

// w = (preference * (d * d)) * (sum of info(5,5) in edge order / n); 0 for no edges
O3D_HD inline double pg_line_process_weight(const double* info55, long long n, long long stride, double preference, double d) {
    if (n <= 0) return 0.0;
    double s = 0.0;
    for (long long e = 0; e < n; ++e) s = s + info55[e * stride];
    return (preference * (d * d)) * (s / (double)n);
}

}  // namespace o3dreg
