// doa_eig.hpp -- the eigendecomposition behind the MUSIC map (bf_doa_set_method(BF_DOA_MUSIC), include/bfcore.h): a cyclic Jacobi iteration
// for a complex Hermitian matrix with a fixed number of sweeps, and the ordering of its eigenvalues without an indexed sort.
// Plain C++: doa_kernels.hip includes it for the kernels (one matrix per lane), the CPU suite compiles it with g++.
//
//   A = V diag(lambda) V^H.  A sweep visits the pairs (p, q), p < q, row by row; a visit rotates rows and columns p and q by the unitary
//   U = [c, -s e^{i phi}; s e^{-i phi}, c] that zeroes A_pq = |A_pq| e^{i phi}:
//     zeta = (A_pp - A_qq) / (2 |A_pq|),  t = sgn(zeta) / (|zeta| + sqrt(zeta^2 + 1)),  c = 1 / sqrt(t^2 + 1),  s = t c
//     A_pp += t |A_pq|,  A_qq -= t |A_pq|,  and for every other k:  (A_kp, A_kq) <- (c A_kp + w A_kq, c A_kq - conj(w) A_kp),  w = s e^{-i phi}
//   (the smaller rotation angle, Rutishauser's form), and the columns p and q of V take the same update.  A pair whose |A_pq| is zero
//   is left alone (t = 0).  The sweep count does not depend on the data (jacobi_sweeps): every lane of a wavefront does the same work, and
//   the bytes of the result depend on the matrix alone.
//
// The matrix lives behind a store S (the lower triangle and V; where they are is the caller's business):
//   double diag(i), set_diag(i, v);  EigC low(i, c), set_low(i, c, z) for i > c (A_ic);  EigC vec(r, c), set_vec(r, c, z) (V_rc).
// N > 0: the size at compile time; the pair loop is a pack expansion and the k loops are unrolled, so a store made of plain arrays is
// only ever indexed with constants (registers).  N = 0: the size is the run-time n (stores in memory).
#pragma once

#include <cmath>
#include <utility>

#if defined(__HIPCC__)
#define BF_EIG_HD __host__ __device__ __forceinline__
#else
#define BF_EIG_HD inline
#endif
#if defined(__clang__)
#define BF_EIG_UNROLL _Pragma("unroll")
#else
#define BF_EIG_UNROLL
#endif

namespace bf {

struct EigC {
    double re, im;
};

// Sweeps after which the off-diagonal norm is below 1e-14 of the Frobenius norm on every matrix of the CPU suite's set
// (tests/test_doa_music_cpu.py prints the residue after every sweep; EXPERIMENTS.md keeps them), plus one.
constexpr int kJacobiSweepsSmall = 8, kJacobiSweepsLarge = 11;  // up to 8 rows (the register kernels) / 9 to 32
BF_EIG_HD constexpr int jacobi_sweeps(int n) { return n <= 8 ? kJacobiSweepsSmall : kJacobiSweepsLarge; }

template <class S>
BF_EIG_HD EigC eig_get(const S &s, int i, int j) {  // A_ij, i != j, out of the lower triangle
    if (i > j) return s.low(i, j);
    const EigC z = s.low(j, i);
    return EigC{z.re, -z.im};
}
template <class S>
BF_EIG_HD void eig_set(S &s, int i, int j, EigC z) {
    if (i > j) s.set_low(i, j, z);
    else s.set_low(j, i, EigC{z.re, -z.im});
}

// (x, y) <- (c x + w y, c y - conj(w) x)
BF_EIG_HD void eig_rot(EigC &x, EigC &y, double c, double wr, double wi) {
    const EigC x0 = x, y0 = y;
    x.re = fma(-wi, y0.im, fma(wr, y0.re, c * x0.re));
    x.im = fma(wi, y0.re, fma(wr, y0.im, c * x0.im));
    y.re = fma(-wi, x0.im, fma(-wr, x0.re, c * y0.re));
    y.im = fma(wi, x0.re, fma(-wr, x0.im, c * y0.im));
}

template <int N, class S>
BF_EIG_HD void jacobi_rotate(S &s, int n, int p, int q) {  // p < q
    const EigC l = s.low(q, p);                             // A_qp = conj(A_pq)
    const double br = l.re, bi = -l.im;
    const double mag = sqrt(fma(br, br, bi * bi));
    const bool zero = !(mag > 0.0);
    const double app = s.diag(p), aqq = s.diag(q);
    const double zeta = (app - aqq) / (2.0 * mag);  // unused where mag is zero; an infinite zeta gives t = 0
    double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
    if (zero) t = 0.0;
    const double c = 1.0 / sqrt(fma(t, t, 1.0)), sn = t * c;
    const double im = zero ? 0.0 : 1.0 / mag;
    const double wr = sn * br * im, wi = -(sn * bi * im);  // w = s e^{-i phi}
    s.set_diag(p, fma(t, mag, app));
    s.set_diag(q, fma(-t, mag, aqq));
    s.set_low(q, p, EigC{0.0, 0.0});
    auto other = [&](int k) {
        if (k == p || k == q) return;
        EigC x = eig_get(s, k, p), y = eig_get(s, k, q);
        eig_rot(x, y, c, wr, wi);
        eig_set(s, k, p, x);
        eig_set(s, k, q, y);
    };
    auto column = [&](int k) {
        EigC x = s.vec(k, p), y = s.vec(k, q);
        eig_rot(x, y, c, wr, wi);
        s.set_vec(k, p, x);
        s.set_vec(k, q, y);
    };
    if constexpr (N > 0) {
        BF_EIG_UNROLL
        for (int k = 0; k < N; ++k) other(k);
        BF_EIG_UNROLL
        for (int k = 0; k < N; ++k) column(k);
    } else {
        for (int k = 0; k < n; ++k) other(k);
        for (int k = 0; k < n; ++k) column(k);
    }
}

// pair number e of a sweep, row by row: (0,1) (0,2) .. (0,N-1) (1,2) ..
constexpr int eig_pair_p(int n, int e) {
    int p = 0;
    while (e >= n - 1 - p) {
        e -= n - 1 - p;
        ++p;
    }
    return p;
}
constexpr int eig_pair_q(int n, int e) {
    int p = 0;
    while (e >= n - 1 - p) {
        e -= n - 1 - p;
        ++p;
    }
    return p + 1 + e;
}

template <int N, int P, int Q, class S>  // the pair as template arguments: constants whatever the optimiser does
BF_EIG_HD void jacobi_rotate_at(S &s) {
    jacobi_rotate<N>(s, N, P, Q);
#if defined(__HIP_DEVICE_COMPILE__)
    // Rotations of disjoint pairs are independent; interleaving them costs the 8-row kernel its last free registers.  One at a time.
    __builtin_amdgcn_sched_barrier(0);
#endif
}
template <int N, class S, int... E>
BF_EIG_HD void jacobi_sweep_static(S &s, std::integer_sequence<int, E...>) {
    (jacobi_rotate_at<N, eig_pair_p(N, E), eig_pair_q(N, E)>(s), ...);
}

template <int N, class S>
BF_EIG_HD void jacobi_sweep(S &s, int n) {
    if constexpr (N > 0) {
        jacobi_sweep_static<N>(s, std::make_integer_sequence<int, N * (N - 1) / 2>{});
    } else {
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) jacobi_rotate<0>(s, n, p, q);
    }
}

// V = I, then `sweeps` sweeps: the diagonal holds the eigenvalues, column i of V the eigenvector of diag(i).
template <int N, class S>
BF_EIG_HD void jacobi_eig(S &s, int n, int sweeps) {
    const int nn = N > 0 ? N : n;
    if constexpr (N > 0) {
        BF_EIG_UNROLL
        for (int r = 0; r < N; ++r) {
            BF_EIG_UNROLL
            for (int c = 0; c < N; ++c) s.set_vec(r, c, EigC{r == c ? 1.0 : 0.0, 0.0});
        }
    } else {
        for (int r = 0; r < nn; ++r)
            for (int c = 0; c < nn; ++c) s.set_vec(r, c, EigC{r == c ? 1.0 : 0.0, 0.0});
    }
    for (int it = 0; it < sweeps; ++it) jacobi_sweep<N>(s, n);
}

// The place of eigenvalue i in descending order, ties by index: #{j : lambda_j > lambda_i, or lambda_j == lambda_i and j < i}.
// Eigenvector i spans noise when its rank is not below the source count; the profile slot of lambda_i is its rank.
template <int N, class S>
BF_EIG_HD int eig_rank(const S &s, int n, int i) {
    const double li = s.diag(i);
    int r = 0;
    if constexpr (N > 0) {
        BF_EIG_UNROLL
        for (int j = 0; j < N; ++j) {
            const double lj = s.diag(j);
            r += (lj > li || (lj == li && j < i)) ? 1 : 0;
        }
    } else {
        for (int j = 0; j < n; ++j) {
            const double lj = s.diag(j);
            r += (lj > li || (lj == li && j < i)) ? 1 : 0;
        }
    }
    return r;
}

}  // namespace bf
