// geometry.hpp -- host-side (double precision) array geometry, frequency vector,
// steering weights and the derived device tables.
//
// Mirrors, for this path only, what the reference computes at start-up and on
// every /theta message:
//   handle_params            util.h:52-134   (dist/angle from RAW yaml xy: quirk Q2)
//   calculate_delays         util.h:136-161
//   calculate_frequency_vector util.h:190-199 (quirk Q1: f[N/2-1]=sr/2, f[N/2] undefined -> 0)
//   hann / create_hann_winn  util.h:201-211
//   update_weights           das.cpp:27-45, lcmv.cpp:44-86
// Header-only so the CPU-side unit tests can compile it with g++.
#pragma once

#include <cmath>
#include <complex>
#include <vector>

#include "fft1024_w64.hpp"
#include "fft32.hpp"

namespace bf {

typedef std::complex<double> cplxd;

constexpr double kPi = 3.141592653589793238462643383279502884;
constexpr double kSoundSpeed = 343.0;  // util.h:25

struct ArrayGeometry {
    int n_mics = 0;
    std::vector<double> dist;     // sqrt(x^2+y^2) of the raw coordinates
    std::vector<double> ang_deg;  // atan2(y,x) in degrees of the raw coordinates

    void set(const double *x, const double *y, int n) {
        n_mics = n;
        dist.resize(n);
        ang_deg.resize(n);
        for (int i = 0; i < n; ++i) {
            dist[i] = std::sqrt(x[i] * x[i] + y[i] * y[i]);
            ang_deg[i] = std::atan2(y[i], x[i]) * (180.0 / kPi);
        }
    }

    // Far-field delay of every mic relative to mic 0 for a source at `angle` degrees.
    void delays(double angle, double *tau) const {
        for (int i = 0; i < n_mics; ++i) {
            if (i == 0) {
                tau[i] = 0.0;
                continue;
            }
            double d = ang_deg[i] - angle;
            if (d > 180)
                d -= 360;
            else if (d < -180)
                d += 360;
            tau[i] = dist[i] * std::cos(d * (kPi / 180.0)) / (-kSoundSpeed);
        }
    }
};

// FFT-bin -> Hz including the reference's two off-by-one quirks (Q1).
inline std::vector<double> frequency_vector(int n_fft, double sample_rate) {
    std::vector<double> f(n_fft, 0.0);
    for (int k = 1; k < n_fft / 2; ++k) {
        f[k] = ((double)k / (double)n_fft) * sample_rate;
        f[n_fft - k] = -((double)k / (double)n_fft) * sample_rate;
    }
    f[n_fft / 2 - 1] = sample_rate / 2;
    return f;
}

// Periodic sqrt-Hann analysis/synthesis window.
inline std::vector<double> sqrt_hann(int n_fft) {
    std::vector<double> h(n_fft);
    for (int i = 0; i < n_fft; ++i) h[i] = std::sqrt(0.5 - 0.5 * std::cos(2 * kPi * i / n_fft));
    return h;
}

// Steering / constraint matrices, [bin][mic][col] with col 0 = look direction and
// col k>=1 = interferer k.  `first` = the reference's update_weights(ini=true):
// row 0 (reference mic) is only ever written then (quirk Q3), so after a
// structural re-allocation it stays 0 until the next cold start.
struct SteeringSet {
    int n_fft = 0, n_mics = 0, n_cols = 1;
    std::vector<cplxd> w;  // [n_fft][n_mics][n_cols]

    cplxd &at(int j, int m, int c) { return w[((size_t)j * n_mics + m) * n_cols + c]; }
    const cplxd &at(int j, int m, int c) const { return w[((size_t)j * n_mics + m) * n_cols + c]; }

    void allocate(int nfft, int mics, int cols) {
        n_fft = nfft;
        n_mics = mics;
        n_cols = cols;
        w.assign((size_t)nfft * mics * cols, cplxd(0, 0));
    }

    void update_column(const ArrayGeometry &g, const std::vector<double> &freqs, int col, double angle, bool first) {
        std::vector<double> tau(n_mics);
        g.delays(angle, tau.data());
        const cplxd minus_i(0, -1);
        for (int m = 0; m < n_mics; ++m) {
            if (m == 0) {
                if (first)
                    for (int j = 0; j < n_fft; ++j) at(j, 0, col) = 1.0;
            } else {
                for (int j = 0; j < n_fft; ++j) at(j, m, col) = std::exp(minus_i * (double)2 * kPi * freqs[j] * tau[m]);
            }
        }
    }
};

struct f32x2 {
    float x, y;
};
struct f64x2 {
    double x, y;
};

// exp(-2 pi i k l / 1024) for k,l in [0,32): the inter-pass twiddles of the 32x32
// decomposition, laid out [k][l] so that lanes (l) read consecutive addresses.
template <typename V>
inline std::vector<V> twiddle_table_32x32() {
    std::vector<V> t(1024);
    for (int k = 0; k < 32; ++k)
        for (int l = 0; l < 32; ++l) {
            double a = -2.0 * kPi * (double)(k * l) / 1024.0;
            t[k * 32 + l].x = (decltype(t[0].x))std::cos(a);
            t[k * 32 + l].y = (decltype(t[0].x))std::sin(a);
        }
    return t;
}

// Per-pair complex gains of the fused DAS kernel.
//
// The reference computes y = Re IFFT( sum_m conj(w[m,k]) X_m[k] / M ) (das.cpp:60-66,
// util.h:249).  Two real mics (a,b) are transformed as one complex signal
// Z = FFT(a + i b); with c_m = conj(w_m)/M and its Hermitian part
// ce_m[k] = (c_m[k] + conj(c_m[N-k]))/2 the same real output is
//   y = Re IFFT( sum_pairs D_p[k] Z_p[k] ),   D_p = ce_a - i ce_b
// (derivation in DESIGN.md).  1/N of util.h:249 is folded in.  Odd mic counts
// get a zero b-channel.  Layout: [pair][pos i][lane l] = D_p[l + 32*brev5(i)],
// the register/lane order in which fft1024 leaves the spectrum.
template <typename V>
inline std::vector<V> das_pair_gains_t(const SteeringSet &s, int n_pairs_alloc) {
    const int N = s.n_fft, M = s.n_mics;
    std::vector<V> D((size_t)n_pairs_alloc * N, V{0, 0});
    auto ce = [&](int m, int k) -> cplxd {
        if (m >= M) return cplxd(0, 0);
        cplxd c1 = std::conj(s.at(k, m, 0)) / (double)M;
        cplxd c2 = std::conj(s.at((N - k) % N, m, 0)) / (double)M;
        return 0.5 * (c1 + std::conj(c2));
    };
    for (int p = 0; p < (M + 1) / 2; ++p)
        for (int i = 0; i < 32; ++i)
            for (int l = 0; l < 32; ++l) {
                int k = l + 32 * brev5(i);
                cplxd d = (ce(2 * p, k) - cplxd(0, 1) * ce(2 * p + 1, k)) / (double)N;
                D[((size_t)p * 32 + i) * 32 + l] = V{(decltype(V{}.x))d.real(), (decltype(V{}.x))d.imag()};
            }
    return D;
}
inline std::vector<f32x2> das_pair_gains(const SteeringSet &s, int n_pairs_alloc) { return das_pair_gains_t<f32x2>(s, n_pairs_alloc); }
// The same gains in natural bin order [pair][k], any FFT size (das_fused_gen.hip: JACK periods 256 and 1024).
inline std::vector<f32x2> das_pair_gains_natural(const SteeringSet &s, int n_pairs_alloc) {
    const int N = s.n_fft, M = s.n_mics;
    std::vector<f32x2> D((size_t)n_pairs_alloc * N, f32x2{0.f, 0.f});
    auto ce = [&](int m, int k) -> cplxd {
        if (m >= M) return cplxd(0, 0);
        const cplxd c1 = std::conj(s.at(k, m, 0)) / (double)M, c2 = std::conj(s.at((N - k) % N, m, 0)) / (double)M;
        return 0.5 * (c1 + std::conj(c2));
    };
    for (int p = 0; p < (M + 1) / 2; ++p)
        for (int k = 0; k < N; ++k) {
            const cplxd d = (ce(2 * p, k) - cplxd(0, 1) * ce(2 * p + 1, k)) / (double)N;
            D[(size_t)p * N + k] = f32x2{(float)d.real(), (float)d.imag()};
        }
    return D;
}


// Frame-interleaving (das_fused.hip, group mode; N = 512 / 256 / 128): the N-point pair gains repeated 1024 / N times over the bins of
// the 1024-point transform, 1/1024 folded in, in the register / lane order of fft1024: [pair][position i][lane l] = D_p[(l + 32 brev5(i)) mod N]
inline std::vector<f32x2> das_pair_gains_interleaved(const SteeringSet &s, int n_pairs_alloc) {
    const int N = s.n_fft, M = s.n_mics;
    std::vector<f32x2> D((size_t)n_pairs_alloc * 1024, f32x2{0.f, 0.f});
    auto ce = [&](int m, int k) -> cplxd {
        if (m >= M) return cplxd(0, 0);
        const cplxd c1 = std::conj(s.at(k, m, 0)) / (double)M, c2 = std::conj(s.at((N - k) % N, m, 0)) / (double)M;
        return 0.5 * (c1 + std::conj(c2));
    };
    for (int p = 0; p < (M + 1) / 2; ++p)
        for (int i = 0; i < 32; ++i)
            for (int l = 0; l < 32; ++l) {
                const int k = (l + 32 * brev5(i)) % N;
                const cplxd d = (ce(2 * p, k) - cplxd(0, 1) * ce(2 * p + 1, k)) / 1024.0;
                D[((size_t)p * 32 + i) * 32 + l] = f32x2{(float)d.real(), (float)d.imag()};
            }
    return D;
}

// Twiddles of the LDS-staged autosort (Stockham) transforms of the generic FFT sizes (das_fused_gen.hip, stft_istft.hip):
//   [0, N/2)            W^m = exp(-2 pi i m / N): the closing radix-2 pass of N = 2 * 4^k reads it in order (and the in-place
//                       transform of N = 8192 with its own strides);
//   [N/2, N/2 + R4)     one block per radix-4 pass ns = 1, 4, 16, ... (4 ns <= N), at offset N/2 + (ns - 1): [q][k] = W^((q + 1) k N / (4 ns)),
//                       q = 0..2, k < ns -- the three twiddles of butterfly k CONTIGUOUS in k.  Read out of the plain W^m table the lanes of
//                       a wavefront (consecutive k) are N / (4 ns) entries apart: up to 16 of them on one LDS bank (measured: half of the
//                       LDS cycles of das_fused_gen_kernel<2048> were bank conflicts).
constexpr int stockham_r4_entries(int n) {
    int ns = 1, tot = 0;
    for (; ns * 4 <= n; ns <<= 2) tot += 3 * ns;
    return tot;
}
template <typename V>
inline std::vector<V> stockham_twiddles(int N) {
    std::vector<V> t((size_t)N / 2 + stockham_r4_entries(N));
    typedef decltype(V{}.x) T;
    for (int m = 0; m < N / 2; ++m) {
        const double a = -2.0 * kPi * (double)m / (double)N;
        t[m] = V{(T)std::cos(a), (T)std::sin(a)};
    }
    for (int ns = 1; ns * 4 <= N; ns <<= 2)
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < ns; ++k) {
                const double a = -2.0 * kPi * (double)((long)(q + 1) * k * (N / (4 * ns))) / (double)N;
                t[(size_t)N / 2 + (ns - 1) + (size_t)q * ns + k] = V{(T)std::cos(a), (T)std::sin(a)};
            }
    return t;
}

// fp64 tables of the 64-lane factorisation with the rotated exchange (fft1024_w64.hpp w64_col_rot; das_f64_w64.hip):
// [0, 1024) = W1024^(k1*lane) as [k1][lane]; [1024, 1092) = tw2'[b][k2] = exp(2 pi i 15 b k2 / 64) in rows of 17 (one element of
// padding: the four rows a wavefront reads at once then start 4 LDS banks apart instead of on the same one)
constexpr int kTw2RowW64Rot = 17;
inline std::vector<f64x2> twiddle_table_w64_rot() {
    std::vector<f64x2> t(1024 + 4 * kTw2RowW64Rot, f64x2{0.0, 0.0});
    for (int k = 0; k < 16; ++k)
        for (int l = 0; l < 64; ++l) {
            const double a = -2.0 * kPi * (double)(k * l) / 1024.0;
            t[k * 64 + l] = f64x2{std::cos(a), std::sin(a)};
        }
    for (int b = 0; b < 4; ++b)
        for (int k = 0; k < 16; ++k) {
            const double a = 2.0 * kPi * (double)((15 * b * k) % 64) / 64.0;
            t[1024 + b * kTw2RowW64Rot + k] = f64x2{std::cos(a), std::sin(a)};
        }
    return t;
}
// das_pair_gains_t<f64x2> (32 x 32 order) -> [pair][register r][lane] = D_p[w64_bin(lane, r)]
inline std::vector<f64x2> das_pair_gains_w64_f64(const std::vector<f64x2> &D32, int n_pairs) {
    std::vector<f64x2> D((size_t)n_pairs * 1024);
    std::vector<f64x2> nat(1024);
    for (int p = 0; p < n_pairs; ++p) {
        for (int i = 0; i < 32; ++i)
            for (int l = 0; l < 32; ++l) nat[l + 32 * brev5(i)] = D32[((size_t)p * 32 + i) * 32 + l];
        for (int r = 0; r < 16; ++r)
            for (int l = 0; l < 64; ++l) D[((size_t)p * 16 + r) * 64 + l] = nat[w64_bin(l, r)];
    }
    return D;
}

// Per-microphone Hermitian-part gains of the frame-pair kernel (das_f64_w64.hip das_f64_pair_kernel): ce_m[k] / N for the bins 0 .. 512
// only (ce_m[N - k] = conj ce_m[k]), [mic][row 2 g + k3, k3 < 2][65]: entry c of row (g, k3) = bin 64 g + 256 k3 + c, c = 0 .. 64.
constexpr int kDasMicGainRow = 65, kDasMicGainRows = 8;
inline std::vector<f64x2> das_mic_gains_w64_f64(const SteeringSet &s, int n_mics_alloc) {
    const int N = s.n_fft, M = s.n_mics;
    std::vector<f64x2> T((size_t)n_mics_alloc * kDasMicGainRows * kDasMicGainRow, f64x2{0, 0});
    for (int m = 0; m < M && m < n_mics_alloc; ++m)
        for (int g = 0; g < 4; ++g)
            for (int k3 = 0; k3 < 2; ++k3)
                for (int c = 0; c <= 64; ++c) {
                    const int k = 64 * g + 256 * k3 + c;
                    const cplxd c1 = std::conj(s.at(k, m, 0)) / (double)M, c2 = std::conj(s.at((N - k) % N, m, 0)) / (double)M;
                    const cplxd ce = 0.5 * (c1 + std::conj(c2)) / (double)N;
                    T[((size_t)m * kDasMicGainRows + 2 * g + k3) * kDasMicGainRow + c] = f64x2{ce.real(), ce.imag()};
                }
    return T;
}

// The same gains in the DELAY-STRUCTURED form the frame-pair kernels read.  A das weight row is a pure delay (das.cpp:27-45): away from
// the bins 511 .. 513, where the reference's frequency vector breaks the ramp (quirk Q1), ce_m[k] / N = e^(i phi k) / (M N) for k < 512 and
// e^(i phi (k - N)) / (M N) above, so over the transform's index digits k = k1 + 16 k2 + 256 k3 the gain is a product A[k1] B[k2] C[k3].
// B rides on the second pass's twiddles (a 4-point transform of the third pass has one k2), and register 4 g + k3 of lane l -- bin
// l + 64 g + 256 k3, k1 = l & 15 -- needs G[k3][k1] = A[k1] C[k3] only: four values per lane instead of sixteen.  Per microphone,
// kDasSepMic entries:
//   [0, 64)      G[k3][k1], 1 / (M N) and, for k3 >= 2, the Hermitian mirror's e^(-i phi N) folded in
//   [64, 128)    register 13 (bins 448 + l, with bin 511) per lane: the TABLE's own entry divided by B[12 + (l >> 4)]
//   [128, 192)   register 2 (bins 512 + l, with bins 512 and 513) per lane: the table's (mirrored) entry divided by B[l >> 4]
//   [192, 260)   tw2'[b][k2] B[k2] in the layout of twiddle_table_w64_rot's second part (that table's doubles times B)
// The factors are read off the steering table itself -- A[k1] = conj w[k1], B[k2] = conj w[16 k2], C[1] = conj w[256], C[3] = conj w[768],
// C[2] = C[3]^2 -- and multiplied in long double, every entry rounded once.
// The check.  ok = for every microphone 1 .. M - 1 and every bin the product the kernel forms (G, or the exception entry, times B) is
// within `bound` of das_mic_gains_w64_f64's entry (its mirror's conjugate above bin 512), relative to 1 / (M N); `worst` = the largest
// deviation seen.  The bound: the reference evaluates every weight as exp(-i 2 pi f tau) in double, where the phase carries four
// roundings (<= 4 u |phase|, u = 2^-53) and exp, the Hermitian mean and the two divisions about 4 u more; a product of three such factors
// carries the phase errors of bins k1, 16 k2 and 256 k3 (together below 4 u x 1.5 x the largest phase) beside the table entry's own:
// (16 + 12 phi_max) u with phi_max = 512 |phi|, |phi| taken from bin 1.  "A few ulp" therefore means a few ulp per radian of the row's
// largest phase: on a 0.2 m array that is 1e-13, where 1.8e-14 is the worst seen.  The factor of six between them is the distance between
// every rounding falling the same way (the bound) and what roundings do on average (the measurement); the bound is the a-priori one on
// purpose, so that no geometry or look angle of a real das table is ever sent to the chain by it, and it still sits an order of magnitude
// below the smallest defect that would show in the float output (1e-12 moves a sample in 1e5).  A table that is not a delay in some row
// misses it by orders of magnitude and goes to the chain (DasF64Shape::tables).
// (The kernel multiplies no twiddle at k2 = 0: it takes B[0] = conj w[0] for 1.  That is exact for das -- f[0] = 0 -- and the check
// multiplies by the table's B[0], so a row with any other w[0] fails it.)
constexpr int kDasSepG = 0, kDasSepE13 = 64, kDasSepE2 = 128, kDasSepTw2 = 192, kDasSepMic = 192 + 4 * kTw2RowW64Rot;
struct DasSepTables {
    std::vector<f64x2> t;  // [microphone][kDasSepMic]
    bool ok = false;
    double bound = 0.0, worst = 0.0;  // relative to 1 / (M N), over every microphone
};
inline DasSepTables das_sep_gains_w64_f64(const SteeringSet &s, const std::vector<f64x2> &T /* das_mic_gains_w64_f64(s, n_mics_alloc) */, int n_mics_alloc) {
    typedef std::complex<long double> cl;
    const int N = s.n_fft, M = s.n_mics;
    DasSepTables r;
    r.t.assign((size_t)n_mics_alloc * kDasSepMic, f64x2{0, 0});
    if (N != 1024 || M < 1) return r;
    const long double scale = 1.0L / ((long double)M * (long double)N);
    const std::vector<f64x2> tw2 = twiddle_table_w64_rot();
    auto wl = [&](int k, int m) { const cplxd w = s.at(k, m, 0); return cl((long double)w.real(), -(long double)w.imag()); };  // conj w
    auto tab = [&](int m, int k) -> cl {  // the table's gain of bin k (bins above 512: the mirror's conjugate, as the kernel read it)
        const int kk = k <= 512 ? k : N - k, k3 = kk >= 512 ? 1 : (kk >> 8) & 1, g = kk >= 512 ? 3 : (kk >> 6) & 3, c = kk - 64 * g - 256 * k3;
        const f64x2 v = T[((size_t)m * kDasMicGainRows + 2 * g + k3) * kDasMicGainRow + c];
        return cl((long double)v.x, k <= 512 ? (long double)v.y : -(long double)v.y);
    };
    auto rnd = [](cl v) { return f64x2{(double)v.real(), (double)v.imag()}; };
    r.ok = true;
    for (int m = 1; m < M && m < n_mics_alloc; ++m) {
        f64x2 *t = r.t.data() + (size_t)m * kDasSepMic;
        cl B[16];
        for (int k2 = 0; k2 < 16; ++k2) B[k2] = wl(16 * k2, m);
        const cl C3 = wl(768, m), C[4] = {cl(1.0L, 0.0L), wl(256, m), C3 * C3, C3};
        for (int k3 = 0; k3 < 4; ++k3)
            for (int k1 = 0; k1 < 16; ++k1) t[kDasSepG + 16 * k3 + k1] = rnd(wl(k1, m) * C[k3] * scale);
        for (int l = 0; l < 64; ++l) {
            t[kDasSepE13 + l] = rnd(tab(m, 448 + l) / B[12 + (l >> 4)]);
            t[kDasSepE2 + l] = rnd(tab(m, 512 + l) / B[l >> 4]);
        }
        for (int b = 0; b < 4; ++b)
            for (int k2 = 0; k2 < 16; ++k2) {
                // (the shared table's own doubles times B: a row of ones leaves the transform's twiddles bit for bit what they were)
                const f64x2 w2 = tw2[1024 + b * kTw2RowW64Rot + k2];
                t[kDasSepTw2 + b * kTw2RowW64Rot + k2] = rnd(cl((long double)w2.x, (long double)w2.y) * B[k2]);
            }
        const cplxd w1 = s.at(1, m, 0);
        const double bound = (16.0 + 12.0 * 512.0 * std::fabs(std::atan2(w1.imag(), w1.real()))) * 0x1p-53;
        if (bound > r.bound) r.bound = bound;
        for (int k = 0; k < N; ++k) {
            const int k1 = k & 15, k2 = (k >> 4) & 15, k3 = k >> 8, l = k & 63, reg = 4 * (k2 >> 2) + k3;
            const f64x2 gv = reg == 13 ? t[kDasSepE13 + l] : reg == 2 ? t[kDasSepE2 + l] : t[kDasSepG + 16 * k3 + k1];
            const f64x2 bv = rnd(B[k2]);  // (the kernel's B sits inside its twiddle; what is checked is the gain, not the twiddle's rounding)
            const cl d = cl((long double)gv.x, (long double)gv.y) * cl((long double)bv.x, (long double)bv.y) - tab(m, k);
            const double dev = (double)(std::abs(d) / scale);
            if (!(dev <= bound)) r.ok = false;  // (a NaN fails)
            if (dev > r.worst || dev != dev) r.worst = dev;
        }
    }
    return r;
}

// What das_f64_pair_kernel needs to know about a das steering table beyond its gains (pipeline_kernels.hpp DasF64Args of the same names):
// whether microphone 0's weight row is identically 1 (das.cpp:33-38 writes it once; quirk Q3 can leave it 0) -- only then may the kernel
// skip that microphone's transform -- and its walk over the others: slot k transforms microphone slot_mic[k], k < n_tr, and extra_mic
// (-1 = none) shares slot 0's transform.
struct DasSlots {
    int n_tr = 0, extra_mic = -1;
    int slot_mic[8] = {1, 2, 3, 4, 5, 6, 7, 0};
    bool mic0_unit = false;
};
// Microphones 1 .. M - 1 whose weight rows compare equal in every bin (same delay: the reference drops z, util.h:82-92, so e.g. aira16's
// microphones 1 and 7 -- beamform_config.yaml:21,27 -- coincide for every look direction) share a forward transform: the first such
// pair (a, b), a < b, goes into slot 0 with extra_mic = b, the other microphones follow in ascending order.  Up to 8 microphones (the
// one-launch kernels' limit); more: the default, which no kernel reads.
inline DasSlots das_f64_slots(const SteeringSet &s) {
    DasSlots sl;
    const int N = s.n_fft, M = s.n_mics;
    if (M < 1 || M > 8) return sl;
    sl.mic0_unit = true;
    for (int j = 0; j < N && sl.mic0_unit; ++j) sl.mic0_unit = s.at(j, 0, 0) == cplxd(1.0, 0.0);
    auto same_row = [&](int a, int b) { int j = 0; while (j < N && s.at(j, a, 0) == s.at(j, b, 0)) ++j; return j == N; };
    int pa = -1;
    for (int a = 1; a < M && pa < 0; ++a)
        for (int b = a + 1; b < M && pa < 0; ++b)
            if (same_row(a, b)) { sl.slot_mic[sl.n_tr++] = pa = a; sl.extra_mic = b; }
    for (int m = 1; m < M; ++m)
        if (m != pa && m != sl.extra_mic) sl.slot_mic[sl.n_tr++] = m;
    return sl;
}

}  // namespace bf
