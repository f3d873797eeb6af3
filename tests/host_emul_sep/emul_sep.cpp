// emul_sep.cpp -- CPU restatement of the frame-pair kernels' DELAY-STRUCTURED gains (geometry.hpp das_sep_gains_w64_f64, das_f64_w64.hip
// das_f64_pair_body) beside the per-bin table form they replace, both through the kernel's own 64-lane x 16-point transform with the
// rotated exchange (tests/host_emul/emul.cpp's helpers, included as they are):
//   form 0  the shared tw2' table, S += g Z with g read per bin from das_mic_gains_w64_f64 (bins above 512: the mirror, conjugated)
//   form 1  the slot's own tw2' B table in the second pass, S += G[k3][k1] Z' -- registers 13 and 2: the exception rows' entry of the lane
// Microphone 0 (unit row) joins in the time domain, h x_0 / M, as in the kernel.  Built by the tests that use it (g++, no GPU).
#include "../host_emul/emul.cpp"

namespace {

struct SepSetup {
    SteeringSet st;
    std::vector<f64x2> T;
    DasSepTables sep;
};
// perturb_bin >= 0: weight (perturb_bin, perturb_mic) is multiplied by (1 + perturb_rel) -- a row that is no longer a delay
SepSetup sep_setup(int M, double sr, const double *mx, const double *my, double theta, int perturb_bin, int perturb_mic, double perturb_rel) {
    SepSetup s;
    ArrayGeometry g;
    g.set(mx, my, M);
    const std::vector<double> freqs = frequency_vector(1024, sr);
    s.st.allocate(1024, M, 1);
    s.st.update_column(g, freqs, 0, theta, true);
    if (perturb_bin >= 0) s.st.at(perturb_bin, perturb_mic, 0) *= (1.0 + perturb_rel);
    s.T = das_mic_gains_w64_f64(s.st, 8);
    s.sep = das_sep_gains_w64_f64(s.st, s.T, 8);
    return s;
}

// forward transform of the kernel with a given second-pass table tw2[b][16]; out[lane][r] stays in the kernel's register / lane order
void fwd_w64(const double *z, const cx<double> *tw1, const cx<double> *tw2, double (*re)[16], double (*im)[16]) {
    for (int l = 0; l < 64; ++l) {
        for (int j = 0; j < 16; ++j) { re[l][j] = z[2 * (64 * j + l)]; im[l][j] = z[2 * (64 * j + l) + 1]; }
        w64_fwd_p1<double>(re[l], im[l], l, tw1);
    }
    w64_T1_fwd<double, true>(re, im);
    for (int l = 0; l < 64; ++l) w64_fwd_p2<double>(re[l], im[l], l, tw2);
    w64_T2_fwd<double>(re, im);
    for (int l = 0; l < 64; ++l) w64_fwd_p3<double>(re[l], im[l]);
}

}  // namespace

extern "C" {

// out[0] = ok, out[1] = bound, out[2] = worst (both relative to 1 / (M N)); out[3], out[4]: the exception rows' entries of bins 512 and 513
// are bit for bit the table's (1 / 0); out[5]: |E13[63] B[15] - table[511]| relative to 1 / (M N), the product in long double;
// out[7]: the same for the product the kernel forms, entry x the slot's ROUNDED tw2' B[15] entry, the shared tw2' divided out, over the four rows b;
// out[6]: what das_f64_decide makes of a planar batch with tables = ok (DasF64Path as an integer; 0 = the chain)
void emul_sep_check(int M, double sr, const double *mx, const double *my, double theta, int perturb_bin, int perturb_mic, double perturb_rel, double *out) {
    const SepSetup s = sep_setup(M, sr, mx, my, theta, perturb_bin, perturb_mic, perturb_rel);
    out[0] = s.sep.ok ? 1.0 : 0.0;
    out[1] = s.sep.bound;
    out[2] = s.sep.worst;
    bool e512 = true, e513 = true;
    long double d511 = 0.0L, d511k = 0.0L;
    const std::vector<f64x2> twt = twiddle_table_w64_rot();
    for (int m = 1; m < M; ++m) {
        const f64x2 *t = s.sep.t.data() + (size_t)m * kDasSepMic;
        const f64x2 *row = s.T.data() + ((size_t)m * kDasMicGainRows + 7) * kDasMicGainRow;  // row (g, k3) = (3, 1): bins 448 .. 512
        e512 = e512 && t[kDasSepE2 + 0].x == row[64].x && t[kDasSepE2 + 0].y == row[64].y;
        e513 = e513 && t[kDasSepE2 + 1].x == row[63].x && t[kDasSepE2 + 1].y == -row[63].y;  // bin 513 = the mirror of bin 511, conjugated
        const cplxd w = s.st.at(240, m, 0);  // B[15] = conj w[240]
        typedef std::complex<long double> cl;
        const cl p = cl(t[kDasSepE13 + 63].x, t[kDasSepE13 + 63].y) * cl(w.real(), -w.imag()) - cl(row[63].x, row[63].y);
        const long double d = std::abs(p) * (long double)M * 1024.0L;
        if (d > d511) d511 = d;
        for (int b = 0; b < 4; ++b) {
            const f64x2 ts = t[kDasSepTw2 + b * kTw2RowW64Rot + 15], t0 = twt[1024 + b * kTw2RowW64Rot + 15];
            const cl pk = cl(t[kDasSepE13 + 63].x, t[kDasSepE13 + 63].y) * cl(ts.x, ts.y) / cl(t0.x, t0.y) - cl(row[63].x, row[63].y);
            const long double dk = std::abs(pk) * (long double)M * 1024.0L;
            if (dk > d511k) d511k = dk;
        }
    }
    out[3] = e512;
    out[4] = e513;
    out[5] = (double)d511;
    out[7] = (double)d511k;
    bf::DasF64Shape c{};
    const DasSlots sl = das_f64_slots(s.st);
    c.layout = BF_PLANAR; c.n_mics = M; c.n_streams = 1; c.n_cus = 256; c.n_frames = 96;
    c.mic0_unit = sl.mic0_unit; c.tables = s.sep.ok; c.n_tr = sl.n_tr; c.das_il_ring = 1; c.das_f64_sched = nullptr;
    out[6] = (double)(int)bf::das_f64_decide(c).path;
}

// x planar [M][F * 512]; y [F * 512] floats (null: not wanted).  The frames are paired as the kernel pairs an even batch: (0, 1), (2, 3), ...,
// a lone last frame in the real part (the pairing rule's solo passes are not restated here: tests/host_emul does that; the callers use level scenes).
// u [ceil(F / 2)][1024][2] (null: not wanted): the backward transform's output in double, frame t in the real and t + 1 in the imaginary part,
// microphone 0's term added -- what the kernel casts to float.  U [ceil(F / 2)][1024][2] (null: not wanted): the summed spectrum in natural bin order.
void emul_sep_das(int M, double sr, const double *mx, const double *my, double theta, const float *x, long F, int form, float *y, double *u_out, double *U_out) {
    const int N = 1024, H = 512;
    const SepSetup s = sep_setup(M, sr, mx, my, theta, -1, 0, 0.0);
    const std::vector<double> h = sqrt_hann(N);
    const std::vector<f64x2> twt = twiddle_table_w64_rot();
    std::vector<cx<double>> tw1(1024), tw2(64), tw2m(64);
    for (int i = 0; i < 1024; ++i) tw1[i] = cx<double>{twt[i].x, twt[i].y};
    for (int b = 0; b < 4; ++b)
        for (int k = 0; k < 16; ++k) tw2[b * 16 + k] = cx<double>{twt[1024 + b * kTw2RowW64Rot + k].x, twt[1024 + b * kTw2RowW64Rot + k].y};
    static double re[64][16], im[64][16], Sr[64][16], Si[64][16];
    std::vector<double> z(2 * N), u(2 * N);
    std::vector<float> tail(H, 0.f);
    auto sample = [&](int m, long sidx) -> double { return sidx < 0 ? 0.0 : (double)x[(size_t)m * F * H + sidx]; };
    const double inv_m = 1.0 / (double)M;
    for (long t = 0; t < F; t += 2) {
        const bool two = t + 1 < F;
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < 16; ++r) Sr[l][r] = Si[l][r] = 0.0;
        for (int m = 1; m < M; ++m) {
            for (int n = 0; n < N; ++n) {
                z[2 * n] = h[n] * sample(m, (t - 1) * (long)H + n);
                z[2 * n + 1] = two ? h[n] * sample(m, t * (long)H + n) : 0.0;
            }
            const f64x2 *sp = s.sep.t.data() + (size_t)m * kDasSepMic;
            if (form == 1)
                for (int b = 0; b < 4; ++b)
                    for (int k = 0; k < 16; ++k) tw2m[b * 16 + k] = cx<double>{sp[kDasSepTw2 + b * kTw2RowW64Rot + k].x, sp[kDasSepTw2 + b * kTw2RowW64Rot + k].y};
            fwd_w64(z.data(), tw1.data(), form == 1 ? tw2m.data() : tw2.data(), re, im);
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 16; ++r) {
                    const int gg = r >> 2, k3 = r & 3;
                    f64x2 G;
                    if (form == 1) {
                        G = r == 13 ? sp[kDasSepE13 + lane] : r == 2 ? sp[kDasSepE2 + lane] : sp[kDasSepG + 16 * k3 + (lane & 15)];
                    } else if (k3 < 2) {
                        G = s.T[((size_t)m * kDasMicGainRows + 2 * gg + k3) * kDasMicGainRow + lane];
                    } else {
                        G = s.T[((size_t)m * kDasMicGainRows + 2 * (3 - gg) + (3 - k3)) * kDasMicGainRow + (64 - lane)];
                        G.y = -G.y;
                    }
                    const double zr = re[lane][r], zi = im[lane][r];  // the kernel's FMA order
                    Sr[lane][r] = std::fma(-G.y, zi, std::fma(G.x, zr, Sr[lane][r]));
                    Si[lane][r] = std::fma(G.y, zr, std::fma(G.x, zi, Si[lane][r]));
                }
        }
        const long pi = t / 2;
        if (U_out)
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 16; ++r) {
                    U_out[((size_t)pi * N + w64_bin(l, r)) * 2] = Sr[l][r];
                    U_out[((size_t)pi * N + w64_bin(l, r)) * 2 + 1] = Si[l][r];
                }
        for (int l = 0; l < 64; ++l) w64_inv_p3<double>(Sr[l], Si[l]);
        w64_T2_inv<double>(Sr, Si);
        for (int l = 0; l < 64; ++l) w64_inv_p2<double>(Sr[l], Si[l], l, tw2.data());
        w64_T1_inv<double, true>(Sr, Si);
        for (int l = 0; l < 64; ++l) {
            w64_inv_p1<double>(Sr[l], Si[l], l, tw1.data());
            for (int j = 0; j < 16; ++j) {
                const int n = 64 * j + l;
                u[2 * n] = std::fma(sample(0, (t - 1) * (long)H + n) * h[n], inv_m, Sr[l][j]);
                u[2 * n + 1] = two ? std::fma(sample(0, t * (long)H + n) * h[n], inv_m, Si[l][j]) : 0.0;
            }
        }
        if (u_out)
            for (int i = 0; i < 2 * N; ++i) u_out[(size_t)pi * 2 * N + i] = u[i];
        if (y)
            for (int f = 0; f < (two ? 2 : 1); ++f)
                for (int n = 0; n < H; ++n) {
                    const float o1 = (float)((double)(float)u[2 * n + f] * h[n]);
                    const float o2 = (float)((double)(float)u[2 * (n + H) + f] * h[n + H]);
                    y[(size_t)(t + f) * H + n] = tail[n] + o1;
                    tail[n] = o2;
                }
    }
}

}  // extern "C"
