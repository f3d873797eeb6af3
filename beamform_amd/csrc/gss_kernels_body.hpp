// gss_kernels_body.hpp -- the two gss kernels, included twice by gsc_gss_kernels.hip (inside bf::nNNNN's anonymous namespace):
//   BF_GSS_ALL 0, BF_GSS_NAME(n) = n        gss_kernel<MP, KM>, gss_lane_kernel<MP, KM>: y_fft = this_yf(0), the reference's output
//   BF_GSS_ALL 1, BF_GSS_NAME(n) = n_all    gss_kernel_all<MP, KM>, gss_lane_kernel_all<MP, KM>: every separated source (bf_config.gss_out_sources)
// Textual inclusion rather than a third template parameter or a shared inlined body: the kernels that serve one row keep their names in
// the launch trace (docs/DISPATCH.md) and compile to the instructions they always were (a wrapper around an inlined body did not).
// No include guard: meant to be included more than once.

// ALL (BF_GSS_ALL = 1, the *_all kernels): every separated source this_yf(0 .. R - 1) of a problem is stored, row r of beam s as output stream s * R + r (R = a.gss_rows;
// bf_config.gss_out_sources), instead of this_yf(0) alone (gss.cpp:120-121).  The recursion is the same instruction for instruction: the
// rows are what it already holds in yf[].  Lane r of a group stores row r (the DPP sums leave every total in every lane); rows r >= S,
// rows r >= 1 behind a closed gate (gss.cpp:139-141) and everything out of band are written as zeros -- nothing relies on a cleared Yh.
template <int MP, int KM>
__global__ __launch_bounds__(256) void BF_GSS_NAME(gss_kernel)(BinsArgs a) {
    constexpr bool ALL = BF_GSS_ALL;
    constexpr bool kDpp = MP <= 16;  // sums over the group's lanes by DPP butterflies (pairwise order) instead of serial walks over LDS
    constexpr int GPB = 256 / MP;
    __shared__ cd s_x[GPB][MP + 1];   // padded rows: see mvdr_lcmv_kernel (gss 256x256: 6.5 -> 5.8 ms)
    __shared__ cd s_p[GPB][KM][MP + 1];
    const int grp = threadIdx.x / MP, m = threadIdx.x % MP;
    const int gq = blockIdx.x * GPB + grp;
    if (gq >= a.n_streams * kNQ) return;
    const int s = gq / kNQ, q = gq % kNQ;
    const int j = q_bin(q);
    const int M = a.n_mics, NP = (M + 1) >> 1, S = a.kp1;
    const int R = ALL ? a.gss_rows : 1;
    f64x2 *yout = a.Yh + ((long)s * R * a.n_frames) * kYhStride + q;  // row r of the beam: + r * n_frames * kYhStride
    const f64x2 *Zs = a.Z + ((long)(s / a.n_dirs) * a.frames_ws + a.frame_off) * NP * kN;
    const f64x2 *steer = a.steer + (long)(s % a.n_dirs) * a.steer_dir_stride;
    const double f = fabs(a.freqs[j]);
    const bool inband = f >= a.cfg.freq_min && f <= a.cfg.freq_max;
    if (!inband) {
        if (m == 0)
            for (long t = 0; t < R * a.n_frames; ++t) yout[t * kYhStride] = f64x2{0, 0};  // (the rows of a beam follow each other)
        return;
    }
    const int ksrc = q_src_bin(q), kneg = (kN - ksrc) & (kN - 1);
    cd C[KM], W[KM];
    f64x2 *Wg = a.gssW + (((long)s * kN + j) * S) * M;
#pragma unroll
    for (int r = 0; r < KM; ++r) {
        C[r] = (r < S && m < M) ? ld(steer + ((long)r * M + m) * kN + j) : cd{0, 0};
        if ((a.gss_reset_mask >> (s % a.n_dirs)) & 1ull)
            W[r] = conj(C[r]);  // sep_matrix[j] = weights[j].adjoint() (gss.cpp:92)
        else
            W[r] = (r < S && m < M) ? ld(Wg + (long)r * M + m) : cd{0, 0};
    }
    const double mu = a.cfg.mu, keep = 1 - a.cfg.lambda_ * a.cfg.mu;
    const double c2 = (double)(size_t)(2 * (1 / (size_t)S));  // integer arithmetic, quirk Q13
    // this lane's two packed-spectrum values of a step are requested four frames ahead: the recursion leaves a wavefront nothing
    // else to cover the load latency with (256 x 256: see EXPERIMENTS)
    constexpr int kAhead = 4;
    const int mz = m < M ? m : 0;
    cd zr_[kAhead], zcr_[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
        const f64x2 *Zf = Zs + (k < a.n_frames ? k : a.n_frames - 1) * NP * kN + (mz >> 1) * kN;
        zr_[k] = ld(Zf + ksrc);
        zcr_[k] = ld(Zf + kneg);
    }
    for (long t0 = 0; t0 < a.n_frames; t0 += kAhead) {
#pragma unroll
      for (int kk = 0; kk < kAhead; ++kk) {
        const long t = t0 + kk;
        if (t >= a.n_frames) break;  // uniform
        cd x{0, 0};
        const cd z = zr_[kk], zc = conj(zcr_[kk]);
        {
            const f64x2 *Zn = Zs + (t + kAhead < a.n_frames ? t + kAhead : a.n_frames - 1) * NP * kN + (mz >> 1) * kN;
            zr_[kk] = ld(Zn + ksrc);
            zcr_[kk] = ld(Zn + kneg);
        }
        if (m < M) {
            if ((m & 1) == 0) {
                x = (z + zc) * 0.5;
            } else {
                const cd d = z - zc;
                x = cd{0.5 * d.y, -0.5 * d.x};
            }
            if (q == kQX) x = conj(x);
        }
        s_x[grp][m] = x;
        if (!kDpp) {
#pragma unroll
            for (int r = 0; r < KM; ++r) s_p[grp][r][m] = W[r] * x;
        }
        __builtin_amdgcn_wave_barrier();
        double mag = 0.0, alpha = 0.0;
        if (kDpp) {  // lanes m >= M hold x = 0
            mag = grp_sum<MP>(cabs(x));
            alpha = grp_sum<MP>(norm2(x));
        } else {
            for (int k = 0; k < M; ++k) {
                const cd v = s_x[grp][k];
                mag += cabs(v);
                alpha += norm2(v);
            }
        }
        mag /= (double)((unsigned)M * (unsigned)kN);
        cd y;
        cd yrow{0, 0};  // ALL: what this lane stores as row m
        if (mag > a.cfg.freq_mag_threshold) {
            cd yf[KM];
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                if (kDpp) {
                    yf[r] = grp_sum<MP>(W[r] * x);
                } else {
                    cd acc{0, 0};
                    for (int k = 0; k < M; ++k) acc = acc + s_p[grp][r][k];
                    yf[r] = acc;
                }
            }
            y = yf[0];
            if (ALL) {
#pragma unroll
                for (int r = 0; r < KM; ++r)
                    if (r == m && r < S) yrow = yf[r];
            }
            alpha *= alpha;
            const double c1 = (double)(4 * (size_t)S) * (1 / alpha);
            cd Ey[KM];
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                cd acc{0, 0};
#pragma unroll
                for (int r2 = 0; r2 < KM; ++r2)
                    if (r2 != r && r < S && r2 < S) acc = acc + (yf[r] * conj(yf[r2])) * yf[r2];
                Ey[r] = acc;
            }
            cd d2[KM];
#pragma unroll
            for (int r = 0; r < KM; ++r) d2[r] = cd{0, 0};
            if (c2 != 0.0) {  // only S == 1: dj2 = 2 (W C - I) C^H
                cd wc{0, 0};
                if (kDpp) {
                    wc = grp_sum<MP>(W[0] * C[0]);
                } else {
                    __builtin_amdgcn_wave_barrier();
                    s_p[grp][0][m] = W[0] * C[0];
                    __builtin_amdgcn_wave_barrier();
                    for (int k = 0; k < M; ++k) wc = wc + s_p[grp][0][k];
                }
                wc.x -= 1.0;
                d2[0] = (wc * conj(C[0])) * c2;
            }
#pragma unroll
            for (int r = 0; r < KM; ++r)
                if (r < S) W[r] = (W[r] * keep) - ((Ey[r] * conj(x)) * c1 + d2[r]) * mu;
        } else {
            y = s_x[grp][0] * 0.01;
            if (ALL && m == 0) yrow = y;
        }
        if (ALL) {  // rows MP, MP + 1, ... lie beyond KM >= S: zeros
            for (int r = m; r < R; r += MP) yout[((long)r * a.n_frames + t) * kYhStride] = r == m ? f64x2{yrow.x, yrow.y} : f64x2{0, 0};
        } else if (m == 0) {
            yout[t * kYhStride] = f64x2{y.x, y.y};
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
#pragma unroll
    for (int r = 0; r < KM; ++r)
        if (r < S && m < M) Wg[(long)r * M + m] = f64x2{W[r].x, W[r].y};
}


// ---- gss, one LANE per (stream, problem): the tuned shapes (<= 8 microphones, <= 4 sources) ------------------------------------------
// The group kernel above spends most of its instructions on DPP sums over the MP lanes of a problem (ten 64-bit group sums per frame).
// Here the whole S x M demixing matrix of a problem lives in one lane's registers (4 x 8 complex = 128 VGPRs: two wavefronts per SIMD),
// every sum is a chain of FMAs inside the lane, the 64 lanes of a wavefront are 64 consecutive problems of one stream (their spectrum rows
// are contiguous: 1 KiB per wave-instruction) and the rows of the next frame travel by global -> LDS DMA while this one is worked on
// (as in mvdr_fast_kernel).  The recursion over the frames (gss.cpp:136) stays serial per problem; 256 streams x 341 in-band problems
// are 1 364 wavefronts, all resident at once.  Sums over the microphones run m = 0, 1, ... (the group kernel: pairwise).
// ALL (see gss_kernel): the deferred store becomes one value per row a lane can hold (KM of them: rows r >= KM >= S are zeros); each row's
// store is one wave-instruction over 64 consecutive problems, 1 KiB, as row 0's is.  Row 0 keeps its own variables, so that the one-row
// kernels read as they always did.
template <int MP, int KM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void BF_GSS_NAME(gss_lane_kernel)(BinsArgs a) {
    constexpr bool ALL = BF_GSS_ALL;
    constexpr int NX = (ALL && KM > 1) ? KM - 1 : 0;  // rows 1 .. NX held beside row 0 (deferred like it); NXA: the arrays' length
    constexpr int NXA = NX > 0 ? NX : 1;
    const int lane = threadIdx.x;
    constexpr int wps = (kNQ + 63) / 64;  // wavefronts per stream
    const int s = blockIdx.x / wps;
    int q = (blockIdx.x - s * wps) * 64 + lane;
    const bool live = q < kNQ;
    if (!live) q = kNQ - 1;
    const int j = q_bin(q);
    const int M = a.n_mics, NP = (M + 1) >> 1, S = a.kp1;
    const int R = ALL ? a.gss_rows : 1;
    f64x2 *yout = a.Yh + ((long)s * R * a.n_frames) * kYhStride + q;  // row r of the beam: + r * n_frames * kYhStride
    const double f = fabs(a.freqs[j]);
    const bool inband = live && f >= a.cfg.freq_min && f <= a.cfg.freq_max;
    if (__builtin_amdgcn_ballot_w64(inband) == 0) {  // nothing to separate in this wavefront (gss.cpp:150: y_fft = 0 out of band)
        if (live)
            for (long t = 0; t < R * a.n_frames; ++t) yout[t * kYhStride] = f64x2{0, 0};  // (the rows of a beam follow each other)
        return;
    }
    // frame 0 of this stream's spectra (uniform) + a per-lane byte offset; rows 2p / 2p + 1 of a buffer = Z_t[p][k] / Z_t[p][N - k]
    const char *Zu = reinterpret_cast<const char *>(a.Z + ((long)(s / a.n_dirs) * a.frames_ws + a.frame_off) * NP * kN);
    const int ksrc = q_src_bin(q), kneg = (kN - ksrc) & (kN - 1);
    const unsigned vk = (unsigned)ksrc * 16u, vn = (unsigned)kneg * 16u;
    const long frame_bytes = (long)NP * kN * 16;
    __shared__ __attribute__((aligned(16))) f64x2 s_pf[2][MP][64];
    auto dma_frame = [&](long t, int buf) {
        const char *b = Zu + t * frame_bytes;
#pragma unroll
        for (int p = 0; p < MP / 2; ++p)
            if (p < NP) {  // uniform
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(b + (long)p * kN * 16 + vk),
                                                 (__attribute__((address_space(3))) void *)&s_pf[buf][2 * p][0], 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(b + (long)p * kN * 16 + vn),
                                                 (__attribute__((address_space(3))) void *)&s_pf[buf][2 * p + 1][0], 16, 0, 0);
            }
    };
    const f64x2 *steer = a.steer + (long)(s % a.n_dirs) * a.steer_dir_stride;
    f64x2 *Wg = a.gssW + (((long)s * kN + j) * S) * M;
    cd W[KM][MP], C0[MP];
    const bool reset = ((a.gss_reset_mask >> (s % a.n_dirs)) & 1ull) != 0;
#pragma unroll
    for (int r = 0; r < KM; ++r)
#pragma unroll
        for (int m = 0; m < MP; ++m) {
            cd w{0, 0};
            if (r < S && m < M) w = reset ? conj(ld(steer + ((long)r * M + m) * kN + j)) : ld(Wg + (long)r * M + m);  // sep_matrix[j] = weights[j].adjoint() (gss.cpp:92)
            W[r][m] = w;
        }
#pragma unroll
    for (int m = 0; m < MP; ++m) C0[m] = (KM == 1 && m < M) ? ld(steer + (long)m * kN + j) : cd{0, 0};  // only S == 1 reads the constraint in the loop
    const double mu = a.cfg.mu, keep = 1 - a.cfg.lambda_ * a.cfg.mu;
    const double c2 = (double)(size_t)(2 * (1 / (size_t)S));  // integer arithmetic, quirk Q13
    const float thr32 = (float)(a.cfg.freq_mag_threshold * (double)((unsigned)M * (unsigned)kN));
    int pb = 0;
    if (a.n_frames > 0) dma_frame(0, pb);
    cd y_prev{0, 0};  // frame t - 1's output: stored one iteration late (behind the wait, in front of the next DMA), so that the wait at the
                      // top of an iteration never waits for a store issued a few instructions earlier
    cd yx_prev[NXA];  // ALL: the same for rows 1 .. NX
#pragma unroll
    for (int r = 0; r < NXA; ++r) yx_prev[r] = cd{0, 0};
    for (long t = 0; t < a.n_frames; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // frame t has landed in s_pf[pb]
        __builtin_amdgcn_wave_barrier();
        if (t > 0 && live) yout[(t - 1) * kYhStride] = f64x2{y_prev.x, y_prev.y};
        if (ALL && t > 0 && live) {
#pragma unroll
            for (int r = 1; r <= NX; ++r)
                if (r < R) yout[((long)r * a.n_frames + t - 1) * kYhStride] = f64x2{yx_prev[r - 1].x, yx_prev[r - 1].y};
            for (int r = NX + 1; r < R; ++r) yout[((long)r * a.n_frames + t - 1) * kYhStride] = f64x2{0, 0};
        }
        if (t + 1 < a.n_frames) dma_frame(t + 1, pb ^ 1);
        cd X[MP];
#pragma unroll
        for (int p = 0; p < MP / 2; ++p) {
            const cd z = ld(&s_pf[pb][2 * p][lane]), zc = conj(ld(&s_pf[pb][2 * p + 1][lane]));
            const cd d = z - zc;
            X[2 * p] = (2 * p < M) ? (z + zc) * 0.5 : cd{0, 0};
            X[2 * p + 1] = (2 * p + 1 < M) ? cd{0.5 * d.y, -0.5 * d.x} : cd{0, 0};  // (an odd count's partner channel is rounding residue, not zero)
        }
        if (q == kQX) {
#pragma unroll
            for (int m = 0; m < MP; ++m) X[m].y = -X[m].y;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the rows have been read: the DMA after next may overwrite them
        // magnitude gate (gss.cpp:118): decided in fp32 unless the fp32 sum is within 1e-4 of the threshold
        float m32 = 0.f;
#pragma unroll
        for (int m = 0; m < MP; ++m) m32 += __builtin_amdgcn_sqrtf((float)norm2(X[m]));
        bool open = m32 > thr32;
        if (__builtin_amdgcn_ballot_w64(__builtin_fabsf(m32 - thr32) <= 1e-4f * thr32) != 0) {
            double mag = 0.0;
#pragma unroll
            for (int m = 0; m < MP; ++m) mag += cabs(X[m]);
            mag /= (double)((unsigned)M * (unsigned)kN);
            open = mag > a.cfg.freq_mag_threshold;
        }
        open = open && inband;
        cd y = X[0] * 0.01;  // gate closed (gss.cpp:152)
        cd yx[NXA];          // ALL: rows 1 .. NX; gate closed: zero (gss.cpp:139-141)
#pragma unroll
        for (int r = 0; r < NXA; ++r) yx[r] = cd{0, 0};
        if (__builtin_amdgcn_ballot_w64(open) != 0) {
            double alpha = 0.0;
#pragma unroll
            for (int m = 0; m < MP; ++m) alpha += norm2(X[m]);
            cd yf[KM];
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                cd acc{0, 0};
#pragma unroll
                for (int m = 0; m < MP; ++m) acc = acc + W[r][m] * X[m];
                yf[r] = acc;
            }
            alpha *= alpha;
            // a lane whose gate is closed keeps its matrix: W * 1 - (.. * 0 + d2) * 0 is W bit for bit -- three selects per frame instead of
            // four per matrix entry
            const double c1 = open ? (double)(4 * (size_t)S) * (1 / alpha) : 0.0;
            const double keep_l = open ? keep : 1.0, mu_l = open ? mu : 0.0;
            cd Ey[KM];
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                cd acc{0, 0};
#pragma unroll
                for (int r2 = 0; r2 < KM; ++r2)
                    if (r2 != r && r < S && r2 < S) acc = acc + (yf[r] * conj(yf[r2])) * yf[r2];
                Ey[r] = acc;
            }
            cd wc{0, 0};
            if (KM == 1 && c2 != 0.0) {  // only S == 1: dj2 = 2 (W C - I) C^H
#pragma unroll
                for (int m = 0; m < MP; ++m) wc = wc + W[0][m] * C0[m];
                wc.x -= 1.0;
            }
#pragma unroll
            for (int r = 0; r < KM; ++r)
                if (r < S) {  // uniform
#pragma unroll
                    for (int m = 0; m < MP; ++m) {
                        cd d2{0, 0};
                        if (KM == 1 && r == 0 && c2 != 0.0) d2 = (wc * conj(C0[m])) * c2;
                        W[r][m] = (W[r][m] * keep_l) - ((Ey[r] * conj(X[m])) * c1 + d2) * mu_l;
                    }
                }
            if (open) y = yf[0];
            if (ALL) {
#pragma unroll
                for (int r = 1; r <= NX; ++r)
                    if (open) yx[r - 1] = yf[r];  // (rows r >= S of W are zeros)
            }
        }
        if (!inband) y = cd{0, 0};
        y_prev = y;
        if (ALL) {
#pragma unroll
            for (int r = 0; r < NX; ++r) yx_prev[r] = inband ? yx[r] : cd{0, 0};
        }
        pb ^= 1;
    }
    if (live && a.n_frames > 0) yout[(a.n_frames - 1) * kYhStride] = f64x2{y_prev.x, y_prev.y};
    if (ALL && live && a.n_frames > 0) {
#pragma unroll
        for (int r = 1; r <= NX; ++r)
            if (r < R) yout[((long)r * a.n_frames + a.n_frames - 1) * kYhStride] = f64x2{yx_prev[r - 1].x, yx_prev[r - 1].y};
        for (int r = NX + 1; r < R; ++r) yout[((long)r * a.n_frames + a.n_frames - 1) * kYhStride] = f64x2{0, 0};
    }
#pragma unroll
    for (int r = 0; r < KM; ++r)
#pragma unroll
        for (int m = 0; m < MP; ++m)
            if (inband && r < S && m < M) Wg[(long)r * M + m] = f64x2{W[r][m].x, W[r][m].y};
}
