// cov2d_kernel_body.hpp -- cov2d_kernel, included twice by cov_kernels.hip (inside bf::nNNNN's anonymous namespace, behind its DPP helpers):
//   BF_COV_ROWS 0, BF_COV2D_NAME = cov2d_kernel        one output row per stream: y = (G^-1 g)_0
//   BF_COV_ROWS 1, BF_COV2D_NAME = cov2d_rows_kernel   lcmv with bf_config.lcmv_out_beams > 1: the lane that solves a frame's system holds the whole
//                                                      solution and stores entry r as row r of the stream's a.gss_rows rows (Yh = [stream][rows]
//                                                      [frame][kYhStride]); rows past the columns in force are zero, a closed gate leaves 0.01 X_0
//                                                      on every row in force (lcmv.cpp:121).  Same arithmetic: row 0 is cov2d_kernel's output
// Textual inclusion, as cov_kernels_body.hpp: the one-row kernel keeps its name in the launch trace and its instructions.
// No include guard: meant to be included more than once.
// Z128: the spectra are complex doubles (the default, BF_PRECISION_REFERENCE: 16 bytes per element, stored halved like z48) instead of z48
template <int KM, int WPS, bool Z128>
__global__ __launch_bounds__(256, WPS) void BF_COV2D_NAME(BinsArgs a, int tile, int tiles_per_stream) {
    constexpr bool ROWS = BF_COV_ROWS;
    constexpr int NB = KM + 1, NS = (NB + 3) / 4;  // right-hand sides, slots per lane
    constexpr int NG = GramIdx<KM>::NG, NE = GramIdx<KM>::NE;
    // Row paddings against bank conflicts (round-3 PMC, profiles/r03_lcmv16_chain_pmc.txt: 53 % of this kernel's LDS cycles were
    // conflicts, 16 % of its wave cycles waited to issue an LDS instruction).  A ds_read_b128 serves 16 lanes at a time, drawn
    // from two of the wavefront's four problems; with 256-byte rows per problem both read the same banks:
    //   s_x: 320-byte rows (problem stride = 64 B mod 256): the four column entries x(4k+q) of two problems land 64 B apart;
    //   s_u: 272-byte rows: the Gram sums read the SAME row index i of up to five different columns at once (16 B apart now),
    //        and a problem's block of NB rows is 80 B mod 256 (NB = 5) / 32 B (NB = 2) from its neighbour's;
    //   s_g: 272-byte rows: every lane of a problem reads the same entry, two problems per access.
    __shared__ __attribute__((aligned(16))) f64x2 s_x[4][2][4][20];   // [wave][new / old][problem][mic]
    __shared__ __attribute__((aligned(16))) f64x2 s_u[4][4][NB][17];  // [wave][problem][column][row]: U = L^-1 [C | x]
    __shared__ __attribute__((aligned(16))) f64x2 s_g[4][4][4][17];   // [wave][problem][frame slot][Gram entry]: four frames' systems wait here
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int l16 = lane & 15, grp = lane >> 4, p = l16 >> 2, q = l16 & 3;
    // Workgroup b runs on XCD b % 8 (round-robin dispatch), each XCD behind its own L2.  A block's 16 problems are 192 contiguous
    // bytes of every spectrum row -- one and a half cache lines -- so neighbouring problem groups share lines: XCD x takes the
    // (stream, tile) units x, x + 8, ... and walks the problem groups of a unit back to back, which puts the blocks that share
    // lines into the same L2 at the same time (a 2-D grid had them 1.5 residency windows apart: every shared line came twice).
    const int n_grp = (kNQ + 15) / 16;
    const int unit = (int)(blockIdx.x >> 3) / n_grp * 8 + (int)(blockIdx.x & 7);
    if (unit >= tiles_per_stream * a.n_streams) return;
    const int pq = ((int)(blockIdx.x >> 3) % n_grp) * 16 + wv * 4 + grp;
    const int s = unit / tiles_per_stream;
    const long tA = (long)(unit % tiles_per_stream) * tile;
    long tB = tA + tile;
    if (tB > a.n_frames) tB = a.n_frames;
    const int M = a.n_mics, NP = (M + 1) >> 1, KP1 = a.kp1, P = a.cfg.past_windows;
    const bool live = pq < kNQ;
    const int qq = live ? pq : kNQ - 1;
    const int j = q_bin(qq);
    const bool lcmv = a.cfg.algo == BF_LCMV;
    const int n_rows = ROWS ? a.gss_rows : 1;
    const long yidx = ROWS ? ((long)s * n_rows * a.n_frames) * kYhStride + qq : ((long)s * a.n_frames) * kYhStride + qq;
    // ROWS: one value on every row in force (zero behind them), or the solution vector row by row
    auto st_same = [&](long idx, cd y) {
        const long yrow = a.n_frames * kYhStride;
        for (int r = 0; r < n_rows; ++r) st_y(a, idx + r * yrow, qq, r < KP1 ? y : cd{0, 0});
    };
    auto st_vec = [&](long idx, const cd (&v)[KM]) {
        const long yrow = a.n_frames * kYhStride;
#pragma unroll
        for (int r = 0; r < KM; ++r)
            if (r < n_rows) st_y(a, idx + r * yrow, qq, r < KP1 ? v[r] : cd{0, 0});
        for (int r = KM; r < n_rows; ++r) st_y(a, idx + r * yrow, qq, cd{0, 0});
    };
    (void)st_same; (void)st_vec;
    typedef typename std::conditional<Z128, f64x2, z48>::type zel;  // stored element
    const zel *Zs = reinterpret_cast<const zel *>(a.Z) + ((long)(s / a.n_dirs) * a.frames_ws + a.frame_off) * NP * kN;
    const f64x2 *steer = a.steer + (long)(s % a.n_dirs) * a.steer_dir_stride;
    const int ksrc = q_src_bin(qq), kneg = (kN - ksrc) & (kN - 1);
    const int addrT = 4 * ((lane & ~15) | (q << 2) | p);  // my transpose partner (q, p)

    // microphone l16's spectrum at this bin, frame t (may be negative: history).  Requested a frame ahead (load_raw) and unpacked
    // where it is needed (finish_mic): a load issued where its value is used costs its full latency every frame -- the compiler cannot
    // move it above the st_y in between -- and two wavefronts per SIMD do not hide that
    struct RawMic {
        zel z, zc;
    };
    const int mic_pair = (l16 < M ? l16 : 0) >> 1;
    auto load_raw = [&](long t) -> RawMic {
        const zel *Zf = Zs + t * NP * kN + mic_pair * kN;
        return RawMic{Zf[ksrc], Zf[kneg]};
    };
    auto dec = [](const zel &v) -> cd {
        if constexpr (Z128) return cd{v.x, v.y};  // (stored halved, like z48)
        else return dec48(v);
    };
    auto finish_mic = [&](const RawMic &r) -> cd {
        if (l16 >= M) return cd{0, 0};
        const cd z = dec(r.z), zc = conj(dec(r.zc));
        cd x;
        if ((l16 & 1) == 0) {
            x = z + zc;  // z48 spectra are stored halved
        } else {
            const cd d = z - zc;
            x = cd{d.y, -d.x};
        }
        return qq == kQX ? conj(x) : x;
    };
    auto load_mic = [&](long t) -> cd { return finish_mic(load_raw(t)); };
    // one microphone per lane -> LDS -> this lane's four row entries x(4a+p) and four column entries x(4b+q).
    // LDS operations of one wavefront execute in issue order: compiler barriers only.
    auto spread = [&](cd x, int slot, cd (&xr)[4], cd (&xc)[4]) {
        s_x[wv][slot][grp][l16] = f64x2{x.x, x.y};
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            xr[k] = ld(&s_x[wv][slot][grp][4 * k + p]);
            xc[k] = ld(&s_x[wv][slot][grp][4 * k + q]);
        }
        __builtin_amdgcn_wave_barrier();
    };
    const double f = fabs(a.freqs[j]);
    const bool inband = live && f >= a.cfg.freq_min && f <= a.cfg.freq_max && !(j == 0 && !lcmv);
    if (__builtin_amdgcn_ballot_w64(inband) == 0) {  // nothing to solve in this wavefront
        for (long t = tA; t < tB; ++t) {
            cd y{0, 0};
            if (j == 0 && !lcmv) y = rowbc<0>(load_mic(t));  // mvdr.cpp:76
            if (live && l16 == 0) {
                if constexpr (ROWS) st_same(yidx + t * kYhStride, y);
                else st_y(a, yidx + t * kYhStride, qq, y);
            }
        }
        return;
    }
    // Right-hand sides: lane (p, q) holds rows 4a + q (a = 0..3) of column p + 4 sl -- rows by q, columns by p -- so that
    // the per-step u = b(jj, col) / L_jj comes from lane (p, qj) of the SAME quad (one DPP broadcast) and the update uses
    // Lcol.  Columns 0..KM-1 = constraints, column KM = the frame's x.
    auto rhs_init = [&](int arow, int col, const cd (&xc)[4]) -> cd {
        const int i = 4 * arow + q;
        if (col == KM) return xc[arow];
        return (col < KP1 && col < KM && i < M) ? ld(steer + ((long)col * M + i) * kN + j) : cd{0, 0};
    };

    // The constraint columns do not change over the tile: the two-wavefront build (195 registers of 256) keeps this lane's four
    // entries of column p instead of fetching them again every frame; the three-wavefront build has no register to spare.
    constexpr bool kKeepC = WPS == 2;
    cd cst[4];
    {
        const cd none[4] = {};
#pragma unroll
        for (int ar = 0; ar < 4; ++ar) cst[ar] = (kKeepC && p < KM) ? rhs_init(ar, p, none) : cd{0, 0};
    }

    cd R[10];
#pragma unroll
    for (int e = 0; e < 10; ++e) R[e] = cd{0, 0};
    // (the three-wavefront build has no registers for the 12 raw dwords in flight: 132 bytes of scratch, mvdr 16-mic 9.4 -> 10.0 ms; it
    // keeps the loads where the values are used.  Two-wavefront build, lcmv 16-mic K = 3: 10.7 -> 10.2 ms)
    constexpr bool kAhead = WPS == 2;
    RawMic nxt = load_raw(kAhead ? (P > 0 ? tA - 1 : tA) : tA);
    for (int pp = 1; pp <= P; ++pp) {  // covariance of the P frames in front of the tile
        const RawMic cur = kAhead ? nxt : load_raw(tA - pp);
        if (kAhead) nxt = load_raw(pp < P ? tA - pp - 1 : tA);  // (the last one: the tile's first frame)
        cd xr[4], xc[4];
        spread(finish_mic(cur), 0, xr, xc);
#pragma unroll
        for (int ar = 0; ar < 4; ++ar)
#pragma unroll
            for (int bc = 0; bc <= ar; ++bc) R[LT(ar, bc)] = cfma_conj(R[LT(ar, bc)], xr[ar], xc[bc]);
    }
    // The (K+1) x (K+1) system G y = g of a frame has no successor in the recursion (only R slides on), and every lane of a
    // problem's row would solve it redundantly: the Gram entries of four consecutive frames are parked in LDS instead and
    // lanes 0..3 of the row solve one frame each -- one pass of the small solve per four frames.
    unsigned open_mask = 0;  // frame slots of this row whose system waits (uniform per row)
    for (long t = tA; t < tB; ++t) {
        const int slot = (int)(t - tA) & 3;
        const cd xm = finish_mic(kAhead ? nxt : load_raw(t));
        RawMic old = nxt;
        if (kAhead) {
            old = load_raw(t - P);                       // needed behind the factorisation
            nxt = load_raw(t + 1 < tB ? t + 1 : t);      // next iteration's frame
        }
        cd xr[4], xc[4];
        spread(xm, 0, xr, xc);
        const double mag = row_sum(fast_sqrt(norm2(xm))) / (double)((unsigned)M * (unsigned)kN);
        const cd x0 = rowbc<0>(xm);
        cd y{0, 0};
        bool deferred = false;
        if (mag > a.cfg.freq_mag_threshold) {  // uniform per row
            cd A[10], b[4][NS];
#pragma unroll
            for (int ar = 0; ar < 4; ++ar) {
#pragma unroll
                for (int bc = 0; bc <= ar; ++bc) {
                    cd v = R[LT(ar, bc)];
                    if (ar == bc) {
                        const int i = 4 * ar + p;
                        if (p == q) v = (i < M) ? v * 1.001 : cd{1.0, 0.0};  // whiteR diagonal (mvdr.cpp:239-243); padding = identity
                    }
                    A[LT(ar, bc)] = v;
                }
#pragma unroll
                for (int sl = 0; sl < NS; ++sl) {
                    if (kKeepC && sl == 0 && KM <= 4)
                        b[ar][0] = p == KM ? xc[ar] : (p < KM ? cst[ar] : cd{0, 0});
                    else
                        b[ar][sl] = (p + 4 * sl < NB) ? rhs_init(ar, p + 4 * sl, xc) : cd{0, 0};
                }
            }
            RowStep<0, 16>::run([&](auto jc) {
                constexpr int jj = decltype(jc)::value, bj = jj >> 2, qj = jj & 3;
                const double inv = fast_rsqrt1(rowbc<5 * qj>(A[LT(bj, bj)].x));  // 1 / L_jj from lane (qj, qj)
                cd Lrow[4], Lcol[4], u[NS];
#pragma unroll
                for (int ar = bj; ar < 4; ++ar) Lrow[ar] = quadbc<qj>(A[LT(ar, bj)] * inv);  // L(4ar+p, jj) from lane (p, qj)
                if (p <= qj) Lrow[bj] = cd{0, 0};                                              // rows i <= jj are final
#pragma unroll
                for (int bc = bj; bc < 4; ++bc) Lcol[bc] = bperm_c(addrT, Lrow[bc]);            // L(4bc+q, jj), 0 for rows <= jj
                const double inv_q = q == qj ? inv : 1.0;  // row jj itself becomes U(jj, col); the other rows of the block keep their value (x 1.0 is exact)
#pragma unroll
                for (int sl = 0; sl < NS; ++sl) {  // meanwhile: u_jj of my column(s), from lane (p, qj) of my quad
                    b[bj][sl] = b[bj][sl] * inv_q;
                    u[sl] = quadbc<qj>(b[bj][sl]);
                }
#pragma unroll
                for (int ar = bj; ar < 4; ++ar)
#pragma unroll
                    for (int bc = bj; bc <= ar; ++bc) A[LT(ar, bc)] = cfms_conj(A[LT(ar, bc)], Lrow[ar], Lcol[bc]);
#pragma unroll
                for (int sl = 0; sl < NS; ++sl)
#pragma unroll
                    for (int ar = bj; ar < 4; ++ar) b[ar][sl] = cfms(b[ar][sl], Lcol[ar], u[sl]);
            });
            // b = rows 4a + q of U for column(s) p + 4 sl.  Through LDS: [column][row]; Gram entry e is summed by lane e of
            // the row over the 16 rows, published, and read back by every lane (the small solve runs redundantly).
#pragma unroll
            for (int sl = 0; sl < NS; ++sl)
                if (p + 4 * sl < NB) {
#pragma unroll
                    for (int ar = 0; ar < 4; ++ar) {
                        const cd v = (4 * ar + q < M) ? b[ar][sl] : cd{0, 0};
                        s_u[wv][grp][p + 4 * sl][4 * ar + q] = f64x2{v.x, v.y};
                    }
                }
            __builtin_amdgcn_wave_barrier();
            {
                // entry l16 < NG: G(r1, r2), r1 <= r2, row-major upper triangle; NG <= l16 < NE: g(r1) = U(:, r1)^H u_x
                int r1 = 0, r2 = KM;
                if (l16 < NG) {
                    int rem = l16;
                    while (rem >= KM - r1) { rem -= KM - r1; ++r1; }
                    r2 = r1 + rem;
                } else {
                    r1 = l16 - NG;
                }
                cd acc{0, 0};
                if (l16 < NE) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc = cfma_conj(acc, ld(&s_u[wv][grp][r2][i]), ld(&s_u[wv][grp][r1][i]));
                }
                s_g[wv][grp][slot][l16] = f64x2{acc.x, acc.y};
            }
            deferred = true;
        } else {
            y = x0 * 0.01;  // in_fft(0,j)*0.01 (mvdr.cpp:96)
        }
        if (!inband) {
            y = (j == 0 && !lcmv) ? x0 : cd{0, 0};
            deferred = false;
        }
        if (deferred)
            open_mask |= 1u << slot;
        else if (live && l16 == 0) {
            if constexpr (ROWS) st_same(yidx + t * kYhStride, y);
            else st_y(a, yidx + t * kYhStride, qq, y);
        }
        if (slot == 3 || t == tB - 1) {  // uniform: the parked systems, one frame per lane 0..3 of the row
            __builtin_amdgcn_wave_barrier();
            const int fs = l16 & 3;
            cd ge[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) ge[e] = ld(&s_g[wv][grp][fs][e]);
            __builtin_amdgcn_wave_barrier();
            // (K+1) x (K+1) system G y = g on the upper triangle (one system per lane)
            cd gv[KM];
            auto UI = [](int r, int c) { return r * KM - r * (r - 1) / 2 + (c - r); };
#pragma unroll
            for (int r1 = 0; r1 < KM; ++r1) gv[r1] = ge[NG + r1];
#pragma unroll
            for (int r1 = 0; r1 < KM; ++r1)
                if (r1 >= KP1) {
#pragma unroll
                    for (int r2 = 0; r2 < r1; ++r2) ge[UI(r2, r1)] = cd{0, 0};
                    ge[UI(r1, r1)] = cd{1.0, 0.0};
#pragma unroll
                    for (int c = r1 + 1; c < KM; ++c) ge[UI(r1, c)] = cd{0, 0};
                    gv[r1] = cd{0, 0};
                }
            cd pinvs[KM];  // reciprocals of the pivots: formed once, used by the elimination and by the back substitution
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                const cd pinv = crcp(ge[UI(k, k)]);
                pinvs[k] = pinv;
#pragma unroll
                for (int r1 = k + 1; r1 < KM; ++r1) {
                    const cd fct = conj(ge[UI(k, r1)]) * pinv;
#pragma unroll
                    for (int c = r1; c < KM; ++c) ge[UI(r1, c)] = ge[UI(r1, c)] - fct * ge[UI(k, c)];
                    gv[r1] = gv[r1] - fct * gv[k];
                }
            }
#pragma unroll
            for (int k = KM - 1; k >= 0; --k) {
                cd acc = gv[k];
#pragma unroll
                for (int c = k + 1; c < KM; ++c) acc = acc - ge[UI(k, c)] * gv[c];
                gv[k] = acc * pinvs[k];
            }
            // lane fs of the row holds frame (t - slot + fs)
            if (live && l16 < 4 && fs <= slot && ((open_mask >> fs) & 1u)) {
                if constexpr (ROWS) st_vec(yidx + (t - slot + fs) * kYhStride, gv);
                else st_y(a, yidx + (t - slot + fs) * kYhStride, qq, gv[0]);
            }
            open_mask = 0;
        }
        // slide the covariance window: + x_t x_t^H - x_{t-P} x_{t-P}^H (mvdr.cpp:100-101).  x_t is read back from its LDS slot
        // (still there) instead of being kept in 32 registers across the factorisation.
        cd xor_[4], xoc[4];
        spread(finish_mic(kAhead ? old : load_raw(t - P)), 1, xor_, xoc);
#pragma unroll
        for (int ar = 0; ar < 4; ++ar) {
            const cd xra = kKeepC ? xr[ar] : ld(&s_x[wv][0][grp][4 * ar + p]);
#pragma unroll
            for (int bc = 0; bc <= ar; ++bc) {
                const cd xcb = kKeepC ? xc[bc] : ld(&s_x[wv][0][grp][4 * bc + q]);
                R[LT(ar, bc)] = cfms_conj(cfma_conj(R[LT(ar, bc)], xra, xcb), xor_[ar], xoc[bc]);
            }
        }
    }
}
