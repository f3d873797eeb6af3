// cov_kernels_body.hpp -- mvdr_fast_kernel and mvdr_lcmv_kernel, included twice by cov_kernels.hip (inside bf::nNNNN's anonymous namespace):
//   BF_COV_TRACK 0, BF_COV_NAME(n) = n_kernel         mvdr_fast_kernel<MP, KC, Z128>, mvdr_lcmv_kernel<MP, KM>: one set of constraint columns per batch
//   BF_COV_TRACK 1, BF_COV_NAME(n) = n_track_kernel   mvdr_fast_track_kernel, mvdr_lcmv_track_kernel: the columns of a frame come from the batch's
//                                                     column track (bf_process_batch_device_ctracked, BinsArgs::track / track_cols)
// Textual inclusion, as gss_kernels_body.hpp: the untracked kernels keep their names in the launch trace and compile to the instructions
// they always were (a __global__ wrapper around a shared inlined body moved their SGPR counts and a few AGPR / scratch figures).
//   BF_COV_ROWS 1 (with either BF_COV_TRACK)          mvdr_fast_rows_kernel, mvdr_fast_track_rows_kernel: the lane kernel's twins that store
//                                                     every beam of lcmv (bf_config.lcmv_out_beams, BinsArgs::gss_rows rows per stream); the
//                                                     group kernel is defined by the BF_COV_ROWS 0 inclusions only: it counts its rows at run time
// No include guard: meant to be included more than once.

// KC = constraint columns: 1 = mvdr (the steering vector); 2..4 = lcmv with up to KC - 1 interferers (lcmv.cpp:102-130): the
// columns C ride through the factorisation like the steering vector does (U = L^-1 C, v = L^-1 x), then G = U^H U, g = U^H v and
// y = (G^-1 g)_0 -- the first row of W^H x with W = R^-1 C (C^H R^-1 C)^-1.  Unused columns are padded with the identity.
// Z128: the spectra are complex doubles (the default, BF_PRECISION_REFERENCE: 16 bytes per element) instead of z48 (BF_PRECISION_MIXED: 12 bytes); both stored halved
// TRACK (mvdr_fast_track_kernel): a column-tracked batch (bf_process_batch_device_ctracked) -- the columns of frame t come from the tables its
// track entries name (BinsArgs::track: [stream][frame][track_cols]), looked up per lane, since the lanes of a wavefront sit in different tiles.
// BF_COV_ROWS (mvdr_fast_rows_kernel, mvdr_fast_track_rows_kernel; lcmv only, KC >= 2): the whole solution gv[0 .. KC-1] of G y = g is stored, entry r
// = column r of W^H x = the beam that looks at constraint column r with nulls on the others, as row r of the stream's a.gss_rows rows
// (Yh = [stream][rows][frame][kYhStride]).  Rows past the columns in force are zero; behind a closed gate every row in force is 0.01 X_0
// (lcmv.cpp:121).  The arithmetic is the one-row kernel's: row 0 is its output bit for bit.  With BF_COV_ROWS 0 the preprocessor leaves the
// kernel's tokens as they were before the rows existed.
template <int MP, int KC, bool Z128>
__global__ __launch_bounds__(64, 1) void BF_COV_NAME(mvdr_fast)(BinsArgs a, FastPlan fp) {
    constexpr bool TRACK = BF_COV_TRACK;
#if BF_COV_ROWS
    constexpr int NR = KC;  // rows whose value lives in registers
#endif
    constexpr int NT = MP * (MP + 1) / 2;
    constexpr long kZB = Z128 ? (long)sizeof(f64x2) : (long)sizeof(z48);  // bytes per stored element
    const int lane = threadIdx.x;
    const int s = blockIdx.x / fp.waves_per_stream;  // output stream: uniform per wavefront
    const int id0 = (blockIdx.x - s * fp.waves_per_stream) * 64;
    int id = id0 + lane;
    const bool live = id < fp.tiles * fp.nb;
    if (!live) id = fp.tiles * fp.nb - 1;
    const int tl0 = id0 / fp.nb, tl = id / fp.nb;  // time tile of lane 0 / of this lane
    const int k = id - tl * fp.nb;
    const int q = k == 0 ? 0 : k <= fp.n_main ? fp.q_lo + k - 1 : fp.extra_q[k - 1 - fp.n_main];
    const bool solve_q = q != 0 || fp.solve0 != 0;
    const int j = q_bin(q);
    const long tA0 = (long)tl0 * fp.tile;          // first frame of lane 0's tile: the wavefront's time origin (uniform)
    const int dt = (tl - tl0) * fp.tile;           // this lane's tile starts dt frames later
    long n_it = a.n_frames - tA0;                  // frames the wavefront walks (lane 0 has the longest tile)
    if (n_it > fp.tile) n_it = fp.tile;
    long cnt = a.n_frames - (tA0 + dt);            // frames this lane owns
    if (cnt > fp.tile) cnt = fp.tile;
    if (!live) cnt = 0;
    const int M = a.n_mics, NP = (M + 1) >> 1, P = a.cfg.past_windows;
    // frame tA0 of this stream's packed spectra (uniform) + a 32-bit per-lane byte offset: SGPR base + VGPR offset addressing
    const char *Zu = reinterpret_cast<const char *>(a.Z) + ((long)(s / a.n_dirs) * a.frames_ws + a.frame_off + tA0) * NP * kN * kZB;
    const int ksrc = q_src_bin(q), kneg = (kN - ksrc) & (kN - 1);
    const unsigned vk = (unsigned)(((long)dt * NP * kN + ksrc) * kZB);
    const unsigned vn = (unsigned)(((long)dt * NP * kN + kneg) * kZB);
    const long frame_bytes = (long)NP * kN * kZB;
    const f64x2 *steer = a.steer + (long)(s % a.n_dirs) * a.steer_dir_stride + j;
#if BF_COV_ROWS
    const int n_rows = a.gss_rows;
    const long yidx = ((long)s * n_rows * a.n_frames + tA0 + dt) * kYhStride + q;
    // the frame's values into its rows -- the KC in registers, exact zeros behind them (rows past the kernel's columns)
    auto st_rows = [&](long idx, const cd (&yv)[NR]) {
        const long yrow = a.n_frames * kYhStride;
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (r < n_rows) st_y(a, idx + r * yrow, q, yv[r]);
        for (int r = NR; r < n_rows; ++r) st_y(a, idx + r * yrow, q, cd{0, 0});
    };
#else
    const long yidx = ((long)s * a.n_frames + tA0 + dt) * kYhStride + q;
#endif

    // Spectra are prefetched one frame ahead by global->LDS DMA (global_load_lds_dwordx3: no VGPRs; lane l's 12 bytes
    // land at row base + 16 l -- measured, tools/ubench/lds_dma_x3.hip -- so a row is 64 slots of 16 bytes): a wavefront
    // that owns its SIMD has nobody to hide HBM latency behind (PMC of the register-only version: 57 % of its cycles in
    // s_waitcnt).  Row 2p / 2p+1 = Z_t[p][k] / Z_t[p][N-k]; rows MP + 2p, MP + 2p + 1 = the same of frame t - P.
    struct alignas(16) z48slot {
        z48 v;
        unsigned pad;
    };
    __shared__ z48slot s_pf[2][2 * MP][64];
    auto dma_frame = [&](long i, bool with_old, int buf) {  // frame tA0 + i (+ dt per lane) into s_pf[buf]
        const char *bn = Zu + i * frame_bytes, *bo = Zu + (i - P) * frame_bytes;
#pragma unroll
        for (int p = 0; p < MP / 2; ++p) {
                const long po = (long)p * kN * kZB;
                lds_dma<Z128>(bn + po + vk, &s_pf[buf][2 * p][0]);
                lds_dma<Z128>(bn + po + vn, &s_pf[buf][2 * p + 1][0]);
                if (with_old) {
                    lds_dma<Z128>(bo + po + vk, &s_pf[buf][MP + 2 * p][0]);
                    lds_dma<Z128>(bo + po + vn, &s_pf[buf][MP + 2 * p + 1][0]);
                }
            }
    };
    auto unpack = [&](int buf, int base, cd (&X)[MP]) {  // microphone spectra out of the prefetched rows (z48 is stored halved)
#pragma unroll
        for (int p = 0; p < MP / 2; ++p) {
            cd z, c;  // Z[k] / 2 and Z[N-k] / 2 (stored halved: StftArgs::halve; the latter conjugated on the fly)
            if constexpr (Z128) {
                z = ld(reinterpret_cast<const f64x2 *>(&s_pf[buf][base + 2 * p][lane]));
                c = ld(reinterpret_cast<const f64x2 *>(&s_pf[buf][base + 2 * p + 1][lane]));
            } else {
                z = dec48(s_pf[buf][base + 2 * p][lane].v);
                c = dec48(s_pf[buf][base + 2 * p + 1][lane].v);
            }
            X[2 * p] = cd{z.x + c.x, z.y - c.y};      // (Z[k] + conj Z[N-k]) / 2
            X[2 * p + 1] = cd{z.y + c.y, c.x - z.x};  // (Z[k] - conj Z[N-k]) / (2i)
        }
        if (q == kQX) {  // the extra problem: bin N/2+1 holds the conjugate of bin N/2-1's spectrum
#pragma unroll
            for (int m = 0; m < MP; ++m) X[m].y = -X[m].y;
        }
    };
#define BF_DMA_WAIT() do { asm volatile("" ::: "memory"); __builtin_amdgcn_s_waitcnt(0x0F70); asm volatile("" ::: "memory"); } while (0)  /* vmcnt(0): the builtin, so that hipcc's own counter model sees the drain */
    // mvdr (KC == 1), round 6: the same 32 KB seen as FOUR half-buffers of MP rows -- a ring of three for the NEWEST frames, requested TWO frames
    // ahead, and one for the frame that leaves the window, requested one frame ahead (it used to travel two ahead and the newest one: the rows
    // fresh from the STFT kernel are the ones that come from HBM).  With the steering vector in registers the loop has no load that returns
    // to a register, so hipcc places no vector-memory wait of its own and the counted s_waitcnt vmcnt(MP) at the loop's top is the only one.
    // A tracked batch has no steering vector to keep: mvdr takes the path lcmv has always used (columns re-read per frame, below).
    constexpr bool DEEP = KC == 1 && !TRACK;
    auto hrow = [&](int h, int row) { return &s_pf[h >> 1][(h & 1) * MP + row][0]; };
    auto dma_rows = [&](const char *b, int h) {  // the MP rows of the frame at byte base b (+ dt per lane) into half-buffer h
#pragma unroll
        for (int p = 0; p < MP / 2; ++p) {
            const long po = (long)p * kN * kZB;
            lds_dma<Z128>(b + po + vk, hrow(h, 2 * p));
            lds_dma<Z128>(b + po + vn, hrow(h, 2 * p + 1));
        }
    };
    auto unpack_h = [&](int h, cd (&X)[MP]) { unpack(h >> 1, (h & 1) * MP, X); };

    cd R[NT];       // strict lower triangle, row-major: R[i*(i+1)/2 + c], c < i (the diagonal slots are unused)
    double Rd[MP];  // the diagonal is real: kept and updated as such (two FMAs per rank-1 term instead of four)
#pragma unroll
    for (int e = 0; e < NT; ++e) R[e] = cd{0, 0};
#pragma unroll
    for (int i = 0; i < MP; ++i) Rd[i] = 0.0;
    int pb = 0;  // buffer the next consumer reads
    // tracked: the table indices of the frame this lane solves next, one per constraint column, fetched one frame ahead.  The frame looked
    // up is clamped to the stream's last one (lanes past their cnt, the idle last iterations): nothing outside the track is ever read
    int ix[KC];
    const int tcols = TRACK ? a.track_cols : 0;
    auto trk_load = [&](long it, int (&o)[KC]) {
        long f = tA0 + dt + it;
        if (f > a.n_frames - 1) f = a.n_frames - 1;
        const int32_t *row = a.track + ((long)s * a.n_frames + f) * tcols;
#pragma unroll
        for (int c = 0; c < KC; ++c) o[c] = c < tcols ? row[c] : -1;
    };
    if constexpr (TRACK) trk_load(0, ix);
    else { (void)ix; (void)tcols; (void)trk_load; }
    cd Uk[MP];   // mvdr: the steering vector stays in registers for the whole tile (the factorisation scales its copy in place)
#pragma unroll
    for (int m = 0; m < MP; ++m) Uk[m] = (DEEP && m < M) ? ld(steer + (long)m * kN) : cd{0, 0};
    if constexpr (DEEP) {  // the tile's first two frames into ring slots 0 and 1; the warm-up below walks half-buffers 2 and 3
        dma_rows(Zu, 0);
        dma_rows(Zu + (n_it > 1 ? 1 : 0) * frame_bytes, 1);
        dma_rows(Zu - frame_bytes, 2);
    } else {
        dma_frame(-1, false, pb);
    }
    for (int p = 1; p <= P; ++p) {  // covariance of the P frames in front of the tile
        BF_DMA_WAIT();
        __builtin_amdgcn_wave_barrier();
        if constexpr (DEEP) {
            if (p < P) dma_rows(Zu - (long)(p + 1) * frame_bytes, 2 + (p & 1));
            cd X[MP];
            unpack_h(2 + ((p - 1) & 1), X);
#pragma unroll
            for (int i = 0; i < MP; ++i) {
#pragma unroll
                for (int c = 0; c < i; ++c) R[i * (i + 1) / 2 + c] = cfma_conj(R[i * (i + 1) / 2 + c], X[i], X[c]);
                Rd[i] = fma(X[i].y, X[i].y, fma(X[i].x, X[i].x, Rd[i]));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the half-buffer is rewritten two steps on)
            continue;
        }
        if (p < P)
            dma_frame(-p - 1, false, pb ^ 1);
        else
            dma_frame(0, true, pb ^ 1);  // first frame of the tile
        cd X[MP];
        unpack(pb, 0, X);
#pragma unroll
        for (int i = 0; i < MP; ++i) {
#pragma unroll
            for (int c = 0; c < i; ++c) R[i * (i + 1) / 2 + c] = cfma_conj(R[i * (i + 1) / 2 + c], X[i], X[c]);
            Rd[i] = fma(X[i].y, X[i].y, fma(X[i].x, X[i].x, Rd[i]));
        }
        pb ^= 1;
    }
    const float thr32 = (float)(a.cfg.freq_mag_threshold * (double)((unsigned)M * (unsigned)kN));
    cd y_prev{0, 0};  // frame it - 1's output: stored one iteration late, behind the next frame's DMA requests, so that no s_waitcnt vmcnt(0)
                      // of an iteration waits for a store issued a few instructions earlier
#if BF_COV_ROWS
    cd yr_prev[NR];   // the same, a value per row
#pragma unroll
    for (int r = 0; r < NR; ++r) yr_prev[r] = cd{0, 0};
#endif
    if constexpr (DEEP) BF_DMA_WAIT();  // (the steering vector and the ring's first two frames are there whatever P is: hipcc's model enters the loop with nothing pending)
    int sn = 0;  // DEEP: ring slot of frame it (it mod 3)
    for (long it = 0; it < n_it; ++it) {
        if constexpr (DEEP) {
            // frame it (requested two iterations ago) and frame it - 1 - P (one ago) have landed, frame it - 2's output has been stored; the MP
            // requests of frame it + 1 may still travel (vector loads return in order: at most MP outstanding = only those)
            if constexpr (MP == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if constexpr (MP == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else if constexpr (MP == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            BF_DMA_WAIT();  // frame it (and it - P) have landed in s_pf[pb]; frame it - 2's output has been stored
        }
        __builtin_amdgcn_wave_barrier();
        const int sp = sn == 0 ? 2 : sn - 1;  // DEEP: slot of frame it - 1 = the slot frame it + 2 goes into
        // The constraint columns: re-read per frame (L2-resident, consecutive lanes = consecutive bins) instead of living in registers
        // that the factorisation needs.  Requested HERE, in front of the slide that covers their L2 round trip, and drained (vmcnt(0),
        // the builtin: hipcc's counter model sees it) in front of the next frame's DMA: hipcc prices any vector-memory wait with an
        // LDS-DMA request in flight at vmcnt(0), so until round 6 -- DMA first, then these loads -- the factorisation's first use of U
        // waited for the rows requested a few hundred instructions earlier (SQ_WAIT_ANY 17 % of the wave cycles).
        cd U[KC][MP];
#pragma unroll
        for (int c = 0; c < KC; ++c)
#pragma unroll
            for (int m = 0; m < MP; ++m) {
                if constexpr (DEEP) {
                    U[c][m] = Uk[m];
                } else if constexpr (TRACK) {
                    // an index that names a table: that angle's column; any other: the handle's own column c.  Microphone 0's entry is
                    // always the handle's own (quirk Q3: 1 after create, 0 after a structural interferer change)
                    const f64x2 *own = steer + (long)c * M * kN;
                    const f64x2 *col = (unsigned)ix[c] < (unsigned)a.track_n ? a.track_tables + (long)ix[c] * a.track_stride + j : own;
                    U[c][m] = (m < M && c < a.kp1) ? ld(m == 0 ? own : col + (long)m * kN) : cd{0, 0};
                } else {
                    U[c][m] = (m < M && c < a.kp1) ? ld(steer + ((long)c * M + m) * kN) : cd{0, 0};
                }
            }
        if constexpr (TRACK) trk_load(it + 1, ix);  // behind this frame's column requests; drained with them in front of the next DMA
        cd(&ua)[MP] = U[0];
        __builtin_amdgcn_sched_barrier(0);
        if (it > 0) {
            // slide the covariance window over the PREVIOUS frame (mvdr.cpp:100-101), whose rows still sit in the other buffer:
            // done here, not behind the solve, so that the updated R is at once the factorisation's working copy -- R itself
            // then rests (in the accumulator half of the register file) while the solve has the 256 arithmetic registers
            cd Xn[MP], Xo[MP];
#pragma unroll
            for (int m = 0; m < MP; ++m)  // parked by the previous iteration
                Xn[m] = ld(reinterpret_cast<const f64x2 *>(DEEP ? reinterpret_cast<z48slot *>(hrow(sp, m)) + lane : &s_pf[pb ^ 1][m][lane]));
            if constexpr (DEEP) unpack_h(3, Xo);
            else unpack(pb ^ 1, MP, Xo);
#pragma unroll
            for (int i = 0; i < MP; ++i) {
#pragma unroll
                for (int c = 0; c < i; ++c)
                    R[i * (i + 1) / 2 + c] = cfms_conj(cfma_conj(R[i * (i + 1) / 2 + c], Xn[i], Xn[c]), Xo[i], Xo[c]);
                Rd[i] = fma(-Xo[i].y, Xo[i].y, fma(-Xo[i].x, Xo[i].x, fma(Xn[i].y, Xn[i].y, fma(Xn[i].x, Xn[i].x, Rd[i]))));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the rows have been read: the next DMA may overwrite them
        }
        // the next frame's rows: requested on every path (the last iteration re-requests its own frame into the idle buffer), with
        // nothing older in flight; the previous frame's output goes out behind them (the wait at the top of the loop covers it)
        if constexpr (DEEP) {
            // the frame that leaves the window at the NEXT slide, the previous frame's output, then frame it + 2 into the slot the slide has just
            // emptied -- in this order: the next top-of-loop wait lets exactly the youngest MP requests stand
            __builtin_amdgcn_sched_barrier(0);
            dma_rows(Zu + (it - P) * frame_bytes, 3);
#if BF_COV_ROWS
            if (it > 0 && it - 1 < cnt) st_rows(yidx + (it - 1) * kYhStride, yr_prev);
#else
            if (it > 0 && it - 1 < cnt) st_y(a, yidx + (it - 1) * kYhStride, q, y_prev);
#endif
            dma_rows(Zu + (it + 2 < n_it ? it + 2 : n_it - 1) * frame_bytes, sp);
            __builtin_amdgcn_sched_barrier(0);
        } else {
            BF_DMA_WAIT();
            __builtin_amdgcn_sched_barrier(0);
            dma_frame(it + 1 < n_it ? it + 1 : it, true, pb ^ 1);
#if BF_COV_ROWS
            if (it > 0 && it - 1 < cnt) st_rows(yidx + (it - 1) * kYhStride, yr_prev);
#else
            if (it > 0 && it - 1 < cnt) st_y(a, yidx + (it - 1) * kYhStride, q, y_prev);
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
        cd X[MP];
        if constexpr (DEEP) unpack_h(sn, X);
        else unpack(pb, 0, X);
        // park the unpacked spectra in the slots their packed form came from (a 16-byte slot holds one complex double): the
        // next iteration's slide reads them back with one LDS read each instead of unpacking the frame again
#pragma unroll
        for (int m = 0; m < MP; ++m)
            *reinterpret_cast<f64x2 *>(DEEP ? reinterpret_cast<z48slot *>(hrow(sn, m)) + lane : &s_pf[pb][m][lane]) = f64x2{X[m].x, X[m].y};
        // magnitude gate (mvdr.cpp:85,95): sum |X_m| / (M N) > threshold.  Decided in fp32 unless the fp32 sum is within 1e-4
        // of the threshold (its own error is < 1e-6): then, for that wavefront and frame, in the reference's double arithmetic.
        float m32 = 0.f;  // (a zero partner channel of an odd microphone count adds its ~1e-16 |X| rounding residue: irrelevant here)
#pragma unroll
        for (int m = 0; m < MP; ++m) m32 += __builtin_amdgcn_sqrtf((float)norm2(X[m]));
        bool open = m32 > thr32;
        if (__builtin_amdgcn_ballot_w64(__builtin_fabsf(m32 - thr32) <= 1e-4f * thr32) != 0) {
            double mag = 0.0;
#pragma unroll
            for (int m = 0; m < MP; ++m)
                if (m < M) mag += fast_sqrt(norm2(X[m]));  // |X| well inside double range: no hypot scaling needed
            mag /= (double)((unsigned)M * (unsigned)kN);
            open = mag > a.cfg.freq_mag_threshold;
        }
        cd y = X[0] * 0.01;  // gate closed: mvdr.cpp:96
        if (q == 0 && !fp.solve0) y = a.cfg.algo == BF_LCMV ? cd{0, 0} : X[0];  // mvdr.cpp:76; lcmv has no such rule: problem 0 out of band reads as zero
#if BF_COV_ROWS
        cd yr[NR];  // what a closed gate or an out-of-band problem 0 leaves on every row in force
#pragma unroll
        for (int r = 0; r < NR; ++r) yr[r] = r < a.kp1 ? y : cd{0, 0};
#endif
        if (__builtin_amdgcn_ballot_w64(open && solve_q) != 0) {
            cd A[NT];
#pragma unroll
            for (int i = 0; i < MP; ++i) {
#pragma unroll
                for (int c = 0; c < i; ++c) A[i * (i + 1) / 2 + c] = R[i * (i + 1) / 2 + c];
                A[i * (i + 1) / 2 + i] = cd{(i < M) ? Rd[i] * 1.001 : 1.0, 0.0};  // whiteR diagonal (mvdr.cpp:239-243); padding = identity
            }
#pragma unroll
            for (int jj = 0; jj < MP; ++jj) {
                const double inv = fast_rsqrt1(A[jj * (jj + 1) / 2 + jj].x);  // 1/L_jj; L_jj itself is never needed
#pragma unroll
                for (int c = 0; c < KC; ++c) U[c][jj] = U[c][jj] * inv;
                X[jj] = X[jj] * inv;  // X turns into v = L^-1 x in place
#pragma unroll
                for (int i = jj + 1; i < MP; ++i) {
                    const cd Lij = A[i * (i + 1) / 2 + jj] * inv;
                    A[i * (i + 1) / 2 + jj] = Lij;
#pragma unroll
                    for (int c = 0; c < KC; ++c) U[c][i] = cfms(U[c][i], Lij, U[c][jj]);
                    X[i] = cfms(X[i], Lij, X[jj]);
                }
#pragma unroll
                for (int c = jj + 1; c < MP; ++c) {
                    const cd Lc = A[c * (c + 1) / 2 + jj];
#pragma unroll
                    for (int i = c; i < MP; ++i) {
                        if (i == c)  // diagonal: only the real part is ever read
                            A[i * (i + 1) / 2 + c].x = fma(-Lc.y, Lc.y, fma(-Lc.x, Lc.x, A[i * (i + 1) / 2 + c].x));
                        else
                            A[i * (i + 1) / 2 + c] = cfms_conj(A[i * (i + 1) / 2 + c], A[i * (i + 1) / 2 + jj], Lc);
                    }
                }
            }
            if constexpr (KC == 1) {
                cd num{0, 0};
                double den = 0.0;
#pragma unroll
                for (int i = 0; i < MP; ++i) {
                    num = cfma_conj(num, X[i], ua[i]);
                    den += norm2(ua[i]);
                }
                const double rden = fast_rcp(den);
                if (open && solve_q) y = cd{num.x * rden, num.y * rden};
            } else {
                // G (Hermitian, upper triangle row-major) and g, then the KC x KC system by elimination (as cov2d_kernel)
                auto UI = [](int r, int c) { return r * KC - r * (r - 1) / 2 + (c - r); };
                cd ge[KC * (KC + 1) / 2], gv[KC];
#pragma unroll
                for (int r1 = 0; r1 < KC; ++r1) {
#pragma unroll
                    for (int r2 = r1; r2 < KC; ++r2) {
                        cd acc{0, 0};
#pragma unroll
                        for (int i = 0; i < MP; ++i) acc = cfma_conj(acc, U[r2][i], U[r1][i]);
                        ge[UI(r1, r2)] = acc;
                    }
                    cd acc{0, 0};
#pragma unroll
                    for (int i = 0; i < MP; ++i) acc = cfma_conj(acc, X[i], U[r1][i]);
                    gv[r1] = acc;
                }
#pragma unroll
                for (int r1 = 0; r1 < KC; ++r1)
                    if (r1 >= a.kp1) {
#pragma unroll
                        for (int r2 = 0; r2 < r1; ++r2) ge[UI(r2, r1)] = cd{0, 0};
                        ge[UI(r1, r1)] = cd{1.0, 0.0};
#pragma unroll
                        for (int c = r1 + 1; c < KC; ++c) ge[UI(r1, c)] = cd{0, 0};
                        gv[r1] = cd{0, 0};
                    }
                cd pinvs[KC];
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const cd pinv = crcp(ge[UI(k, k)]);
                    pinvs[k] = pinv;
#pragma unroll
                    for (int r1 = k + 1; r1 < KC; ++r1) {
                        const cd fct = conj(ge[UI(k, r1)]) * pinv;
#pragma unroll
                        for (int c = r1; c < KC; ++c) ge[UI(r1, c)] = ge[UI(r1, c)] - fct * ge[UI(k, c)];
                        gv[r1] = gv[r1] - fct * gv[k];
                    }
                }
#pragma unroll
                for (int k = KC - 1; k >= 0; --k) {
                    cd acc = gv[k];
#pragma unroll
                    for (int c = k + 1; c < KC; ++c) acc = acc - ge[UI(k, c)] * gv[c];
                    gv[k] = acc * pinvs[k];
                }
                if (open && solve_q) y = gv[0];
#if BF_COV_ROWS
                if (open && solve_q) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) yr[r] = r < a.kp1 ? gv[r] : cd{0, 0};
                }
#endif
            }
        }
        y_prev = y;
#if BF_COV_ROWS
#pragma unroll
        for (int r = 0; r < NR; ++r) yr_prev[r] = yr[r];
#endif
        pb ^= 1;
        sn = sn == 2 ? 0 : sn + 1;
    }
    BF_DMA_WAIT();  // (the last iterations' idle requests)
#if BF_COV_ROWS
    if (n_it > 0 && n_it - 1 < cnt) st_rows(yidx + (n_it - 1) * kYhStride, yr_prev);
#else
    if (n_it > 0 && n_it - 1 < cnt) st_y(a, yidx + (n_it - 1) * kYhStride, q, y_prev);
#endif
#undef BF_DMA_WAIT
}

#if !BF_COV_ROWS

// TRACK (mvdr_lcmv_track_kernel): a column-tracked batch -- cst[] is reloaded at every frame from the tables the frame's track entries name
// (the rule of the lane kernel above).  Correct, not tuned: the entries are read where they are used.
// Rows (lcmv_out_beams; a.gss_rows > 1, lcmv only): entry r of the solution of G y = g goes to row r of the stream's rows, as the lane kernel's
// twins have it -- counted at run time here: with one row the loop runs once over today's value.
template <int MP, int KM>
__global__ __launch_bounds__(256) void BF_COV_NAME(mvdr_lcmv)(BinsArgs a, int tile, int tiles_per_stream) {
    constexpr bool TRACK = BF_COV_TRACK;
    constexpr int GPB = 256 / MP;          // problem groups per block
    constexpr int NB = KM + 1;             // right-hand sides: constraints + current frame
    constexpr int NE = GramIdx<KM>::NE;
    // +1 element of padding per row: the groups of a wavefront read the same [row][k] at the same time (broadcast
    // inside a group), and with a group stride that is a multiple of 128 B all of them would hit the same 4 banks
    // (PMC before the padding: SQ_LDS_BANK_CONFLICT = 1.7x SQ_ACTIVE_INST_LDS; lcmv 16-mic 37.5 -> 34.0 ms)
    __shared__ cd s_col[GPB][MP + 1];
    __shared__ cd s_x[GPB][MP + 1];
    __shared__ cd s_xo[GPB][MP + 1];
    __shared__ cd s_u[GPB][NB][MP + 1];
    __shared__ cd s_e[GPB][NE + 1];

    const int grp = threadIdx.x / MP;
    const int i = threadIdx.x % MP;
    const int q = blockIdx.y * GPB + grp;
    if (q >= kNQ) return;
    const int s = blockIdx.x / tiles_per_stream;
    const long tA = (long)(blockIdx.x % tiles_per_stream) * tile;
    long tB = tA + tile;
    if (tB > a.n_frames) tB = a.n_frames;
    const int M = a.n_mics, NP = (M + 1) >> 1, KP1 = a.kp1, P = a.cfg.past_windows;
    const int j = q_bin(q);
    const bool lcmv = a.cfg.algo == BF_LCMV;
    const int n_rows = a.gss_rows;
    const long yidx = ((long)s * n_rows * a.n_frames) * kYhStride + q, yrow = a.n_frames * kYhStride;
    const long z0 = ((long)(s / a.n_dirs) * a.frames_ws + a.frame_off) * NP * kN;  // element index of frame 0 of this batch
    const f64x2 *steer = a.steer + (long)(s % a.n_dirs) * a.steer_dir_stride;

    // one microphone's spectrum at this problem's bin, frame t (may be negative: history); z48 elements (stored halved) or,
    // (the default) full doubles; stored halved either way
    const int ksrc = q_src_bin(q), kneg = (kN - ksrc) & (kN - 1);
    auto ldz = [&](long e) -> cd { return a.z48 ? ld(reinterpret_cast<const z48 *>(a.Z) + e) : ld(a.Z + e); };  // (either way stored halved)
    auto load_xi = [&](long t) -> cd {
        if (i >= M) return cd{0, 0};
        const long ef = z0 + t * NP * kN + (long)(i >> 1) * kN;
        const cd z = ldz(ef + ksrc), zc = conj(ldz(ef + kneg));
        cd x;
        if ((i & 1) == 0) {
            x = z + zc;  // z48 spectra are stored halved
        } else {
            const cd d = z - zc;
            x = cd{d.y, -d.x};
        }
        return q == kQX ? conj(x) : x;
    };

    const double f = fabs(a.freqs[j]);
    const bool inband = f >= a.cfg.freq_min && f <= a.cfg.freq_max;
    if (!inband || (!lcmv && j == 0)) {
        // mvdr.cpp:76 y_fft[0] = in_fft(0,0); out of band: y_fft[j] = 0 (mvdr.cpp:103)
        for (long t = tA; t < tB; ++t) {
            cd y{0, 0};
            if (!lcmv && j == 0) {
                const cd x = load_xi(t);
                s_x[grp][i] = x;
                __builtin_amdgcn_wave_barrier();
                y = s_x[grp][0];
                __builtin_amdgcn_wave_barrier();
            }
            if (i == 0)
                for (int r = 0; r < n_rows; ++r) st_y(a, yidx + r * yrow + t * kYhStride, q, y);  // (more than one row: lcmv, y = 0)
        }
        return;
    }

    cd cst[KM];  // this mic's entries of the constraint columns (weights[j](i, r))
#pragma unroll
    for (int r = 0; r < KM; ++r)
        cst[r] = (r < KP1 && i < M) ? ld(steer + ((long)r * M + i) * kN + j) : cd{0, 0};

    // R row i (lower triangle c <= i is what the factorisation reads)
    cd R[MP];
#pragma unroll
    for (int c = 0; c < MP; ++c) R[c] = cd{0, 0};
    for (int p = 1; p <= P; ++p) {
        const cd x = load_xi(tA - p);
        s_x[grp][i] = x;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < MP; ++c) R[c] = cfma_conj(R[c], x, s_x[grp][c]);
        __builtin_amdgcn_wave_barrier();
    }

    for (long t = tA; t < tB; ++t) {
        if constexpr (TRACK) {
            const int32_t *row = a.track + ((long)s * a.n_frames + t) * a.track_cols;
#pragma unroll
            for (int r = 0; r < KM; ++r) {
                cst[r] = cd{0, 0};
                if (r < KP1 && i < M) {
                    const int ix = r < a.track_cols ? row[r] : -1;
                    const f64x2 *own = steer + (long)r * M * kN + j;
                    const f64x2 *col = (unsigned)ix < (unsigned)a.track_n ? a.track_tables + (long)ix * a.track_stride + j : own;
                    cst[r] = ld(i == 0 ? own : col + (long)i * kN);  // microphone 0: always the handle's own entry (quirk Q3)
                }
            }
        }
        const cd x = load_xi(t);
        const cd xo = load_xi(t - P);
        s_x[grp][i] = x;
        s_xo[grp][i] = xo;
        __builtin_amdgcn_wave_barrier();
        double mag = 0.0;
        for (int m = 0; m < M; ++m) mag += fast_sqrt(norm2(s_x[grp][m]));
        mag /= (double)((unsigned)M * (unsigned)kN);
        cd y;
        if (mag > a.cfg.freq_mag_threshold) {
            cd A[MP], b[NB];
#pragma unroll
            for (int c = 0; c < MP; ++c) A[c] = R[c];
            if (i < M) {
                // cwiseProduct(whiteR): diagonal * 1.001 (mvdr.cpp:239-243)
#pragma unroll
                for (int c = 0; c < MP; ++c)
                    if (c == i) A[c] = A[c] * 1.001;
            } else {
#pragma unroll
                for (int c = 0; c < MP; ++c) A[c] = cd{c == i ? 1.0 : 0.0, 0.0};
            }
#pragma unroll
            for (int r = 0; r < KM; ++r) b[r] = cst[r];
            b[KM] = x;
#pragma unroll
            for (int jj = 0; jj < MP; ++jj) {
                s_col[grp][i] = A[jj];  // raw column jj, row i
                if (i == jj) {
#pragma unroll
                    for (int r = 0; r < NB; ++r) s_u[grp][r][0] = b[r];
                }
                __builtin_amdgcn_wave_barrier();
                const double inv = fast_rsqrt1(s_col[grp][jj].x);  // 1 / L_jj
                const cd Lij = A[jj] * inv;
                if (i > jj) {
#pragma unroll
                    for (int c = jj + 1; c < MP; ++c)
                        if (c <= i) A[c] = cfms_conj(A[c], Lij, s_col[grp][c] * inv);
#pragma unroll
                    for (int r = 0; r < NB; ++r) b[r] = cfms(b[r], Lij, s_u[grp][r][0] * inv);
                } else if (i == jj) {
#pragma unroll
                    for (int r = 0; r < NB; ++r) b[r] = b[r] * inv;
                }
                __builtin_amdgcn_wave_barrier();
            }
            // b[r] is now row i of U = L^-1 [C | x]
#pragma unroll
            for (int r = 0; r < NB; ++r) s_u[grp][r][i] = (i < M) ? b[r] : cd{0, 0};
            __builtin_amdgcn_wave_barrier();
            // Gram entries: e < NG: G(r,r2) with r <= r2; e >= NG: g(r)
            for (int e = i; e < NE; e += MP) {
                int r = 0, r2 = 0;
                if (e < GramIdx<KM>::NG) {
                    int rem = e;
                    while (rem >= KM - r) { rem -= KM - r; ++r; }
                    r2 = r + rem;
                } else {
                    r = e - GramIdx<KM>::NG;
                    r2 = KM;
                }
                cd acc{0, 0};
                for (int m = 0; m < M; ++m) acc = cfma_conj(acc, s_u[grp][r2][m], s_u[grp][r][m]);
                s_e[grp][e] = acc;
            }
            __builtin_amdgcn_wave_barrier();
            // every lane solves the (KP1 x KP1) system G y = g redundantly; padding rows are identity
            cd Gm[KM][KM], gv[KM];
            {
                int e = 0;
#pragma unroll
                for (int r = 0; r < KM; ++r)
#pragma unroll
                    for (int r2 = r; r2 < KM; ++r2) {
                        const cd v = s_e[grp][e++];
                        Gm[r][r2] = v;
                        Gm[r2][r] = conj(v);
                    }
#pragma unroll
                for (int r = 0; r < KM; ++r) gv[r] = s_e[grp][GramIdx<KM>::NG + r];
#pragma unroll
                for (int r = 0; r < KM; ++r)
                    if (r >= KP1) {
#pragma unroll
                        for (int r2 = 0; r2 < KM; ++r2) {
                            Gm[r][r2] = cd{r == r2 ? 1.0 : 0.0, 0.0};
                            Gm[r2][r] = cd{r == r2 ? 1.0 : 0.0, 0.0};
                        }
                        gv[r] = cd{0, 0};
                    }
            }
            cd pinvs[KM];  // reciprocals of the pivots: formed once, used by the elimination and by the back substitution
#pragma unroll
            for (int k = 0; k < KM; ++k) {  // Gaussian elimination (G is Hermitian positive definite)
                const cd pinv = crcp(Gm[k][k]);
                pinvs[k] = pinv;
#pragma unroll
                for (int r = k + 1; r < KM; ++r) {
                    const cd fct = Gm[r][k] * pinv;
#pragma unroll
                    for (int c = k + 1; c < KM; ++c) Gm[r][c] = Gm[r][c] - fct * Gm[k][c];
                    gv[r] = gv[r] - fct * gv[k];
                }
            }
#pragma unroll
            for (int k = KM - 1; k >= 0; --k) {
                cd acc = gv[k];
#pragma unroll
                for (int c = k + 1; c < KM; ++c) acc = acc - Gm[k][c] * gv[c];
                gv[k] = acc * pinvs[k];
            }
            y = gv[0];
            if (i == 0) {  // the other beams: entry r looks at column r; rows past the columns in force are zero
#pragma unroll
                for (int r = 1; r < KM; ++r)
                    if (r < n_rows) st_y(a, yidx + r * yrow + t * kYhStride, q, r < KP1 ? gv[r] : cd{0, 0});
                for (int r = KM; r < n_rows; ++r) st_y(a, yidx + r * yrow + t * kYhStride, q, cd{0, 0});
            }
        } else {
            y = s_x[grp][0] * 0.01;  // in_fft(0,j)*0.01 (mvdr.cpp:96), on every row in force (lcmv.cpp:121)
            if (i == 0)
                for (int r = 1; r < n_rows; ++r) st_y(a, yidx + r * yrow + t * kYhStride, q, r < KP1 ? y : cd{0, 0});
        }
        if (i == 0) st_y(a, yidx + t * kYhStride, q, y);
        // slide the covariance window: + x_t x_t^H - x_{t-P} x_{t-P}^H (mvdr.cpp:100-101)
#pragma unroll
        for (int c = 0; c < MP; ++c) R[c] = cfms_conj(cfma_conj(R[c], x, s_x[grp][c]), xo, s_xo[grp][c]);
        __builtin_amdgcn_wave_barrier();
    }
}
#endif  // !BF_COV_ROWS
