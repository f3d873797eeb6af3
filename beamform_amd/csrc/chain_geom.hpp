// chain_geom.hpp -- the launch geometry of one batch of the STFT -> per-bin -> ISTFT chain, beside its ChainPlan (chain_plan.hpp): how the
// batch is cut into runs, tiles and rounds, every grid, and every integer a kernel decodes its work from.  Plain C++ and pure: values in,
// values out, no HIP header.  BinPipelineImpl::run_chain (pipeline.hip) decides it once per batch, right behind chain_decide, and the
// launchers (pipeline_kernels.hpp) only read it (ChainPlan::geom); the CPU suite checks it through tests/host_emul (tests/test_chain_geom_cpu.py).
// Next to each scheme stands the formula by which its kernel turns an item index into (stream, first frame, count), as a plain function
// of the same arithmetic (chain_*_item): the kernels keep their own code, the tests walk these.
// A value that does not fit what it is narrowed to -- an `int` kernel argument, grid.x <= 2^31 - 1, grid.y <= 65 535 -- makes the whole
// geometry invalid (ChainGeom::ok): run_chain refuses such a batch before its first launch.
#pragma once

#include <climits>
#include <cmath>
#include <cstddef>
#include <vector>

#include "chain_plan.hpp"
#include "geometry.hpp"

namespace bf {

// problem index -> FFT bin, on the host (the kernels' q_bin, bins_common.hpp)
inline int q_bin_host(int q) { return q; }

// ---- the band of a handle: one scan, at init ---------------------------------------------------------------------------------------------
// The problems that need a solve: 0, the in-band run inside 1 .. N/2-1, and N/2 / N/2+1 when in band (the irregular problems of quirk Q1,
// util.h:190-199: f[N/2] = 0, f[N/2+1] = -(N/2-1) sr/N).  Everything the host derives from the band comes from this one enumeration, so
// the rows the backward transform reads (yh_lo / yh_hi) and the rows mvdr_fast_kernel writes (q_lo ... nb, FastPlan) cannot disagree.
struct BandPlan {
    int skip_lo, skip_hi;  // StftArgs::skip_lo / skip_hi (N, 0 = store everything)
    int yh_lo, yh_hi;      // ChainShape::band_yh_lo / band_yh_hi (every problem unless mvdr / lcmv; (1, 0): an empty band, only problem 0)
    int q_lo, n_main;      // FastPlan's members of these names
    int n_extra;
    int extra_q[2];
    int solve0;
    int nb;
    bool ok;               // false: an in-band problem behind the run (cannot happen: |f| rises with q below N/2)
};

inline BandPlan band_plan(int n_fft, double sample_rate, double freq_min, double freq_max, int algo) {
    const int N = n_fft, NQ = N / 2 + 2;
    const bool cov = algo == BF_MVDR || algo == BF_LCMV, band_node = cov || algo == BF_GSS;
    BandPlan b{};
    b.skip_lo = N; b.skip_hi = 0; b.yh_lo = 0; b.yh_hi = NQ - 1; b.ok = true;
    if (!band_node) return b;  // only the bins inside [freq_min, freq_max] are processed by mvdr / lcmv / gss
    const std::vector<double> fr = frequency_vector(N, sample_rate);  // the table the kernels read (BinsArgs::freqs)
    auto inb = [&](int q) {
        const double f = std::fabs(fr[q_bin_host(q)]);
        return f >= freq_min && f <= freq_max;
    };
    b.q_lo = 1;
    while (b.q_lo < N / 2 && !inb(b.q_lo)) ++b.q_lo;
    b.n_main = 0;
    while (b.q_lo + b.n_main < N / 2 && inb(b.q_lo + b.n_main)) ++b.n_main;
    for (int q = b.q_lo + b.n_main; q < N / 2; ++q)
        if (cov && inb(q)) b.ok = false;  // (gss never depended on it: only mvdr_fast_kernel enumerates the run)
    b.n_extra = 0;
    b.extra_q[0] = b.extra_q[1] = 0;
    if (inb(N / 2)) b.extra_q[b.n_extra++] = N / 2;          // f[N/2] := 0 (quirk Q1): in band when 0 Hz is
    if (inb(N / 2 + 1)) b.extra_q[b.n_extra++] = N / 2 + 1;  // the conjugate problem
    b.solve0 = (algo == BF_LCMV && inb(0)) ? 1 : 0;          // (mvdr passes X_0 through, mvdr.cpp:76)
    b.nb = 1 + b.n_main + b.n_extra;
    // the lowest and the highest in-band problem past 0 (problem q = bin q for q <= N/2 + 1)
    const int klo = b.n_main ? b.q_lo : b.n_extra ? b.extra_q[0] : N;
    const int khi = b.n_extra ? b.extra_q[b.n_extra - 1] : b.n_main ? b.q_lo + b.n_main - 1 : 0;
    // the STFT stores everything except, for the band-limited nodes, the bins between the highest in-band bin k and its mirror N-k
    // (quirk Q1 makes bins 511..513 irregular: only skip when the band ends below them)
    if (khi < N / 2 - 2) { b.skip_lo = khi; b.skip_hi = N - khi; }
    // mvdr / lcmv rows in front of a backward transform: only problem 0 and the band's problems exist (everything else is zero,
    // mvdr.cpp:103, and is neither written nor read)
    if (cov && khi < N / 2 - 1 && klo <= khi) { b.yh_lo = klo; b.yh_hi = khi; }
    else if (cov && klo > khi) { b.yh_lo = 1; b.yh_hi = 0; }  // empty band: only problem 0
    return b;
}

// Narrowing with a verdict: a value outside its range clears `ok`
struct GeomFit {
    bool ok = true;
    int i(long v) { if (v < 0 || v > INT_MAX) ok = false; return (int)v; }
    unsigned gx(long v) { if (v < 1 || v > 2147483647L) ok = false; return (unsigned)v; }
    unsigned gy(long v) { if (v < 1 || v > 65535L) ok = false; return (unsigned)v; }
};

// ---- STFT runs (also the front of the DOA maps, doa.cpp) -----------------------------------------------------------------------------------
// A half-wavefront (kStft, kStftSmall: 8 per block) or a wavefront (kStftWave2048: 4 per block) owns (stream, microphone pair, run of
// run_len consecutive frames); kStftGeneric: a block per (stream, frame, pair), grid-strided.
inline StftGeom chain_stft_geom(ChainFront front, int n_fft, int n_streams, long n_frames, int n_fft_mics, int n_cus) {
    const long np = (n_fft_mics + 1) / 2;
    GeomFit fit;
    StftGeom g{};
    g.run_len = 1;
    if (front == ChainFront::kStft) {
        // 256 threads, twiddles in LDS: a 512-thread block spills (44 VGPRs) and twiddles read from global memory cost 40 % (measured)
        constexpr int halves = 256 / 32;
        // frames per run: one run per half-wavefront slot (one block per CU) when the batch is long enough -- the first frame of a
        // run fetches its leading hop a second time (1/run_len of the input)
        const long slots = (long)n_cus * halves;  // (1 / 2 / 4 / 8 runs per slot measured: 0.713 / 0.720 / 0.732 / 0.739 ms)
        long L = ((long)n_streams * n_frames * np + slots - 1) / slots;
        if (L < 1) L = 1;
        if (L > 256) L = 256;
        g.run_len = (int)L;
        const long total = (long)n_streams * ((n_frames + L - 1) / L) * np;
        long blocks = (total + halves - 1) / halves;
        const long cap = (long)n_cus * 4;
        if (blocks > cap) blocks = cap;
        g.blocks = fit.gx(blocks);
    } else if (front == ChainFront::kStftSmall) {  // the in-register kernel
        constexpr int halves = 8;
        const int kG = 1024 / n_fft;                  // frames per group: 32 / (N / 32)
        const long slots = (long)n_cus * halves * 2;  // two rounds of runs per half-wavefront slot
        long L = ((long)n_streams * n_frames * np + slots - 1) / slots;
        L = ((L + kG - 1) / kG) * kG;  // whole groups of frames
        if (L > 256) L = 256;
        if (L < kG) L = kG;
        g.run_len = (int)L;
        const long items = (long)n_streams * ((n_frames + L - 1) / L) * np;
        long blocks = (items + halves - 1) / halves;
        if (blocks > (long)n_cus * 4) blocks = (long)n_cus * 4;
        g.blocks = fit.gx(blocks);
    } else if (front == ChainFront::kStftWave2048) {  // one 2048-point transform per full wavefront
        constexpr int waves = 4;
        const long slots = (long)n_cus * waves * 2;
        long L = ((long)n_streams * n_frames * np + slots - 1) / slots;
        if (L > 256) L = 256;
        if (L < 1) L = 1;
        g.run_len = (int)L;
        const long items = (long)n_streams * ((n_frames + L - 1) / L) * np;
        long blocks = (items + waves - 1) / waves;
        if (blocks > (long)n_cus * 4) blocks = (long)n_cus * 4;
        g.blocks = fit.gx(blocks);
    } else {  // kStftGeneric
        const long total = (long)n_streams * n_frames * np;
        long blocks = total < (long)n_cus * 8 ? total : (long)n_cus * 8;
        if (blocks < 1) blocks = 1;
        g.blocks = fit.gx(blocks);
    }
    g.ok = fit.ok;
    return g;
}

// ---- item index -> work, as the kernels decode it ------------------------------------------------------------------------------------------
struct ChainItem {
    long stream, t0, n;  // n <= 0: an item its kernel's own guard drops
    long sub;            // the microphone pair (STFT), the problem slot k (mvdr_fast), 0 otherwise
};
// stft_kernel / stft_small_kernel / stft_wave2048_kernel (L = run_len), stft_generic_kernel (L = 1): items 0 .. n_streams * runs * np - 1,
// pair fastest, then the run, then the stream; runs = ceil(n_frames / L)
inline ChainItem chain_stft_item(long item, long n_frames, long L, long np) {
    const long runs = (n_frames + L - 1) / L;
    const long p = item % np, sr = item / np, run = sr % runs, s = sr / runs;
    long te = (run + 1) * L;
    if (te > n_frames) te = n_frames;
    return ChainItem{s, run * L, te - run * L, p};
}
// Runs numbered stream * runs_per_stream + run, `per_run` frames each: the fused fronts' rounds (per_run = fpr, runs_per_stream = rps),
// istft32_kernel's chunks, istft_small_kernel / istft_split_kernel (runs_per_stream = ceil(n_frames / L)), the group kernels' tiles
// (mvdr_lcmv_kernel: blockIdx.x; cov2d_kernel: its unit).  An item whose stream is >= n_streams (a grid rounded up) is dropped by the kernel
inline ChainItem chain_run_item(long item, long n_frames, long per_run, long runs_per_stream) {
    const long s = item / runs_per_stream, t0 = (item - s * runs_per_stream) * per_run;
    long t1 = t0 + per_run;
    if (t1 > n_frames) t1 = n_frames;
    return ChainItem{s, t0, t1 - t0, 0};
}
// istft_w64_kernel: runs of pairs_per_run frame pairs; in (stream, pair) units -- the last pair of an odd stream holds one frame
inline ChainItem chain_w64_item(long run, long n_frames, long pairs_per_run, long runs_per_stream) {
    return chain_run_item(run, (n_frames + 1) / 2, pairs_per_run, runs_per_stream);
}
// cov2d_kernel: block -> (unit = (stream, tile), problem group); units x, x + 8, ... belong to XCD x
inline void chain_cov2d_block(long block, int n_fft, long *unit, int *group) {
    const int n_grp = (n_fft / 2 + 2 + 15) / 16;
    *unit = (long)((int)(block >> 3) / n_grp * 8 + (int)(block & 7));
    *group = (int)(block >> 3) % n_grp;
}
// mvdr_fast_kernel: (block, lane) -> stream, problem slot k (sub), first frame and frames owned; *tA0 / *dt / *n_it: the wavefront's time
// origin, this lane's offset from it and the frames the wavefront walks -- lane `lane` prefetches frames tA0 + dt .. tA0 + dt + n_it - 1
inline ChainItem chain_fast_lane(const FastPlan &fp, long n_frames, long block, int lane, long *tA0_out, long *dt_out, long *n_it_out) {
    const int s = (int)(block / fp.waves_per_stream);
    const int id0 = (int)(block - (long)s * fp.waves_per_stream) * 64;
    int id = id0 + lane;
    const bool live = id < fp.tiles * fp.nb;
    if (!live) id = fp.tiles * fp.nb - 1;
    const int tl0 = id0 / fp.nb, tl = id / fp.nb;
    const int k = id - tl * fp.nb;
    const long tA0 = (long)tl0 * fp.tile;
    const int dt = (tl - tl0) * fp.tile;
    long n_it = n_frames - tA0;
    if (n_it > fp.tile) n_it = fp.tile;
    long cnt = n_frames - (tA0 + dt);
    if (cnt > fp.tile) cnt = fp.tile;
    if (!live) cnt = 0;
    *tA0_out = tA0; *dt_out = dt; *n_it_out = n_it;
    return ChainItem{s, tA0 + dt, cnt, k};
}
// problem slot k of a FastPlan -> problem
inline int chain_fast_problem(const FastPlan &fp, int k) { return k == 0 ? 0 : k <= fp.n_main ? fp.q_lo + k - 1 : fp.extra_q[k - 1 - fp.n_main]; }

// ---- the geometry of a batch ---------------------------------------------------------------------------------------------------------------
inline ChainGeom chain_geom(const ChainShape &c, const ChainPlan &p, const BandPlan &band) {
    const int N = c.n_fft, NQ = N / 2 + 2, M = c.n_mics, hop = N / 2;
    const bool gsc = c.algo == BF_GSC;
    const int S = c.n_streams, D = gsc ? M : c.n_dirs;  // gsc: one aligned output per microphone
    const long So = (long)S * D, F = c.n_frames;         // beams: the streams of everything behind the STFT
    const int n_cus = c.n_cus;
    GeomFit fit;
    ChainGeom g{};
    fit.i(So);  // BinsArgs::n_streams
    auto lane_blocks = [&] { return fit.gx(((long)fit.i(So * NQ) + 63) / 64); };  // the kernels' n_streams * kNQ is an int

    if (p.fused()) {
        FusedGeom &f = g.fused;
        // frames per round of a block: N = 1024 walks single frames
        f.fpr = N == 1024 ? 1 : N == 2048 ? (p.mp == 4 ? 2 : 1) : (p.mp == 4 ? 4 : 2) * (1024 / N);
        f.rps = (F + f.fpr - 1) / f.fpr;
        f.total = f.rps * S;  // rounds, numbered stream * rps + round; one contiguous range per block
        long blocks = f.total < n_cus ? f.total : n_cus;
        if (blocks < 1) blocks = 1;
        f.rpb = (f.total + blocks - 1) / blocks;
        f.grid = fit.gx((f.total + f.rpb - 1) / f.rpb);
        const long tail_items = So * F * 2;
        f.tail_blocks = fit.gx((tail_items + 255) / 256);
    } else {
        g.stft = chain_stft_geom(p.front, N, S, F, c.algo == BF_MCRA ? 1 : M, n_cus);
        if (!g.stft.ok) fit.ok = false;
    }

    BinsGeom &b = g.bins;
    // lcmv with bf_config.lcmv_out_beams > 1: every kernel stores p.rows rows per stream
    const bool rows = p.rows > 1;
    switch (p.bins) {
        case ChainBins::kFusedTail: break;
        case ChainBins::kPointwise:
        case ChainBins::kMpfMask:
        case ChainBins::kGscAlign: b.ew_blocks = fit.gx((So * F * NQ + 255) / 256); break;
        case ChainBins::kMcra: b.lane_blocks = lane_blocks(); break;
        case ChainBins::kMvdrLcmv:
        case ChainBins::kCov2d: {
            int tile = 64;
            if (F < tile) tile = (int)F;
            b.tile = tile;
            b.tps = fit.i((F + tile - 1) / tile);
            const long units = (long)b.tps * So;  // the kernels' tiles_per_stream * n_streams
            fit.i(units);
            if (p.bins == ChainBins::kMvdrLcmv) {  // a group of MP lanes per problem, padding rows / columns are identity
                b.gx = fit.gx(units);
                b.gy = fit.gy((NQ + (256 / p.mp) - 1) / (256 / p.mp));
            } else {
                b.cov2d_grid = fit.gx((units + 7) / 8 * 8 * ((NQ + 15) / 16));  // (unit, problem group) -> XCD-aware order in the kernel
            }
            break;
        }
        case ChainBins::kMvdrFast: {
            FastPlan &fp = b.fp;
            fp.q_lo = band.q_lo; fp.n_main = band.n_main; fp.n_extra = band.n_extra;
            fp.extra_q[0] = band.extra_q[0]; fp.extra_q[1] = band.extra_q[1];
            fp.solve0 = band.solve0; fp.nb = band.nb;
            if (!band.ok) fit.ok = false;
            // tile length: the wavefronts (64 lanes = 64 (tile, problem) pairs) should fill the 4 x CUs slots a whole number of times;
            // cost of a choice = rounds x (frames walked + P warm-up frames); BF_MVDR_TILE forces a length (tests: lanes that straddle tiles,
            // a short last tile), held to the 512 frames of slack that chain_decide puts behind Z for the prefetch past a short last tile
            const int ft_env = c.mvdr_tile;
            // resident wavefronts per CU: the prefetch buffers (2 x 2 MP rows of 1 KiB in LDS) and the register count of the instantiation
            // that will run decide -- 8 microphones: one per SIMD (512 registers); fewer microphones: more
            const int km = rows && p.km == 1 ? 2 : p.km;  // columns of the instantiation that runs
            const int wpc = p.mp == 2 ? 16 : p.mp == 4 ? (km <= 2 ? 9 : 8) : p.mp == 6 ? (km == 1 ? 6 : 4) : 4;
            b.fast_km = km; b.wpc = wpc;
            const long slots = (long)n_cus * wpc;
            long best_t = 1;
            double best_c = 1e300;
            for (long t = 1; t <= 512 && t <= F; ++t) {
                const long tiles = (F + t - 1) / t;
                const long waves = (long)So * ((tiles * fp.nb + 63) / 64);
                const long rounds = (waves + slots - 1) / slots;
                const double cst = (double)rounds * (double)(t + c.past_windows + 2);
                if (cst <= best_c) { best_c = cst; best_t = t; }
            }
            if (ft_env > 0) best_t = ft_env < F ? ft_env : F;
            if (best_t > 512) best_t = 512;
            fp.tile = (int)best_t;
            fp.tiles = fit.i((F + best_t - 1) / best_t);
            const long lanes = (long)fp.tiles * fp.nb;  // the kernel's fp.tiles * fp.nb, and its id0 + lane
            fit.i(lanes + 63);
            fp.waves_per_stream = fit.i((lanes + 63) / 64);
            if (!p.yh32 && !p.band_rows)  // f64x2 rows read in full (spectrum dump, other FFT sizes, a band up to Nyquist): the rows nobody solves read as zero (mvdr.cpp:103)
                b.zero = ChainZero::kF64Rows;
            else if (p.yh32 && p.yh_lo == 0 && fp.nb < NQ)  // f32x2 rows that the backward transform reads in full (a band up to the Nyquist problems) while part of them is out of band
                b.zero = ChainZero::kF32Rows;
            b.fast_grid = fit.gx((long)fp.waves_per_stream * So);
            break;
        }
        case ChainBins::kGssLane: b.gss_grid = fit.gx(So * ((NQ + 63) / 64)); break;
        case ChainBins::kGss: b.gss_grid = fit.gx(((long)fit.i(So * NQ) + (256 / p.mp) - 1) / (256 / p.mp)); break;
    }
    if (p.rec == ChainRec::kRecursion || p.postfilter) b.lane_blocks = lane_blocks();
    if (p.rec == ChainRec::kRecIstft) b.rec_blocks = fit.gx(So);
    if (p.expand) b.expand_blocks = fit.gx((So * p.rows * F * N + 255) / 256);

    IstftGeom &is = g.istft;
    const long Si = So * p.rows;  // IstftArgs::n_streams: every row of a beam is an output stream
    fit.i(Si);
    switch (p.istft) {
        case ChainIstft::kNone: break;
        case ChainIstft::kF32: {  // fp32 backward transform of f32x2 rows, one frame per FFT
            constexpr int kI32Halves = 8;
            // two blocks per CU are resident (213-228 VGPRs): one chunk per half-wavefront slot = one round; every chunk recomputes one
            // warm-up frame.  Measured per 65 536 frames: x1 0.181, x2 0.127, x3 0.160 (round 2's value), x4 0.134, x8 0.148 ms
            long slots = (long)n_cus * kI32Halves * 2 / Si;
            if (slots < 1) slots = 1;
            long cps = slots < F ? slots : F;
            const long fpc = (F + cps - 1) / cps;
            cps = (F + fpc - 1) / fpc;
            const long chunks = cps * Si;
            is.per_run = fit.i(fpc); is.runs_per_stream = fit.i(cps);
            is.grid = fit.gx((chunks + kI32Halves - 1) / kI32Halves);
            break;
        }
        case ChainIstft::kW64: {
            constexpr int kIw64Waves = 4;
            const long pairs = (F + 1) / 2;
            // one run per wavefront slot (2 blocks x 4 wavefronts per CU), every run recomputes one warm-up frame
            long slots = (long)n_cus * kIw64Waves * 2 / Si;
            if (slots < 1) slots = 1;
            long rps = slots < pairs ? slots : pairs;
            const long ppr = (pairs + rps - 1) / rps;
            rps = (pairs + ppr - 1) / ppr;
            const long runs = rps * Si;
            is.per_run = fit.i(ppr); is.runs_per_stream = fit.i(rps);
            is.grid = fit.gx((runs + kIw64Waves - 1) / kIw64Waves);
            break;
        }
        case ChainIstft::kSmall: {  // backward transform, window and overlap-add in registers
            constexpr int halves = 8;
            const int kG = 1024 / N;
            const long slots = (long)n_cus * halves;
            long L = (Si * F + slots - 1) / slots;
            L = ((L + kG - 1) / kG) * kG;  // whole groups of frames
            if (L < 4 * kG) L = 4 * kG;    // a run recomputes one group
            const long items = Si * ((F + L - 1) / L);
            is.per_run = fit.i(L);  // (runs per stream: the kernel's own ceil(n_frames / L))
            is.grid = fit.gx((items + halves - 1) / halves);
            break;
        }
        case ChainIstft::kSplit: {  // one FFT-1024 per frame, window and overlap-add in registers
            constexpr int halves = 8;
            const long slots = (long)n_cus * halves;
            long L = (Si * F + slots - 1) / slots;
            if (L < 8) L = 8;  // a run recomputes one frame
            const long items = Si * ((F + L - 1) / L);
            is.per_run = fit.i(L);  // (runs per stream: the kernel's own ceil(n_frames / L))
            is.grid = fit.gx((items + halves - 1) / halves);
            break;
        }
        case ChainIstft::kGeneric: {  // windowed frames through IstftArgs::frames, overlap-added by a second pass
            const long total = Si * F;
            long blocks = total < (long)n_cus * 8 ? total : (long)n_cus * 8;
            if (blocks < 1) blocks = 1;
            is.per_run = 1;
            is.grid = fit.gx(blocks);
            const long samples = total * hop;
            is.ola_grid = fit.gx((samples + 255) / 256);
            break;
        }
    }

    TailGeom &t = g.tail;
    if (p.tail == ChainTail::kSmooth4 || p.tail == ChainTail::kSmooth) {
        const long n = F * hop;
        const long total = n * So;
        t.smooth4_grid = fit.gx((total / 4 + 255) / 256);
        t.smooth_grid = fit.gx((total + 255) / 256);
        t.state_grid = fit.gx((64 * So + 255) / 256);
        fit.i(64 * So);  // smooth_state_kernel's 64 * n_streams
    } else if (p.tail != ChainTail::kNone) {
        const int fs = c.gsc_filter_size, nb = M - 1, nbr = nb > 0 ? nb : 1;
        const bool serial = p.tail == ChainTail::kNlms;
        const int kp = serial || p.tail == ChainTail::kNlmsPar ? p.t1 : p.t2;  // KPL
        t.lds_serial = sizeof(float) * ((size_t)nbr * ((fs + 64 * kp + 8) | 1) + (size_t)nbr * ((64 * kp + 8) | 1) + 2 * fs + 16 +
                                        (size_t)nbr * 64 + 64 + 16 + 64);
        t.lds_par = sizeof(float) * ((size_t)nbr * ((fs + 64 * kp + 8) | 1) + 2 * fs + 64 * kp + 16 + (size_t)nbr * 64 + 64 + 64 + 64);
        t.nlms_grid = fit.gx(S);
    }
    g.ok = fit.ok;
    if (!g.ok) g = ChainGeom{};  // an invalid geometry is invalid and nothing else
    return g;
}

}  // namespace bf
