// chain_plan.hpp -- what one batch of the STFT -> per-bin -> ISTFT chain launches (every node except fused fp32 das and the one-launch das
// in double): which kernel of each stage with which template arguments, the row formats between the stages and the workspace sizes, host
// arithmetic (docs/DISPATCH.md lists the outcome per shape).  Plain C++: the CPU suite checks it through tests/host_emul (every chain row of
// the dispatch table, random shapes, every switch).  BinPipelineImpl::run_chain (pipeline.hip) decides once per batch and the launchers of
// the batch's FFT size (pipeline_kernels.hpp) carry the plan out.  The launch geometry of the plan -- runs, tiles, rounds, grids and the
// integers the kernels decode their work from -- is decided at the same moment, as values too: chain_geom.hpp (included below).
#pragma once

#include <cstddef>

#include "../../include/bfcore.h"

namespace bf {

// One batch, as values.  n_streams counts INPUT streams and n_dirs look directions per input stream (>= 1); kp1 = constraint columns of the
// batch (look direction + interferers; 1 unless lcmv / gss).  band_yh_lo / band_yh_hi: the in-band problems of mvdr / lcmv
// (BinPipelineImpl::init).  aligned16: the output pointer is 16-byte aligned (device workspaces always are).  The last six: the switches of
// those names (switches.hpp).  gss_rows (last, so that a shape written without it means one): separated sources gss emits per beam
// (bf_config.gss_out_sources; 0 = 1, ignored by every other node).  track (last again: a shape written without it means false): the batch
// carries a steering track (bf_process_batch_device_tracked: a table index per (stream, frame); das / phase / phasempf, one look direction).
// ctrack_cols (last once more: a shape written without it means 0 = none): the batch carries a column track
// (bf_process_batch_device_ctracked: a table index per (stream, frame, constraint column); mvdr / lcmv, one look direction).
// gss_postfilter (last yet again: a shape written without it means 0 = off): bf_config.gss_postfilter, ignored by every node but gss.
// lcmv_rows (last, as the others: a shape written without it means one): beams lcmv emits per stream and look direction
// (bf_config.lcmv_out_beams; 0 = 1, ignored by every other node).
// mvdr_tile (last, as the others: a shape written without it means 0 = chosen by cost): the switch of that name, read by the geometry only
// (chain_geom.hpp).
struct ChainShape {
    int algo, n_fft, layout, n_mics, n_streams, n_dirs, kp1, past_windows, precision;
    bool dump;
    long n_frames;
    int n_cus, gsc_filter_size, smooth_size, band_yh_lo, band_yh_hi;
    bool aligned16;
    int fused_bins;
    bool stft_small, stft_split, mvdr_group;
    int gss_group;
    bool gsc_serial;
    int gss_rows;
    bool track;
    int ctrack_cols;
    int gss_postfilter;
    int lcmv_rows;
    int mvdr_tile;
};

// The kernels of each stage, template arguments behind them as ChainPlan holds them:
//   front  stft_kernel / stft_small_kernel / stft_wave2048_kernel <layout, z48>, stft_generic_kernel<layout>, or STFT and per-bin stage in
//          one launch: stft_bins_w64_kernel / stft_bins_small_kernel / stft_bins_split_kernel <layout, mp, algo> + fused_tail_kernel<mp, algo>
//   bins   pointwise_bins_kernel<mp, algo>, mpf_mask_kernel<mp>, mcra_node_kernel, gsc_align_kernel, mvdr_fast_kernel<mp, km, !z48>,
//          cov2d_kernel<km, wps, !z48>, mvdr_lcmv_kernel<mp, km>, gss_kernel<mp, km>, gss_lane_kernel<mp, km>
//   rec    phasempf's pass over the frames: mpf_recursion_kernel, or mpf_rec_istft_kernel, which runs the backward transform too
//   post   gss_postfilter_kernel<RP> behind gss's per-bin kernel (ChainPlan::postfilter), in front of expand_spectrum_kernel
//   istft  istft_w64_kernel<band_rows>, istft32_kernel, istft_small_kernel, istft_split_kernel, istft_generic_kernel + ola_generic_kernel
//          with ChainPlan::track their twins that resolve the steering table per frame: stft_bins_w64_track_kernel + fused_tail_track_kernel,
//          pointwise_track_kernel<mp, algo>, mpf_mask_track_kernel<mp>; with ChainPlan::ctrack mvdr_fast_track_kernel<mp, km, !z48> and
//          mvdr_lcmv_track_kernel<mp, km> (cov2d_kernel has no twin: 9 .. 16 microphones run the group kernel's)
//   tail   smooth4_kernel<t0> or smooth_kernel, then smooth_state_kernel (phasempf); gsc_nlms_kernel / gsc_nlms_par_kernel <t0 = NBM, t1 = KPL>
//          or gsc_nlms_mw_kernel<t0 = NW, t1 = NBL, t2 = KPL> (gsc)
enum class ChainFront { kStft, kStftSmall, kStftWave2048, kStftGeneric, kFusedW64, kFusedSmall, kFusedSplit };
enum class ChainBins { kFusedTail, kPointwise, kMpfMask, kMcra, kGscAlign, kMvdrFast, kCov2d, kMvdrLcmv, kGss, kGssLane };
enum class ChainRec { kNone, kRecursion, kRecIstft };
enum class ChainIstft { kNone, kW64, kF32, kSmall, kSplit, kGeneric };
enum class ChainTail { kNone, kSmooth4, kSmooth, kNlms, kNlmsPar, kNlmsMw };

// ---- the launch geometry of a plan, one small record per scheme (filled by chain_geom, chain_geom.hpp) ----------------------------------
// mvdr_fast_kernel's argument (by value: members, order and types are the kernel's ABI).  Lanes enumerate (time tile, problem) pairs of
// ONE output stream, problem fastest, over the problems that need a solve only
struct FastPlan {
    int q_lo, n_main;  // problems q_lo .. q_lo + n_main - 1 are in band (a contiguous run inside 1 .. N/2-1)
    int n_extra;       // the irregular problems of quirk Q1 that are in band: N/2 (f := 0) when 0 Hz is, N/2+1 (|f| = (N/2-1) sr/N)
    int extra_q[2];
    int solve0;        // lcmv with 0 Hz in band: problem 0 is an ordinary problem (mvdr passes X_0 through, mvdr.cpp:76)
    int nb;            // 1 + n_main + n_extra
    int tile, tiles, waves_per_stream;
};

// what the batch has to zero in Yh before mvdr_fast_kernel runs: the rows nobody solves but the backward transform reads
enum class ChainZero { kNone, kF64Rows, kF32Rows };

// kStft / kStftSmall / kStftWave2048 / kStftGeneric (StftArgs::run_len, blocks of 256 threads; kStftGeneric: run_len 1)
struct StftGeom {
    int run_len;
    unsigned blocks;
    bool ok;
};
// kFusedW64 / kFusedSmall / kFusedSplit: a round = fpr consecutive frames of one stream, rounds numbered stream * rps + round, one contiguous
// range of rpb rounds per block (the N = 1024 kernel walks single frames: its frames_per_block / total_frames are rpb / total)
struct FusedGeom {
    int fpr;
    long rps, total, rpb;
    unsigned grid, tail_blocks;  // tail_blocks: fused_tail_kernel, one thread per (stream, frame, problem N/2 | N/2+1)
};
struct BinsGeom {
    unsigned ew_blocks;      // pointwise_bins / mpf_mask / gsc_align: a thread per (stream, frame, problem), 256 per block
    unsigned lane_blocks;    // mcra_node / mpf_recursion / gss_postfilter: a lane per (stream, problem), 64 per block
    unsigned rec_blocks;     // mpf_rec_istft_kernel: a block per stream
    unsigned expand_blocks;  // expand_spectrum_kernel: a thread per (stream, row, frame, bin)
    int tile, tps;           // the group kernels (mvdr_lcmv_kernel, cov2d_kernel): frames per tile, tiles per stream
    unsigned gx, gy;         // mvdr_lcmv_kernel: (tile of a stream, group of 256 / MP problems)
    unsigned cov2d_grid;     // (unit, problem group) -> XCD-aware order in the kernel
    FastPlan fp;             // kMvdrFast
    unsigned fast_grid;
    int fast_km, wpc;        // columns of the instantiation that runs; resident wavefronts per CU
    ChainZero zero;
    unsigned gss_grid;       // gss_kernel / gss_lane_kernel
};
// kF32: frames per chunk, chunks per stream; kW64: frame PAIRS per run, runs per stream; kSmall / kSplit: frames per run (runs per stream
// is the kernel's own ceil(n_frames / L)); kGeneric: a block per (stream, frame) item, grid-strided, and the overlap-add pass
struct IstftGeom {
    int per_run, runs_per_stream;
    unsigned grid, ola_grid;
};
struct TailGeom {
    unsigned smooth_grid, smooth4_grid, state_grid;  // smooth_kernel, smooth4_kernel, smooth_state_kernel
    size_t lds_serial, lds_par;                      // dynamic LDS bytes of gsc_nlms_kernel / of gsc_nlms_par_kernel and gsc_nlms_mw_kernel
    unsigned nlms_grid;                              // a block per stream
};
struct ChainGeom {
    bool ok;
    StftGeom stft;
    FusedGeom fused;
    BinsGeom bins;
    IstftGeom istft;
    TailGeom tail;
};

struct ChainPlan {
    int algo, layout;
    ChainFront front;
    bool z48;  // mvdr / lcmv with BF_PRECISION_MIXED: 12-byte spectra
    ChainBins bins;
    int mp, km, wps;
    ChainRec rec;
    bool expand;  // expand_spectrum_kernel behind the per-bin stage (spectrum dump)
    ChainIstft istft;
    ChainTail tail;
    int t0, t1, t2;
    // row formats between the per-bin stage and the backward transform (BinsArgs / IstftArgs of the same names)
    bool yh32, mpf32, band_rows;  // band_rows: only problem 0 and yh_lo .. yh_hi exist
    int yh_lo, yh_hi;
    size_t z_bytes, yh_bytes, yraw_elems, frames_elems;  // d_Z_, d_Yh_, d_yraw_, d_frames_ of BinPipelineImpl
    // gss: rows per beam behind the per-bin stage (1: gss_kernel / gss_lane_kernel store y_fft = this_yf(0), gss.cpp:120-121; more: their
    // _all variants store this_yf(0 .. rows - 1) as output streams beam * rows + r, and everything behind them runs over So * rows streams).
    // lcmv: beams per stream and look direction (1: the per-bin kernels store (G^-1 g)_0; more: mvdr_fast_rows_kernel / mvdr_fast_track_rows_kernel /
    // cov2d_rows_kernel, or the group kernel counting at run time, store (G^-1 g)_r as row r -- which kernel family runs does not depend on it)
    int rows;
    // the front / per-bin kernels are the track twins: the steering pointer of a frame comes from the batch's track (BinsArgs::track)
    bool track;
    // the per-bin kernel is the column-track twin of mvdr_fast_kernel / mvdr_lcmv_kernel: the constraint columns of a frame come from the
    // batch's track (BinsArgs::track with track_cols entries per frame); mvdr / lcmv with one look direction only
    bool ctrack;
    // gss with bf_config.gss_postfilter: gss_postfilter_kernel<post_rp> runs in place over the rows of the per-bin stage (one lane owns
    // all rows of its (beam, problem): no second row buffer, yh_bytes stays what it is); post_rp = the rows padded to 1 / 2 / 4 / 8 / 16
    bool postfilter;
    int post_rp;
    // how the batch is cut into runs, tiles and rounds, every grid and every integer the kernels decode their work from: chain_geom
    // (chain_geom.hpp) fills it right behind chain_decide; the launchers read nothing else
    ChainGeom geom;
    bool fused() const { return front >= ChainFront::kFusedW64; }
    bool rec_istft() const { return rec == ChainRec::kRecIstft; }
};

// the separate STFT of an FFT size (also the front of the DOA maps, doa.cpp): the register-resident transforms unless their switch is 0
inline ChainFront chain_stft_front(int n_fft, bool stft_small, bool stft_split) {
    return n_fft == 1024 ? ChainFront::kStft : (n_fft <= 512 && stft_small) ? ChainFront::kStftSmall
           : (n_fft == 2048 && stft_split) ? ChainFront::kStftWave2048 : ChainFront::kStftGeneric;
}

inline ChainPlan chain_decide(const ChainShape &c) {
    const int N = c.n_fft, M = c.n_mics, a = c.algo, kp1 = c.kp1;
    const bool cov = a == BF_MVDR || a == BF_LCMV, gsc = a == BF_GSC, mpf = a == BF_PHASEMPF, pointwise = a == BF_DAS || a == BF_PHASE;
    const bool dump = c.dump && !gsc;  // time-domain node: there is no single y_fft, the dump reads as zeros
    const bool mixed = c.precision == BF_PRECISION_MIXED;
    const int NP = ((a == BF_MCRA ? 1 : M) + 1) / 2, D = gsc ? M : c.n_dirs;  // gsc: one aligned output per microphone
    const int R = (a == BF_GSS && c.gss_rows > 1) ? c.gss_rows : (a == BF_LCMV && c.lcmv_rows > 1) ? c.lcmv_rows : 1;
    const size_t S = (size_t)c.n_streams, So = S * D, F = (size_t)c.n_frames, P = cov ? (size_t)c.past_windows : 0;
    const int mp4 = M <= 4 ? 4 : M <= 8 ? 8 : M <= 16 ? 16 : 32, km = kp1 <= 1 ? 1 : 4;
    ChainPlan p{};
    p.algo = a; p.layout = c.layout; p.z48 = cov && mixed; p.rows = R;
    p.track = c.track && D == 1 && (pointwise || mpf);
    p.ctrack = c.ctrack_cols > 0 && D == 1 && cov;
    p.postfilter = a == BF_GSS && c.gss_postfilter != 0;
    p.post_rp = !p.postfilter ? 0 : R <= 1 ? 1 : R <= 2 ? 2 : R <= 4 ? 4 : R <= 8 ? 8 : 16;
    // nodes without a frame history, up to 8 microphones, one look direction: STFT and per-bin stage in one launch, spectra never leave the CU.
    // A tracked batch only at N = 1024: the fused fronts of the other sizes keep a thread's steering entries in registers across frames
    const bool fused = c.fused_bins != 0 && N <= 2048 && M <= 8 && D == 1 && (pointwise || mpf) && (!p.track || N == 1024);
    // the register-resident transforms of the other sizes (stft_small / stft_split = 0: the generic kernels; the fused front has no generic twin)
    const bool small = N <= 512 && c.stft_small, split = N == 2048 && c.stft_split;
    if (fused) p.front = N == 1024 ? ChainFront::kFusedW64 : N == 2048 ? ChainFront::kFusedSplit : ChainFront::kFusedSmall;
    else p.front = chain_stft_front(N, c.stft_small, c.stft_split);
    // Backward transform in fp32 (BF_PRECISION_MIXED, N = 1024, no dump, not gsc): the per-bin stage emits f32x2 rows -- mvdr / lcmv, das / phase --
    // and phasempf's recursion leaves y_fft as f32x2 rows in the slots of its |out_int|^2 input
    const bool want32 = mixed && !gsc && N == 1024 && !dump;
    p.yh32 = want32 && (cov || pointwise);
    p.mpf32 = want32 && mpf;
    // mvdr / lcmv rows in front of a backward transform (no dump): only problem 0 and the band's problems exist
    const bool band = cov && !dump && N == 1024;
    p.yh_lo = band ? c.band_yh_lo : 0; p.yh_hi = band ? c.band_yh_hi : N / 2 + 1;
    p.band_rows = p.yh_lo > 0 || p.yh_hi < p.yh_lo;
    if (fused) {
        p.bins = ChainBins::kFusedTail; p.mp = M <= 4 ? 4 : 8;
    } else if (pointwise || mpf) {
        p.bins = mpf ? ChainBins::kMpfMask : ChainBins::kPointwise; p.mp = mp4;
    } else if (a == BF_MCRA || gsc) {
        p.bins = gsc ? ChainBins::kGscAlign : ChainBins::kMcra;
    } else if (kp1 > 4 || M > 16) {
        // beyond the tuned shapes (more than 3 interferers or 16 microphones): the group kernels' next larger (lanes per problem, columns)
        p.bins = cov ? ChainBins::kMvdrLcmv : ChainBins::kGss;
        p.km = kp1 <= 1 ? 1 : kp1 <= 4 ? 4 : kp1 <= 8 ? 8 : 16;
        p.mp = kp1 <= 4 ? 32 : kp1 <= 8 ? (M <= 8 ? 8 : mp4) : (M <= 16 ? 16 : 32);
    } else if (cov && !c.mvdr_group && M > 8 && !p.ctrack) {
        p.bins = ChainBins::kCov2d; p.km = km; p.wps = km == 1 ? 3 : 2;  // 2-D cyclic 4 x 4 lanes per problem; wavefronts per SIMD
    } else if (cov && !c.mvdr_group && M <= 8 && (M > 2 || kp1 <= 2)) {  // (a column-tracked batch of 9 .. 16 microphones: the group kernel below)
        // one lane per (tile, problem); lcmv's columns ride along while they fit the register file (K = 3 only at 7-8 microphones).
        // Two microphones hold at most two columns: more go to the group kernel
        p.bins = ChainBins::kMvdrFast; p.mp = M <= 2 ? 2 : M <= 4 ? 4 : M <= 6 ? 6 : 8;
        p.km = kp1 <= 2 ? kp1 : (p.mp == 8 && kp1 == 3) ? 3 : 4;
    } else if (cov) {
        p.bins = ChainBins::kMvdrLcmv; p.mp = mp4 < 16 ? mp4 : 16; p.km = km;
    } else {
        // gss: one lane per problem once the lanes fill the chip (two wavefronts per CU); gss_group = 1 / 0 forces the group / the lane kernel.
        // Problems are counted per beam: the rows a problem stores do not change who computes it
        const bool lane = c.gss_group >= 0 ? c.gss_group == 0 : (long)So * ((N / 2 + 2 + 63) / 64) >= 2L * c.n_cus;
        p.bins = (M <= 8 && lane) ? ChainBins::kGssLane : ChainBins::kGss; p.mp = mp4; p.km = km;
    }
    // phasempf with at least a quarter as many streams as CUs (N = 1024, f64x2 rows, no dump): the recursion kernel runs the backward transform too
    if (mpf) p.rec = (N == 1024 && !dump && !p.mpf32 && (long)So * 4 >= c.n_cus) ? ChainRec::kRecIstft : ChainRec::kRecursion;
    p.expand = dump;
    p.istft = p.rec_istft() ? ChainIstft::kNone : N == 1024 ? (p.yh32 || p.mpf32 ? ChainIstft::kF32 : ChainIstft::kW64)
              : small ? ChainIstft::kSmall : split ? ChainIstft::kSplit : ChainIstft::kGeneric;
    if (mpf) {  // four outputs per thread for windows of up to 8 samples
        p.tail = (c.aligned16 && c.smooth_size >= 1 && c.smooth_size <= 8) ? ChainTail::kSmooth4 : ChainTail::kSmooth;
        p.t0 = c.smooth_size;
    } else if (gsc) {
        // gsc_serial: the sums in the reference's tap order, one branch per lane; default: taps over the lanes, the branches dealt out to
        // 8 wavefronts per stream from five branches on, 4 from three, 2 at two
        const int nb = M - 1, kpl = (c.gsc_filter_size + 63) / 64, kp = kpl <= 1 ? 1 : kpl <= 2 ? 2 : 4;
        const int nw = c.gsc_serial ? 1 : nb >= 5 ? 8 : nb >= 3 ? 4 : nb >= 2 ? 2 : 1;
        if (nw > 1) {
            p.tail = ChainTail::kNlmsMw; p.t0 = nw; p.t1 = (nb + nw - 1) / nw <= 1 ? 1 : 2; p.t2 = kp;
        } else {
            p.tail = c.gsc_serial ? ChainTail::kNlms : ChainTail::kNlmsPar; p.t0 = nb <= 1 ? 1 : nb <= 3 ? 3 : nb <= 7 ? 7 : 15; p.t1 = kp;
        }
    }
    // Z: the packed spectra of history + batch (+ 512 frames of slack for mvdr_fast_kernel's prefetch past a short last tile); the fused front
    // parks the unpacked spectra of two bins per frame there instead.  Yh: phasempf keeps one double per problem behind the rows
    p.z_bytes = fused ? S * F * 2 * 8 * 16 : (S * (P + F) + (cov ? 512 : 0)) * NP * N * (p.z48 ? 12 : 16);
    p.yh_bytes = So * R * F * (N / 2 + 4) * (mpf ? 24 : 16);
    p.yraw_elems = (mpf || gsc) ? So * F * (N / 2) : 0;
    p.frames_elems = N != 1024 ? So * R * F * N : 0;
    return p;
}

}  // namespace bf

#include "chain_geom.hpp"  // the geometry of a plan (needs the types above)
