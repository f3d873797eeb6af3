// pipeline.hip -- fp64 bin pipeline for gfx950: the engine (pipeline.hpp) of every node except fused fp32 das.
//
//   stft_kernel   : overlap_and_add_prepare_input + fftw_execute(x_forward) for all mics
//                   (util.h:217-242, das.cpp:51-57); two real mics per complex FFT-1024,
//                   packed spectra Z_p = FFT(a + i b) go to an HBM workspace
//   *_bins_kernel : the node's per-bin loop of apply_weights(); unpacks
//                   X_a[k] = (Z[k] + conj Z[N-k])/2, X_b[k] = (Z[k] - conj Z[N-k])/(2i) on load
//   istft_w64_kernel / istft32_kernel : fftw_execute(y_inverse) + overlap_and_add_prepare_output + do_overlap's
//                   overlap-add (das.cpp:66, util.h:244-253,301-302), two frames per complex
//                   IFFT (Hermitian half-spectra in, real frames out as re / im)
//
// fp64 throughout: the covariance solves of mvdr/lcmv amplify input error by the
// condition number (1e3..1e4 on coherent scenes), and the phase / MCRA threshold
// decisions flip on fp32 noise; 1e-5 on the complex spectrum needs double
// (DESIGN.md "Precision").  The reference itself is double everywhere.
#include "pipeline.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>
#include <vector>

#include "device_mem.hpp"
#include "fft1024.hpp"
#include "pipeline_kernels.hpp"
#include "switches.hpp"

namespace bf {

// ============================================================================
//                                   host side
// ============================================================================
namespace {

class BinPipelineImpl : public Engine {
    static constexpr int kMaxCols = BF_MAX_INTERF + 1;  // look direction + up to 15 interferers (per-bin kernels: KM <= 16)
   public:
    BinPipelineImpl(const bf_config &c, int n_cus) : cfg_(c), n_cus_(n_cus) {
        M_ = c.n_mics;
        H_ = c.hop;
        N_ = 2 * c.hop;
        NQ_ = problems_per_frame(N_);
        YS_ = yh_stride(N_);
        ks_ = kernel_set(N_);
        MF_ = single_ch_ ? 1 : M_;
        NP_ = (MF_ + 1) / 2;
        S_ = c.n_streams;                                   // input streams
        D_ = c.n_dirs > 1 ? c.n_dirs : 1;                   // look directions per input stream
        if (time_node_) D_ = M_;                            // gsc: one aligned output per microphone (do_overlap_bymic)
        So_ = S_ * D_;                                      // beams (output streams of every node but gss with several rows)
        R_ = (c.algo == BF_GSS && c.gss_out_sources > 1) ? c.gss_out_sources : 1;  // separated sources emitted per beam (gss.cpp:120-121 keeps one)
        if (c.algo == BF_LCMV && c.lcmv_out_beams > 1) R_ = c.lcmv_out_beams;     // lcmv: a beam per constraint column (lcmv.cpp:119 keeps column 0)
        const bool multi = (c.algo == BF_LCMV || c.algo == BF_GSS);
        KP1_ = multi ? c.n_interf + 1 : 1;
        Phist_ = cov_node_ ? c.past_windows : 0;
        // BF_PRECISION_MIXED: mvdr / lcmv park their spectra as 12-byte z48 elements (pipeline_kernels.hpp); the default keeps complex doubles
        z48_ = cov_node_ && c.precision == BF_PRECISION_MIXED;
        zsz_ = z48_ ? sizeof(z48) : sizeof(f64x2);
    }

    int init() override {
        if (ks_ == nullptr) {
            err_ = "hop (JACK period) must be a power of two from 64 to 4096 frames";
            return BF_ENOSYS;
        }
        if (M_ > 32 && band_node_) {
            err_ = "mvdr/lcmv/gss kernels are built for up to 32 microphones";
            return BF_ENOSYS;
        }
        if (KP1_ > kMaxCols && (cfg_.algo == BF_LCMV || cfg_.algo == BF_GSS)) {
            err_ = "lcmv/gss kernels are built for up to 15 interferers";
            return BF_ENOSYS;
        }
        if (cov_node_ && (Phist_ < 1 || Phist_ > 64)) {
            err_ = "past_windows must be in 1..64";
            return BF_EINVAL;
        }
        if (time_node_ && (M_ > 16 || cfg_.gsc_filter_size < 1 || cfg_.gsc_filter_size > 256)) {
            err_ = "gsc is built for up to 16 microphones and filter_size 1..256";
            return M_ > 16 ? BF_ENOSYS : BF_EINVAL;
        }
        if (cfg_.algo == BF_PHASEMPF && (cfg_.smooth_size < 1 || cfg_.smooth_size > 64)) {
            err_ = "smooth_size must be in 1..64";
            return BF_EINVAL;
        }
        // N = 1024: inter-pass twiddles of the 32 x 32 factorisation; other sizes: exp(-2 pi i m / N), m < N/2 (Stockham passes)
        ENGINE_HIP(d_tw_.upload(N_ == 1024 ? twiddle_table_32x32<f64x2>() : stockham_twiddles<f64x2>(N_)));
        ENGINE_HIP(d_tw32_.upload(twiddle_table_32x32<f32x2>()));
        ENGINE_HIP(d_win_.upload(sqrt_hann(N_)));
        freqs_ = frequency_vector(N_, cfg_.sample_rate);
        ENGINE_HIP(d_freq_.upload(freqs_));
        // the band, scanned once: what the STFT may skip, the rows mvdr / lcmv leave for the backward transform, the problems
        // mvdr_fast_kernel enumerates (chain_geom.hpp)
        band_ = band_plan(N_, cfg_.sample_rate, cfg_.freq_min, cfg_.freq_max, cfg_.algo);
        if (!band_.ok) {
            err_ = "the band [freq_min, freq_max] is not one run of bins";  // (cannot happen: |f| rises with the bin below N/2)
            return BF_EINVAL;
        }
        for (auto &b : d_steer_) ENGINE_HIP(b.alloc(steer_elems()));
        if (das_one_launch_shape()) {
            for (auto &t : das_) ENGINE_HIP(t.gains_w64.alloc((size_t)4 * 1024));
            for (auto &t : das_) ENGINE_HIP(t.gains_sep.alloc((size_t)8 * kDasSepMic));
            ENGINE_HIP(d_das_sched_.alloc(das_f64_sched_ws_bytes()));  // das_f64_pair_kernel's work queue (chunk table + counter)
        }
        if (N_ == 1024) ENGINE_HIP(d_tw_w64_.upload(twiddle_table_w64_rot()));
        for (auto &b : d_hist2_) ENGINE_HIP(b.alloc(hist_elems()));
        for (auto &b : d_tail_) ENGINE_HIP(b.alloc(tail_elems()));
        if (Phist_ > 0) ENGINE_HIP(d_zhist_.alloc(zhist_bytes()));
        if (cfg_.algo == BF_GSS) {
            ENGINE_HIP(d_gssW_.alloc(gss_bytes() / sizeof(f64x2)));
            ENGINE_HIP(hipMemset(d_gssW_.get(), 0, gss_bytes()));  // defined content until the first run applies W = C^H
        }
        if (mpf_bytes()) ENGINE_HIP(d_mpf_.alloc(mpf_bytes() / sizeof(double)));  // phasempf, mcra, gss with its post-filter
        if (cfg_.algo == BF_PHASEMPF) ENGINE_HIP(d_smooth_.alloc(smooth_bytes() / sizeof(double)));
        if (time_node_) ENGINE_HIP(d_nlms_.alloc(nlms_bytes() / sizeof(float)));
        return BF_OK;
    }

    int reset(hipStream_t st) override {
        ENGINE_HIP(hipMemsetAsync(d_hist2_[0].get(), 0, hist_elems() * sizeof(float), st));
        hist_cur_ = 0;
        for (auto &b : d_tail_) ENGINE_HIP(hipMemsetAsync(b.get(), 0, tail_elems() * sizeof(float), st));
        tail_cur_ = 0;
        if (d_zhist_.get()) ENGINE_HIP(hipMemsetAsync(d_zhist_.get(), 0, zhist_bytes(), st));  // past_ffts setZero (mvdr.cpp:228-232); zero bits = z48 zero
        if (d_mpf_.get()) ENGINE_HIP(hipMemsetAsync(d_mpf_.get(), 0, mpf_bytes(), st));          // phasempf.cpp:535-545, current_L=0/first_L
        if (d_smooth_.get()) ENGINE_HIP(hipMemsetAsync(d_smooth_.get(), 0, smooth_bytes(), st)); // calloc past_samples (phasempf.cpp:510)
        if (d_nlms_.get()) ENGINE_HIP(hipMemsetAsync(d_nlms_.get(), 0, nlms_bytes(), st));       // calloc block_matrix/filter/last_outputs (gsc.cpp:278-285)
        gss_reset_mask_ = ~0ull;  // sep_matrix = weights^H (gss.cpp:90-93), done on the stream at next run
        // (until then the matrices are dead; zeroed as init() leaves them, so that a reset handle's state blob is a new handle's)
        if (d_gssW_.get()) ENGINE_HIP(hipMemsetAsync(d_gssW_.get(), 0, gss_bytes(), st));
        return BF_OK;
    }

    int upload_steering(const std::vector<SteeringSet> &dirs, hipStream_t stream) override {
        // device layout [dir][col][mic][bin] so that lanes (bins) read consecutive addresses
        const int nc = dirs[0].n_cols, nd = (int)dirs.size();  // nd = look directions (gsc: 1, although D_ = M outputs)
        if ((size_t)nd * nc * M_ * N_ > steer_elems()) {
            err_ = "steering table larger than the device buffer";
            return BF_EINVAL;
        }
        std::vector<f64x2> t((size_t)nd * N_ * M_ * nc);
        for (int d = 0; d < nd; ++d)
            for (int c = 0; c < nc; ++c)
                for (int m = 0; m < M_; ++m)
                    for (int j = 0; j < N_; ++j) {
                        const cplxd w = dirs[d].at(j, m, c);
                        t[(((size_t)d * nc + c) * M_ + m) * N_ + j] = f64x2{w.real(), w.imag()};
                    }
        const int nxt = steer_cur_ ^ 1;
        std::vector<f64x2> dg64, dgm;  // das in double in one launch: the gains of the (single) look direction and its summary, same double buffering
        DasSepTables sep;              // (lives until the synchronisation below, like the others: the copies read pageable memory)
        if (das_one_launch_shape()) {
            dg64 = das_pair_gains_w64_f64(das_pair_gains_t<f64x2>(dirs[0], 4), 4);
            dgm = das_mic_gains_w64_f64(dirs[0], 8);
            das_[nxt].slots = das_f64_slots(dirs[0]);
            // the delay-structured form the frame-pair kernels read, checked entry by entry against dgm: a row that is not a delay sends
            // the batches of this table to the chain (run_das_one_launch: DasF64Shape::tables)
            sep = das_sep_gains_w64_f64(dirs[0], dgm, 8);
            das_[nxt].sep_ok = sep.ok; das_[nxt].sep_bound = sep.bound; das_[nxt].sep_worst = sep.worst;
            ENGINE_HIP(hipMemcpyAsync(das_[nxt].gains_sep.get(), sep.t.data(), sep.t.size() * sizeof(f64x2), hipMemcpyHostToDevice, stream));
            ENGINE_HIP(hipMemcpyAsync(das_[nxt].gains_w64.get(), dg64.data(), dg64.size() * sizeof(f64x2), hipMemcpyHostToDevice, stream));
        }
        ENGINE_HIP(hipMemcpyAsync(d_steer_[nxt].get(), t.data(), t.size() * sizeof(f64x2), hipMemcpyHostToDevice, stream));
        ENGINE_HIP(hipStreamSynchronize(stream));  // `t` is pageable and about to go out of scope
        steer_cur_ = nxt;
        steer_dir_stride_ = (long)nc * M_ * N_;
        return BF_OK;
    }

    bool can_track() const override { return (cfg_.algo == BF_DAS || cfg_.algo == BF_PHASE || cfg_.algo == BF_PHASEMPF) && D_ == 1; }
    bool can_ctrack() const override { return cov_node_ && D_ == 1; }
    int install_track_tables(const std::vector<f64x2> &tables, int n_angles) override {
        if (!can_track() && !can_ctrack()) return Engine::install_track_tables(tables, n_angles);
        // The tables in force are RETIRED, not freed: another thread may have taken them in its snapshot and still be enqueueing the kernels
        // of that batch, which no synchronisation here can wait for.  What the previous call retired goes now: every batch that could
        // hold it was begun before that call returned, and the device is idle with respect to what has been enqueued
        ENGINE_HIP(hipDeviceSynchronize());
        d_track_retired_ = std::move(d_track_);
        track_n_ = 0;
        if (n_angles > 0) {
            ENGINE_HIP(d_track_.upload(tables));
            track_n_ = n_angles;
        }
        return BF_OK;
    }

    void on_theta_changed(int dir) override { gss_reset_mask_ |= dir < 0 ? ~0ull : (1ull << dir); }
    void set_columns(int kp1) override {
        KP1_ = kp1;
        gss_reset_mask_ = ~0ull;
    }

    RunSnapshot snapshot_for_run() override {
        RunSnapshot sn;
        sn.kp1 = KP1_;
        sn.gss_reset_mask = gss_reset_mask_;
        sn.steer = d_steer_[steer_cur_].get();
        sn.steer_dir_stride = steer_dir_stride_;
        sn.das = DasSnapshot{das_[steer_cur_].gains_w64.get(),
                             das_[steer_cur_].sep_ok ? das_[steer_cur_].gains_sep.get() : nullptr, das_[steer_cur_].slots};
        sn.track_tables = d_track_.get();
        sn.track_n = track_n_;
        gss_reset_mask_ = 0;
        return sn;
    }
    int columns() const override { return KP1_; }
    unsigned long long pending_resets() const override { return gss_reset_mask_; }
    void set_pending_resets(unsigned long long mask) override { gss_reset_mask_ = mask; }

    int run(const float *x, long F, float *y, f64x2 *spectrum, hipStream_t stream, int layout, long mic_stride,
            const RunSnapshot &snap) override;

    size_t state_bytes() const override {
        return (hist_elems() + tail_elems()) * sizeof(float) + zhist_bytes() + gss_bytes() + mpf_bytes() + smooth_bytes() +
               nlms_bytes();
    }
    int get_state(void *host) override { return copy_state((char *)host, true); }
    int set_state(const void *host) override { return copy_state((char *)host, false); }

   private:
    static constexpr int kDeclined = 1;  // (every BF_* code is <= 0)
    int run_das_one_launch(const float *x, long F, float *y, hipStream_t stream, int layout, long mic_stride, const RunSnapshot &snap);
    int run_chain(const float *x, long F, float *y, f64x2 *spectrum, hipStream_t stream, int layout, long mic_stride, const RunSnapshot &snap);
    // das through this pipeline on the tuned shape: eligible for the one-launch kernels of das_f64_w64.hip (das_f64_plan.hpp das_f64_decide per batch)
    bool das_one_launch_shape() const { return cfg_.algo == BF_DAS && N_ == 1024 && M_ <= 8 && D_ == 1; }
    size_t steer_elems() const { return (size_t)D_ * N_ * M_ * kMaxCols; }
    size_t hist_elems() const { return (size_t)S_ * M_ * H_; }  // the carried hop of every input stream
    size_t tail_elems() const { return (size_t)So_ * R_ * H_; }  // the overlap-add tail of every output stream
    size_t zhist_bytes() const { return Phist_ ? (size_t)S_ * Phist_ * NP_ * N_ * zsz_ : 0; }
    // recursive per-beam state is sized by OUTPUT streams (input streams x look directions)
    size_t gss_bytes() const { return cfg_.algo == BF_GSS ? (size_t)So_ * N_ * kMaxCols * M_ * sizeof(f64x2) : 0; }
    size_t mpf_bytes() const {
        if (post_filter_) return (size_t)So_ * R_ * (kMpfVecs * N_ + 8) * sizeof(double);  // gss's post-filter: phasempf's block per output row
        return (cfg_.algo == BF_PHASEMPF || cfg_.algo == BF_MCRA) ? (size_t)So_ * (kMpfVecs * N_ + 8) * sizeof(double) : 0;
    }
    size_t smooth_bytes() const { return cfg_.algo == BF_PHASEMPF ? (size_t)So_ * 64 * sizeof(double) : 0; }
    size_t nlms_bytes() const {
        return time_node_ ? (size_t)S_ * (2 * (M_ - 1) + 1) * cfg_.gsc_filter_size * sizeof(float) : 0;
    }

    int copy_state(char *p, bool to_host) {
        ENGINE_HIP(hipDeviceSynchronize());
        struct Seg { void *d; size_t n; } segs[] = {
            {d_hist2_[hist_cur_].get(), hist_elems() * sizeof(float)}, {d_tail_[tail_cur_].get(), tail_elems() * sizeof(float)},
            {d_zhist_.get(), zhist_bytes()}, {d_gssW_.get(), gss_bytes()}, {d_mpf_.get(), mpf_bytes()}, {d_smooth_.get(), smooth_bytes()},
            {d_nlms_.get(), nlms_bytes()}};
        for (auto &s : segs) {
            if (!s.n) continue;
            if (to_host)
                ENGINE_HIP(hipMemcpy(p, s.d, s.n, hipMemcpyDeviceToHost));
            else
                ENGINE_HIP(hipMemcpy(s.d, p, s.n, hipMemcpyHostToDevice));
            p += s.n;
        }
        return BF_OK;  // the pending-reset mask travels in the blob's control-plane section (capi.cpp)
    }

    bf_config cfg_;
    int n_cus_, M_, MF_, NP_, S_, D_, So_, R_, KP1_, Phist_;
    // what kind of node this is
    const bool cov_node_ = cfg_.algo == BF_MVDR || cfg_.algo == BF_LCMV;  // covariance over a frame history; halved (or z48) spectra, band-limited rows
    const bool band_node_ = cov_node_ || cfg_.algo == BF_GSS;             // only the bins inside [freq_min, freq_max] are processed
    const bool time_node_ = cfg_.algo == BF_GSC;                          // the adaptive stage runs on samples: no single y_fft
    const bool single_ch_ = cfg_.algo == BF_MCRA;                         // only channel 0 is transformed (mcra.cpp:72-73)
    const bool post_filter_ = cfg_.algo == BF_GSS && cfg_.gss_postfilter != 0;  // the multi-source post-filter runs behind the gss kernels
    const bool post_amp_ = band_node_;                                    // out_amp is applied behind the backward transform
    const bool yraw_target_ = cfg_.algo == BF_PHASEMPF || time_node_;     // the backward transform feeds the smoother / the NLMS stage through d_yraw_
    BandPlan band_{};  // init(): StftArgs::skip_lo / skip_hi, the band-limited rows of mvdr / lcmv, FastPlan's problems (chain_geom.hpp)
    bool z48_ = false;
    size_t zsz_ = sizeof(f64x2);  // bytes per packed-spectrum element
    int H_ = 512, N_ = 1024, NQ_ = 514, YS_ = 516;  // hop, FFT size, problems per frame, row stride of Yh
    const KernelSet *ks_ = nullptr;                 // launchers compiled for N_
    long steer_dir_stride_ = 0;
    std::vector<double> freqs_;
    DeviceBuffer<f64x2> d_tw_;
    DeviceBuffer<f32x2> d_tw32_;
    DeviceBuffer<double> d_win_, d_freq_;
    DeviceBuffer<f64x2> d_steer_[2];     // double-buffered with steer_cur_: a batch in flight keeps the table it was launched with
    // das in double in one launch, of the same table (geometry.hpp): das_pair_gains_w64_f64 (microphone-pair kernel), das_mic_gains_w64_f64
    // (frame-pair kernels), das_f64_slots (is row 0 identically 1, which microphones get a forward transform in which order)
    // das_sep_gains_w64_f64 (the frame-pair kernels' delay-structured gains; sep_ok: its check against the per-bin table das_mic_gains_w64_f64, host only, held, with the bound it
    // used and the worst deviation it saw)
    struct DasTables { DeviceBuffer<f64x2> gains_w64, gains_sep; DasSlots slots; bool sep_ok = false; double sep_bound = 0.0, sep_worst = 0.0; } das_[2];
    DeviceBuffer<f64x2> d_tw_w64_;       // twiddle_table_w64_rot
    DeviceBuffer<char> d_das_sched_;     // das_f64_pair_kernel: chunk table + counter (das_f64_sched_ws_bytes())
    int steer_cur_ = 0;
    DeviceBuffer<f64x2> d_track_;        // steering tracks: [angle][mic][N], the [dir][col][mic][N] layout with one column (install_track_tables)
    DeviceBuffer<f64x2> d_track_retired_;  // the tables the last install replaced: a batch being enqueued may still name them
    int track_n_ = 0;
    DeviceBuffer<float> d_hist2_[2];  // ring hop in front of the next batch; two buffers: das_f64_pair_kernel writes the carry itself
    int hist_cur_ = 0;
    DeviceBuffer<float> d_tail_[2];
    int tail_cur_ = 0;
    DeviceBuffer<char> d_zhist_;     // [stream][Phist][NP][N] elements of zsz_ bytes: packed spectra of the previous Phist frames
    DeviceBuffer<f64x2> d_gssW_;     // [stream][bin][KP1][M]
    DeviceBuffer<double> d_mpf_;     // [stream][kMpfVecs*N + 8]; gss's post-filter: [stream][row][kMpfVecs*N + 8]
    DeviceBuffer<double> d_smooth_;  // [stream][64]
    DeviceBuffer<float> d_nlms_;     // gsc: [stream][(2(M-1)+1) * filter_size]
    unsigned long long gss_reset_mask_ = ~0ull;  // look directions whose demixing matrices restart at the next run
    // workspaces (grown on demand; sized in bytes: their element follows the node and its precision)
    DeviceBuffer<char> d_Z_;        // [stream][Phist+F][NP][N] elements of zsz_ bytes
    DeviceBuffer<char> d_Yh_;       // [stream][F][YS_] f64x2 (+ one double per problem behind them for phasempf)
    DeviceBuffer<float> d_yraw_;
    DeviceBuffer<float> d_planar_;  // das in double on [sample][mic] input: the frame-pair kernel's hop rings, or the batch (+ carried hop) transposed
    DeviceBuffer<float> d_frames_;  // N != 1024: windowed frames between the generic ISTFT and its overlap-add
};

// das at the reference's precision on the tuned shape, no spectrum dump: ONE launch, spectra never leave the CU.  Decide (das_f64_plan.hpp
// das_f64_decide: a pure function of the batch's shape, the steering summary and the two switches names the kernel or declines), reserve the
// scratch, fill the argument block, enqueue (das_f64_w64.hip), flip the double buffers.  BF_FUSED_BINS=0 keeps the chain (cross-checks).
// BF_OK: handled; kDeclined: run_chain serves the batch; an error otherwise.
int BinPipelineImpl::run_das_one_launch(const float *x, long F, float *y, hipStream_t stream, int layout, long mic_stride, const RunSnapshot &snap) {
    const Switches &sw = switches();
    if (!das_one_launch_shape() || sw.fused_bins != 1 || snap.das.gains_w64 == nullptr) return kDeclined;
    const DasSlots &sl = snap.das.slots;
    const DasF64Launch d = das_f64_decide(DasF64Shape{layout, M_, S_, n_cus_, F, sl.mic0_unit, snap.das.gains_sep && d_das_sched_.get(), sl.n_tr,
                                                      sw.das_il_ring, sw.das_f64_sched});
    if (d.path == DasF64Path::kChain) return kDeclined;
    ENGINE_HIP(d_planar_.reserve((d.scratch_bytes + sizeof(float) - 1) / sizeof(float)));
    float *const hist = d_hist2_[hist_cur_].get();
    DasF64Args da;
    da.x = x; da.hist = hist; da.hist_out = d_hist2_[hist_cur_ ^ 1].get(); da.y = y;
    da.tail_in = d_tail_[tail_cur_].get(); da.tail_out = d_tail_[tail_cur_ ^ 1].get();
    da.win = d_win_.get(); da.n_frames = F; da.mic_stride = mic_stride;
    da.stream_stride_x = (long)M_ * F * H_; da.n_streams = S_; da.n_mics = M_; da.run_len = 1; da.layout = layout;
    da.gains = snap.das.gains_w64; da.gains_sep = snap.das.gains_sep; da.tw = d_tw_w64_.get();
    da.mic0_unit = sl.mic0_unit ? 1 : 0; da.n_tr = sl.n_tr; da.extra_mic = sl.extra_mic;
    for (int k = 0; k < 8; ++k) da.slot_mic[k] = sl.slot_mic[k];
    da.sched_ws = d_das_sched_.get(); da.sched_ws_bytes = d_das_sched_.get() ? das_f64_sched_ws_bytes() : 0;
    ENGINE_HIP(enqueue_das_f64(da, d, d_planar_.get(), stream, kev0, kev1, &kev_recorded));
    if (d.writes_hist)
        hist_cur_ ^= 1;  // das_f64_pair_kernel stored the last hop into the other buffer
    else  // the carried hop stays in the handle's layout
        ENGINE_HIP(carry_last_hop(hist, x, F, H_, M_, S_, layout, mic_stride, (long)F * H_ * M_, stream));
    tail_cur_ ^= 1;
    return BF_OK;
}

int BinPipelineImpl::run(const float *x, long F, float *y, f64x2 *spectrum, hipStream_t stream, int layout, long mic_stride,
                         const RunSnapshot &snap) {
    // (a tracked batch never takes the one-launch kernels: the frame-pair kernel puts two frames, so two tables, into one transform)
    const int rc = (spectrum || snap.track) ? kDeclined : run_das_one_launch(x, F, y, stream, layout, mic_stride, snap);
    return rc == kDeclined ? run_chain(x, F, y, spectrum, stream, layout, mic_stride, snap) : rc;
}

int BinPipelineImpl::run_chain(const float *x, long F, float *y, f64x2 *spectrum, hipStream_t stream, int layout, long mic_stride,
                               const RunSnapshot &snap) {
    // One pass over the whole batch: cutting it into Infinity-Cache-sized frame tiles was measured (3.9-12 ms for mvdr instead of
    // 3.0: per-tile launches underfill the chip and the per-bin kernels lose their parallelism over time) -- DESIGN.md 3.2
    const Switches &sw = switches();
    // everything this batch launches, its row formats and workspace sizes: decided once, from values (chain_plan.hpp)
    const ChainShape shape{cfg_.algo, N_, layout, M_, S_, cfg_.n_dirs > 1 ? cfg_.n_dirs : 1, snap.kp1, cfg_.past_windows,
                           cfg_.precision, spectrum != nullptr, F, n_cus_, cfg_.gsc_filter_size, cfg_.smooth_size,
                           band_.yh_lo, band_.yh_hi, (reinterpret_cast<size_t>(y) & 15) == 0, sw.fused_bins,
                           sw.stft_small, sw.stft_split, sw.mvdr_group, sw.gss_group, sw.gsc_serial, cfg_.algo == BF_GSS ? R_ : 1,
                           snap.track != nullptr && snap.track_cols == 0, snap.track != nullptr ? snap.track_cols : 0, post_filter_ ? 1 : 0,
                           cfg_.algo == BF_LCMV ? R_ : 1, sw.mvdr_tile};
    ChainPlan p = chain_decide(shape);
    // ... and how it is cut into runs, tiles and rounds, with every grid (chain_geom.hpp); a batch whose geometry does not fit the kernels'
    // integers is refused here, before anything is enqueued
    p.geom = chain_geom(shape, p, band_);
    if (!p.geom.ok) {
        err_ = "batch too large: a run, tile or grid count of its launch geometry exceeds what the kernels take";
        return BF_EINVAL;
    }
    float *const hist = d_hist2_[hist_cur_].get();
    const long FT = Phist_ + F;  // frames in the Z workspace per stream
    ENGINE_HIP(d_Z_.reserve(p.z_bytes));
    ENGINE_HIP(d_Yh_.reserve(p.yh_bytes));
    ENGINE_HIP(d_yraw_.reserve(p.yraw_elems));
    ENGINE_HIP(d_frames_.reserve(p.frames_elems));
    f64x2 *const Z = (f64x2 *)d_Z_.get();
    f64x2 *const Yh = (f64x2 *)d_Yh_.get();
    const size_t frame_elems = (size_t)NP_ * N_;

    // covariance history in front of the new frames
    if (Phist_ > 0)
        ENGINE_HIP(hipMemcpy2DAsync(Z, (size_t)FT * frame_elems * zsz_, d_zhist_.get(), (size_t)Phist_ * frame_elems * zsz_,
                                  (size_t)Phist_ * frame_elems * zsz_, (size_t)S_, hipMemcpyDeviceToDevice, stream));

    StftArgs sa;
    sa.x = x; sa.hist = hist; sa.Z = Z; sa.tw = d_tw_.get(); sa.win = d_win_.get();
    sa.n_frames = F; sa.frames_ws = FT; sa.frame_off = Phist_; sa.mic_stride = mic_stride;
    sa.stream_stride_x = (long)M_ * F * H_; sa.n_streams = S_; sa.n_mics = M_; sa.n_fft_mics = MF_; sa.layout = layout;
    sa.skip_lo = band_.skip_lo; sa.skip_hi = band_.skip_hi;
    sa.z48 = p.z48 ? 1 : 0; sa.run_len = 1; sa.tw_w64 = d_tw_w64_.get();
    sa.halve = cov_node_ ? 1 : 0;
    if (time_node_ && spectrum) {  // time-domain node: there is no single y_fft; the dump reads as zeros
        ENGINE_HIP(hipMemsetAsync(spectrum, 0, (size_t)S_ * F * N_ * sizeof(f64x2), stream));
        spectrum = nullptr;
    }
    // Backward transform.  BF_PRECISION_REFERENCE (the default): in double behind every node (istft_w64_kernel at N = 1024: with it the float
    // output of das, phase, phasempf, gss and mcra equals the oracle's bit for bit).  BF_PRECISION_MIXED: in fp32 (istft32_kernel) wherever
    // the per-bin stage can emit f32x2 rows: mvdr / lcmv (band-limited rows: half the row traffic, no zero-fill), das / phase through the
    // bin pipeline, phasempf.  gsc (its sample-serial NLMS branches on the aligned signals), a spectrum dump and the other FFT sizes: always
    // in double.
    BinsArgs ba;
    ba.Z = Z; ba.Yh = Yh; ba.spectrum = spectrum; ba.steer = snap.steer; ba.freqs = d_freq_.get();
    ba.n_frames = F; ba.frames_ws = FT; ba.frame_off = Phist_; ba.n_streams = So_; ba.n_mics = MF_; ba.kp1 = snap.kp1;
    ba.n_dirs = D_; ba.steer_dir_stride = snap.steer_dir_stride;
    ba.z48 = p.z48 ? 1 : 0;
    ba.cfg = cfg_; ba.gssW = d_gssW_.get(); ba.mpf = d_mpf_.get(); ba.gss_reset_mask = snap.gss_reset_mask;
    ba.yh32 = p.yh32 ? 1 : 0; ba.mpf32 = p.mpf32 ? 1 : 0; ba.yh_lo = p.yh_lo; ba.yh_hi = p.yh_hi;
    ba.gss_rows = p.rows;
    if (p.track || p.ctrack) {  // the per-frame table: tables + track[stream][frame] * stride where the index names a table, ba.steer otherwise
        ba.track = snap.track; ba.track_tables = snap.track_tables; ba.track_n = snap.track_n; ba.track_stride = (long)M_ * N_;
        ba.track_cols = p.ctrack ? snap.track_cols : 0;  // mvdr / lcmv: an index per frame and constraint column
    }
    if (p.rec_istft()) {  // mpf_rec_istft_kernel: a block per stream, the y_fft rows stay in LDS
        ba.rec_istft = 1;
        ba.rec_y = d_yraw_.get(); ba.rec_tail_in = d_tail_[tail_cur_].get(); ba.rec_tail_out = d_tail_[tail_cur_ ^ 1].get();
        ba.rec_tw_w64 = d_tw_w64_.get(); ba.rec_win = d_win_.get();
    }
    IstftArgs ia;
    ia.Yh = Yh; ia.y = yraw_target_ ? d_yraw_.get() : y; ia.tail_in = d_tail_[tail_cur_].get();
    ia.tail_out = d_tail_[tail_cur_ ^ 1].get(); ia.tw = d_tw_.get(); ia.win = d_win_.get(); ia.n_frames = F;
    ia.n_streams = So_ * p.rows;  // gss, lcmv with several beams: every row of a beam is an output stream (beam * rows + r) with its own overlap-add tail
    ia.tw32 = d_tw32_.get();
    ia.tw_w64 = d_tw_w64_.get();
    ia.yh32 = ba.yh32; ia.yh_lo = ba.yh_lo; ia.yh_hi = ba.yh_hi;
    if (p.mpf32) {  // rows of 8-byte elements behind the f64x2 rows (where aux lives), every problem written
        ia.Yh = Yh + (size_t)So_ * F * YS_;
        ia.yh32 = 1; ia.yh_lo = 0; ia.yh_hi = NQ_ - 1;
    }
    ia.frames = d_frames_.get();
    ia.post_amp = post_amp_ ? cfg_.out_amp : 1.0;
    ia.use_post_amp = post_amp_ ? 1 : 0;
    // das in double promises the same bytes for every cut of a stream.  The backward transform sees spectra, not hops: it cannot tell a frame
    // that straddles a change of level (das_f64_plan.hpp das_f64_may_pair), so behind das every frame goes alone
    if (cfg_.algo == BF_DAS) ia.pair_span = -1;

    if (p.fused())
        ENGINE_HIP(ks_->stft_bins(p, sa, ba, n_cus_, stream));
    else
        ENGINE_HIP(ks_->stft(p, sa, n_cus_, stream));
    ENGINE_HIP(carry_last_hop(hist, x, F, H_, M_, S_, layout, mic_stride, (long)F * H_ * M_, stream));
    if (!p.fused()) ENGINE_HIP(ks_->bins(p, ba, n_cus_, stream));
    if (p.postfilter) ENGINE_HIP(ks_->gss_postfilter(p, ba, stream));  // gss: the rows are filtered in place in front of the dump and the backward transform
    if (Phist_ > 0)  // keep the last Phist frames' spectra for the next call
        ENGINE_HIP(hipMemcpy2DAsync(d_zhist_.get(), (size_t)Phist_ * frame_elems * zsz_, (const char *)Z + (size_t)F * frame_elems * zsz_,
                                  (size_t)FT * frame_elems * zsz_, (size_t)Phist_ * frame_elems * zsz_, (size_t)S_,
                                  hipMemcpyDeviceToDevice, stream));
    if (p.istft != ChainIstft::kNone) ENGINE_HIP(ks_->istft(p, ia, n_cus_, stream));
    tail_cur_ ^= 1;
    if (p.tail == ChainTail::kSmooth4 || p.tail == ChainTail::kSmooth)
        ENGINE_HIP(ks_->smooth(p, d_yraw_.get(), y, d_smooth_.get(), F, So_, stream));
    else if (p.tail != ChainTail::kNone)
        ENGINE_HIP(ks_->gsc_nlms(p, d_yraw_.get(), y, d_nlms_.get(), F * H_, S_, M_, cfg_, stream));
    return BF_OK;
}

}  // namespace

Engine *Engine::create(const bf_config &cfg, int n_cus) {
    if (cfg.algo == BF_DAS && cfg.das_impl == BF_DAS_FUSED_F32) return make_das_fused_engine(cfg, n_cus);
    return new BinPipelineImpl(cfg, n_cus);
}

}  // namespace bf
