// das_fused_engine.cpp -- the engine of BF_DAS with BF_DAS_FUSED_F32: tables and carried state of the fused fp32 das kernels; which
// kernel serves a batch and in which runs: das_fused_plan.hpp.  The 512-frame period has the register-resident kernels (32 x 32
// in-register FFT-1024, das_fused.hip), which also take the shorter periods as groups of interleaved frames; the longer ones the
// kernels on LDS-staged transforms (das_fused_gen.hip) or, at 1024 frames, a wavefront per 2048-point frame.  Host work here is
// start-up / control-plane only; every per-frame operation runs in the gfx950 kernels.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "device_mem.hpp"
#include "kernels.hpp"
#include "pipeline.hpp"
#include "switches.hpp"

namespace bf {
namespace {

class FusedDasEngine : public Engine {
   public:
    FusedDasEngine(const bf_config &c, int n_cus)
        : M_(c.n_mics), H_(c.hop), N_(2 * c.hop), S_(c.n_streams), D_(c.n_dirs > 1 ? c.n_dirs : 1), So_(S_ * D_), n_cus_(n_cus), gen_(c.hop != 512) {}

    int init() override {
        const size_t np = (size_t)(M_ + 1) / 2;
        for (auto &g : d_gains_) ENGINE_HIP(g.alloc(np * N_ * D_));
        // period 512: inter-pass twiddles of the 32 x 32 factorisation; others: W^m, m < N/2, + the per-pass radix-4 blocks (geometry.hpp)
        ENGINE_HIP(d_twiddle_.upload(gen_ ? stockham_twiddles<f32x2>(N_) : twiddle_table_32x32<f32x2>()));
        if (N_ < 1024) {  // the tables of group mode (das_fused_plan.hpp: group_tables)
            ENGINE_HIP(d_twiddle_1024_.upload(twiddle_table_32x32<f32x2>()));
            for (auto &g : d_gains_il_) ENGINE_HIP(g.alloc(np * 1024 * D_));
        }
        const std::vector<double> hd = sqrt_hann(N_);
        ENGINE_HIP(d_window_.upload(std::vector<float>(hd.begin(), hd.end())));
        ENGINE_HIP(d_zeros_.alloc(2048));
        ENGINE_HIP(hipMemset(d_zeros_.get(), 0, 2048 * sizeof(float)));
        for (auto &b : d_hist_) ENGINE_HIP(b.alloc(hist_elems()));
        for (auto &b : d_tail_) ENGINE_HIP(b.alloc(tail_elems()));
        return BF_OK;
    }

    // prepare_overlap_and_add: ring pre-filled with one hop of zeros, out_buff calloc'ed (util.h:272-286)
    int reset(hipStream_t s) override {
        for (auto &b : d_hist_) ENGINE_HIP(hipMemsetAsync(b.get(), 0, hist_elems() * sizeof(float), s));
        for (auto &b : d_tail_) ENGINE_HIP(hipMemsetAsync(b.get(), 0, tail_elems() * sizeof(float), s));
        tail_cur_ = 0;
        return BF_OK;
    }

    int upload_steering(const std::vector<SteeringSet> &dirs, hipStream_t s) override {
        const int np = (M_ + 1) / 2;
        const bool il = N_ < 1024;  // as init() allocated them
        std::vector<f32x2> g, gil;  // [dir][pair][N], [dir][pair][1024]
        for (const SteeringSet &st : dirs) {
            if (il) {
                const std::vector<f32x2> gi = das_pair_gains_interleaved(st, np);
                gil.insert(gil.end(), gi.begin(), gi.end());
            }
            const std::vector<f32x2> gd = gen_ ? das_pair_gains_natural(st, np) : das_pair_gains(st, np);
            g.insert(g.end(), gd.begin(), gd.end());
        }
        const int nxt = gains_cur_ ^ 1;
        ENGINE_HIP(hipMemcpyAsync(d_gains_[nxt].get(), g.data(), g.size() * sizeof(f32x2), hipMemcpyHostToDevice, s));
        if (il) ENGINE_HIP(hipMemcpyAsync(d_gains_il_[nxt].get(), gil.data(), gil.size() * sizeof(f32x2), hipMemcpyHostToDevice, s));
        ENGINE_HIP(hipStreamSynchronize(s));  // pageable staging vectors go out of scope
        gains_cur_ = nxt;
        return BF_OK;
    }

    // das has one constraint column and no demixing matrices
    void on_theta_changed(int) override {}
    void set_columns(int) override {}
    RunSnapshot snapshot_for_run() override { return RunSnapshot(); }
    int columns() const override { return 1; }
    unsigned long long pending_resets() const override { return 0; }
    void set_pending_resets(unsigned long long) override {}

    int run(const float *x, long F, float *y, f64x2 *spectrum, hipStream_t s, int layout, long mic_stride, const RunSnapshot &) override;

    // checkpoint payload: the carried hop, then the overlap-add tail
    size_t state_bytes() const override { return (hist_elems() + tail_elems()) * sizeof(float); }
    int get_state(void *host) override {
        ENGINE_HIP(hipMemcpy(host, d_hist_[tail_cur_].get(), hist_elems() * sizeof(float), hipMemcpyDeviceToHost));
        ENGINE_HIP(hipMemcpy((float *)host + hist_elems(), d_tail_[tail_cur_].get(), tail_elems() * sizeof(float), hipMemcpyDeviceToHost));
        return BF_OK;
    }
    int set_state(const void *host) override {
        ENGINE_HIP(hipMemcpy(d_hist_[tail_cur_].get(), host, hist_elems() * sizeof(float), hipMemcpyHostToDevice));
        ENGINE_HIP(hipMemcpy(d_tail_[tail_cur_].get(), (const float *)host + hist_elems(), tail_elems() * sizeof(float), hipMemcpyHostToDevice));
        return BF_OK;
    }

   private:
    size_t hist_elems() const { return (size_t)S_ * M_ * H_; }
    size_t tail_elems() const { return (size_t)So_ * H_; }

    const int M_, H_, N_, S_, D_, So_, n_cus_;  // microphones, hop, FFT size, input streams, look directions, output streams
    const bool gen_;                            // every period but 512: das_fused_gen.hip and its tables
    DeviceBuffer<f32x2> d_gains_[2];            // double-buffered: a batch in flight keeps the table it was launched with
    int gains_cur_ = 0;
    DeviceBuffer<f32x2> d_twiddle_;
    DeviceBuffer<f32x2> d_gains_il_[2];   // hop < 512: das_pair_gains_interleaved tables (das_fused.hip, group mode), double-buffered with d_gains_
    DeviceBuffer<f32x2> d_twiddle_1024_;  // hop < 512: twiddle_table_32x32 (the frame-interleaving kernel runs the 1024-point machinery)
    DeviceBuffer<float> d_window_, d_zeros_;
    DeviceBuffer<float> d_hist_[2];  // the hop before the next frame (the reference's ring buffer content)
    DeviceBuffer<float> d_tail_[2];
    int tail_cur_ = 0;  // index of the valid hist/tail pair; the kernel writes the other one
    DeviceBuffer<f32x2> d_sdump_;  // spectrum dump: the kernels' accumulated pair spectra, grown on demand
};

int FusedDasEngine::run(const float *x, long F, float *y, f64x2 *spectrum, hipStream_t s, int layout, long mic_stride, const RunSnapshot &) {
    const Switches &sw = switches();
    const DasFusedLaunch d = das_fused_decide(H_, layout, M_, S_, D_, spectrum != nullptr, F, n_cus_, sw.das_interleave, sw.das_split2048, sw.das_shared_dirs);

    if (spectrum) ENGINE_HIP(d_sdump_.reserve((size_t)So_ * F * N_));

    DasFusedArgs a;
    a.x = x;
    a.hist_in = d_hist_[tail_cur_].get();
    a.hist_out = d_hist_[tail_cur_ ^ 1].get();
    a.y = y;
    a.tail_in = d_tail_[tail_cur_].get();
    a.tail_out = d_tail_[tail_cur_ ^ 1].get();
    a.gains = d.group_tables ? d_gains_il_[gains_cur_].get() : d_gains_[gains_cur_].get();
    a.twiddle = d.group_tables ? d_twiddle_1024_.get() : d_twiddle_.get();
    a.window = d_window_.get();
    a.zeros = d_zeros_.get();
    a.sdump = spectrum ? d_sdump_.get() : nullptr;
    a.n_frames = F;
    a.mic_stride = mic_stride;
    a.stream_stride_x = (long)M_ * F * H_;
    a.n_streams = So_;
    a.n_dirs = D_;
    a.n_mics = M_;
    a.frames_per_chunk = d.frames_per_chunk;
    a.chunks_per_stream = d.chunks_per_stream;
    a.layout = layout;
    a.group = d.group;
    ENGINE_HIP(enqueue_das_fused(a, d, N_, s, kev0, kev1, &kev_recorded));
    tail_cur_ ^= 1;

    if (spectrum)
        ENGINE_HIP(gen_ ? launch_das_hermitian_dump_gen(d_sdump_.get(), spectrum, (long)So_ * F, N_, s)
                        : launch_das_hermitian_dump(d_sdump_.get(), spectrum, (long)So_ * F, s));
    return BF_OK;
}

}  // namespace

Engine *make_das_fused_engine(const bf_config &cfg, int n_cus) { return new FusedDasEngine(cfg, n_cus); }

}  // namespace bf
