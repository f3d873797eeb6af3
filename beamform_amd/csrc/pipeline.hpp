// pipeline.hpp -- the engine behind a bf_handle: what capi.cpp drives, whatever the node.  Two implementations:
//   the fused fp32 das kernels (das_fused_engine.cpp), one launch per batch, and
//   the fp64 "bin pipeline" of every other node (pipeline.hip):
//     STFT kernel (window + forward FFTs, spectra to HBM)
//     -> per-bin kernel (the node's apply_weights loop body)
//     -> ISTFT kernel (backward FFT, synthesis window, overlap-add).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/bfcore.h"
#include "geometry.hpp"

namespace bf {

// das in double in one launch: the gain tables of the batch's steering table and what the kernel has to know about it
struct DasSnapshot {
    // das_pair_gains_w64_f64: pair gains in the register / lane order of the 64-lane kernel (das_f64_w64.hip); das_mic_gains_w64_f64:
    // per-microphone Hermitian gains, one entry per bin (host only); das_sep_gains_w64_f64: the same gains delay-structured, what the
    // frame-pair kernels (das_f64_pair_kernel, das_f64_ring_kernel) read -- null where the table is not a delay in every row (the host's check)
    const f64x2 *gains_w64 = nullptr, *gains_sep = nullptr;
    DasSlots slots;  // geometry.hpp das_f64_slots of that table
};

// What one run() reads of the state the control plane (bf_set_theta / bf_set_interference, another thread) may change:
// taken under the handle's mutex right after the table upload, so a batch sees ONE consistent
// {column count, steering table, pending demixing resets} (the reference guards the same window with READY=false
// plus a sleep, lcmv.cpp:262-307).
struct RunSnapshot {
    int kp1 = 1;
    unsigned long long gss_reset_mask = 0;
    const f64x2 *steer = nullptr;
    long steer_dir_stride = 0;
    DasSnapshot das;
    // steering tracks (bf_track_set_angles): the installed tables [angle][mic][N] and their count, taken with the rest; `track` is not the
    // engine's: the caller of run() points it at the batch's [stream][frame] indices (null: an untracked batch)
    const f64x2 *track_tables = nullptr;
    int track_n = 0;
    const int32_t *track = nullptr;
    // > 0: `track` is a column track, [stream][frame][track_cols] (bf_process_batch_device_ctracked; mvdr / lcmv)
    int track_cols = 0;
};

class Engine {
   public:
    // the fused fp32 das engine for BF_DAS with BF_DAS_FUSED_F32, the bin pipeline otherwise; never null
    static Engine *create(const bf_config &cfg, int n_cus);
    virtual ~Engine() {}
    virtual int init() = 0;
    virtual int reset(hipStream_t stream) = 0;  // clears enqueued on `stream`
    // one set per look direction; stream-ordered and double-buffered, so a batch already in flight keeps reading the table it was launched with
    virtual int upload_steering(const std::vector<SteeringSet> &dirs, hipStream_t stream) = 0;
    virtual void on_theta_changed(int dir = -1) = 0;  // dir < 0: every look direction
    virtual void set_columns(int kp1) = 0;  // interferer added/removed (lcmv.cpp:266-305)
    // steering tracks: can this engine weight every frame of a batch with a table of its own (das in double, phase, phasempf on the bin
    // pipeline, one look direction)?  install_track_tables replaces the tables a tracked run() chooses from: `tables` = [n_angles][mic][N]
    // on the host, n_angles = 0 drops them.  Host-synchronous (waits for the device); the replaced tables stay allocated until the next
    // call, so a run() another thread is still enqueueing with them in its snapshot reads live memory.  Caller holds the control-plane mutex
    virtual bool can_track() const { return false; }
    // column tracks (mvdr / lcmv with one look direction: a table index per frame and constraint column); the tables are installed by
    // the same install_track_tables
    virtual bool can_ctrack() const { return false; }
    virtual int install_track_tables(const std::vector<f64x2> &, int) {
        err_ = "steering tracks: das in double, phase and phasempf with one look direction";
        return BF_ENOSYS;
    }
    // caller holds the control-plane mutex: hands the pending demixing resets to this run and clears them
    virtual RunSnapshot snapshot_for_run() = 0;
    virtual int run(const float *x_dev, long n_frames, float *y_dev, f64x2 *spectrum_dev, hipStream_t stream, int layout,
                    long mic_stride, const RunSnapshot &snap) = 0;
    // checkpoint of the control-plane side (caller holds the mutex)
    virtual int columns() const = 0;
    virtual unsigned long long pending_resets() const = 0;
    virtual void set_pending_resets(unsigned long long mask) = 0;
    virtual size_t state_bytes() const = 0;
    virtual int get_state(void *host) = 0;
    virtual int set_state(const void *host) = 0;
    const std::string &error() const { return err_; }
    // set by the caller around run(): when non-null and the run has ONE dominant kernel (fused fp32 das; das fp64 in one launch), the two
    // events are recorded on the run's stream right before and after that launch (or its launches, one per 16 look directions) and
    // kev_recorded is raised once the second record has succeeded (bf_kernel_timing_begin / _end)
    hipEvent_t kev0 = nullptr, kev1 = nullptr;
    bool kev_recorded = false;

   protected:
    std::string err_;
};

Engine *make_das_fused_engine(const bf_config &cfg, int n_cus);  // das_fused_engine.cpp

// inside a member of an Engine: a failed HIP call becomes error() = "<call>: <HIP string>" and BF_EIO
#define ENGINE_HIP(call)                                                      \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            err_ = std::string(#call) + ": " + hipGetErrorString(e_);         \
            return BF_EIO;                                                    \
        }                                                                     \
    } while (0)

}  // namespace bf
