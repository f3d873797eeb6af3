// capi.cpp -- the C ABI of libbfcore.so (include/bfcore.h) and the host-side
// state a reference node keeps in file-scope globals (util.h:24-50, das.cpp:15-25).
//
// Host work done here is start-up / control-plane only (geometry, steering
// weights in double precision, table upload, launch sizing); every per-frame
// operation runs in the gfx950 kernels.  There is no CPU compute fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <cxxabi.h>

#include "../../include/bfcore.h"
#include "device_mem.hpp"
#include "doa.hpp"
#include "geometry.hpp"
#include "kernels.hpp"
#include "launch_trace.hpp"
#include "pipeline.hpp"

using namespace bf;

static thread_local std::string g_last_error;
// what bf_last_error(NULL) reports; the handles of other files (doa.cpp) record their errors here too
void bf::set_last_error(const std::string &msg) { g_last_error = msg; }

// ---- launch trace (launch_trace.hpp): the kernels the calling thread launches between bf_trace_begin and bf_trace_end ----------
static thread_local std::vector<const void *> *g_trace = nullptr;
void bf::trace_note(const void *host_fn) {
    if (g_trace) g_trace->push_back(host_fn);
}

struct bf_handle {
    bf_config cfg;
    int M = 0, H = 0, N = 0, S = 1, n_streams = 1;  // n_streams: input streams
    int n_dirs = 1, n_out = 1;                      // look directions per input stream; output streams = n_streams * n_dirs * n_rows
    int n_rows = 1;                                 // gss: separated sources emitted per beam (bf_config.gss_out_sources); lcmv: beams (lcmv_out_beams)
    int device = 0, n_cus = 256;
    std::string err;

    // control plane (guarded by mu): what update_weights() owns in the reference
    std::mutex mu;
    ArrayGeometry geo;
    std::vector<double> freqs;
    std::vector<SteeringSet> steer;  // one per look direction
    std::vector<double> angle;       // /theta of every look direction
    std::vector<double> interf;
    bool tables_dirty = true;

    // the node's device side: the fused fp32 das kernels or the bin pipeline (pipeline.hpp); never null once bf_create has succeeded
    std::unique_ptr<Engine> engine;
    DeviceBuffer<double> d_sumsq;  // bf_stream_rms scratch

    // staging for the host-buffer entry points
    DeviceBuffer<float> d_x, d_y;  // grown on demand
    // bf_process_batch pipelining: copies on their own streams, chunk by chunk, around the compute stream
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    std::vector<hipEvent_t> ev_in, ev_out;
    PinnedBuffer<float> h_pin;  // pinned [n_mics*hop | n_out*hop]: bf_process_hop stages through it (no pageable-copy detour)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // per-launch timing of the dominant kernel: a pool of event pairs, created on demand (bf_kernel_timing_begin reserves a batch so
    // that the caller's timed loop only records), reused by every session and destroyed with the handle
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    int timing = 0;  // 0: off; 1: bf_kernel_timing_begin .. _end; 2: inside bf_time_batch_device
    bool row0_written = true;  // reference-mic weight row: written by the cold start's update_weights(true), left zero by a
                               // structural interferer change (quirk Q3, lcmv.cpp:243-252,281,304)
};

namespace {

int fail(bf_handle *h, int code, const char *what, hipError_t e = hipSuccess) {
    std::string msg = what ? what : "";
    if (e != hipSuccess) {
        msg += ": ";
        msg += hipGetErrorString(e);
    }
    if (h) h->err = msg;
    g_last_error = msg;
    return code;
}

#define BF_HIP(h, call)                                                  \
    do {                                                                 \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) return fail((h), BF_EIO, #call, e_);       \
    } while (0)

// update_weights(): recompute every steering column from the current angles.
void rebuild_steering(bf_handle *h, bool first, int only_dir = -1) {
    for (int d = 0; d < h->n_dirs; ++d) {
        if (only_dir >= 0 && d != only_dir) continue;
        h->steer[d].update_column(h->geo, h->freqs, 0, h->angle[d], first);
        for (int k = 0; k < h->S - 1; ++k) h->steer[d].update_column(h->geo, h->freqs, k + 1, h->interf[k], first);
    }
    h->tables_dirty = true;
}

// Upload whatever set_theta changed; stream-ordered, double-buffered so a batch
// already in flight keeps reading the table it was launched with.
int sync_tables(bf_handle *h, hipStream_t s, RunSnapshot *snap) {
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->tables_dirty) {
        int rc = h->engine->upload_steering(h->steer, s);
        if (rc != BF_OK) return fail(h, rc, h->engine->error().c_str());
        h->tables_dirty = false;
    }
    // one consistent view of {columns, table, pending gss resets} for this batch, taken under the same lock
    *snap = h->engine->snapshot_for_run();
    return BF_OK;
}

// Event pair for the next launch of the dominant kernel (both null when no timing session is active).
int timing_reserve(bf_handle *h, size_t n) {
    while (h->ev_pool.size() < n) {
        hipEvent_t k0 = nullptr, k1 = nullptr;
        BF_HIP(h, hipEventCreate(&k0));
        hipError_t e = hipEventCreate(&k1);
        if (e != hipSuccess) {
            (void)hipEventDestroy(k0);
            return fail(h, BF_EIO, "hipEventCreate", e);
        }
        h->ev_pool.push_back(std::make_pair(k0, k1));
    }
    return BF_OK;
}
int timing_acquire(bf_handle *h, hipEvent_t *k0, hipEvent_t *k1) {
    *k0 = *k1 = nullptr;
    if (!h->timing) return BF_OK;
    int rc = timing_reserve(h, h->ev_used + 1);
    if (rc != BF_OK) return rc;
    *k0 = h->ev_pool[h->ev_used].first;
    *k1 = h->ev_pool[h->ev_used].second;
    ++h->ev_used;
    return BF_OK;
}
// mean duration of the pairs recorded since the session began; ends the session
int timing_collect(bf_handle *h, float *ms_mean, int *n_launches) {
    float sum = 0.f;
    int n = 0;
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < h->ev_used; ++i) {
        float t = 0.f;
        if (e == hipSuccess) e = hipEventSynchronize(h->ev_pool[i].second);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, h->ev_pool[i].first, h->ev_pool[i].second);
        if (e == hipSuccess) { sum += t; ++n; }
    }
    h->ev_used = 0;
    h->timing = 0;
    if (e != hipSuccess) return fail(h, BF_EIO, "kernel timing", e);
    *ms_mean = n ? sum / (float)n : 0.f;
    if (n_launches) *n_launches = n;
    return BF_OK;
}

// track (nullable): the batch's steering track, [stream][frame] indices into the tables bf_track_set_angles installed; with track_cols > 0
// a column track, [stream][frame][track_cols] indices into the tables bf_ctrack_set_angles installed
int run_batch_device(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *spectrum_dev, hipStream_t s,
                     int layout, long mic_stride, const int32_t *track = nullptr, int track_cols = 0) {
    if (n_frames == 0) return BF_OK;
    RunSnapshot snap;
    int rc = sync_tables(h, s, &snap);
    if (rc != BF_OK) return rc;
    if (track) {
        if (snap.track_n == 0)
            return fail(h, BF_EINVAL, track_cols > 0 ? "column-tracked batch: no track angles installed (bf_ctrack_set_angles)"
                                                     : "tracked batch: no track angles installed (bf_track_set_angles)");
        if (track_cols > snap.kp1) return fail(h, BF_EINVAL, "column-tracked batch: n_cols above the handle's column count");
        snap.track = track;
        snap.track_cols = track_cols;
    }
    // the engine brackets its dominant kernel with this pair when it has one (fused fp32 das, das fp64 in one launch); otherwise the pair
    // stays unrecorded and the session's mean is taken over nothing (callers fall back to the call time)
    hipEvent_t k0 = nullptr, k1 = nullptr;
    rc = timing_acquire(h, &k0, &k1);
    if (rc != BF_OK) return rc;
    Engine *eng = h->engine.get();
    eng->kev0 = k0;
    eng->kev1 = k1;
    eng->kev_recorded = false;
    rc = eng->run(x_dev, (long)n_frames, y_dev, (f64x2 *)spectrum_dev, s, layout, mic_stride, snap);
    eng->kev0 = eng->kev1 = nullptr;
    if (k0 && !eng->kev_recorded) --h->ev_used;  // nothing was bracketed, or a launch failed between the two records: hand the pair back
    if (rc != BF_OK) return fail(h, rc, eng->error().c_str());
    return BF_OK;
}

}  // namespace

extern "C" {

const char *bf_version(void) { return "bfcore-mi355x 0.1 (gfx950)"; }

const char *bf_strerror(int code) {
    switch (code) {
        case BF_OK: return "ok";
        case BF_EINVAL: return "invalid argument or configuration";
        case BF_ENOMEM: return "out of memory";
        case BF_ENODEV: return "no usable HIP device (this library has no CPU fallback)";
        case BF_ENOSYS: return "algorithm or variant not available in this build";
        case BF_EIO: return "HIP runtime error";
        case BF_ENOENT: return "file not found";
        default: return "unknown error";
    }
}

const char *bf_last_error(const bf_handle *h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int bf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bf_create(const bf_config *cfg, bf_handle **out) {
    if (!cfg || !out) return BF_EINVAL;
    *out = nullptr;
    if (cfg->algo < BF_DAS || cfg->algo > BF_GSC) return fail(nullptr, BF_EINVAL, "algo out of range");
    if (cfg->n_mics < 1 || cfg->n_mics > BF_MAX_MICS) return fail(nullptr, BF_EINVAL, "n_mics out of range");
    if (cfg->hop < 64 || cfg->hop > 4096 || (cfg->hop & (cfg->hop - 1)) != 0)  // jackd -p takes powers of two; rosjack.cpp:131-134 whatever it reports
        return fail(nullptr, BF_ENOSYS, "hop (JACK period) must be a power of two from 64 to 4096 frames (fft_win 128 ... 8192)");
    if (cfg->n_streams < 1) return fail(nullptr, BF_EINVAL, "n_streams < 1");
    if (cfg->n_dirs < 0 || cfg->n_dirs > BF_MAX_DIRS) return fail(nullptr, BF_EINVAL, "n_dirs out of range");
    if (cfg->n_dirs > 1 && (cfg->algo == BF_MCRA || cfg->algo == BF_GSC))
        return fail(nullptr, BF_ENOSYS, "look-direction batches: mcra has no look direction, gsc is not built for them");
    if (cfg->n_interf < 0 || cfg->n_interf > BF_MAX_INTERF) return fail(nullptr, BF_EINVAL, "n_interf out of range");
    if (cfg->gss_out_sources < 0 || cfg->gss_out_sources > BF_MAX_INTERF + 1) return fail(nullptr, BF_EINVAL, "gss_out_sources out of range");
    if (cfg->gss_out_sources > 1 && cfg->algo != BF_GSS)
        return fail(nullptr, BF_EINVAL, "gss_out_sources: only gss separates sources (the other nodes have one output per beam)");
    if (cfg->lcmv_out_beams < 0 || cfg->lcmv_out_beams > BF_MAX_INTERF + 1) return fail(nullptr, BF_EINVAL, "lcmv_out_beams out of range");
    if (cfg->lcmv_out_beams > 1 && cfg->algo != BF_LCMV)
        return fail(nullptr, BF_EINVAL, "lcmv_out_beams: only lcmv has a beam per constraint column");
    if (cfg->lcmv_out_beams > 1 && cfg->gss_out_sources > 1) return fail(nullptr, BF_EINVAL, "lcmv_out_beams and gss_out_sources exclude each other");
    if (cfg->gss_postfilter != 0 && cfg->gss_postfilter != 1) return fail(nullptr, BF_EINVAL, "gss_postfilter must be 0 or 1");
    if (cfg->gss_postfilter != 0 && cfg->algo != BF_GSS)
        return fail(nullptr, BF_EINVAL, "gss_postfilter: only gss has separated sources to filter");
    if (cfg->layout != BF_PLANAR && cfg->layout != BF_INTERLEAVED) return fail(nullptr, BF_EINVAL, "layout");
    if (cfg->precision != BF_PRECISION_REFERENCE && cfg->precision != BF_PRECISION_MIXED) return fail(nullptr, BF_EINVAL, "precision");
    if (cfg->das_impl != BF_DAS_FUSED_F32 && cfg->das_impl != BF_DAS_F64) return fail(nullptr, BF_EINVAL, "das_impl");
    int ndev = bf_device_count();
    if (ndev <= 0) return fail(nullptr, BF_ENODEV, "no HIP device visible; libbfcore has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, BF_ENODEV, "device ordinal out of range");

    bf_handle *h = new bf_handle();
    h->cfg = *cfg;
    h->M = cfg->n_mics;
    h->H = cfg->hop;
    h->N = 2 * cfg->hop;
    const bool multi = (cfg->algo == BF_LCMV || cfg->algo == BF_GSS);
    h->S = multi ? cfg->n_interf + 1 : 1;
    h->n_streams = cfg->n_streams;
    h->n_dirs = cfg->n_dirs > 1 ? cfg->n_dirs : 1;
    h->cfg.n_dirs = h->n_dirs;
    h->n_rows = cfg->gss_out_sources > 1 ? cfg->gss_out_sources : cfg->lcmv_out_beams > 1 ? cfg->lcmv_out_beams : 1;
    h->n_out = h->n_streams * h->n_dirs * h->n_rows;
    h->device = cfg->device;
    h->angle.assign(h->n_dirs, cfg->theta);
    for (int k = 0; k < h->S - 1; ++k) h->interf.push_back(cfg->interf_angle[k]);

#define BF_CREATE_HIP(call)                                   \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) {                               \
            int rc_ = fail(nullptr, BF_EIO, #call, e_);       \
            bf_destroy(h);                                    \
            return rc_;                                       \
        }                                                     \
    } while (0)

    BF_CREATE_HIP(hipSetDevice(h->device));
    hipDeviceProp_t prop;
    BF_CREATE_HIP(hipGetDeviceProperties(&prop, h->device));
    h->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

    // handle_params + calculate_frequency_vector + update_weights(true)
    h->geo.set(cfg->mic_x, cfg->mic_y, h->M);
    h->freqs = frequency_vector(h->N, cfg->sample_rate);
    h->steer.resize(h->n_dirs);
    for (auto &st : h->steer) st.allocate(h->N, h->M, h->S);
    rebuild_steering(h, true);
    h->row0_written = true;

    BF_CREATE_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    BF_CREATE_HIP(hipEventCreate(&h->ev0));
    BF_CREATE_HIP(hipEventCreate(&h->ev1));

#undef BF_CREATE_HIP
    h->engine.reset(Engine::create(h->cfg, h->n_cus));
    int rc = h->engine->init();
    if (rc != BF_OK) {
        fail(nullptr, rc, h->engine->error().c_str());
        bf_destroy(h);
        return rc;
    }
    rc = bf_reset(h);
    if (rc != BF_OK) {
        bf_destroy(h);
        return rc;
    }
    *out = h;
    return BF_OK;
}

void bf_destroy(bf_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto &pr : h->ev_pool) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    for (hipEvent_t e : h->ev_in) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_out) (void)hipEventDestroy(e);
    if (h->s_h2d) (void)hipStreamDestroy(h->s_h2d);
    if (h->s_d2h) (void)hipStreamDestroy(h->s_d2h);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;  // the engine and every buffer are freed here: after the synchronisation above
}

// The clears are enqueued on `s` (hipMemsetAsync): they order against the batches the caller runs on the same stream -- a plain
// hipMemset goes to the NULL stream, which does not order against non-blocking streams (every torch.cuda.Stream is one).
int bf_reset_async(bf_handle *h, void *hip_stream) {
    if (!h) return BF_EINVAL;
    BF_HIP(h, hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);  // reset() re-arms the gss demixing reset, which /theta also writes
    int rc = h->engine->reset((hipStream_t)hip_stream);
    if (rc != BF_OK) return fail(h, rc, h->engine->error().c_str());
    return BF_OK;
}

// Host-synchronous form: the device is idle with respect to this handle before and after.
int bf_reset(bf_handle *h) {
    if (!h) return BF_EINVAL;
    BF_HIP(h, hipSetDevice(h->device));
    BF_HIP(h, hipDeviceSynchronize());
    const int rc = bf_reset_async(h, nullptr);
    if (rc != BF_OK) return rc;
    BF_HIP(h, hipStreamSynchronize(nullptr));
    return BF_OK;
}

int bf_set_theta_dir(bf_handle *h, int dir, double degrees) {
    if (!h) return BF_EINVAL;
    if (dir < 0 || dir >= h->n_dirs) return fail(h, BF_EINVAL, "look direction index out of range");
    std::lock_guard<std::mutex> lk(h->mu);
    h->angle[dir] = degrees;
    rebuild_steering(h, false, dir);
    h->engine->on_theta_changed(dir);  // gss resets that beam's demixing matrices (gss.cpp:90-93)
    return BF_OK;
}

int bf_set_theta(bf_handle *h, double degrees) { return bf_set_theta_dir(h, 0, degrees); }

int bf_set_thetas(bf_handle *h, const double *degrees, int n) {
    if (!h || !degrees) return BF_EINVAL;
    if (n < 1 || n > h->n_dirs) return fail(h, BF_EINVAL, "more angles than look directions");
    std::lock_guard<std::mutex> lk(h->mu);
    for (int d = 0; d < n; ++d) {
        h->angle[d] = degrees[d];
        rebuild_steering(h, false, d);
        h->engine->on_theta_changed(d);
    }
    return BF_OK;
}

int bf_stream_rms(bf_handle *h, const float *y_dev, size_t n_frames, double *rms_host, void *hip_stream) {
    if (!h || !y_dev || !rms_host || n_frames == 0) return BF_EINVAL;
    BF_HIP(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    BF_HIP(h, h->d_sumsq.reserve(h->n_out));
    const long n = (long)n_frames * h->H;
    BF_HIP(h, launch_stream_rms(y_dev, n, h->n_out, h->d_sumsq.get(), s));
    BF_HIP(h, hipMemcpyAsync(rms_host, h->d_sumsq.get(), sizeof(double) * h->n_out, hipMemcpyDeviceToHost, s));
    BF_HIP(h, hipStreamSynchronize(s));
    for (int i = 0; i < h->n_out; ++i) rms_host[i] = std::sqrt(rms_host[i] / (double)n);  // energy2theta.py:23-27
    return BF_OK;
}

int bf_set_interference(bf_handle *h, unsigned id, double degrees) {
    if (!h) return BF_EINVAL;
    if (h->cfg.algo != BF_LCMV && h->cfg.algo != BF_GSS) return fail(h, BF_EINVAL, "node has no interferers");
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<double> &ia = h->interf;
    const double thr = h->cfg.interf_angle_threshold;
    bool structural = false;
    if (id >= 1 && id <= ia.size()) {  // lcmv.cpp:259-281
        ia[id - 1] = degrees;
        for (size_t i = 0; i < ia.size(); ++i) {
            if (i != (id - 1) && std::abs(ia[i] - degrees) < thr) {
                ia.erase(ia.begin() + id - 1);
                structural = true;
                break;
            }
        }
    } else if (id > ia.size()) {  // lcmv.cpp:282-305
        size_t i;
        for (i = 0; i < ia.size(); ++i)
            if (std::abs(ia[i] - degrees) < thr) break;
        if (i != ia.size()) return BF_OK;  // too close to an existing interferer: ignored, as the reference does
        if (ia.size() + 1 > BF_MAX_INTERF) return fail(h, BF_ENOSYS, "per-bin kernels are built for up to 15 interferers");
        ia.push_back(degrees);
        structural = true;
    } else {
        return fail(h, BF_EINVAL, "interference id must be >= 1");
    }
    if (structural) {
        // free_interf_buffers + allocate_interf_buffers: weights come back zeroed, row 0 is not rewritten (Q3)
        h->S = (int)ia.size() + 1;
        for (auto &st : h->steer) st.allocate(h->N, h->M, h->S);
        h->row0_written = false;
        h->engine->set_columns(h->S);
    }
    rebuild_steering(h, false);
    h->engine->on_theta_changed();  // gss: sep_matrix = weights^H (gss.cpp:90-93)
    return BF_OK;
}

int bf_n_interferers(bf_handle *h) {
    if (!h) return BF_EINVAL;
    std::lock_guard<std::mutex> lk(h->mu);
    return (int)h->interf.size();
}

int bf_get_weights(bf_handle *h, double *w_host) {
    if (!h || !w_host) return BF_EINVAL;
    std::lock_guard<std::mutex> lk(h->mu);
    memcpy(w_host, h->steer[0].w.data(), h->steer[0].w.size() * sizeof(cplxd));  // look direction 0
    return BF_OK;
}

int bf_process_batch_device(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *spectrum_dev,
                            void *hip_stream) {
    if (!h || !x_dev || !y_dev) return BF_EINVAL;
    BF_HIP(h, hipSetDevice(h->device));
    return run_batch_device(h, x_dev, n_frames, y_dev, spectrum_dev, (hipStream_t)hip_stream, h->cfg.layout,
                            (long)n_frames * h->H);
}

// ---- steering tracks ---------------------------------------------------------------------------------------------------------------
// One table per candidate angle: the bytes bf_set_theta(h, angle) would leave in look direction 0's table (the same update_weights
// code; microphone 0's row as it stands: written by the cold start, quirk Q3).  Device layout [angle][mic][N].
namespace {
int install_angle_tables(bf_handle *h, const double *angles_deg, int n_angles) {
    if (n_angles < 0 || n_angles > BF_TRACK_MAX_ANGLES) return fail(h, BF_EINVAL, "track angles: n_angles must be 0 .. BF_TRACK_MAX_ANGLES");
    if (n_angles > 0 && !angles_deg) return fail(h, BF_EINVAL, "track angles: angles is NULL");
    for (int a = 0; a < n_angles; ++a)
        if (!std::isfinite(angles_deg[a])) return fail(h, BF_EINVAL, "track angles: angle not finite");
    const size_t per = (size_t)h->M * h->N;
    if (per * (size_t)n_angles * sizeof(f64x2) > (512ull << 20))
        return fail(h, BF_EINVAL, "track angles: tables (angles x mics x bins) above 512 MiB");
    BF_HIP(h, hipSetDevice(h->device));
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<f64x2> t(per * (size_t)n_angles);
    SteeringSet st;
    st.allocate(h->N, h->M, 1);
    for (int j = 0; j < h->N; ++j) st.at(j, 0, 0) = h->steer[0].at(j, 0, 0);
    for (int a = 0; a < n_angles; ++a) {
        st.update_column(h->geo, h->freqs, 0, angles_deg[a], false);
        for (int m = 0; m < h->M; ++m)
            for (int j = 0; j < h->N; ++j) {
                const cplxd w = st.at(j, m, 0);
                t[(size_t)a * per + (size_t)m * h->N + j] = f64x2{w.real(), w.imag()};
            }
    }
    const int rc = h->engine->install_track_tables(t, n_angles);
    return rc == BF_OK ? BF_OK : fail(h, rc, h->engine->error().c_str());
}
}  // namespace

int bf_track_set_angles(bf_handle *h, const double *angles_deg, int n_angles) {
    if (!h) return BF_EINVAL;
    if (!h->engine->can_track()) return fail(h, BF_ENOSYS, "steering tracks: das in double, phase and phasempf with one look direction");
    return install_angle_tables(h, angles_deg, n_angles);
}

// Column tracks (mvdr / lcmv): the same tables -- calculate_interf_delays is calculate_delays with another angle (util.h:136-188), so one
// table per candidate angle serves every constraint column.  The kernels never read a table's microphone-0 row: that entry is the handle's
// own column's (quirk Q3), so a structural bf_set_interference after this call leaves nothing stale behind.
int bf_ctrack_set_angles(bf_handle *h, const double *angles_deg, int n_angles) {
    if (!h) return BF_EINVAL;
    if (h->cfg.algo != BF_MVDR && h->cfg.algo != BF_LCMV) return fail(h, BF_ENOSYS, "column tracks: mvdr and lcmv with one look direction");
    if (h->n_dirs > 1 || !h->engine->can_ctrack()) return fail(h, BF_EINVAL, "column tracks: one look direction per handle");
    return install_angle_tables(h, angles_deg, n_angles);
}

int bf_process_batch_device_ctracked(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *spectrum_dev,
                                     const int32_t *track_dev, int n_cols, void *hip_stream) {
    if (!h || !x_dev || !y_dev) return BF_EINVAL;
    if (h->cfg.algo != BF_MVDR && h->cfg.algo != BF_LCMV) return fail(h, BF_ENOSYS, "column tracks: mvdr and lcmv with one look direction");
    if (h->n_dirs > 1) return fail(h, BF_EINVAL, "column-tracked batch: one look direction per handle");
    if (!track_dev) return fail(h, BF_EINVAL, "column-tracked batch: track is NULL");
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (n_cols < 1 || n_cols > h->S) return fail(h, BF_EINVAL, "column-tracked batch: n_cols must be 1 .. 1 + the handle's interferers");
    }
    BF_HIP(h, hipSetDevice(h->device));
    return run_batch_device(h, x_dev, n_frames, y_dev, spectrum_dev, (hipStream_t)hip_stream, h->cfg.layout, (long)n_frames * h->H,
                            track_dev, n_cols);
}

int bf_process_batch_device_tracked(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *spectrum_dev,
                                    const int32_t *track_dev, void *hip_stream) {
    if (!h || !x_dev || !y_dev) return BF_EINVAL;
    if (h->n_dirs > 1) return fail(h, BF_EINVAL, "tracked batch: one look direction per handle");
    if (!h->engine->can_track()) return fail(h, BF_ENOSYS, "steering tracks: das in double, phase and phasempf with one look direction");
    if (!track_dev) return fail(h, BF_EINVAL, "tracked batch: track is NULL");
    BF_HIP(h, hipSetDevice(h->device));
    return run_batch_device(h, x_dev, n_frames, y_dev, spectrum_dev, (hipStream_t)hip_stream, h->cfg.layout, (long)n_frames * h->H,
                            track_dev);
}

void *bf_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void bf_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int bf_process_batch(bf_handle *h, const float *x_host, size_t n_frames, float *y_host) {
    if (!h || !x_host || !y_host) return BF_EINVAL;
    if (n_frames == 0) return BF_OK;
    BF_HIP(h, hipSetDevice(h->device));
    const size_t xe = (size_t)h->n_streams * h->M * n_frames * h->H;
    const size_t ye = (size_t)h->n_out * n_frames * h->H;
    BF_HIP(h, h->d_x.reserve(xe));
    BF_HIP(h, h->d_y.reserve(ye));
    float *const d_x = h->d_x.get(), *const d_y = h->d_y.get();
    int rc = BF_OK;
    constexpr int kChunks = 8;
    if (h->n_out == 1 && n_frames >= 8192) {
        // One stream of a long batch: H2D of chunk c+1, compute of chunk c and D2H of chunk c-1 overlap (three HIP streams,
        // events in between).  Consecutive chunks are consecutive batches of the same stream, so the carried state does the
        // rest.  (Only page-locked host buffers -- bf_host_alloc -- make the copies truly asynchronous.)
        if (!h->s_h2d) {
            // all-or-nothing: a half-built set must not survive a failed create (later calls would record on null events)
            hipStream_t a = nullptr, b = nullptr;
            std::vector<hipEvent_t> ei(kChunks, nullptr), eo(kChunks, nullptr);
            hipError_t e = hipStreamCreateWithFlags(&a, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&b, hipStreamNonBlocking);
            for (int c = 0; c < kChunks && e == hipSuccess; ++c) {
                e = hipEventCreateWithFlags(&ei[c], hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&eo[c], hipEventDisableTiming);
            }
            if (e != hipSuccess) {
                for (hipEvent_t v : ei) if (v) (void)hipEventDestroy(v);
                for (hipEvent_t v : eo) if (v) (void)hipEventDestroy(v);
                if (a) (void)hipStreamDestroy(a);
                if (b) (void)hipStreamDestroy(b);
                return fail(h, BF_EIO, "bf_process_batch: copy streams / events", e);
            }
            h->s_h2d = a;
            h->s_d2h = b;
            h->ev_in.swap(ei);
            h->ev_out.swap(eo);
        }
        const size_t F = n_frames, H = (size_t)h->H, M = (size_t)h->M;
        const size_t cf = (F + kChunks - 1) / kChunks;
        hipError_t e = hipSuccess;
        rc = BF_OK;
        const char *what = "";
#define BF_CHUNK(call)                                   \
        if (e == hipSuccess && rc == BF_OK) {            \
            e = (call);                                  \
            if (e != hipSuccess) what = #call;           \
        }
        for (int c = 0; c < kChunks && e == hipSuccess && rc == BF_OK; ++c) {
            const size_t c0 = (size_t)c * cf;
            if (c0 >= F) break;
            const size_t n = (c0 + cf <= F) ? cf : F - c0;
            const float *xd;
            if (h->cfg.layout == BF_PLANAR) {  // M rows of F*H samples: a chunk is a column block
                BF_CHUNK(hipMemcpy2DAsync(d_x + c0 * H, F * H * sizeof(float), x_host + c0 * H, F * H * sizeof(float),
                                          n * H * sizeof(float), M, hipMemcpyHostToDevice, h->s_h2d));
                xd = d_x + c0 * H;
            } else {
                BF_CHUNK(hipMemcpyAsync(d_x + c0 * H * M, x_host + c0 * H * M, n * H * M * sizeof(float), hipMemcpyHostToDevice,
                                        h->s_h2d));
                xd = d_x + c0 * H * M;
            }
            BF_CHUNK(hipEventRecord(h->ev_in[c], h->s_h2d));
            BF_CHUNK(hipStreamWaitEvent(h->stream, h->ev_in[c], 0));
            if (e == hipSuccess)
                rc = run_batch_device(h, xd, n, d_y + c0 * H, nullptr, h->stream, h->cfg.layout, (long)(F * H));
            BF_CHUNK(hipEventRecord(h->ev_out[c], h->stream));
            BF_CHUNK(hipStreamWaitEvent(h->s_d2h, h->ev_out[c], 0));
            BF_CHUNK(hipMemcpyAsync(y_host + c0 * H, d_y + c0 * H, n * H * sizeof(float), hipMemcpyDeviceToHost, h->s_d2h));
        }
#undef BF_CHUNK
        // success or not: nothing may still be copying from / into the caller's buffers when this returns
        const hipError_t e1 = hipStreamSynchronize(h->s_h2d), e2 = hipStreamSynchronize(h->stream), e3 = hipStreamSynchronize(h->s_d2h);
        if (rc != BF_OK) return rc;
        if (e != hipSuccess) return fail(h, BF_EIO, what, e);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
            return fail(h, BF_EIO, "bf_process_batch: stream synchronisation", e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3));
        return BF_OK;
    }
    BF_HIP(h, hipMemcpyAsync(d_x, x_host, xe * sizeof(float), hipMemcpyHostToDevice, h->stream));
    rc = run_batch_device(h, d_x, n_frames, d_y, nullptr, h->stream, h->cfg.layout, (long)n_frames * h->H);
    if (rc != BF_OK) return rc;
    BF_HIP(h, hipMemcpyAsync(y_host, d_y, ye * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    BF_HIP(h, hipStreamSynchronize(h->stream));
    return BF_OK;
}

int bf_process_hop(bf_handle *h, const float *const *in, float *out, uint32_t nframes) {
    if (!h || !in || !out) return BF_EINVAL;
    if ((int)nframes != h->H) return fail(h, BF_EINVAL, "nframes must equal the configured hop");
    if (h->n_streams != 1) return fail(h, BF_EINVAL, "bf_process_hop drives stream 0 of a single-stream handle");
    BF_HIP(h, hipSetDevice(h->device));
    const size_t n_in = (size_t)h->M * h->H, n_outv = (size_t)h->n_out * h->H;
    BF_HIP(h, h->d_x.reserve(n_in));
    BF_HIP(h, h->d_y.reserve(n_outv));
    BF_HIP(h, h->h_pin.reserve(n_in + n_outv));
    float *const d_x = h->d_x.get(), *const d_y = h->d_y.get();
    float *packed = h->h_pin.get(), *res = packed + n_in;
    if (h->cfg.layout == BF_PLANAR) {
        for (int m = 0; m < h->M; ++m) memcpy(packed + (size_t)m * h->H, in[m], sizeof(float) * h->H);
    } else {
        for (int m = 0; m < h->M; ++m)
            for (int n = 0; n < h->H; ++n) packed[(size_t)n * h->M + m] = in[m][n];
    }
    BF_HIP(h, hipMemcpyAsync(d_x, packed, n_in * sizeof(float), hipMemcpyHostToDevice, h->stream));
    int rc = run_batch_device(h, d_x, 1, d_y, nullptr, h->stream, h->cfg.layout, (long)h->H);
    if (rc != BF_OK) return rc;
    BF_HIP(h, hipMemcpyAsync(res, d_y, n_outv * sizeof(float), hipMemcpyDeviceToHost, h->stream));  // [dir][row][hop]
    BF_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(out, res, n_outv * sizeof(float));
    return BF_OK;
}

// ---- frame-range sharding (beamform_amd/shard.py is the same plan in Python) ------------------------------------------------
// A column range of a longer planar buffer: microphone m starts at x_dev + m * mic_stride (samples).  One input stream.
int bf_process_batch_device_strided(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *hip_stream,
                                    long mic_stride) {
    if (!h || !x_dev || !y_dev || mic_stride < (long)(n_frames * (size_t)h->H)) return BF_EINVAL;
    // (several look directions write [dir][n_frames * hop] rows: a piece of a longer output buffer would need its own row stride)
    if (h->cfg.layout != BF_PLANAR || h->n_streams != 1 || h->n_dirs != 1)
        return fail(h, BF_EINVAL, "strided batches: planar layout, one input stream, one look direction");
    BF_HIP(h, hipSetDevice(h->device));
    return run_batch_device(h, x_dev, n_frames, y_dev, nullptr, (hipStream_t)hip_stream, h->cfg.layout, mic_stride);
}

int bf_shard_halo(const bf_config *cfg) {
    if (!cfg) return -1;
    switch (cfg->algo) {
        case BF_DAS:
        case BF_PHASE: return 1;                       // overlap-add neighbour only (util.h:301-302)
        case BF_MVDR:
        case BF_LCMV: return cfg->past_windows + 1;    // covariance history of frame lo-1, plus that frame (mvdr.cpp:87,100-101)
        default: return -1;                            // gss / phasempf / mcra recurse over frames, gsc over samples
    }
}

int bf_shard_plan(size_t n_frames, int world, int rank, int halo, bf_shard *out) {
    if (!out || world < 1 || rank < 0 || rank >= world || halo < 0) return BF_EINVAL;
    const long long n = (long long)n_frames, base = n / world, rem = n % world;
    out->lo = rank * base + (rank < rem ? rank : rem);
    out->hi = out->lo + base + (rank < rem ? 1 : 0);
    out->warm = (int)(halo < out->lo ? halo : out->lo);
    out->lead = (halo > 0 && out->lo - out->warm > 0) ? 1 : 0;
    return BF_OK;
}

long long bf_shard_first_feed(const bf_shard *s) { return s ? s->lo - s->warm - s->lead : 0; }
long long bf_shard_n_feed(const bf_shard *s) { return s ? s->hi - bf_shard_first_feed(s) : 0; }
long long bf_shard_n_drop(const bf_shard *s) { return s ? (long long)s->warm + s->lead : 0; }

int bf_shard_run(bf_handle *h, const float *x_feed_dev, const bf_shard *sh, float *y_feed_dev, void *hip_stream) {
    if (!h || !sh) return BF_EINVAL;
    if (h->n_streams != 1 || h->n_dirs != 1)
        return fail(h, BF_EINVAL, "frame-range sharding drives one input stream and one look direction per handle");
    if (h->cfg.algo == BF_LCMV && h->n_rows > 1) return fail(h, BF_EINVAL, "frame-range sharding: the feed buffer is one stream (lcmv_out_beams > 1)");
    const long long n_feed = bf_shard_n_feed(sh);
    if (n_feed < 0 || sh->warm < 0 || sh->lead < 0) return fail(h, BF_EINVAL, "malformed shard");
    int rc = bf_reset_async(h, hip_stream);  // the rank's node knows nothing about the frames before its slice
    if (rc != BF_OK || n_feed == 0) return rc;
    return bf_process_batch_device(h, x_feed_dev, (size_t)n_feed, y_feed_dev, nullptr, hip_stream);
}

// Per-launch timing of the dominant kernel for launches the CALLER issues (bench.py's timed loop): between begin and end every
// launch of the fused kernel is bracketed by its own event pair on the stream it is launched on.
int bf_kernel_timing_begin(bf_handle *h) {
    if (!h) return BF_EINVAL;
    if (h->timing) return fail(h, BF_EINVAL, "kernel timing already active");
    BF_HIP(h, hipSetDevice(h->device));
    int rc = timing_reserve(h, 256);  // the caller's timed loop then only records
    if (rc != BF_OK) return rc;
    h->ev_used = 0;
    h->timing = 1;
    return BF_OK;
}

int bf_trace_begin(void) {
    if (g_trace) return BF_EINVAL;
    g_trace = new std::vector<const void *>();
    return BF_OK;
}

// rocprofv3's spelling of a kernel name: the demangled name without its parameter list, "void" prefix and anonymous namespaces
static std::string trace_kernel_name(const void *fn) {
    const char *m = hipKernelNameRefByPtr(fn, nullptr);
    if (!m) return "?";
    int st = 0;
    char *d = abi::__cxa_demangle(m, nullptr, nullptr, &st);
    std::string n = (st == 0 && d) ? d : m;
    free(d);
    int depth = 0;   // cut the parameter list: the last '(' at template depth 0
    size_t cut = std::string::npos;
    for (size_t i = 0; i < n.size(); ++i) {
        if (n[i] == '<') ++depth;
        else if (n[i] == '>') --depth;
        else if (n[i] == '(' && depth == 0 && n.compare(i, 21, "(anonymous namespace)") != 0) { cut = i; break; }
    }
    if (cut != std::string::npos) n.resize(cut);
    if (n.compare(0, 5, "void ") == 0) n.erase(0, 5);
    for (size_t p; (p = n.find("(anonymous namespace)::")) != std::string::npos;) n.erase(p, 23);
    return n;
}

long bf_trace_end(char *buf, size_t cap) {
    if (!g_trace) return BF_EINVAL;
    std::string out;
    for (const void *fn : *g_trace) {
        if (!out.empty()) out += '\n';
        out += trace_kernel_name(fn);
    }
    delete g_trace;
    g_trace = nullptr;
    if (buf && cap) {
        const size_t n = out.size() < cap - 1 ? out.size() : cap - 1;
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (long)out.size();
}

int bf_kernel_timing_end(bf_handle *h, float *ms_mean, int *n_launches) {
    if (!h || !ms_mean) return BF_EINVAL;
    if (h->timing != 1) return fail(h, BF_EINVAL, "kernel timing is not active");
    return timing_collect(h, ms_mean, n_launches);
}

int bf_time_batch_device(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *hip_stream, int iters,
                         float *ms_per_call, float *ms_kernel) {
    if (!h || !x_dev || !y_dev || iters < 1 || !ms_per_call) return BF_EINVAL;
    if (h->timing) return fail(h, BF_EINVAL, "bf_time_batch_device inside a bf_kernel_timing_begin session");
    BF_HIP(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    if (ms_kernel) {
        int rc0 = timing_reserve(h, (size_t)iters);
        if (rc0 != BF_OK) return rc0;
        h->ev_used = 0;
        h->timing = 2;
    }
    int rc = BF_OK;
    hipError_t e = hipEventRecord(h->ev0, s);
    for (int i = 0; i < iters && rc == BF_OK && e == hipSuccess; ++i)
        rc = run_batch_device(h, x_dev, n_frames, y_dev, nullptr, s, h->cfg.layout, (long)n_frames * h->H);
    if (e == hipSuccess) e = hipEventRecord(h->ev1, s);
    if (e == hipSuccess) e = hipEventSynchronize(h->ev1);
    float ms = 0.f, msk = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->ev0, h->ev1);
    int nk = 0;
    if (h->timing == 2) {
        int trc = (e == hipSuccess && rc == BF_OK) ? timing_collect(h, &msk, &nk) : BF_OK;
        h->timing = 0;
        h->ev_used = 0;
        if (rc == BF_OK) rc = trc;
    }
    if (rc != BF_OK) return rc;
    if (e != hipSuccess) return fail(h, BF_EIO, "bf_time_batch_device", e);
    *ms_per_call = ms / (float)iters;
    if (ms_kernel) *ms_kernel = nk ? msk : 0.f;
    return BF_OK;
}

// ---- checkpoint -------------------------------------------------------------
struct bf_state_header {
    uint32_t magic, algo, n_mics, n_streams, hop, das_impl;
    uint64_t payload;
};
static const uint32_t kStateMagic = 0x42465333;  // "BFS3"
// control-plane part of a checkpoint: what /theta and /theta_interference have made of the node since start-up
struct bf_state_control {
    uint32_t kp1;              // constraint columns (1 + interferers)
    uint32_t row0_written;     // reference-mic weight row: 1 after a cold start, 0 after a structural change (quirk Q3)
    uint64_t gss_pending;      // look directions whose demixing matrices restart at the next run (gss.cpp:90-93)
    uint64_t cfg_hash;         // the bf_config fields that give the state its meaning (geometry, rate, band, history length, ...)
    double theta[BF_MAX_DIRS];
    double interf[BF_MAX_INTERF];
};

// FNV-1a over the configuration a checkpoint is only valid under: restoring covariance history or demixing matrices next to
// another geometry, sample rate, band or window count would silently pair them with the wrong steering
static uint64_t state_cfg_hash(const bf_handle *h) {
    uint64_t x = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) {
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i < n; ++i) { x ^= b[i]; x *= 1099511628211ull; }
    };
    const bf_config &c = h->cfg;
    mix(c.mic_x, sizeof(double) * h->M);
    mix(c.mic_y, sizeof(double) * h->M);
    const double d[] = {c.sample_rate, c.freq_mag_threshold, c.freq_max, c.freq_min, c.mu, c.lambda_, c.min_phase, c.min_mag,
                        c.mcra_alphaS, c.mcra_alphaD, c.mcra_alphaD2, c.mcra_delta, c.mpf_alphaS, c.mpf_eta, c.mpf_rev_gamma,
                        c.mpf_rev_delta, c.gsc_mu0, c.gsc_mu_max};
    mix(d, sizeof(d));
    const int i[] = {c.past_windows, c.smooth_size, c.mcra_L, c.layout, c.gsc_filter_size, h->n_dirs, c.precision};  // (precision: the stored element of the covariance history)
    mix(i, sizeof(i));
    return x;
}

// header word `das_impl`: the das arithmetic, and above it gss's (lcmv's) rows per beam minus one (the blob carries that many overlap-add tails per
// beam: a handle of another row count must refuse it; one row leaves the word, and so the blob, as it always was), and in bit 24 gss's
// post-filter (the blob then carries the filter's state per row; off leaves the word as it was)
static uint32_t state_impl_word(const bf_handle *h) {
    return (uint32_t)h->cfg.das_impl | ((uint32_t)(h->n_rows - 1) << 16) | ((uint32_t)(h->cfg.gss_postfilter != 0) << 24);
}

size_t bf_state_size(const bf_handle *h) {
    if (!h) return 0;
    return sizeof(bf_state_header) + sizeof(bf_state_control) + h->engine->state_bytes();
}

int bf_get_state(bf_handle *h, void *blob, size_t size) {
    if (!h || !blob) return BF_EINVAL;
    {
        std::lock_guard<std::mutex> lk(h->mu);  // the payload size follows the interferer count, which /theta_interference changes
        if (size < bf_state_size(h)) return BF_EINVAL;
    }
    BF_HIP(h, hipSetDevice(h->device));
    BF_HIP(h, hipDeviceSynchronize());
    bf_state_header hd = {kStateMagic, (uint32_t)h->cfg.algo, (uint32_t)h->M, (uint32_t)h->n_streams | ((uint32_t)h->n_dirs << 20),
                          (uint32_t)h->H, state_impl_word(h), (uint64_t)(bf_state_size(h) - sizeof(bf_state_header))};
    memcpy(blob, &hd, sizeof(hd));
    bf_state_control ct;
    memset(&ct, 0, sizeof(ct));
    {
        std::lock_guard<std::mutex> lk(h->mu);
        ct.kp1 = (uint32_t)h->S;
        ct.row0_written = h->row0_written ? 1u : 0u;
        ct.cfg_hash = state_cfg_hash(h);
        ct.gss_pending = h->engine->pending_resets();
        for (int d = 0; d < h->n_dirs; ++d) ct.theta[d] = h->angle[d];
        for (size_t k = 0; k < h->interf.size(); ++k) ct.interf[k] = h->interf[k];
    }
    memcpy((char *)blob + sizeof(hd), &ct, sizeof(ct));
    char *p = (char *)blob + sizeof(hd) + sizeof(ct);
    int rc = h->engine->get_state(p);
    return rc == BF_OK ? BF_OK : fail(h, rc, h->engine->error().c_str());
}

int bf_set_state(bf_handle *h, const void *blob, size_t size) {
    if (!h || !blob) return BF_EINVAL;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (size < bf_state_size(h)) return BF_EINVAL;
    }
    bf_state_header hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != kStateMagic || hd.algo != (uint32_t)h->cfg.algo || hd.n_mics != (uint32_t)h->M ||
        hd.n_streams != ((uint32_t)h->n_streams | ((uint32_t)h->n_dirs << 20)) || hd.hop != (uint32_t)h->H || hd.das_impl != state_impl_word(h))
        return fail(h, BF_EINVAL, "state blob does not match this handle");
    bf_state_control ct;
    memcpy(&ct, (const char *)blob + sizeof(hd), sizeof(ct));
    BF_HIP(h, hipSetDevice(h->device));
    BF_HIP(h, hipDeviceSynchronize());
    {
        // the per-bin state (covariance history, demixing matrices) only means something together with the steering it
        // was built under: restore the angles, the interferer list and the pending demixing resets with it
        std::lock_guard<std::mutex> lk(h->mu);
        if ((int)ct.kp1 != h->S) return fail(h, BF_EINVAL, "state blob was taken with a different number of interferers");
        if (ct.cfg_hash != state_cfg_hash(h))
            return fail(h, BF_EINVAL, "state blob was taken under another configuration (geometry, rate, band, window count or node parameters)");
        for (int d = 0; d < h->n_dirs; ++d)
            if (!std::isfinite(ct.theta[d])) return fail(h, BF_EINVAL, "state blob holds a non-finite look angle");
        for (size_t k = 0; k < h->interf.size(); ++k)
            if (!std::isfinite(ct.interf[k])) return fail(h, BF_EINVAL, "state blob holds a non-finite interferer angle");
        h->row0_written = ct.row0_written != 0;
        for (int d = 0; d < h->n_dirs; ++d) h->angle[d] = ct.theta[d];
        for (size_t k = 0; k < h->interf.size(); ++k) h->interf[k] = ct.interf[k];
        for (auto &st : h->steer)
            for (int c = 0; c < st.n_cols; ++c)
                for (int j = 0; j < st.n_fft; ++j) st.at(j, 0, c) = ct.row0_written ? cplxd(1.0, 0.0) : cplxd(0.0, 0.0);
        rebuild_steering(h, false);
        h->engine->set_pending_resets(ct.gss_pending);
    }
    const char *p = (const char *)blob + sizeof(hd) + sizeof(ct);
    int rc = h->engine->set_state(p);
    return rc == BF_OK ? BF_OK : fail(h, rc, h->engine->error().c_str());
}

}  // extern "C"
