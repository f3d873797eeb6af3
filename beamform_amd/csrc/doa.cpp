// doa.cpp -- bf_doa_*: SRP-PHAT, Capon and MUSIC direction-of-arrival maps over the nodes' frames (include/bfcore.h, DESIGN.md "Direction-of-arrival
// maps").  Host side: argument checks, the steering table (SteeringSet, the weights das steers with), and one batch path for the three
// methods: doa_decide's plan (doa.hpp) sizes the scratch and the chunks, and one loop runs a chunk's launch sequence.  Every per-frame
// operation runs in the gfx950 kernels (pipeline_kernels.hpp launch_stft, doa_kernels.hip); there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bfcore.h"
#include "device_mem.hpp"
#include "doa.hpp"
#include "doa_assign.hpp"
#include "geometry.hpp"
#include "pipeline_kernels.hpp"
#include "switches.hpp"

using namespace bf;

struct bf_doa {
    int M = 0, H = 0, N = 0, S = 1, NP = 1, layout = 0, device = 0, n_cus = 256;
    int D = 0, W = 1, klo = 0, nK = 0;
    double eps = 1e-10;
    int method = BF_DOA_SRP_PHAT;                 // bf_doa_set_method
    double delta = 1e-3;                          // bf_doa_set_loading
    int n_sources = 1;                            // bf_doa_set_sources
    double mu = 1e-2;                             // bf_doa_set_music_floor
    std::string err;
    const KernelSet *ks = nullptr;
    hipStream_t stream = nullptr;                 // bf_doa_process (host buffers)
    DeviceBuffer<f64x2> d_steer, d_tw;            // [bin - klo][mic][angle]; forward-transform twiddles
    DeviceBuffer<f64x2> d_steer_cov;              // [angle][mic][bin - klo]: built when Capon or MUSIC is first selected
    DeviceBuffer<double> d_win;                   // sqrt-Hann
    DeviceBuffer<float> d_hist;                   // [stream][hop before the next frame], layout as the input
    // scratch for one chunk (ensure_scratch: grown to the largest plan so far, kept)
    DeviceBuffer<f64x2> d_Z;
    DeviceBuffer<unsigned> d_flags;               // SRP-PHAT
    DeviceBuffer<double> d_part;
    DeviceBuffer<f64x2> d_ws;                     // Capon and MUSIC above 8 microphones: the per-bin matrices
    // staging of bf_doa_process (grown on demand)
    DeviceBuffer<float> d_x;
    DeviceBuffer<double> d_map;
    DeviceBuffer<int32_t> d_peak;
    DeviceBuffer<double> d_eig;
};

namespace {

static_assert((int)kDoaSrpPhat == (int)BF_DOA_SRP_PHAT && (int)kDoaCapon == (int)BF_DOA_CAPON && (int)kDoaMusic == (int)BF_DOA_MUSIC,
              "doa_decide takes the handle's method");
constexpr size_t kDoaMaxTableBytes = 512ull << 20;

int fail(bf_doa *d, int code, const std::string &what, hipError_t e = hipSuccess) {
    std::string msg = what;
    if (e != hipSuccess) {
        msg += ": ";
        msg += hipGetErrorString(e);
    }
    if (d) d->err = msg;
    set_last_error(msg);
    return code;
}

#define DOA_HIP(d, call)                                                  \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return fail((d), BF_EIO, #call, e_);        \
    } while (0)

// the buffers one chunk of the plan needs; they only ever grow, and a failed growth leaves a buffer empty (it grows again next time)
int ensure_scratch(bf_doa *d, const DoaPlan &p) {
    const size_t z = p.z_bytes / sizeof(f64x2), flags = p.flags_bytes / sizeof(unsigned), part = p.part_bytes / sizeof(double),
                 ws = p.ws_bytes / sizeof(f64x2);
    if (z <= d->d_Z.size() && flags <= d->d_flags.size() && part <= d->d_part.size() && ws <= d->d_ws.size()) return BF_OK;
    DOA_HIP(d, hipDeviceSynchronize());  // a batch still in flight may read the old buffers
    if (d->d_Z.reserve(z) != hipSuccess || d->d_flags.reserve(flags) != hipSuccess || d->d_part.reserve(part) != hipSuccess ||
        d->d_ws.reserve(ws) != hipSuccess) {
        (void)hipGetLastError();
        return fail(d, BF_ENOMEM, "bf_doa scratch");
    }
    return BF_OK;
}

// the forward transforms of frames [0, n) at xc into d_Z (rows of frames_ws frames per stream): packed pairs, halved, band rows only
int enqueue_stft(bf_doa *d, const float *xc, long n, long frames_ws, long mic_stride, long stream_stride, hipStream_t s) {
    StftArgs sa{};
    sa.x = xc;
    sa.hist = d->d_hist.get();
    sa.Z = d->d_Z.get();
    sa.tw = d->d_tw.get();
    sa.win = d->d_win.get();
    sa.n_frames = n;
    sa.frames_ws = frames_ws;
    sa.frame_off = 0;
    sa.mic_stride = mic_stride;
    sa.stream_stride_x = stream_stride;
    sa.n_streams = d->S;
    sa.n_mics = d->M;
    sa.layout = d->layout;
    sa.n_fft_mics = d->M;
    sa.skip_lo = d->N;  // store everything ...
    sa.skip_hi = 0;
    const int khi = d->klo + d->nK - 1;
    if (khi < d->N / 2 - 2) {  // ... but the bins between the band's top bin and its mirror
        sa.skip_lo = khi;
        sa.skip_hi = d->N - khi;
    }
    sa.z48 = 0;
    sa.halve = 1;  // X_a = Z[k] + conj Z[N-k], X_b = -i (Z[k] - conj Z[N-k])
    sa.run_len = 1;
    ChainPlan front{};  // only the STFT of the chain runs here
    front.layout = d->layout;
    front.front = chain_stft_front(d->N, switches().stft_small, switches().stft_split);
    front.geom.stft = chain_stft_geom(front.front, d->N, d->S, n, d->M, d->n_cus);  // run length and blocks (chain_geom.hpp)
    if (!front.geom.stft.ok) return fail(d, BF_EINVAL, "bf_doa: batch too large for the STFT's launch geometry");
    DOA_HIP(d, d->ks->stft(front, sa, d->n_cus, s));
    return BF_OK;
}

}  // namespace

int bf_doa_create(const bf_config *cfg, const double *angles_deg, int n_angles, double freq_lo, double freq_hi, int frames_per_block,
                  bf_doa **out) {
    if (!out) return fail(nullptr, BF_EINVAL, "bf_doa_create: out is NULL");
    *out = nullptr;
    if (!cfg) return fail(nullptr, BF_EINVAL, "bf_doa_create: cfg is NULL");
    if (cfg->n_mics < 2 || cfg->n_mics > BF_MAX_MICS) return fail(nullptr, BF_EINVAL, "bf_doa_create: n_mics must be 2 .. BF_MAX_MICS");
    if (cfg->hop < 64 || cfg->hop > 4096 || (cfg->hop & (cfg->hop - 1)) != 0)
        return fail(nullptr, BF_EINVAL, "bf_doa_create: hop must be a power of two from 64 to 4096");
    if (!(cfg->sample_rate > 0) || !std::isfinite(cfg->sample_rate)) return fail(nullptr, BF_EINVAL, "bf_doa_create: sample_rate");
    if (cfg->n_streams < 1) return fail(nullptr, BF_EINVAL, "bf_doa_create: n_streams < 1");
    if (cfg->layout != BF_PLANAR && cfg->layout != BF_INTERLEAVED) return fail(nullptr, BF_EINVAL, "bf_doa_create: layout");
    if (!angles_deg || n_angles < 1 || n_angles > BF_DOA_MAX_ANGLES)
        return fail(nullptr, BF_EINVAL, "bf_doa_create: n_angles must be 1 .. BF_DOA_MAX_ANGLES");
    for (int i = 0; i < n_angles; ++i)
        if (!std::isfinite(angles_deg[i])) return fail(nullptr, BF_EINVAL, "bf_doa_create: angle not finite");
    if (frames_per_block < 1) return fail(nullptr, BF_EINVAL, "bf_doa_create: frames_per_block < 1");
    if (!(freq_lo <= freq_hi)) return fail(nullptr, BF_EINVAL, "bf_doa_create: freq_lo > freq_hi");
    const int M = cfg->n_mics, H = cfg->hop, N = 2 * H;
    // the band: bins 1 .. N/2-1 whose frequency (frequency_vector, quirk Q1 included) lies in [freq_lo, freq_hi]; the vector is
    // nondecreasing there, so the band is one run of bins
    const std::vector<double> freqs = frequency_vector(N, cfg->sample_rate);
    int klo = -1, khi = -1;
    for (int k = 1; k <= N / 2 - 1; ++k)
        if (freqs[k] >= freq_lo && freqs[k] <= freq_hi) {
            if (klo < 0) klo = k;
            khi = k;
        }
    if (klo < 0) return fail(nullptr, BF_EINVAL, "bf_doa_create: no bin in [freq_lo, freq_hi]");
    const int nK = khi - klo + 1;
    const size_t table = (size_t)nK * M * n_angles * sizeof(f64x2);
    if (table > kDoaMaxTableBytes) return fail(nullptr, BF_EINVAL, "bf_doa_create: steering table (angles x bins x mics) above 512 MiB");
    const int ndev = bf_device_count();
    if (ndev <= 0) return fail(nullptr, BF_ENODEV, "no HIP device visible; libbfcore has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, BF_ENODEV, "device ordinal out of range");

    bf_doa *d = new bf_doa();
    d->M = M;
    d->H = H;
    d->N = N;
    d->S = cfg->n_streams;
    d->NP = (M + 1) / 2;
    d->layout = cfg->layout;
    d->device = cfg->device;
    d->D = n_angles;
    d->W = frames_per_block;
    d->klo = klo;
    d->nK = nK;
    d->ks = kernel_set(N);
#define DOA_CREATE_HIP(call)                                  \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) {                               \
            int rc_ = fail(nullptr, BF_EIO, #call, e_);       \
            bf_doa_destroy(d);                                \
            return rc_;                                       \
        }                                                     \
    } while (0)
    if (!d->ks) {
        delete d;
        return fail(nullptr, BF_ENOSYS, "bf_doa_create: no forward transform for this hop");
    }
    DOA_CREATE_HIP(hipSetDevice(d->device));
    hipDeviceProp_t prop;
    DOA_CREATE_HIP(hipGetDeviceProperties(&prop, d->device));
    d->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    DOA_CREATE_HIP(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));

    // w_m(theta_d, k): exactly the column das steers with (update_weights(true), das.cpp:27-45), [bin - klo][mic][angle]
    ArrayGeometry geo;
    geo.set(cfg->mic_x, cfg->mic_y, M);
    std::vector<f64x2> T((size_t)nK * M * n_angles);
    SteeringSet st;
    st.allocate(N, M, 1);
    for (int a = 0; a < n_angles; ++a) {
        st.update_column(geo, freqs, 0, angles_deg[a], true);
        for (int kk = 0; kk < nK; ++kk)
            for (int m = 0; m < M; ++m) {
                const cplxd w = st.at(klo + kk, m, 0);
                T[((size_t)kk * M + m) * n_angles + a] = f64x2{w.real(), w.imag()};
            }
    }
    DOA_CREATE_HIP(d->d_steer.upload(T));
    DOA_CREATE_HIP(d->d_tw.upload(N == 1024 ? twiddle_table_32x32<f64x2>() : stockham_twiddles<f64x2>(N)));
    DOA_CREATE_HIP(d->d_win.upload(sqrt_hann(N)));
    DOA_CREATE_HIP(d->d_hist.alloc((size_t)d->S * M * H));
    DOA_CREATE_HIP(hipMemset(d->d_hist.get(), 0, (size_t)d->S * M * H * sizeof(float)));
#undef DOA_CREATE_HIP
    *out = d;
    return BF_OK;
}

int bf_doa_set_phat_floor(bf_doa *d, double eps) {
    if (!d || !(eps >= 0) || !std::isfinite(eps)) return fail(d, BF_EINVAL, "bf_doa_set_phat_floor: eps must be finite and >= 0");
    d->eps = eps;
    return BF_OK;
}

int bf_doa_set_method(bf_doa *d, int method) {
    if (!d || (method != BF_DOA_SRP_PHAT && method != BF_DOA_CAPON && method != BF_DOA_MUSIC))
        return fail(d, BF_EINVAL, "bf_doa_set_method: NULL handle or unknown method");
    if (method != BF_DOA_SRP_PHAT && d->d_steer_cov.size() == 0) {  // the first selection: the table with the bins innermost
        DOA_HIP(d, hipSetDevice(d->device));
        if (d->d_steer_cov.alloc(d->d_steer.size()) != hipSuccess) {
            (void)hipGetLastError();
            return fail(d, BF_ENOMEM, "bf_doa_set_method: steering table");
        }
        hipError_t e = launch_doa_cov_table(d->d_steer.get(), d->d_steer_cov.get(), d->nK, d->M, d->D, d->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) {
            d->d_steer_cov = DeviceBuffer<f64x2>();
            return fail(d, BF_EIO, "bf_doa_set_method: steering table", e);
        }
    }
    d->method = method;
    return BF_OK;
}

int bf_doa_set_loading(bf_doa *d, double delta) {
    if (!d || !std::isfinite(delta) || !(delta > 0) || !(delta <= 1))
        return fail(d, BF_EINVAL, "bf_doa_set_loading: delta must be finite and in (0, 1]");
    d->delta = delta;
    return BF_OK;
}

int bf_doa_set_sources(bf_doa *d, int n_sources) {
    if (!d || n_sources < 1 || n_sources > d->M - 1)
        return fail(d, BF_EINVAL, "bf_doa_set_sources: n_sources must be in 1 .. n_mics - 1");
    d->n_sources = n_sources;
    return BF_OK;
}

int bf_doa_set_music_floor(bf_doa *d, double mu) {
    if (!d || !std::isfinite(mu) || !(mu > 0) || !(mu <= 1))
        return fail(d, BF_EINVAL, "bf_doa_set_music_floor: mu must be finite and in (0, 1]");
    d->mu = mu;
    return BF_OK;
}

int bf_doa_process_device(bf_doa *d, const float *x_dev, size_t n_frames, double *map_dev, int32_t *peak_dev, void *hip_stream) {
    if (!d) return fail(nullptr, BF_EINVAL, "bf_doa_process_device: handle is NULL");
    if (!map_dev && !peak_dev) return fail(d, BF_EINVAL, "bf_doa_process_device: map and peak are both NULL");
    return bf_doa_process_device_eig(d, x_dev, n_frames, map_dev, peak_dev, nullptr, hip_stream);
}

int bf_doa_process_device_eig(bf_doa *d, const float *x_dev, size_t n_frames, double *map_dev, int32_t *peak_dev, double *eig_dev,
                              void *hip_stream) {
    if (!d) return fail(nullptr, BF_EINVAL, "bf_doa_process_device: handle is NULL");
    if (!map_dev && !peak_dev && !eig_dev) return fail(d, BF_EINVAL, "bf_doa_process_device: map, peak and eig are all NULL");
    if (eig_dev && d->method != BF_DOA_MUSIC) return fail(d, BF_EINVAL, "bf_doa_process_device: eig needs the MUSIC method");
    if (n_frames % (size_t)d->W != 0) return fail(d, BF_EINVAL, "bf_doa_process_device: n_frames is not a multiple of frames_per_block");
    if (n_frames == 0) return BF_OK;
    if (!x_dev) return fail(d, BF_EINVAL, "bf_doa_process_device: x is NULL");
    hipStream_t s = (hipStream_t)hip_stream;
    DOA_HIP(d, hipSetDevice(d->device));
    const bool srp = d->method == BF_DOA_SRP_PHAT, music = d->method == BF_DOA_MUSIC;
    const int M = d->M, H = d->H, W = d->W;
    const long F = (long)n_frames;
    const DoaPlan plan = doa_decide(DoaShape{M, d->S, d->N, d->D, d->nK, W, F}, d->method);
    int rc = ensure_scratch(d, plan);
    if (rc != BF_OK) return rc;
    const long CF = plan.chunk_frames;
    const long mic_stride = d->layout == BF_PLANAR ? F * H : 1;
    const long stream_stride = (long)M * F * H;
    DoaMapArgs ma;  // SRP-PHAT
    ma.Z = d->d_Z.get();
    ma.flags = d->d_flags.get();
    ma.steer = d->d_steer.get();
    ma.part = d->d_part.get();
    ma.eps = d->eps;
    ma.frames_ws = CF;
    ma.n_streams = d->S;
    ma.n_mics = M;
    ma.nfft = d->N;
    ma.n_angles = d->D;
    ma.klo = d->klo;
    ma.n_bins = d->nK;
    DoaCovArgs ca;  // Capon and MUSIC
    ca.Z = d->d_Z.get();
    ca.steer = d->d_steer_cov.get();
    ca.part = d->d_part.get();
    ca.ws = d->d_ws.get();
    ca.delta = d->delta;
    ca.frames_ws = CF;
    ca.blocks_ws = plan.chunk_blocks;
    ca.n_streams = d->S;
    ca.n_mics = M;
    ca.nfft = d->N;
    ca.n_angles = d->D;
    ca.klo = d->klo;
    ca.n_bins = d->nK;
    ca.n_segments = plan.segments;
    ca.frames_per_block = W;
    if (music) {
        ca.epart = d->d_part.get() + plan.epart_offset;
        ca.n_sources = d->n_sources;
    }
    // SRP-PHAT keeps a row of partial sums per frame and the reduction adds a block's W rows; the covariance methods keep one per block
    DoaReduceArgs ra;
    ra.part = d->d_part.get();
    ra.map = map_dev;
    ra.peak = peak_dev;
    ra.scale = srp ? 1.0 / ((double)W * d->nK * M * M) : 1.0 / (double)d->nK;
    ra.frames_ws = srp ? CF : plan.chunk_blocks;
    ra.map_blocks = F / W;
    ra.n_streams = d->S;
    ra.n_angles = d->D;
    ra.n_segments = plan.segments;
    ra.frames_per_block = srp ? W : 1;
    if (music) {  // P = mu / (mu + sum / |K|)
        ra.mu = d->mu;
        ra.denom = (double)d->nK;
    }
    for (long c0 = 0; c0 < F; c0 += CF) {
        const long n = std::min(CF, F - c0);
        const float *xc = x_dev + (d->layout == BF_PLANAR ? c0 * H : c0 * (long)H * M);
        if (srp) DOA_HIP(d, launch_doa_hop_flags(xc, d->d_hist.get(), d->d_flags.get(), n, mic_stride, stream_stride, d->S, M, H, d->layout, s));
        rc = enqueue_stft(d, xc, n, CF, mic_stride, stream_stride, s);
        if (rc != BF_OK) return rc;
        if (srp) {
            ma.n_frames = n;
            DOA_HIP(d, launch_doa_map(ma, plan, s));
        } else {
            ca.n_blocks = n / W;
            DOA_HIP(d, launch_doa_cov(ca, plan, s));
        }
        ra.block0 = c0 / W;
        ra.n_blocks = n / W;
        if (map_dev || peak_dev) DOA_HIP(d, launch_doa_reduce(ra, s));
        if (eig_dev) {  // the profile: M "angles" per block, the plain mean over the band, no peak
            DoaReduceArgs ea = ra;
            ea.part = ca.epart;
            ea.map = eig_dev;
            ea.peak = nullptr;
            ea.n_angles = M;
            ea.mu = 0.0;
            DOA_HIP(d, launch_doa_reduce(ea, s));
        }
        // the chunk's last hop is the next chunk's (and the next call's) hop -1
        DOA_HIP(d, carry_last_hop(d->d_hist.get(), xc, n, H, M, d->S, d->layout, mic_stride, stream_stride, s));
    }
    return BF_OK;
}

int bf_doa_process(bf_doa *d, const float *x_host, size_t n_frames, double *map_host, int32_t *peak_host) {
    if (!d) return fail(nullptr, BF_EINVAL, "bf_doa_process: handle is NULL");
    if (!map_host && !peak_host) return fail(d, BF_EINVAL, "bf_doa_process: map and peak are both NULL");
    return bf_doa_process_eig(d, x_host, n_frames, map_host, peak_host, nullptr);
}

int bf_doa_process_eig(bf_doa *d, const float *x_host, size_t n_frames, double *map_host, int32_t *peak_host, double *eig_host) {
    if (!d) return fail(nullptr, BF_EINVAL, "bf_doa_process: handle is NULL");
    if (!map_host && !peak_host && !eig_host) return fail(d, BF_EINVAL, "bf_doa_process: map, peak and eig are all NULL");
    if (eig_host && d->method != BF_DOA_MUSIC) return fail(d, BF_EINVAL, "bf_doa_process: eig needs the MUSIC method");
    if (n_frames % (size_t)d->W != 0) return fail(d, BF_EINVAL, "bf_doa_process: n_frames is not a multiple of frames_per_block");
    if (n_frames == 0) return BF_OK;
    if (!x_host) return fail(d, BF_EINVAL, "bf_doa_process: x is NULL");
    DOA_HIP(d, hipSetDevice(d->device));
    const size_t xe = (size_t)d->S * d->M * n_frames * d->H, nb = (size_t)d->S * (n_frames / d->W), me = nb * d->D, ee = nb * d->M;
    if (xe > d->d_x.size() || (map_host && me > d->d_map.size()) || (peak_host && nb > d->d_peak.size()) ||
        (eig_host && ee > d->d_eig.size())) {
        DOA_HIP(d, hipStreamSynchronize(d->stream));  // a batch still in flight may use the old staging
        if (d->d_x.reserve(xe) != hipSuccess || (map_host && d->d_map.reserve(me) != hipSuccess) ||
            (peak_host && d->d_peak.reserve(nb) != hipSuccess) || (eig_host && d->d_eig.reserve(ee) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(d, BF_ENOMEM, "bf_doa_process staging");
        }
    }
    float *const d_x = d->d_x.get();
    double *const d_map = map_host ? d->d_map.get() : nullptr;
    int32_t *const d_peak = peak_host ? d->d_peak.get() : nullptr;
    double *const d_eig = eig_host ? d->d_eig.get() : nullptr;
    DOA_HIP(d, hipMemcpyAsync(d_x, x_host, xe * sizeof(float), hipMemcpyHostToDevice, d->stream));
    const int rc = bf_doa_process_device_eig(d, d_x, n_frames, d_map, d_peak, d_eig, d->stream);
    if (rc != BF_OK) return rc;
    if (eig_host) DOA_HIP(d, hipMemcpyAsync(eig_host, d_eig, ee * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if (map_host) DOA_HIP(d, hipMemcpyAsync(map_host, d_map, me * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    if (peak_host) DOA_HIP(d, hipMemcpyAsync(peak_host, d_peak, nb * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
    DOA_HIP(d, hipStreamSynchronize(d->stream));
    return BF_OK;
}

// ---- steering tracks: from the peaks of the maps to a table index per frame (no handle) ---------------------------------------------
int bf_track_from_peaks_device(const int32_t *peak_dev, const double *map_dev, int n_angles, int n_streams, size_t n_blocks,
                               int frames_per_block, int latency_blocks, double min_peak, int32_t *carry_dev, int32_t *track_dev,
                               void *hip_stream) {
    if (n_angles < 1 || n_streams < 1 || frames_per_block < 1 || latency_blocks < 0)
        return fail(nullptr, BF_EINVAL, "bf_track_from_peaks_device: n_angles, n_streams, frames_per_block >= 1 and latency_blocks >= 0");
    if (!peak_dev || !carry_dev || !track_dev) return fail(nullptr, BF_EINVAL, "bf_track_from_peaks_device: peak, carry or track is NULL");
    if (!map_dev && min_peak > 0) return fail(nullptr, BF_EINVAL, "bf_track_from_peaks_device: min_peak > 0 needs the map");
    if (n_blocks == 0) return BF_OK;  // carry stays: what block 0 of the next call gets
    TrackFromPeaksArgs a;
    a.peak = peak_dev;
    a.map = map_dev;
    a.carry = carry_dev;
    a.track = track_dev;
    a.min_peak = min_peak;
    a.n_blocks = (long)n_blocks;
    a.n_angles = n_angles;
    a.frames_per_block = frames_per_block;
    a.latency = latency_blocks;
    DOA_HIP(nullptr, launch_track_from_peaks(a, n_streams, (hipStream_t)hip_stream));
    return BF_OK;
}

// ---- multi-source picks and the column track they publish (no handle) ------------------------------------------------------------------
static_assert(BF_DOA_MAX_PICKS == kPickMax && BF_DOA_MAX_PICKS == BF_MAX_INTERF + 1, "a look direction and every interferer");
static_assert(BF_DOA_MAX_ANGLES == 64 * kPickSlots, "doa_pick_kernel keeps a whole row in one wavefront's registers");

int bf_doa_pick_device(const double *map_dev, const double *angles_dev, int n_angles, int n_streams, size_t n_blocks, int k,
                       double min_sep_deg, double rel_floor, int32_t *picks_dev, void *hip_stream) {
    if (n_angles < 1 || n_angles > BF_DOA_MAX_ANGLES || n_streams < 1)
        return fail(nullptr, BF_EINVAL, "bf_doa_pick_device: n_angles must be in 1 .. BF_DOA_MAX_ANGLES and n_streams >= 1");
    if (k < 1 || k > BF_DOA_MAX_PICKS) return fail(nullptr, BF_EINVAL, "bf_doa_pick_device: k must be in 1 .. BF_DOA_MAX_PICKS");
    if (!std::isfinite(min_sep_deg) || min_sep_deg < 0 || !std::isfinite(rel_floor))
        return fail(nullptr, BF_EINVAL, "bf_doa_pick_device: min_sep_deg must be finite and >= 0, rel_floor finite");
    if (!map_dev || !angles_dev || !picks_dev) return fail(nullptr, BF_EINVAL, "bf_doa_pick_device: map, angles or picks is NULL");
    if (n_blocks == 0) return BF_OK;
    DoaPickArgs a;
    a.map = map_dev;
    a.angles = angles_dev;
    a.picks = picks_dev;
    a.min_sep = min_sep_deg;
    a.rel_floor = rel_floor;
    a.n_rows = (long)n_streams * (long)n_blocks;
    a.n_angles = n_angles;
    a.k = k;
    DOA_HIP(nullptr, launch_doa_pick(a, (hipStream_t)hip_stream));
    return BF_OK;
}

int bf_ctrack_from_picks_device(const int32_t *picks_dev, const double *map_dev, int n_angles, int k, int n_streams, size_t n_blocks,
                                int frames_per_block, int latency_blocks, double min_peak, int n_cols, int32_t *carry_dev,
                                int32_t *track_dev, void *hip_stream) {
    if (n_angles < 1 || n_streams < 1 || frames_per_block < 1 || latency_blocks < 0)
        return fail(nullptr, BF_EINVAL, "bf_ctrack_from_picks_device: n_angles, n_streams, frames_per_block >= 1 and latency_blocks >= 0");
    if (k < 1 || k > BF_DOA_MAX_PICKS) return fail(nullptr, BF_EINVAL, "bf_ctrack_from_picks_device: k must be in 1 .. BF_DOA_MAX_PICKS");
    if (n_cols < 1 || n_cols > BF_MAX_INTERF + 1)
        return fail(nullptr, BF_EINVAL, "bf_ctrack_from_picks_device: n_cols must be in 1 .. BF_MAX_INTERF + 1");
    if (!picks_dev || !carry_dev || !track_dev) return fail(nullptr, BF_EINVAL, "bf_ctrack_from_picks_device: picks, carry or track is NULL");
    if (!map_dev && min_peak > 0) return fail(nullptr, BF_EINVAL, "bf_ctrack_from_picks_device: min_peak > 0 needs the map");
    if (n_blocks == 0) return BF_OK;  // carry stays: what block 0 of the next call gets
    CtrackFromPicksArgs a;
    a.picks = picks_dev;
    a.map = map_dev;
    a.carry = carry_dev;
    a.track = track_dev;
    a.min_peak = min_peak;
    a.n_blocks = (long)n_blocks;
    a.n_angles = n_angles;
    a.k = k;
    a.n_cols = n_cols;
    a.frames_per_block = frames_per_block;
    a.latency = latency_blocks;
    DOA_HIP(nullptr, launch_ctrack_from_picks(a, n_streams, (hipStream_t)hip_stream));
    return BF_OK;
}

static_assert(BF_ASSIGN_STATE_INTS == kAssignStateInts && kAssignMax == kPickMax, "a slot per column, a candidate per pick");

int bf_ctrack_assign_device(const int32_t *picks_dev, const double *map_dev, const double *angles_dev, int n_angles, int k,
                            int n_streams, size_t n_blocks, int frames_per_block, int latency_blocks, double min_peak,
                            double gate_deg, int min_hits, int max_coast, int n_cols, int32_t *state_dev, int32_t *track_dev,
                            int32_t *active_dev, void *hip_stream) {
    if (n_angles < 1 || n_angles > BF_DOA_MAX_ANGLES) return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: n_angles must be in 1 .. BF_DOA_MAX_ANGLES");
    if (k < 1 || k > BF_DOA_MAX_PICKS) return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: k must be in 1 .. BF_DOA_MAX_PICKS");
    if (n_streams < 1 || frames_per_block < 1 || latency_blocks < 0)
        return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: n_streams, frames_per_block >= 1 and latency_blocks >= 0");
    if (n_cols < 1 || n_cols > BF_MAX_INTERF + 1) return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: n_cols must be in 1 .. BF_MAX_INTERF + 1");
    if (!std::isfinite(gate_deg) || gate_deg < 0) return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: gate_deg must be finite and >= 0");
    if (min_hits < 1 || max_coast < 0) return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: min_hits >= 1 and max_coast >= 0");
    if (!picks_dev || !angles_dev || !state_dev || !track_dev)
        return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: picks, angles, state or track is NULL");
    if (!map_dev && min_peak > 0) return fail(nullptr, BF_EINVAL, "bf_ctrack_assign_device: min_peak > 0 needs the map");
    if (n_blocks == 0) return BF_OK;  // the state stays: what block 0 of the next call finds
    CtrackAssignArgs a;
    a.picks = picks_dev;
    a.map = map_dev;
    a.angles = angles_dev;
    a.state = state_dev;
    a.track = track_dev;
    a.active = active_dev;
    a.min_peak = min_peak;
    a.gate = gate_deg;
    a.n_blocks = (long)n_blocks;
    a.n_angles = n_angles;
    a.k = k;
    a.n_cols = n_cols;
    a.frames_per_block = frames_per_block;
    a.latency = latency_blocks;
    a.min_hits = min_hits;
    a.max_coast = max_coast;
    DOA_HIP(nullptr, launch_ctrack_assign(a, n_streams, (hipStream_t)hip_stream));
    return BF_OK;
}

int bf_doa_reset(bf_doa *d) {
    if (!d) return fail(nullptr, BF_EINVAL, "bf_doa_reset: handle is NULL");
    DOA_HIP(d, hipSetDevice(d->device));
    DOA_HIP(d, hipDeviceSynchronize());  // batches enqueued on any stream finish with the old history
    DOA_HIP(d, hipMemset(d->d_hist.get(), 0, (size_t)d->S * d->M * d->H * sizeof(float)));
    return BF_OK;
}

void bf_doa_destroy(bf_doa *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;  // the buffers are freed here: after the synchronisation above
}
