// Kernel launchers of libbfcore stubbed for the host ThreadSanitizer harness (TEST INFRASTRUCTURE).
// No arithmetic of the hot path happens here: every launcher only (1) reads the tables it was handed, on the calling
// (processing) thread, so that ThreadSanitizer sees the same host-memory accesses a real launch would order on the
// stream, and (2) checks that the arguments of ONE batch are consistent with each other.
#include <atomic>
#include <cmath>

#include "../../beamform_amd/csrc/kernels.hpp"
#include "../../beamform_amd/csrc/pipeline_kernels.hpp"

std::atomic<long> g_inconsistent{0};
std::atomic<long> g_launches{0};

namespace bf {

static hipError_t launch_stft(const ChainPlan &, const StftArgs &, int, hipStream_t) { return hipSuccess; }
static hipError_t launch_istft(const ChainPlan &, const IstftArgs &, int, hipStream_t) { return hipSuccess; }
static hipError_t launch_smooth(const ChainPlan &, const float *, float *, double *, long, int, hipStream_t) { return hipSuccess; }
static hipError_t launch_gsc_nlms(const ChainPlan &, const float *, float *, float *, long, int, int, const bf_config &, hipStream_t) { return hipSuccess; }

// The per-bin stage: the batch must see ONE consistent {column count, steering table}.  The table is laid out
// [dir][col][mic][bin] with kp1 columns; every uploaded steering entry of mic >= 1 has modulus 1, memory that was never
// uploaded reads 0 (the stub's hipMalloc zero-fills).
static hipError_t launch_bins(const ChainPlan &, const BinsArgs &a, int, hipStream_t) {
    g_launches++;
    const int M = a.n_mics, kp1 = a.kp1;
    if (a.steer_dir_stride != (long)kp1 * M * 1024) g_inconsistent++;
    if (M > 1)
        for (int d = 0; d < a.n_dirs; ++d)
            for (int c = 0; c < kp1; ++c)
                for (int j = 1; j < 1024; j += 97) {
                    const f64x2 w = a.steer[d * a.steer_dir_stride + ((long)c * M + 1) * 1024 + j];
                    if (std::fabs(w.x * w.x + w.y * w.y - 1.0) > 1e-9) g_inconsistent++;
                }
    return hipSuccess;
}

// the fused STFT + per-bin launcher (the chain decision itself is pure host arithmetic, chain_plan.hpp): the per-bin stage's checks
static hipError_t launch_stft_bins(const ChainPlan &p, const StftArgs &, const BinsArgs &b, int n, hipStream_t s) { return launch_bins(p, b, n, s); }

// the harness runs at hop 512; the other sizes share the same host code
static const KernelSet g_stub_set = {1024, &launch_stft, &launch_bins, &launch_stft_bins, &launch_istft, &launch_smooth, &launch_gsc_nlms};
const KernelSet *kernel_set_n128() { return &g_stub_set; }
const KernelSet *kernel_set_n256() { return &g_stub_set; }
const KernelSet *kernel_set_n512() { return &g_stub_set; }
const KernelSet *kernel_set_n1024() { return &g_stub_set; }
const KernelSet *kernel_set_n2048() { return &g_stub_set; }
const KernelSet *kernel_set_n4096() { return &g_stub_set; }
const KernelSet *kernel_set_n8192() { return &g_stub_set; }
// das in double in one launch: the decision (das_f64_plan.hpp) and the steering summary (geometry.hpp) are pure host arithmetic and run
// for real; only carrying the decision out is stubbed.  The harness's das case is planar with a unit row 0: the frame-pair kernel, and
// a walk that names every microphone past 0 exactly once, whichever table the batch was launched with.
hipError_t enqueue_das_f64(DasF64Args a, const DasF64Launch &d, float *, hipStream_t, hipEvent_t, hipEvent_t, bool *) {
    g_launches++;
    unsigned seen = a.extra_mic > 0 ? 1u << a.extra_mic : 0;
    int named = a.extra_mic > 0 ? 1 : 0;
    for (int k = 0; k < a.n_tr; ++k, ++named) seen |= 1u << a.slot_mic[k];
    if (d.path != DasF64Path::kFramePair || !a.mic0_unit || named != a.n_mics - 1 || seen != (1u << a.n_mics) - 2) g_inconsistent++;
    return hipSuccess;
}

// the fused fp32 das decision is pure host arithmetic (das_fused_plan.hpp, through kernels.hpp): only carrying it out is stubbed
hipError_t enqueue_das_fused(const DasFusedArgs &a, const DasFusedLaunch &, int, hipStream_t, hipEvent_t, hipEvent_t, bool *) {
    g_launches++;
    const int np = (a.n_mics + 1) / 2;
    double acc = 0;  // read the whole gain table this launch was given
    for (long i = 0; i < (long)a.n_dirs * np * 1024; ++i) acc += a.gains[i].x;
    if (!(acc == acc)) g_inconsistent++;
    return hipSuccess;
}
hipError_t launch_stream_rms(const float *, long, int, double *, hipStream_t) { return hipSuccess; }
hipError_t launch_das_hermitian_dump(const f32x2 *, f64x2 *, long, hipStream_t) { return hipSuccess; }
hipError_t launch_das_hermitian_dump_gen(const f32x2 *, f64x2 *, long, int, hipStream_t) { return hipSuccess; }

}  // namespace bf
