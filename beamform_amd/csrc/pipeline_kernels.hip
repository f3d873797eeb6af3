// pipeline_kernels.hip -- dispatch of the per-bin stage of the fp64 bin pipeline.  The kernels live in
// stft_istft.hip, mask_kernels.hip (das / phase / phasempf / mcra), cov_kernels.hip (mvdr / lcmv) and
// gsc_gss_kernels.hip.
#include "pipeline_kernels.hpp"

#include <hip/hip_runtime.h>

namespace bf {
namespace BF_NTAG {

hipError_t launch_bins(const ChainPlan &p, const BinsArgs &a, int, hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;  // (kFusedTail: the fused front ran the per-bin stage)
    switch (p.bins) {
        case ChainBins::kFusedTail: break;
        case ChainBins::kPointwise: e = launch_pointwise(p, a, s); break;
        case ChainBins::kMpfMask: e = launch_mpf_mask(p, a, s); break;
        case ChainBins::kMcra: e = launch_mcra_node(p, a, s); break;
        case ChainBins::kGscAlign: e = launch_gsc_align(p, a, s); break;
        case ChainBins::kMvdrFast:
        case ChainBins::kCov2d:
        case ChainBins::kMvdrLcmv: e = launch_mvdr_lcmv(p, a, s); break;
        case ChainBins::kGss:
        case ChainBins::kGssLane: e = launch_gss(p, a, s); break;
    }
    return e != hipSuccess ? e : launch_bins_end(p, a, s);
}

}  // namespace BF_NTAG

// the launchers of this FFT size, as the host pipeline sees them
const KernelSet *BF_CAT2(kernel_set_n, BF_NFFT)() {
    static const KernelSet ks = {BF_NFFT, &BF_NTAG::launch_stft, &BF_NTAG::launch_bins, &BF_NTAG::launch_stft_bins_fused,
                                 &BF_NTAG::launch_istft,
                                 &BF_NTAG::launch_smooth, &BF_NTAG::launch_gsc_nlms, &BF_NTAG::launch_gss_postfilter};
    return &ks;
}

}  // namespace bf
