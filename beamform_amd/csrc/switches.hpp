// switches.hpp -- every environment switch of the library, read ONCE per process (DESIGN.md 8 describes what each one selects).
// A switch is for A/B runs and cross-checks: tests and tools set it through the environment of a child process.
#pragma once

#include <cstdlib>
#include <string>

namespace bf {

struct Switches {
    static int num(const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; }
    static const char *keep(const char *v) { static std::string s; return v ? (s = v).c_str() : nullptr; }  // (a later setenv may move the environment)
    const char *const das_f64_sched = keep(getenv("BF_DAS_F64_SCHED"));  // as das_f64_plan's `env` takes it: null = unset
    const int das_interleave = num("BF_DAS_INTERLEAVE", 1);    // 0 = periods below 512 of fused fp32 das run the generic kernel
    const int das_il_ring = num("BF_DAS_IL_RING", 1);          // 0 = das in double on [sample][mic] input always goes through the transposition
    const int das_split2048 = num("BF_DAS_SPLIT2048", 3);      // 0 = period 1024 of fused fp32 das runs the generic kernel
    const int das_shared_dirs = num("BF_DAS_SHARED_DIRS", 6);  // the smallest direction count that takes das_fused_dirs_kernel (0: never)
    const int fused_bins = num("BF_FUSED_BINS", 1);            // 0 = the STFT -> per-bin chain instead of the one-launch kernels
    const bool stft_small = num("BF_STFT_SMALL", 1) != 0;      // off only when set and equal to 0: the generic kernels at N = 128 / 256 / 512
    const bool stft_split = num("BF_STFT_SPLIT", 1) != 0;      // likewise: the generic kernels at N = 2048
    const bool mvdr_group = num("BF_MVDR_GROUP", 0) != 0;      // on when set and non-zero: the group-per-problem kernel only
    const int mvdr_tile = num("BF_MVDR_TILE", 0);              // tile length of mvdr_fast_kernel (0 = chosen by cost); held to min(value, frames, 512),
                                                               // the slack the spectra workspace has for the prefetch past a short last tile (chain_geom.hpp)
    const int gss_group = num("BF_GSS_GROUP", -1);             // 1 / 0 force the group / the lane kernel (-1 = by shape)
    const bool gsc_serial = num("BF_GSC_SERIAL", 0) == 1;      // on only when equal to 1: the sums in the reference's tap order
};

inline const Switches &switches() {
    static const Switches sw;  // filled on first use (thread-safe)
    return sw;
}

}  // namespace bf
