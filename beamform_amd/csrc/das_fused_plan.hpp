// das_fused_plan.hpp -- which fused fp32 das kernel serves a batch and how the batch is cut into runs, host arithmetic (docs/DISPATCH.md
// lists the outcome per shape).  Plain C++: the CPU suite checks it through tests/host_emul (every das (fp32) row of the dispatch table,
// and on random shapes that the runs cover a stream, keep the chosen kernel's multiple and stay inside the run budget).
// enqueue_das_fused (kernels.hpp) carries a decision out.
#pragma once

#include "../../include/bfcore.h"

namespace bf {

// The kernels a batch can get:
//   kRegs      das_fused_kernel<layout, npl, unr, group>: the 32 x 32 in-register FFT-1024, one block of 16 half-wavefronts per run
//   kIl4       das_fused_il_kernel<2, 1>: [sample][mic] input, 4 microphones: one 16-byte load = the whole sample, two frames per wavefront
//   kIl8       das_fused_il8_kernel: [sample][mic] input, 8 microphones: each half-wavefront loads its 16 bytes of the 32-byte sample
//   kWave2048  das_fused_wave2048_kernel<layout>: period 1024, one 2048-point transform per frame on a full wavefront, eight frames in
//              flight per block, tails through an LDS ring
//   kDirs      das_fused_dirs_kernel: one set of forward transforms per frame serves up to 16 look directions per launch
//   kGen       das_fused_gen_kernel<n_fft>: LDS-staged transforms (das_fused_gen.hip), any period
enum class DasFusedKernel { kRegs, kIl4, kIl8, kWave2048, kDirs, kGen };

// Everything about one batch.  A run = consecutive frames of one stream that one block works through; the first frame of a run that does not
// start the stream is recomputed for its overlap-add tail.
struct DasFusedLaunch {
    DasFusedKernel kernel;
    // the template arguments of kRegs: pairs whose gains sit in LDS (0: all of them read through L2), the unrolled pair count (0: a loop),
    // and 1024 / n_fft frames of a period below 512 interleaved per unit of work (group mode; 1 otherwise)
    int npl, unr, group;
    int frames_per_chunk, chunks_per_stream;  // the runs of a stream (of an INPUT stream for kDirs)
    unsigned blocks;       // one per run
    bool zero_run_heads;   // the first hop of every run but a stream's first is completed by atomic adds: zero before the launch
    bool group_tables;     // group mode: das_pair_gains_interleaved tables and the 1024-point twiddles, not the period's own
};

// das_interleave / das_split2048 / das_shared_dirs: the switches of those names (switches.hpp).  n_streams counts INPUT streams; every
// input stream yields n_dirs output streams.  n_frames >= 1.
inline DasFusedLaunch das_fused_decide(int hop, int layout, int n_mics, int n_streams, int n_dirs, bool dump, long n_frames, int n_cus,
                                       int das_interleave, int das_split2048, int das_shared_dirs) {
    const int n_fft = 2 * hop, np = (n_mics + 1) / 2, n_out = n_streams * n_dirs;
    const bool planar = layout == BF_PLANAR;
    DasFusedLaunch d{};
    d.group = 1;
    long budget = n_cus, multiple = 1;  // runs in flight; a run is a multiple of this many frames
    if (hop == 512) {
        // several look directions, planar input, <= 8 microphones: das_shared_dirs = the smallest direction count that shares the transforms
        // (not bit for bit the per-direction kernel: the window products are fused differently)
        const bool shared = planar && n_mics <= 8 && !dump && das_shared_dirs > 0 && n_dirs >= das_shared_dirs;
        d.kernel = shared ? DasFusedKernel::kDirs : !planar && n_mics == 4 ? DasFusedKernel::kIl4 : !planar && n_mics == 8 ? DasFusedKernel::kIl8 : DasFusedKernel::kRegs;
        multiple = 16;  // sixteen half-wavefronts per block
    } else if (hop == 1024 && !dump && das_split2048 != 0) {
        d.kernel = DasFusedKernel::kWave2048;
        multiple = 8;  // eight frames per pass of a block
    } else if (hop < 512 && !dump && das_interleave != 0) {
        d.kernel = DasFusedKernel::kRegs;  // the period-512 kernel on groups of interleaved frames: HBM sees every hop once
        d.group = 1024 / n_fft;
        d.group_tables = true;
        multiple = 16 * d.group;  // sixteen groups per pass of a block
    } else {
        d.kernel = DasFusedKernel::kGen;
        // blocks of 13 n_fft bytes of LDS (26 n_fft at 8192) share a CU
        budget *= n_fft <= 512 ? 8 : n_fft <= 1024 ? 6 : n_fft <= 2048 ? 3 : 1;
    }
    // (read by kRegs only) up to 8 microphones the gain tables fit beside the transpose buffers and the tail ring; planar input: the pair
    // loop unrolled for the exact pair count, the next pair's loads issued from inside the gain loop
    d.npl = np <= 2 ? np : np <= 4 ? 4 : 0;
    d.unr = planar && np <= 4 ? np : 0;
    const int launch_streams = d.kernel == DasFusedKernel::kDirs ? n_streams : n_out;
    const long runs = budget > launch_streams ? budget / launch_streams : 1;
    const long fpc = ((n_frames + runs - 1) / runs + multiple - 1) / multiple * multiple;
    const long cps = (n_frames + fpc - 1) / fpc;
    d.frames_per_chunk = (int)fpc;
    d.chunks_per_stream = (int)cps;
    d.blocks = (unsigned)(cps * launch_streams);
    d.zero_run_heads = cps > 1 && d.kernel != DasFusedKernel::kGen;
    return d;
}

}  // namespace bf
