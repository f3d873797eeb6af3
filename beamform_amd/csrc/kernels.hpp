// kernels.hpp -- host-visible launchers of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "das_fused_plan.hpp"
#include "geometry.hpp"

namespace bf {

// ---- fused fp32 DAS (das_fused.hip) ------------------------------------------
struct DasFusedArgs {
    const float *x;        // input samples, layout per `layout`
    const float *hist_in;  // [stream][mic][hop] (planar) or [stream][hop][mic]: the hop before frame 0
    float *hist_out;       // same layout: the last hop of this batch (ring-buffer carry, util.h:305-308)
    float *y;              // [stream][n_frames*hop]
    const float *tail_in;  // [stream][hop] second half of the frame before frame 0 (out_buff[0], util.h:302)
    float *tail_out;       // [stream][hop] second half of the last frame of this batch
    const f32x2 *gains;    // das_pair_gains() tables, one per look direction: [dir][pair][1024]
    const f32x2 *twiddle;  // twiddle_table_32x32<f32x2>()
    const float *window;   // sqrt-Hann, fp32, natural order [1024]
    const float *zeros;    // >= 1024 zero floats: partner channel of the last mic when n_mics is odd
    f32x2 *sdump;          // nullable: [stream][frame][1024] accumulated pair spectrum S (1/N folded in)
    long n_frames;         // frames per stream
    long mic_stride;       // planar: samples between mics of one stream
    long stream_stride_x;  // samples between streams in x
    int n_streams;         // OUTPUT streams = input streams * n_dirs (stream = input * n_dirs + dir)
    int n_dirs;            // look directions per input stream (>= 1); x / hist are indexed by the input stream
    int n_mics;
    int frames_per_chunk;
    int chunks_per_stream;
    int layout;            // bf_layout
    int group = 1;         // das_fused_kernel only: R = 1024 / n_fft frames of a period below 512 interleaved per unit of work (1: period 512)
};
// Carries out d = das_fused_decide(...) (das_fused_plan.hpp) on `stream`; a.frames_per_chunk / chunks_per_stream / group are d's, a.gains /
// a.twiddle / a.window the tables of d's kernel:
//   kRegs, kIl4, kIl8, kDirs  das_pair_gains tables [dir][pair][1024] and twiddle_table_32x32, as above; in group mode (d.group_tables) the
//                             das_pair_gains_interleaved tables of the period, same shape
//   kWave2048, kGen           das_pair_gains_natural tables [dir][pair][n_fft], stockham_twiddles(n_fft), window n_fft floats; kGen's sdump
//                             rows are n_fft long, natural order
// The zeroing d asks for comes first, then kev0 / kev1 (nullable) are recorded right around the kernel launches (kDirs: one launch per 16
// look directions); *kev_recorded is raised once the second record has succeeded (pipeline.hpp Engine::kev0).
hipError_t enqueue_das_fused(const DasFusedArgs &a, const DasFusedLaunch &d, int n_fft, hipStream_t stream, hipEvent_t kev0, hipEvent_t kev1, bool *kev_recorded);
// enqueue_das_fused's kGen launch (das_fused_gen.hip holds those kernels)
hipError_t enqueue_das_fused_gen(const DasFusedArgs &a, int n_fft, unsigned blocks, hipStream_t stream);

// per-stream root-mean-square of y [n_streams][n_samples] -> rms[n_streams] (double); `sumsq` = n_streams doubles of scratch
hipError_t launch_stream_rms(const float *y, long n_samples, int n_streams, double *sumsq, hipStream_t stream);

// S dump -> Hermitian part of the reference's y_fft as double2 [frames][1024]
hipError_t launch_das_hermitian_dump(const f32x2 *sdump, f64x2 *out, long n_frames_total, hipStream_t stream);

// the generic periods' S dump (rows n_fft long, natural order) -> double2 [frames][n_fft]
hipError_t launch_das_hermitian_dump_gen(const f32x2 *sdump, f64x2 *out, long n_frames_total, int n_fft, hipStream_t stream);

}  // namespace bf
