// doa.hpp -- SRP-PHAT direction-of-arrival maps (bf_doa_*, include/bfcore.h): argument blocks and launchers of doa_kernels.hip.
// The spectra come from the bin pipeline's forward transform (pipeline_kernels.hpp launch_stft, packed microphone pairs, halved).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "geometry.hpp"

namespace bf {

void set_last_error(const std::string &msg);  // capi.cpp: the text bf_last_error(NULL) returns

// Frames of one map tile (a workgroup: 4 wavefronts x 4 lane groups x 4 frames) and angles of one tile (16 lanes x 2 angles).
constexpr int kDoaTileFrames = 64, kDoaTileAngles = 32;
// In-band bins of one segment of the band: a workgroup sums |y|^2 over one segment, the reduction kernel adds the segments in order.
// The partition depends only on the band, so every frame's sum is formed the same way however a batch is cut.
constexpr int kDoaSegBins = 48;
inline int doa_segments(int n_bins) { return (n_bins + kDoaSegBins - 1) / kDoaSegBins; }

struct DoaMapArgs {
    const f64x2 *Z;            // [stream][frames_ws][NP][N] packed pair spectra, stored halved (StftArgs::halve)
    const unsigned *flags;     // [stream][n_frames + 1][2]: per hop (hop -1 first) the microphones with a nonzero sample in 1..H-1 / in 0..H-1
    const f64x2 *steer;        // [bin - klo][mic][angle]: w_m(theta_d, k) of SteeringSet::update_column(first = true)
    double *part;              // [segment][stream][frames_ws][angle]: sum over the segment's bins of |sum_m conj(w) X^|^2
    double eps;                // PHAT floor
    long n_frames, frames_ws;
    int n_streams, n_mics, nfft, n_angles, klo, n_bins;
};
struct DoaReduceArgs {
    const double *part;
    double *map;               // [stream][map_blocks][angle] (nullable)
    int *peak;                 // [stream][map_blocks] (nullable)
    double scale;              // 1 / (W |K| M^2)
    long frames_ws, map_blocks, block0;  // block0: index of the chunk's first block in the caller's map
    long n_blocks;             // blocks of this chunk
    int n_streams, n_angles, n_segments, frames_per_block;
};

// bf_track_from_peaks_device: peaks (and maps) of the blocks -> the steering track of their frames
struct TrackFromPeaksArgs {
    const int32_t *peak;       // [stream][n_blocks]
    const double *map;         // [stream][n_blocks][n_angles]; null: every block publishes
    int32_t *carry;            // [stream]: in, the index in force in front of block 0; out, the one a block n_blocks would get
    int32_t *track;            // [stream][n_blocks * frames_per_block]
    double min_peak;
    long n_blocks;
    int n_angles, frames_per_block, latency;
};

// per hop of x (hops -1 .. n_frames-1, hop -1 = hist) the microphones with a nonzero sample: layout as the stft kernel reads it
hipError_t launch_doa_hop_flags(const float *x, const float *hist, unsigned *flags, long n_frames, long mic_stride, long stream_stride_x,
                                int n_streams, int n_mics, int hop, int layout, hipStream_t s);
hipError_t launch_doa_map(const DoaMapArgs &a, hipStream_t s);
hipError_t launch_doa_reduce(const DoaReduceArgs &a, hipStream_t s);
hipError_t launch_track_from_peaks(const TrackFromPeaksArgs &a, int n_streams, hipStream_t s);

}  // namespace bf
