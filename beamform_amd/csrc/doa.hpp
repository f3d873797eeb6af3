// doa.hpp -- SRP-PHAT direction-of-arrival maps (bf_doa_*, include/bfcore.h): argument blocks and launchers of doa_kernels.hip.
// The spectra come from the bin pipeline's forward transform (pipeline_kernels.hpp launch_stft, packed microphone pairs, halved).
//
// The Capon (MVDR) map is the handle's second method (bf_doa_set_method): its launch decisions are the plain C++ of capon_decide below,
// which the CPU suite compiles on its own (-DBF_DOA_PLAN_ONLY: no HIP header is read in front of the #ifndef).  The MUSIC map, the third
// method, runs on the same per-bin covariances: music_decide is capon_decide with the eigenvectors' room and the profile's partial sums.
#pragma once

#include <cstddef>
#include <cstdint>

namespace bf {

// ---- Capon map: one pure launch decision per batch -----------------------------------------------------------------------------------
// One lane per (stream, block, in-band bin) problem, one wavefront per 64 consecutive bins of a block: a band segment.  The segments
// depend on |K| only, so a block's sum over the band is formed the same way however a stream is cut into calls or chunks.
constexpr int kCaponSegBins = 64;
constexpr int kCaponRegMics = 8;                    // up to here the covariance and its factor live in registers
constexpr size_t kCaponChunkBytes = 256ull << 20;   // spectra + partial sums + work space of one chunk (never less than one block)
inline int capon_segments(int n_bins) { return (n_bins + kCaponSegBins - 1) / kCaponSegBins; }

enum class CaponPath : int { kRegisters = 0, kWorkspace = 1 };

struct CaponShape {
    int n_mics, n_streams, nfft, n_angles, n_bins, frames_per_block;
    long n_frames;  // of the batch: a multiple of frames_per_block
};
struct CaponPlan {
    CaponPath path;         // by microphone count alone
    int mp;                 // kRegisters: the kernel's compile-time row count, 2 x microphone pairs (2, 4, 6, 8); kWorkspace: 0
    int segments;           // of the band: by |K| alone
    int ws_elems;           // kWorkspace: complex doubles per problem, the lower triangle of R with its diagonal + the solve's vector
    long chunk_blocks;      // blocks of one chunk: what fits the budget, at least one, at most the batch
    long chunk_frames;      // chunk_blocks x frames_per_block
    unsigned grid_x, grid_y;  // of a full chunk: (segments x chunk_blocks, streams); 64 lanes per workgroup
    size_t z_bytes;         // packed pair spectra of one chunk
    size_t part_bytes;      // partial sums of one chunk: [segment][stream][chunk block][angle] doubles
    size_t ws_bytes;        // kWorkspace: [element][stream][chunk block][segment][lane] complex doubles; kRegisters: 0
    size_t table_bytes;     // the steering table in the kernel's layout, [angle][mic][bin - klo] complex doubles
};

// ws_elems: complex doubles per problem in the work space (kWorkspace); part_cols: doubles per (segment, stream, block) of partial sums
inline CaponPlan cov_decide(const CaponShape &c, size_t ws_elems, size_t part_cols) {
    CaponPlan p{};
    const size_t M = (size_t)c.n_mics, S = (size_t)c.n_streams, NP = (M + 1) / 2, W = (size_t)c.frames_per_block;
    p.path = c.n_mics <= kCaponRegMics ? CaponPath::kRegisters : CaponPath::kWorkspace;
    p.mp = p.path == CaponPath::kRegisters ? 2 * (int)NP : 0;
    p.segments = capon_segments(c.n_bins);
    p.ws_elems = p.path == CaponPath::kWorkspace ? (int)ws_elems : 0;
    const size_t G = (size_t)p.segments;
    const size_t z_block = W * S * NP * (size_t)c.nfft * 16, part_block = G * S * part_cols * 8;
    const size_t ws_block = (size_t)p.ws_elems * S * G * kCaponSegBins * 16;
    long nb = (long)(kCaponChunkBytes / (z_block + part_block + ws_block));
    const long batch = c.n_frames / c.frames_per_block;
    if (nb < 1) nb = 1;
    if (nb > batch) nb = batch;
    p.chunk_blocks = nb;
    p.chunk_frames = nb * c.frames_per_block;
    p.grid_x = (unsigned)(G * (size_t)nb);
    p.grid_y = (unsigned)S;
    p.z_bytes = z_block * (size_t)nb;
    p.part_bytes = part_block * (size_t)nb;
    p.ws_bytes = ws_block * (size_t)nb;
    p.table_bytes = (size_t)c.n_angles * M * (size_t)c.n_bins * 16;
    return p;
}

// Capon: the lower triangle of R with its diagonal + the solve's vector; one partial sum per angle
inline CaponPlan capon_decide(const CaponShape &c) {
    const size_t M = (size_t)c.n_mics;
    return cov_decide(c, M * (M + 1) / 2 + M, (size_t)c.n_angles);
}

// MUSIC: the triangle, the frame's spectra (then the columns' noise weights), the eigenvectors; one partial sum per angle, then, behind
// the chunk's angle rows, one per eigenvalue: [segment][stream][chunk block][angle] ++ [segment][stream][chunk block][mic]
inline CaponPlan music_decide(const CaponShape &c) {
    const size_t M = (size_t)c.n_mics;
    return cov_decide(c, M * (M + 1) / 2 + M + M * M, (size_t)c.n_angles + M);
}

}  // namespace bf

#ifndef BF_DOA_PLAN_ONLY
#include <hip/hip_runtime.h>

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
    double mu = 0.0, denom = 1.0;  // mu > 0 (MUSIC): the value is mu / (mu + sum / denom) and scale is not used
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

// bf_doa_pick_device: the k strongest separated peaks of every map row (the rule: doa_pick.hpp and include/bfcore.h)
constexpr int kPickSlots = 16;  // angles per lane: lane l keeps angles l, l + 64, ... (64 x 16 = BF_DOA_MAX_ANGLES)
constexpr int kPickMax = 16;    // BF_DOA_MAX_PICKS, and the most columns of a column track (BF_MAX_INTERF + 1)
struct DoaPickArgs {
    const double *map;         // [row][n_angles], row = stream x block
    const double *angles;      // [n_angles] degrees
    int32_t *picks;            // [row][k], strongest first, -1 where nothing was picked
    double min_sep, rel_floor;
    long n_rows;
    int n_angles, k;
};

// bf_ctrack_from_picks_device: picks (and maps) of the blocks -> the column track of their frames
struct CtrackFromPicksArgs {
    const int32_t *picks;      // [stream][n_blocks][k]
    const double *map;         // [stream][n_blocks][n_angles]; null: every block with a valid first pick publishes
    int32_t *carry;            // [stream][n_cols]: in, the indices in force in front of block 0; out, those a block n_blocks would get
    int32_t *track;            // [stream][n_blocks * frames_per_block][n_cols]
    double min_peak;
    long n_blocks;
    int n_angles, k, n_cols, frames_per_block, latency;
};

// per hop of x (hops -1 .. n_frames-1, hop -1 = hist) the microphones with a nonzero sample: layout as the stft kernel reads it
hipError_t launch_doa_hop_flags(const float *x, const float *hist, unsigned *flags, long n_frames, long mic_stride, long stream_stride_x,
                                int n_streams, int n_mics, int hop, int layout, hipStream_t s);
hipError_t launch_doa_map(const DoaMapArgs &a, hipStream_t s);
hipError_t launch_doa_reduce(const DoaReduceArgs &a, hipStream_t s);
hipError_t launch_track_from_peaks(const TrackFromPeaksArgs &a, int n_streams, hipStream_t s);
hipError_t launch_doa_pick(const DoaPickArgs &a, hipStream_t s);
hipError_t launch_ctrack_from_picks(const CtrackFromPicksArgs &a, int n_streams, hipStream_t s);

// ---- Capon map (doa_kernels.hip) -----------------------------------------------------------------------------------------------------
struct CaponArgs {
    const f64x2 *Z;            // [stream][frames_ws][NP][N] packed pair spectra, stored halved (only ratios of R enter the map)
    const f64x2 *steer;        // [angle][mic][bin - klo]: consecutive lanes (bins) read consecutive entries
    double *part;              // [segment][stream][blocks_ws][angle]: sum over the segment's bins of c_d(k), lanes added in one fixed tree
    f64x2 *ws;                 // kWorkspace only: [element][problem lane of the grid]
    double delta;              // the diagonal loading
    long frames_ws, blocks_ws, n_blocks;  // blocks of this chunk
    int n_streams, n_mics, nfft, n_angles, klo, n_bins, n_segments, frames_per_block;
    // MUSIC only (launch_music)
    double *epart = nullptr;   // [segment][stream][blocks_ws][mic]: sum over the segment's bins of lambda_i(k), descending
    int n_sources = 0;         // the signal subspace's dimension, 1 .. n_mics - 1
};
// [bin][mic][angle] -> [angle][mic][bin]
hipError_t launch_capon_table(const f64x2 *src, f64x2 *dst, int n_bins, int n_mics, int n_angles, hipStream_t s);
hipError_t launch_capon(const CaponArgs &a, const CaponPlan &p, hipStream_t s);
// MUSIC: part gets sum over the segment's bins of nu_d(k), epart the eigenvalues (p: music_decide's plan)
hipError_t launch_music(const CaponArgs &a, const CaponPlan &p, hipStream_t s);

}  // namespace bf
#endif  // BF_DOA_PLAN_ONLY
