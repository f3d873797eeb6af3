// doa.hpp -- direction-of-arrival maps (bf_doa_*, include/bfcore.h) by three methods, SRP-PHAT, Capon (MVDR) and MUSIC: the launch plan of
// one batch, and the argument blocks and launchers of doa_kernels.hip.  The spectra come from the bin pipeline's forward transform
// (pipeline_kernels.hpp launch_stft, packed microphone pairs, halved).
//
// Every launch decision of a batch is the plain C++ of doa_decide below, which the CPU suite compiles on its own (-DBF_DOA_PLAN_ONLY: no
// HIP header is read in front of the #ifndef).  doa.cpp sizes its scratch and cuts its chunks by the plan alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace bf {

// ---- one pure launch plan per batch ----------------------------------------------------------------------------------------------------
// A batch runs in chunks of whole blocks (frames_per_block frames each).  Per chunk and in-band bin the method's kernel leaves partial
// sums over one segment of the band, which doa_reduce_kernel adds in order.  The segments depend on |K| only, so a sum over the band is
// formed the same way however a stream is cut into calls or chunks.
//   SRP-PHAT       doa_map_kernel: a workgroup per 64 frames x 32 angles x 48-bin segment; partial sums per (segment, stream, frame, angle)
//   Capon, MUSIC   one lane per (stream, block, bin), one wavefront per 64-bin segment of a block: the covariance methods; partial sums per
//                  (segment, stream, block, angle) and, MUSIC only, behind them per (segment, stream, block, eigenvalue slot)
enum DoaMethod : int { kDoaSrpPhat = 0, kDoaCapon = 1, kDoaMusic = 2 };  // BF_DOA_SRP_PHAT, BF_DOA_CAPON, BF_DOA_MUSIC
constexpr int kDoaSegBins = 48;                   // SRP-PHAT: in-band bins of one segment
constexpr int kDoaCovSegBins = 64;                // the covariance methods: a wavefront's lanes
constexpr int kDoaRegMics = 8;                    // the covariance methods: up to here the matrices of a bin live in registers
constexpr size_t kDoaChunkBytes = 256ull << 20;   // spectra, hop flags, partial sums and work space of one chunk (never less than one block)
// Frames of one SRP-PHAT map tile (a workgroup: 4 wavefronts x 4 lane groups x 4 frames) and angles of one tile (16 lanes x 2 angles).
constexpr int kDoaTileFrames = 64, kDoaTileAngles = 32;

enum class DoaPath : int { kRegisters = 0, kWorkspace = 1, kFrameTiles = 2 };

struct DoaShape {
    int n_mics, n_streams, nfft, n_angles, n_bins, frames_per_block;
    long n_frames;  // of the batch: a multiple of frames_per_block
};
struct DoaPlan {
    int method;
    DoaPath path;           // SRP-PHAT: kFrameTiles; the covariance methods: by microphone count alone
    int mp;                 // the kernel's compile-time size.  kRegisters: its row count, 2 x microphone pairs (2, 4, 6, 8); kFrameTiles: the
                            // microphone count where doa_map_kernel has it (2, 4, 8, 16); 0: the count is read at run time
    int seg_bins, segments; // of the band: by the method and |K| alone
    int ws_elems;           // kWorkspace: complex doubles per problem (Capon: the lower triangle of R with its diagonal + the solve's vector;
                            // MUSIC: the triangle, the frame's spectra / the columns' noise weights, the eigenvectors)
    long chunk_blocks;      // blocks of one chunk: what fits the budget, at least one, at most the batch
    long chunk_frames;      // chunk_blocks x frames_per_block
    unsigned grid_x, grid_y, grid_z;  // of a full chunk.  kFrameTiles: (frame tiles x angle tiles, segments, streams), 256 lanes per
                                      // workgroup; otherwise (segments x chunk_blocks, streams, 1), 64 lanes
    size_t z_bytes;         // packed pair spectra of one chunk: [stream][chunk frame][pair][nfft] complex doubles
    size_t flags_bytes;     // SRP-PHAT: [stream][chunk frame + 1][2] unsigned, the hop flags; otherwise 0
    size_t part_bytes;      // partial sums of one chunk, doubles: [segment][stream][chunk frame or block][angle], and for MUSIC
    long epart_offset;      // behind them, epart_offset doubles in, [segment][stream][chunk block][mic]; 0 unless MUSIC
    size_t ws_bytes;        // kWorkspace: [element][stream][chunk block][segment][lane] complex doubles; otherwise 0
    size_t table_bytes;     // the steering table, angles x mics x bins complex doubles (each method's kernel has its layout)
};

inline DoaPlan doa_decide(const DoaShape &c, int method) {
    DoaPlan p{};
    const bool cov = method != kDoaSrpPhat, music = method == kDoaMusic;
    const size_t M = (size_t)c.n_mics, S = (size_t)c.n_streams, NP = (M + 1) / 2, W = (size_t)c.frames_per_block, D = (size_t)c.n_angles;
    p.method = method;
    p.path = !cov ? DoaPath::kFrameTiles : c.n_mics <= kDoaRegMics ? DoaPath::kRegisters : DoaPath::kWorkspace;
    if (cov) p.mp = p.path == DoaPath::kRegisters ? 2 * (int)NP : 0;
    else p.mp = M == 2 || M == 4 || M == 8 || M == 16 ? (int)M : 0;
    p.seg_bins = cov ? kDoaCovSegBins : kDoaSegBins;
    p.segments = (c.n_bins + p.seg_bins - 1) / p.seg_bins;
    if (p.path == DoaPath::kWorkspace) p.ws_elems = (int)(M * (M + 1) / 2 + M + (music ? M * M : 0));
    // one block's share of every buffer; SRP-PHAT keeps a row of partial sums and a pair of hop flags per frame, the others a row per block
    const size_t G = (size_t)p.segments, rows = cov ? 1 : W, cols = D + (music ? M : 0);
    const size_t z_block = W * S * NP * (size_t)c.nfft * 16, part_block = G * S * rows * cols * 8;
    const size_t flags_block = cov ? 0 : W * S * 2 * sizeof(unsigned);
    const size_t ws_block = (size_t)p.ws_elems * S * G * kDoaCovSegBins * 16;
    long nb = (long)(kDoaChunkBytes / (z_block + part_block + flags_block + ws_block));
    const long batch = c.n_frames / c.frames_per_block;
    if (nb < 1) nb = 1;
    if (nb > batch) nb = batch;
    p.chunk_blocks = nb;
    p.chunk_frames = nb * c.frames_per_block;
    if (cov) {
        p.grid_x = (unsigned)(G * (size_t)nb);
        p.grid_y = (unsigned)S;
        p.grid_z = 1;
    } else {
        p.grid_x = (unsigned)(((p.chunk_frames + kDoaTileFrames - 1) / kDoaTileFrames) * ((c.n_angles + kDoaTileAngles - 1) / kDoaTileAngles));
        p.grid_y = (unsigned)G;
        p.grid_z = (unsigned)S;
    }
    p.z_bytes = z_block * (size_t)nb;
    p.flags_bytes = cov ? 0 : S * ((size_t)p.chunk_frames + 1) * 2 * sizeof(unsigned);  // hop -1 in front of the chunk's frames
    p.part_bytes = part_block * (size_t)nb;
    p.epart_offset = music ? (long)(G * S * (size_t)nb * D) : 0;
    p.ws_bytes = ws_block * (size_t)nb;
    p.table_bytes = D * M * (size_t)c.n_bins * 16;
    return p;
}

}  // namespace bf

#ifndef BF_DOA_PLAN_ONLY
#include <hip/hip_runtime.h>

#include <string>

#include "geometry.hpp"

namespace bf {

void set_last_error(const std::string &msg);  // capi.cpp: the text bf_last_error(NULL) returns

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

// bf_ctrack_assign_device: picks (and maps) of the blocks -> a column track in which a column is a talker (the rule: doa_assign.hpp)
struct CtrackAssignArgs {
    const int32_t *picks;      // [stream][n_blocks][k]
    const double *map;         // [stream][n_blocks][n_angles]; null: every block with a valid first pick publishes
    const double *angles;      // [n_angles] degrees, the picker's grid
    int32_t *state;            // [stream][n_cols][4] {idx, hits, misses, out}: in, the slots in front of block 0; out, after the last block
    int32_t *track;            // [stream][n_blocks * frames_per_block][n_cols]
    int32_t *active;           // [stream][n_blocks][n_cols] (nullable)
    double min_peak, gate;
    long n_blocks;
    int n_angles, k, n_cols, frames_per_block, latency, min_hits, max_coast;
};

// per hop of x (hops -1 .. n_frames-1, hop -1 = hist) the microphones with a nonzero sample: layout as the stft kernel reads it
hipError_t launch_doa_hop_flags(const float *x, const float *hist, unsigned *flags, long n_frames, long mic_stride, long stream_stride_x,
                                int n_streams, int n_mics, int hop, int layout, hipStream_t s);
hipError_t launch_doa_map(const DoaMapArgs &a, const DoaPlan &p, hipStream_t s);
hipError_t launch_doa_reduce(const DoaReduceArgs &a, hipStream_t s);
hipError_t launch_track_from_peaks(const TrackFromPeaksArgs &a, int n_streams, hipStream_t s);
hipError_t launch_doa_pick(const DoaPickArgs &a, hipStream_t s);
hipError_t launch_ctrack_from_picks(const CtrackFromPicksArgs &a, int n_streams, hipStream_t s);
hipError_t launch_ctrack_assign(const CtrackAssignArgs &a, int n_streams, hipStream_t s);

// ---- the covariance methods, Capon and MUSIC (doa_kernels.hip) -------------------------------------------------------------------------
struct DoaCovArgs {
    const f64x2 *Z;            // [stream][frames_ws][NP][N] packed pair spectra, stored halved (only ratios of R enter the maps)
    const f64x2 *steer;        // [angle][mic][bin - klo]: consecutive lanes (bins) read consecutive entries
    double *part;              // [segment][stream][blocks_ws][angle]: sum over the segment's bins of c_d(k) (Capon) or nu_d(k) (MUSIC), lanes
                               // added in one fixed tree
    f64x2 *ws;                 // kWorkspace only: [element][problem lane of the grid]
    double delta;              // Capon: the diagonal loading
    long frames_ws, blocks_ws, n_blocks;  // blocks of this chunk
    int n_streams, n_mics, nfft, n_angles, klo, n_bins, n_segments, frames_per_block;
    // MUSIC only
    double *epart = nullptr;   // [segment][stream][blocks_ws][mic]: sum over the segment's bins of lambda_i(k), descending
    int n_sources = 0;         // the signal subspace's dimension, 1 .. n_mics - 1
};
// [bin][mic][angle] -> [angle][mic][bin]
hipError_t launch_doa_cov_table(const f64x2 *src, f64x2 *dst, int n_bins, int n_mics, int n_angles, hipStream_t s);
// the per-bin kernel of p.method (kDoaCapon or kDoaMusic) on the a.n_blocks blocks of one chunk
hipError_t launch_doa_cov(const DoaCovArgs &a, const DoaPlan &p, hipStream_t s);

}  // namespace bf
#endif  // BF_DOA_PLAN_ONLY
