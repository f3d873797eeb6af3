// doa_kernels.hip -- direction-of-arrival maps by SRP-PHAT, Capon and MUSIC (bf_doa_*, include/bfcore.h; DESIGN.md "Direction-of-arrival
// maps"; the launch plan of a batch: doa_decide, doa.hpp).  SRP-PHAT:
//
//   P[s][b][d] = 1 / (W |K| M^2) sum_{t in block b} sum_{k in K} | sum_m conj(w_m(theta_d, k)) X^_{s,m,t}(k) |^2,  X^ = X / |X| (0 at |X| <= eps)
//
// The forward transforms are the bin pipeline's (launch_stft: packed microphone pairs Z = FFT(h a + i h b), stored halved, so that
// X_a = Z[k] + conj Z[N-k] and X_b = -i (Z[k] - conj Z[N-k])).  Three kernels per chunk of frames:
//   doa_hop_flags_kernel  which microphones have a nonzero sample in each hop: a microphone whose windowed frame is exactly zero gets
//                         X^ = 0 exactly (its packed partner's rounding residue never becomes a unit vector)
//   doa_map_kernel        per (frame tile, angle tile, band segment): the per-bin [angles x M] . [M x frames] complex product, |.|^2,
//                         summed over the segment's bins in ascending order -> one partial sum per (segment, stream, frame, angle)
//   doa_reduce_kernel     per (stream, block): segments in order, then the block's frames in order, the scale, and the argmax
// Every sum has one fixed order that depends on the band and W only: map and peak bytes do not depend on how a stream is cut into
// calls or chunks, nor on the launch.  No atomics reach a sum (the hop flags are OR-ed).
//
// The Capon (MVDR) map, the handle's second method (bf_doa_set_method):
//
//   R_{s,b}(k) = sum_{t in block b} X X^H,  tau = trace R,  R~ = R / tau + (delta / M) I,  c_d(k) = M / ((1 + delta) a_d^H R~^-1 a_d)  (0 at tau <= 0)
//   P[s][b][d] = 1 / |K| sum_{k in K} c_d(k)
//
// Two kernels per chunk behind the same forward transforms (no hop flags: there is no PHAT normalisation):
//   doa_capon_kernel      one lane per (stream, block, bin), one wavefront per 64 consecutive bins (a band segment): the covariance over the
//                         block's frames in ascending order, the Cholesky factor R~ = L L^H, and per angle one forward substitution
//                         u = L^-1 a_d, c = M / ((1 + delta) |u|^2); the wavefront's 64 values are added in one fixed butterfly ->
//                         one partial sum per (segment, stream, block, angle).  Up to 8 microphones everything stays in registers
//                         (doa_capon_kernel<MP>); above, the triangle lives in a work space in memory (doa_capon_ws_kernel).
//   doa_reduce_kernel     as above with one "frame" per block: segments in ascending order, the scale 1 / |K|, the argmax
//
// The MUSIC map and the eigenvalue profile, the third method, on the same covariances:
//
//   R / tau = sum_i lambda_i v_i v_i^H (descending),  nu_d(k) = 1 / M sum_{i > n} |v_i^H a_d|^2  (1 at tau <= 0, and lambda = 0)
//   P[s][b][d] = mu / (mu + 1 / |K| sum_{k in K} nu_d(k)),  E[s][b][i] = 1 / |K| sum_{k in K} lambda_i(k)
//
//   doa_music_kernel      doa_capon_kernel's lane and covariance, then doa_eig.hpp's Jacobi sweeps (a fixed count) in registers, the ranks
//                         of the eigenvalues, per angle the products with the noise columns; partial sums per (segment, stream, block,
//                         angle) and per (segment, stream, block, eigenvalue slot).  Above 8 microphones doa_music_ws_kernel, in memory.
//   doa_reduce_kernel     the map (mu / (mu + sum / |K|)) and the peak; a second launch for the profile (the plain mean, no peak)
//
// The four per-bin kernels of the two covariance methods are one skeleton: CovLane (lane -> problem), cov_accumulate (in registers, or in
// the work space through EigMem), and for the register kernels walk_angles (prefetch, butterfly, row stores) around the method's
// per-angle arithmetic.
//
// Behind the maps, without a handle: doa_pick_kernel (bf_doa_pick_device: the k strongest separated peaks of every row) and the two
// track builders, track_from_peaks_kernel and ctrack_from_picks_kernel (one look angle, or one angle per constraint column, per frame),
// and ctrack_assign_kernel (bf_ctrack_assign_device: a column track whose columns are talkers, not loudness ranks).
#include <climits>

#include "doa.hpp"
#include "doa_assign.hpp"
#include "doa_eig.hpp"
#include "doa_pick.hpp"
#include "launch_trace.hpp"

namespace bf {
namespace {

constexpr int kDoaBlock = 256;

__global__ __launch_bounds__(kDoaBlock) void doa_hop_flags_kernel(const float *x, const float *hist, unsigned *flags, long n_frames,
                                                                  long mic_stride, long stream_stride_x, int n_mics, int hop, int layout) {
    __shared__ unsigned sh[2];
    const int tid = threadIdx.x;
    const long h = (long)blockIdx.x - 1;  // hop -1: the carried hop in front of the batch
    const int s = blockIdx.y, M = n_mics, H = hop;
    if (tid < 2) sh[tid] = 0u;
    __syncthreads();
    const float *p;
    long ms;
    if (h < 0) {
        p = hist + (long)s * M * H;  // [mic][hop] (planar) or [hop][mic]
        ms = H;
    } else {
        p = x + (long)s * stream_stride_x + (layout == 0 ? h * H : h * (long)H * M);
        ms = mic_stride;
    }
    unsigned tail = 0u, full = 0u;
    for (int i = tid; i < M * H; i += kDoaBlock) {
        int m, j;
        float v;
        if (layout == 0) {
            m = i / H;
            j = i - m * H;
            v = p[(long)m * ms + j];
        } else {
            j = i / M;
            m = i - j * M;
            v = p[i];
        }
        if (v != 0.f) {
            full |= 1u << m;
            if (j > 0) tail |= 1u << m;
        }
    }
    if (tail) atomicOr(&sh[0], tail);
    if (full) atomicOr(&sh[1], full);
    __syncthreads();
    if (tid < 2) flags[((long)s * (n_frames + 1) + (h + 1)) * 2 + tid] = sh[tid];
}

__device__ __forceinline__ f64x2 phat(double re, double im, double eps, bool live) {
    const double mag = sqrt(re * re + im * im);
    if (!live || !(mag > eps)) return f64x2{0.0, 0.0};
    return f64x2{re / mag, im / mag};
}

// One workgroup: 64 frames (wavefront w, lane group lf = lane / 16: frames 16 w + 4 lf .. + 3) x 32 angles (lane la = lane mod 16: angles
// 2 la, 2 la + 1) x the bins of one band segment.  Per bin the normalised spectra of the tile's frames and the tile's steering column are
// staged in LDS (the next bin's are fetched into registers while this one is multiplied): every steering element is read from memory
// once per 64 frames, every spectrum element once per 32 angles.  MT: microphones known at compile time (0 = run-time count, <= 32).
template <int MT>
__global__ __launch_bounds__(kDoaBlock) void doa_map_kernel(DoaMapArgs a) {
    constexpr int MX = MT ? MT : 32, NPX = (MX + 1) / 2;
    constexpr int kItems = (kDoaTileFrames * NPX + kDoaBlock - 1) / kDoaBlock;
    constexpr int kWItems = (MX * kDoaTileAngles + kDoaBlock - 1) / kDoaBlock;
    constexpr int kUnrollM = MT ? MT : 4;
    constexpr int XS = MX + 1;  // row of one frame in LDS (padded: the four lane groups read rows in different banks)
    __shared__ f64x2 xs[kDoaTileFrames * XS];
    __shared__ f64x2 ws[MX * kDoaTileAngles];
    const int M = MT ? MT : a.n_mics, NP = (M + 1) / 2, N = a.nfft, D = a.n_angles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, la = lane & 15, lf = lane >> 4;
    const int n_at = (D + kDoaTileAngles - 1) / kDoaTileAngles;
    const int at = blockIdx.x % n_at, ft = blockIdx.x / n_at;  // angle tiles fastest: workgroups on the same frames run side by side (L2)
    const int g = blockIdx.y, s = blockIdx.z;
    const long t0 = (long)ft * kDoaTileFrames;
    const int d0 = at * kDoaTileAngles;
    const int kk0 = g * kDoaSegBins, kk1 = min(kk0 + kDoaSegBins, a.n_bins);
    const long FW = a.frames_ws, n = a.n_frames;

    // staging items: (frame f, pair p) of the spectra, (mic m, angle al) of the steering column
    unsigned fm[kItems];  // microphones whose windowed frame is not exactly zero
    f64x2 za[kItems], zb[kItems], wv[kWItems];
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const int idx = tid + kDoaBlock * j;
        fm[j] = 0u;
        za[j] = zb[j] = f64x2{0.0, 0.0};
        if (idx < kDoaTileFrames * NP) {
            const long t = t0 + idx / NP;
            if (t < n) {
                const unsigned *fl = a.flags + ((long)s * (n + 1) + t) * 2;  // hop t-1 (sample 0 carries window 0) and hop t
                fm[j] = fl[0] | fl[3];
            }
        }
    }
    auto fetch = [&](int kk) {
        const int k = a.klo + kk;
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int idx = tid + kDoaBlock * j;
            if (idx < kDoaTileFrames * NP && fm[j]) {
                const long t = t0 + idx / NP;
                const int p = idx % NP;
                const f64x2 *zr = a.Z + (((long)s * FW + t) * NP + p) * N;
                za[j] = zr[k];
                zb[j] = zr[N - k];
            }
        }
#pragma unroll
        for (int j = 0; j < kWItems; ++j) {
            const int idx = tid + kDoaBlock * j;
            if (idx < M * kDoaTileAngles) {
                const int m = idx / kDoaTileAngles, d = min(d0 + idx % kDoaTileAngles, D - 1);
                wv[j] = a.steer[((long)kk * M + m) * D + d];
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const int idx = tid + kDoaBlock * j;
            if (idx < kDoaTileFrames * NP) {
                const int f = idx / NP, p = idx % NP, ma = 2 * p, mb = 2 * p + 1;
                // halved packed pair: X_a = Z[k] + conj Z[N-k], X_b = -i (Z[k] - conj Z[N-k])
                xs[f * XS + ma] = phat(za[j].x + zb[j].x, za[j].y - zb[j].y, a.eps, (fm[j] >> ma) & 1u);
                if (mb < M) xs[f * XS + mb] = phat(za[j].y + zb[j].y, zb[j].x - za[j].x, a.eps, (fm[j] >> mb) & 1u);
            }
        }
#pragma unroll
        for (int j = 0; j < kWItems; ++j) {
            const int idx = tid + kDoaBlock * j;
            if (idx < M * kDoaTileAngles) ws[idx] = wv[j];
        }
    };

    const int fb = wave * 16 + lf * 4;  // first of this lane's four frames in the tile
    double pw[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) pw[j][i] = 0.0;
    fetch(kk0);
    for (int kk = kk0; kk < kk1; ++kk) {
        stage();
        __syncthreads();
        if (kk + 1 < kk1) fetch(kk + 1);
        double yr[2][4], yi[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) yr[j][i] = yi[j][i] = 0.0;
#pragma unroll kUnrollM
        for (int m = 0; m < M; ++m) {
            const f64x2 w0 = ws[m * kDoaTileAngles + 2 * la], w1 = ws[m * kDoaTileAngles + 2 * la + 1];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f64x2 x = xs[(fb + i) * XS + m];
                // conj(w) x = (wr xr + wi xi) + i (wr xi - wi xr)
                yr[0][i] = fma(w0.x, x.x, yr[0][i]);
                yr[0][i] = fma(w0.y, x.y, yr[0][i]);
                yi[0][i] = fma(w0.x, x.y, yi[0][i]);
                yi[0][i] = fma(-w0.y, x.x, yi[0][i]);
                yr[1][i] = fma(w1.x, x.x, yr[1][i]);
                yr[1][i] = fma(w1.y, x.y, yr[1][i]);
                yi[1][i] = fma(w1.x, x.y, yi[1][i]);
                yi[1][i] = fma(-w1.y, x.x, yi[1][i]);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) pw[j][i] = fma(yi[j][i], yi[j][i], fma(yr[j][i], yr[j][i], pw[j][i]));
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long t = t0 + fb + i;
        if (t >= n) continue;
        double *row = a.part + (((long)g * a.n_streams + s) * FW + t) * D;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int d = d0 + 2 * la + j;
            if (d < D) row[d] = pw[j][i];
        }
    }
}

// One workgroup per (stream, block): P = scale * sum_{t in block} (sum_g part[g][t]) in that order, then the lowest index of the maximum.
// MUSIC (mu > 0): P = mu / (mu + sum / denom), a division so that |K| ones give exactly mu / (mu + 1).
__global__ __launch_bounds__(kDoaBlock) void doa_reduce_kernel(DoaReduceArgs a) {
    __shared__ double bv[kDoaBlock];
    __shared__ int bi[kDoaBlock];
    const int tid = threadIdx.x, s = blockIdx.y, D = a.n_angles, W = a.frames_per_block;
    const long b = blockIdx.x;
    double best = -1.0;
    int besti = INT_MAX;
    for (int d = tid; d < D; d += kDoaBlock) {
        double acc = 0.0;
        for (int tt = 0; tt < W; ++tt) {
            const long t = b * W + tt;
            double v = 0.0;
            for (int g = 0; g < a.n_segments; ++g) v += a.part[(((long)g * a.n_streams + s) * a.frames_ws + t) * D + d];
            acc += v;
        }
        const double val = a.mu > 0.0 ? a.mu / (a.mu + acc / a.denom) : acc * a.scale;
        if (a.map) a.map[((long)s * a.map_blocks + a.block0 + b) * D + d] = val;
        if (val > best) {  // ascending d per thread: the first maximum is kept
            best = val;
            besti = d;
        }
    }
    if (!a.peak) return;
    bv[tid] = best;
    bi[tid] = besti;
    __syncthreads();
    for (int w = kDoaBlock / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const double v2 = bv[tid + w];
            const int i2 = bi[tid + w];
            if (v2 > bv[tid] || (v2 == bv[tid] && i2 < bi[tid])) {
                bv[tid] = v2;
                bi[tid] = i2;
            }
        }
        __syncthreads();
    }
    if (tid == 0) a.peak[(long)s * a.map_blocks + a.block0 + b] = bi[0];
}

// One wavefront per stream walks the blocks, 64 at a time.  V(k) = the index published by the latest block <= k that published (a block
// publishes its peak when the map value there is not below min_peak), the carry where there is none; the frames of block b get
// V(b - latency).  Lane l of a round holds k = k0 + l: the published lanes as a ballot, the latest one at or below l through one shuffle.
__global__ __launch_bounds__(64) void track_from_peaks_kernel(TrackFromPeaksArgs a) {
    const int lane = threadIdx.x, W = a.frames_per_block, L = a.latency;
    const long s = blockIdx.x, nb = a.n_blocks;
    const int *peak = a.peak + s * nb;
    const double *map = a.map ? a.map + s * nb * a.n_angles : nullptr;
    int *trk = a.track + s * nb * W;
    const int c_in = a.carry[s];
    // blocks 0 .. latency-1: no block of this call is old enough
    const long n_head = (L < nb ? (long)L : nb) * W;
    for (long i = lane; i < n_head; i += 64) trk[i] = c_in;
    const long klast = nb - L < nb - 1 ? nb - L : nb - 1;  // V(klast) is what a block n_blocks would get
    int cur = c_in;                                        // V(k0 - 1)
    for (long k0 = 0; k0 <= klast; k0 += 64) {
        const long k = k0 + lane;
        int p = 0;
        bool pub = false;
        if (k <= klast) {
            p = peak[k];
            if (map == nullptr) pub = true;
            else if (p >= 0 && p < a.n_angles) pub = !(map[k * a.n_angles + p] < a.min_peak);
        }
        const unsigned long long m = __ballot(pub);
        const unsigned long long below = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
        const int src = below ? 63 - __clzll((long long)below) : 0;
        const int got = __shfl(p, src, 64);
        const int v = below ? got : cur;
        for (long i = lane; i < 64L * W; i += 64) {  // the frames of blocks k0 + latency ..., consecutive lanes on consecutive frames
            const int bl = (int)(i / W);
            const int vv = __shfl(v, bl, 64);
            const long kk = k0 + bl;
            if (kk <= klast && kk + L < nb) trk[(kk + L) * W + (i - (long)bl * W)] = vv;
        }
        cur = __shfl(v, 63, 64);  // lanes past klast publish nothing: V(klast) at the end
    }
    if (lane == 0) a.carry[s] = cur;
}

// One wavefront per map row (a stream's block).  Lane l keeps the values and the angles l, l + 64, ... in registers (kPickSlots of each)
// and one bit per slot: "still free".  A pick: the lane's best free value (ascending slots, so the lane's lowest index wins its ties),
// a butterfly over (value, index) that prefers the lower index on equal values, the winner's angle through one shuffle, then every
// lane takes its angles within min_sep of it out of the running (doa_pick.hpp).  Lane j remembers pick j: one row of stores at the end.
// No LDS, no atomics; rows do not see each other, so the bytes cannot depend on the launch.  A NaN never compares as larger, so it can
// only be picked where nothing else is free: the loop still ends after k rounds and writes indices of the row or -1.
__global__ __launch_bounds__(64) void doa_pick_kernel(DoaPickArgs a) {
    const int lane = threadIdx.x, D = a.n_angles, K = a.k;
    for (long r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const double *row = a.map + r * D;
        double v[kPickSlots], ang[kPickSlots];
        unsigned free_mask = 0u;
        double top = -INFINITY;  // the row's maximum
#pragma unroll
        for (int j = 0; j < kPickSlots; ++j) {
            const int i = lane + 64 * j;
            const bool in = i < D;
            v[j] = in ? row[i] : 0.0;
            ang[j] = in ? a.angles[i] : 0.0;
            if (in) {
                free_mask |= 1u << j;
                if (v[j] > top) top = v[j];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double t = __shfl_xor(top, o, 64);
            if (t > top) top = t;
        }
        const double floor_v = a.rel_floor * top;
        int mine = -1;
        for (int n = 0; n < K; ++n) {
            double bv = 0.0, ba = 0.0;
            int bi = INT_MAX;  // nothing free in this lane
#pragma unroll
            for (int j = 0; j < kPickSlots; ++j)
                if (((free_mask >> j) & 1u) && (bi == INT_MAX || v[j] > bv)) {
                    bv = v[j];
                    ba = ang[j];
                    bi = lane + 64 * j;
                }
            double wv = bv;
            int wi = bi;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(wv, o, 64);
                const int oi = __shfl_xor(wi, o, 64);
                if (oi != INT_MAX && (wi == INT_MAX || ov > wv || (ov == wv && oi < wi))) {
                    wv = ov;
                    wi = oi;
                }
            }
            // every lane follows lane 0 (without a NaN all lanes hold the same winner anyway)
            const int d = __shfl(wi, 0, 64);
            const double dv = __shfl(wv, 0, 64);
            if (d == INT_MAX || dv < floor_v) break;
            const double da = __shfl(ba, d & 63, 64);  // the owner's best is the winner
            if (lane == n) mine = d;
#pragma unroll
            for (int j = 0; j < kPickSlots; ++j)
                if (((free_mask >> j) & 1u) && (lane + 64 * j == d || !pick_stays_free(ang[j], da, a.min_sep))) free_mask &= ~(1u << j);
        }
        if (lane < K) a.picks[r * K + lane] = mine;
    }
}

// track_from_peaks_kernel with a column dimension.  One wavefront per stream walks the blocks, 64 at a time; lane l of a round holds
// block k = k0 + l.  A block publishes when its first pick is an index of the map whose value is not below min_peak; a publishing block
// updates column c < min(n_cols, k) when pick c is an index of the map.  V_c(k) = column c's latest update by a block <= k, the carry
// where there is none: per column a ballot of the updating lanes, the latest one at or below l through one shuffle.  The round's
// [block][column] values go through LDS so that the frames of blocks k0 + latency ... leave as [frame][column] rows, consecutive lanes
// on consecutive int32s.  Lane c keeps V_c(k0 - 1) between the rounds.  A pick or a carry is copied, never used as an index, but for
// the look-up of a first pick that has been checked against the map.
__global__ __launch_bounds__(64) void ctrack_from_picks_kernel(CtrackFromPicksArgs a) {
    __shared__ int vs[64 * kPickMax];  // [block of the round][column]
    const int lane = threadIdx.x, W = a.frames_per_block, L = a.latency, C = a.n_cols, K = a.k, A = a.n_angles;
    const long s = blockIdx.x, nb = a.n_blocks, WC = (long)W * C;
    const int *picks = a.picks + s * nb * K;
    const double *map = a.map ? a.map + s * nb * A : nullptr;
    int *trk = a.track + s * nb * WC;
    int *carry = a.carry + s * C;
    int cur = lane < C ? carry[lane] : -1;  // lane c: V_c(k0 - 1)
    // blocks 0 .. latency-1: no block of this call is old enough
    const long n_head = (L < nb ? (long)L : nb) * WC;
    for (long i0 = 0; i0 < n_head; i0 += 64) {  // every lane takes part in the shuffle, also in a short last round
        const long i = i0 + lane;
        const int c_in = __shfl(cur, (int)(i % C), 64);
        if (i < n_head) trk[i] = c_in;
    }
    const long klast = nb - L < nb - 1 ? nb - L : nb - 1;  // V(klast) is what a block n_blocks would get
    // element i of a round's output and its successor i + 64, without a division per element (WC is a multiple of C)
    const int q64 = (int)(64 / WC), r64 = (int)(64 % WC), c64 = 64 % C;
    const int bl0 = (int)(lane / WC), c0 = lane % C;
    const long rem0 = lane - bl0 * WC;
    for (long k0 = 0; k0 <= klast; k0 += 64) {
        const long k = k0 + lane;
        const bool live = k <= klast;
        bool pub = false;
        if (live) {
            const int p0 = picks[k * K];
            if (p0 >= 0 && p0 < A) pub = map == nullptr || !(map[k * A + p0] < a.min_peak);
        }
        for (int c = 0; c < C; ++c) {
            int p = -1;
            if (pub && c < K) p = picks[k * K + c];
            const bool upd = p >= 0 && p < A;
            const unsigned long long m = __ballot(upd);
            const unsigned long long below = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
            const int src = below ? 63 - __clzll((long long)below) : 0;
            const int got = __shfl(p, src, 64);
            const int before = __shfl(cur, c, 64);
            const int v = below ? got : before;
            vs[lane * C + c] = v;
            const int last = __shfl(v, 63, 64);  // lanes past klast update nothing: V_c(klast) at the end
            if (lane == c) cur = last;
        }
        __syncthreads();
        int bl = bl0, c = c0;
        long rem = rem0;
        for (long i = lane; i < 64 * WC; i += 64) {  // the frames of blocks k0 + latency ..., [frame][column]: i = bl * WC + rem, c = i mod C
            const long kk = k0 + bl;
            if (kk <= klast && kk + L < nb) trk[(kk + L) * WC + rem] = vs[bl * C + c];
            bl += q64;
            rem += r64;
            if (rem >= WC) {
                rem -= WC;
                ++bl;
            }
            c += c64;
            if (c >= C) c -= C;
        }
        __syncthreads();
    }
    if (lane < C) carry[lane] = cur;
}

// bf_ctrack_assign_device: a column is a talker.  The rule is doa_assign.hpp's assign_block, block after block; here one wavefront serves
// one stream and does a block's steps side by side.  Lane l = 16 g + c:
//   slots       every lane keeps slot c = l & 15 {idx, hits, misses, out} and the angle of idx in registers, the four lane groups g as
//               four identical copies: every decision below is wavefront-uniform, so the copies never part and no slot is broadcast.
//   loads       a round is four blocks: lane l asks for pick c of block 4 r + g, and behind it for that pick's angle and, for the
//               publishing rule, the map value there.  The picks are requested two rounds (eight blocks) ahead and the gathers one
//               round ahead of their use: the chain picks -> angles[pick] -> match waits only for loads issued four blocks earlier.
//               Every address is clamped into its buffer first: an invalid pick is a candidate of no block and the index of no load.
//   distances   the 16 x 16 (slot, candidate) matrix is four entries per lane, slot c against candidates g, g + 4, g + 8, g + 12,
//               formed once per block with pick_sep; an entry outside the gate, of a free slot or of no candidate is +infinity.
//   match       per greedy round the lane's least entry (ascending j, strict <), then a butterfly over the key (d, 16 c + j): the least
//               d, then the lowest slot, then the lowest candidate.  Keys of real pairs are distinct and no d is a NaN; the steps whose
//               partner lanes cannot hold a pair (slots >= n_cols, candidates >= k) are left out, lane 0 holds the winner and every
//               lane takes it from there.  At most 16 rounds; the rounds end when the live slots or the candidates run out.
//   births      the unmatched candidates and the free slots are two 16-bit masks of ballots; the lowest bits pair off.
//   track       block b's `out` goes to the frames of block b + latency as [frame][column] rows, consecutive lanes on consecutive
//               int32s, lane i taking column i mod n_cols from the lane that holds it.
// Registers only: no LDS, no atomics, vector stores, and nothing shared between streams, so the bytes cannot depend on the launch.
constexpr int kAssignNone = 0x7fff;  // the key of "no pair"

// lane `l`'s value in every lane; l is the same in every lane
__device__ __forceinline__ double wave_read_lane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ __launch_bounds__(64) void ctrack_assign_kernel(CtrackAssignArgs a) {
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int W = a.frames_per_block, L = a.latency, C = a.n_cols, K = a.k, A = a.n_angles;
    const long s = blockIdx.x, nb = a.n_blocks, WC = (long)W * C;
    const int *__restrict__ picks = a.picks + s * nb * K;
    const double *__restrict__ map = a.map ? a.map + s * nb * A : nullptr;
    const double *__restrict__ angles = a.angles;
    int *__restrict__ trk = a.track + s * nb * WC;
    int *__restrict__ act = a.active ? a.active + s * nb * C : nullptr;
    int *__restrict__ state = a.state + s * C * kAssignStateInts;
    const int KG = K < 4 ? K : 4;  // lane groups that hold a candidate
    const bool in = c < C;  // lanes of the slots past n_cols hold a free slot that nothing is born into
    int idx = -1, hits = 0, misses = 0, out = -1;
    if (in) {
        idx = state[c * kAssignStateInts];
        hits = state[c * kAssignStateInts + 1];
        misses = state[c * kAssignStateInts + 2];
        out = state[c * kAssignStateInts + 3];
    }
    double sang = angles[idx >= 0 && idx < A ? idx : 0];  // of use while the slot is live
    // blocks 0 .. latency-1: no block of this call is old enough, they get `out` as it came in
    const int c_lane = lane % C, c64 = 64 % C;
    const long n_head = (L < nb ? (long)L : nb) * WC;
    {
        int cc = c_lane;
        for (long i0 = 0; i0 < n_head; i0 += 64) {  // every lane takes part in the shuffle, also in a short last round
            const int v = __shfl(out, cc, 64);
            if (i0 + lane < n_head) trk[i0 + lane] = v;
            cc += c64;
            if (cc >= C) cc -= C;
        }
    }
    // this lane's requests of round r: pick c of block 4 r + g, then the angle and the map value at that pick.  The addresses are
    // clamped and the loads unconditional; what a lane past n_blocks or k has read is set to -1 where the round is used, not here, so
    // that no load has to be waited for where it is issued.
    const int jc = c < K ? c : K - 1;
    auto block_of = [&](long r) { return 4 * r + g < nb ? 4 * r + g : nb - 1; };
    auto mine = [&](long r, int p) { return 4 * r + g < nb && c < K ? p : -1; };
    auto load_pick = [&](long r) { return picks[block_of(r) * K + jc]; };
    auto gather = [&](long r, int p, double &ang, double &mv) {
        p = mine(r, p);
        const int pi = p >= 0 && p < A ? p : 0;
        ang = angles[pi];
        mv = map ? map[block_of(r) * A + pi] : 0.0;
    };
    const long n_rounds = (nb + 3) / 4;
    int p_nxt = load_pick(0), p_far = load_pick(1);
    double ang_nxt, mv_nxt;
    gather(0, p_nxt, ang_nxt, mv_nxt);
    // Round 0's values are waited for here, once, rather than inside the loop: the compiler drains every outstanding load in front of a
    // loop of stores that reads a register a load is still on its way to, and it would do so in every round (vmcnt(0), expcnt and
    // lgkmcnt left alone).
    __builtin_amdgcn_s_waitcnt(0x0f70);
    for (long r = 0; r < n_rounds; ++r) {
        // what was asked for a round ago is taken over here, in front of this round's requests: the block loop below then uses no
        // register that a load is still on its way to
        const int p_cur = mine(r, p_nxt);
        const double ang_cur = ang_nxt, mv_cur = mv_nxt;
        p_nxt = p_far;
        p_far = load_pick(r + 2);
        gather(r + 1, p_nxt, ang_nxt, mv_nxt);
        const bool p_ok = p_cur >= 0 && p_cur < A;
        const unsigned long long ok_mask = __ballot(p_ok);
        for (int q = 0; q < 4; ++q) {
            const long b = 4 * r + q;
            if (b >= nb) break;
            const int base = 16 * q;
            // 1. candidates: a bit per valid pick of a publishing block
            const int p0 = __builtin_amdgcn_readlane(p_cur, base);
            const double mv0 = wave_read_lane(mv_cur, base);
            const bool pub = p0 >= 0 && p0 < A && (map == nullptr || !(mv0 < a.min_peak));
            unsigned cm = pub ? (unsigned)((ok_mask >> base) & 0xffffull) : 0u;
            const bool live0 = in && idx >= 0 && idx < A;
            const unsigned lm = (unsigned)(__ballot(live0) & 0xffffull);
            unsigned hit = 0u;  // slots matched or born in this block
            // 2. and 3. match
            if (cm != 0u && lm != 0u) {
                double d[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    d[i] = INFINITY;
                    if ((cm >> (4 * i)) == 0u) continue;  // no candidate from 4 i on, in any lane
                    const int j = g + 4 * i;
                    const double aj = __shfl(ang_cur, base + j, 64);
                    const double dd = pick_sep(sang, aj);
                    if (live0 && ((cm >> j) & 1u) && dd <= a.gate) d[i] = dd;
                }
                unsigned mc = 0u;  // candidates matched
                while ((lm & ~hit) != 0u && (cm & ~mc) != 0u) {  // a live slot and a candidate are still without a partner
                    double bd = INFINITY;
                    int bk = kAssignNone;
                    if (!((hit >> c) & 1u)) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int j = g + 4 * i;
                            if (!((mc >> j) & 1u) && d[i] < bd) {
                                bd = d[i];
                                bk = 16 * c + j;
                            }
                        }
                    }
                    // the butterfly, without the steps whose partner lanes hold no pair: slots >= n_cols (lane bits 0 .. 3), candidates >= k
                    // (lane bits 4 and 5).  Lane 0 ends with the least key of all lanes, and every lane follows lane 0.
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        if (o >= 16 ? (o >> 4) >= KG : o >= C) continue;
                        const double od = __shfl_xor(bd, o, 64);
                        const int ok = __shfl_xor(bk, o, 64);
                        if (od < bd || (od == bd && ok < bk)) {
                            bd = od;
                            bk = ok;
                        }
                    }
                    bk = __builtin_amdgcn_readfirstlane(bk);
                    if (bk == kAssignNone) break;
                    const int cw = bk >> 4, jw = bk & 15;
                    const int pw = __builtin_amdgcn_readlane(p_cur, base + jw);
                    const double aw = wave_read_lane(ang_cur, base + jw);
                    if (c == cw) {
                        idx = pw;
                        sang = aw;
                        hits = assign_count_up(hits);
                        misses = 0;
                    }
                    hit |= 1u << cw;
                    mc |= 1u << jw;
                }
                cm &= ~mc;
            }
            // 4. an unmatched live slot is freed or coasts
            if (live0 && !((hit >> c) & 1u)) {
                if (hits < a.min_hits) idx = -1;
                else {
                    misses = assign_count_up(misses);
                    if (misses > a.max_coast) idx = -1;
                }
            }
            // 5. births: the lowest unmatched candidate into the lowest free slot
            unsigned fm = (unsigned)(__ballot(in && !(idx >= 0 && idx < A)) & 0xffffull);
            while (cm != 0u && fm != 0u) {
                const int jw = __ffs(cm) - 1, cw = __ffs(fm) - 1;
                const int pw = __builtin_amdgcn_readlane(p_cur, base + jw);
                const double aw = wave_read_lane(ang_cur, base + jw);
                if (c == cw) {
                    idx = pw;
                    sang = aw;
                    hits = 1;
                    misses = 0;
                }
                hit |= 1u << cw;
                cm &= cm - 1u;
                fm &= fm - 1u;
            }
            // 6. out and active
            const bool confirmed = in && idx >= 0 && idx < A && hits >= a.min_hits;
            if (confirmed) out = idx;
            if (act != nullptr && lane < C) act[b * C + lane] = confirmed && ((hit >> c) & 1u) ? 1 : 0;
            // 7. the frames of block b + latency
            if (b + L < nb) {
                int *dst = trk + (b + L) * WC;
                int cc = c_lane;
                for (long i0 = 0; i0 < WC; i0 += 64) {
                    const int v = __shfl(out, cc, 64);
                    if (i0 + lane < WC) dst[i0 + lane] = v;
                    cc += c64;
                    if (cc >= C) cc -= C;
                }
            }
        }
    }
    if (lane < C) {
        state[lane * kAssignStateInts] = idx;
        state[lane * kAssignStateInts + 1] = hits;
        state[lane * kAssignStateInts + 2] = misses;
        state[lane * kAssignStateInts + 3] = out;
    }
}

// ---- the covariance methods: Capon and MUSIC ------------------------------------------------------------------------------------------
// The sum of a wavefront's 64 values: a butterfly, so every lane forms the same six sums in the same order whatever the launch.
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// microphone m's spectrum out of its pair's packed rows: X_a = Z[k] + conj Z[N-k], X_b = -i (Z[k] - conj Z[N-k])
__device__ __forceinline__ f64x2 unpack_mic(const f64x2 z, const f64x2 c, bool second) {
    return second ? f64x2{z.y + c.y, c.x - z.x} : f64x2{z.x + c.x, z.y - c.y};
}

__global__ __launch_bounds__(kDoaBlock) void capon_table_kernel(const f64x2 *src, f64x2 *dst, int n_bins, int n_mics, int n_angles) {
    const long n = (long)n_bins * n_mics * n_angles;
    for (long i = (long)blockIdx.x * kDoaBlock + threadIdx.x; i < n; i += (long)gridDim.x * kDoaBlock) {
        const int kk = (int)(i % n_bins);
        const long r = i / n_bins;  // d * M + m
        const int m = (int)(r % n_mics), d = (int)(r / n_mics);
        dst[i] = src[((long)kk * n_mics + m) * n_angles + d];
    }
}

// What the four per-bin kernels share.  One lane per (stream, block, in-band bin) problem, one wavefront per segment of a block: 64
// consecutive bins.  In the band's last segment the lanes past the band work on its last bin and add 0 (live).
struct CovLane {
    long b;           // block of the chunk
    int g, s;         // segment of the band, stream
    int kk, k;        // bin of the band, of the transform
    bool live;
    const f64x2 *zr;  // the block's first frame: [frame][pair][N] packed pair rows
    __device__ __forceinline__ CovLane(const DoaCovArgs &a, int NP) {
        const int G = a.n_segments;
        b = blockIdx.x / G;
        g = (int)(blockIdx.x - b * G);
        s = blockIdx.y;
        kk = g * kDoaCovSegBins + (int)threadIdx.x;
        live = kk < a.n_bins;
        if (!live) kk = a.n_bins - 1;
        k = a.klo + kk;
        zr = a.Z + ((long)s * a.frames_ws + b * a.frames_per_block) * NP * a.nfft;
    }
    // the wavefront's row of partial sums, `cols` doubles: [segment][stream][blocks_ws][cols]
    __device__ __forceinline__ double *sums(const DoaCovArgs &a, double *part, int cols) const {
        return part + (((long)g * a.n_streams + s) * a.blocks_ws + b) * cols;
    }
};

// The store of the register kernels (up to 8 microphones): the strict lower triangle, the real diagonal and, for MUSIC, V as plain arrays.
// doa_eig.hpp indexes them with constants only, so they are registers: 64 + 128 doubles at MP = 8 (DESIGN.md has the compiler's
// resource report).
template <int MP>
struct EigRegs {
    static constexpr int NT = MP * (MP - 1) / 2;
    double Rr[NT], Ri[NT], Rd[MP], Vr[MP * MP], Vi[MP * MP];
    __device__ __forceinline__ double diag(int i) const { return Rd[i]; }
    __device__ __forceinline__ void set_diag(int i, double v) { Rd[i] = v; }
    __device__ __forceinline__ EigC low(int i, int c) const { return EigC{Rr[i * (i - 1) / 2 + c], Ri[i * (i - 1) / 2 + c]}; }
    __device__ __forceinline__ void set_low(int i, int c, EigC z) {
        Rr[i * (i - 1) / 2 + c] = z.re;
        Ri[i * (i - 1) / 2 + c] = z.im;
    }
    __device__ __forceinline__ EigC vec(int r, int c) const { return EigC{Vr[r * MP + c], Vi[r * MP + c]}; }
    __device__ __forceinline__ void set_vec(int r, int c, EigC z) {
        Vr[r * MP + c] = z.re;
        Vi[r * MP + c] = z.im;
    }
};

// The store of the work-space kernels (more than 8 microphones): the same per-lane algorithms in memory, [element][lane of the grid], so
// consecutive lanes touch consecutive addresses.  Elements: the lower triangle with its diagonal (idx(i, c) = i (i + 1) / 2 + c); at
// NT + i the frame's spectra, later the solve's vector (Capon) or per column (noise weight, rank) (MUSIC); MUSIC's eigenvectors V_rc at
// NT + M + r M + c.  Correct, not tuned.
struct EigMem {
    f64x2 *A;
    long stride;
    int M, NT;
    __device__ __forceinline__ explicit EigMem(const DoaCovArgs &a)
        : A(a.ws + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 64 + threadIdx.x), stride((long)gridDim.y * gridDim.x * 64), M(a.n_mics),
          NT(a.n_mics * (a.n_mics + 1) / 2) {}
    __device__ __forceinline__ f64x2 &at(int e) const { return A[(long)e * stride]; }
    __device__ __forceinline__ double diag(int i) const { return at(i * (i + 1) / 2 + i).x; }
    __device__ __forceinline__ void set_diag(int i, double v) { at(i * (i + 1) / 2 + i).x = v; }
    __device__ __forceinline__ EigC low(int i, int c) const {
        const f64x2 z = at(i * (i + 1) / 2 + c);
        return EigC{z.x, z.y};
    }
    __device__ __forceinline__ void set_low(int i, int c, EigC z) { at(i * (i + 1) / 2 + c) = f64x2{z.re, z.im}; }
    __device__ __forceinline__ EigC vec(int r, int c) const {
        const f64x2 z = at(NT + M + r * M + c);
        return EigC{z.x, z.y};
    }
    __device__ __forceinline__ void set_vec(int r, int c, EigC z) { at(NT + M + r * M + c) = f64x2{z.re, z.im}; }
};

// R = sum over the block's W frames (ascending) of X X^H for one bin: the strict lower triangle and the real diagonal, in registers.
// zr: the block's first frame, [frame][pair][N] packed pair rows.  A zero partner channel (an odd count's last pair) is never formed.
template <int MP, int NTA>
__device__ __forceinline__ void cov_accumulate(const f64x2 *zr, int k, int N, int M, int W, double (&Rr)[NTA], double (&Ri)[NTA],
                                               double (&Rd)[MP]) {
    constexpr int NT = MP * (MP - 1) / 2, NP = MP / 2;
#pragma unroll
    for (int e = 0; e < NT; ++e) Rr[e] = Ri[e] = 0.0;
#pragma unroll
    for (int i = 0; i < MP; ++i) Rd[i] = 0.0;
    for (int t = 0; t < W; ++t, zr += (long)NP * N) {
        double xr[MP], xi[MP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const f64x2 z = zr[(long)p * N + k], c = zr[(long)p * N + (N - k)];
            xr[2 * p] = z.x + c.x;
            xi[2 * p] = z.y - c.y;
            const bool has = 2 * p + 1 < M;
            xr[2 * p + 1] = has ? z.y + c.y : 0.0;
            xi[2 * p + 1] = has ? c.x - z.x : 0.0;
        }
#pragma unroll
        for (int i = 0; i < MP; ++i) {
#pragma unroll
            for (int c = 0; c < i; ++c) {  // R_ic += x_i conj(x_c)
                const int e = i * (i - 1) / 2 + c;
                Rr[e] = fma(xi[i], xi[c], fma(xr[i], xr[c], Rr[e]));
                Ri[e] = fma(-xr[i], xi[c], fma(xi[i], xr[c], Ri[e]));
            }
            Rd[i] = fma(xi[i], xi[i], fma(xr[i], xr[i], Rd[i]));
        }
    }
}

// The same sum in the work space: the triangle with its diagonal, the frame's spectra parked at NT + m.
__device__ __forceinline__ void cov_accumulate(const EigMem &e, const f64x2 *zr, int k, int N, int W) {
    const int M = e.M, NP = (M + 1) / 2, NT = e.NT;
    for (int t = 0; t < NT; ++t) e.at(t) = f64x2{0.0, 0.0};
    for (int t = 0; t < W; ++t, zr += (long)NP * N) {
        for (int m = 0; m < M; ++m) {  // never the zero partner of an odd count: m < M
            const f64x2 *pr = zr + (long)(m >> 1) * N;
            e.at(NT + m) = unpack_mic(pr[k], pr[N - k], m & 1);
        }
        for (int i = 0; i < M; ++i) {
            const f64x2 x = e.at(NT + i);
            for (int c = 0; c < i; ++c) {
                const f64x2 y = e.at(NT + c);
                f64x2 &r = e.at(i * (i + 1) / 2 + c);
                r = f64x2{fma(x.y, y.y, fma(x.x, y.x, r.x)), fma(-x.x, y.y, fma(x.y, y.x, r.y))};
            }
            f64x2 &r = e.at(i * (i + 1) / 2 + i);
            r.x = fma(x.y, x.y, fma(x.x, x.x, r.x));
        }
    }
}

// The register kernels' walk over the angles.  The next angle's steering column is requested in front of this angle's arithmetic;
// value(ur, ui) gives the lane's value for the column in (ur, ui), which it may overwrite; the wavefront's 64 values are added in the one
// butterfly, lane d mod 64 keeps angle d's sum, and 64 angles' sums leave in one row of stores.
template <int MP, class Value>
__device__ __forceinline__ void walk_angles(const DoaCovArgs &a, const CovLane &p, Value value) {
    const int lane = threadIdx.x, M = a.n_mics, D = a.n_angles, nK = a.n_bins;
    const f64x2 *st = a.steer + p.kk;
    double *row = p.sums(a, a.part, D);
    f64x2 an[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) an[m] = m < M ? st[(long)m * nK] : f64x2{0.0, 0.0};
    double keep = 0.0;
    for (int d = 0; d < D; ++d) {
        double ur[MP], ui[MP];
#pragma unroll
        for (int m = 0; m < MP; ++m) {
            ur[m] = an[m].x;
            ui[m] = an[m].y;
        }
        const int dn = d + 1 < D ? d + 1 : d;
#pragma unroll
        for (int m = 0; m < MP; ++m)
            if (m < M) an[m] = st[((long)dn * M + m) * nK];
        const double sum = wave_sum64(value(ur, ui));
        if (lane == (d & 63)) keep = sum;
        if ((d & 63) == 63 || d == D - 1) {
            const int dd = (d & ~63) + lane;
            if (dd <= d) row[dd] = keep;
        }
    }
}

// ---- Capon --------------------------------------------------------------------------------------------------------------------------
// MP = 2 x microphone pairs (2, 4, 6, 8).  An odd count's last pair has a zero partner channel: its spectrum (the transform's rounding
// residue) is never formed -- row MP-1 of R~ is pinned to the identity and its steering entry to 0, so it adds nothing to |u|^2.
// The strict lower triangle of R (then of L) and the real diagonal (then 1 / L_ii) are registers; every loop below is unrolled.
template <int MP>
__global__ __launch_bounds__(64) void doa_capon_kernel(DoaCovArgs a) {
    constexpr int NT = MP * (MP - 1) / 2;
    const CovLane p(a, MP / 2);
    const int M = a.n_mics;
    double Rr[NT > 0 ? NT : 1], Ri[NT > 0 ? NT : 1], Rd[MP];
    cov_accumulate<MP>(p.zr, p.k, a.nfft, M, a.frames_per_block, Rr, Ri, Rd);
    double tau = 0.0;
#pragma unroll
    for (int i = 0; i < MP; ++i) tau += Rd[i];  // (the pinned row's entry is an exact 0)
    const bool ok = tau > 0.0;
    const double inv = ok ? 1.0 / tau : 0.0, load = a.delta / (double)M;  // tau = 0: R~ = (delta / M) I, and c is forced to 0 below
#pragma unroll
    for (int e = 0; e < NT; ++e) {
        Rr[e] *= inv;
        Ri[e] *= inv;
    }
#pragma unroll
    for (int i = 0; i < MP; ++i) Rd[i] = i < M ? fma(Rd[i], inv, load) : 1.0;
    // R~ = L L^H in place, column by column; Rd[j] becomes 1 / L_jj
#pragma unroll
    for (int j = 0; j < MP; ++j) {
        const double rinv = 1.0 / sqrt(Rd[j]);
        Rd[j] = rinv;
#pragma unroll
        for (int i = j + 1; i < MP; ++i) {
            Rr[i * (i - 1) / 2 + j] *= rinv;
            Ri[i * (i - 1) / 2 + j] *= rinv;
        }
#pragma unroll
        for (int c = j + 1; c < MP; ++c) {
            const double lr = Rr[c * (c - 1) / 2 + j], li = Ri[c * (c - 1) / 2 + j];
            Rd[c] = fma(-li, li, fma(-lr, lr, Rd[c]));
#pragma unroll
            for (int i = c + 1; i < MP; ++i) {  // A_ic -= L_ij conj(L_cj)
                const double pr = Rr[i * (i - 1) / 2 + j], pi = Ri[i * (i - 1) / 2 + j];
                Rr[i * (i - 1) / 2 + c] = fma(-pi, li, fma(-pr, lr, Rr[i * (i - 1) / 2 + c]));
                Ri[i * (i - 1) / 2 + c] = fma(pr, li, fma(-pi, lr, Ri[i * (i - 1) / 2 + c]));
            }
        }
    }
    const double cnum = (double)M / (1.0 + a.delta);
    const bool counts = p.live && ok;
    walk_angles<MP>(a, p, [&](double (&ur)[MP], double (&ui)[MP]) {
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < MP; ++i) {  // u_i = (a_i - sum_{c < i} L_ic u_c) / L_ii
#pragma unroll
            for (int c = 0; c < i; ++c) {
                const int e = i * (i - 1) / 2 + c;
                ur[i] = fma(Ri[e], ui[c], fma(-Rr[e], ur[c], ur[i]));
                ui[i] = fma(-Ri[e], ur[c], fma(-Rr[e], ui[c], ui[i]));
            }
            ur[i] *= Rd[i];
            ui[i] *= Rd[i];
            q = fma(ui[i], ui[i], fma(ur[i], ur[i], q));
        }
        const double c = cnum / q;  // formed on every lane: the choice below is a select, not a branch round the solve
        return counts ? c : 0.0;
    });
}

// More than 8 microphones: the same per-lane algorithm through the work space, the solve's vector at NT + i.
__global__ __launch_bounds__(64) void doa_capon_ws_kernel(DoaCovArgs a) {
    const int lane = threadIdx.x, M = a.n_mics, D = a.n_angles, nK = a.n_bins;
    const CovLane p(a, (M + 1) / 2);
    EigMem e(a);
    const int NT = e.NT;
    cov_accumulate(e, p.zr, p.k, a.nfft, a.frames_per_block);
    double tau = 0.0;
    for (int i = 0; i < M; ++i) tau += e.diag(i);
    const bool ok = tau > 0.0;
    const double inv = ok ? 1.0 / tau : 0.0, load = a.delta / (double)M;
    for (int i = 0; i < M; ++i) {
        for (int c = 0; c < i; ++c) {
            f64x2 &r = e.at(i * (i + 1) / 2 + c);
            r = f64x2{r.x * inv, r.y * inv};
        }
        f64x2 &r = e.at(i * (i + 1) / 2 + i);
        r.x = fma(r.x, inv, load);
    }
    for (int j = 0; j < M; ++j) {
        const double rinv = 1.0 / sqrt(e.at(j * (j + 1) / 2 + j).x);
        e.at(j * (j + 1) / 2 + j).x = rinv;
        for (int i = j + 1; i < M; ++i) {
            f64x2 &r = e.at(i * (i + 1) / 2 + j);
            r = f64x2{r.x * rinv, r.y * rinv};
        }
        for (int c = j + 1; c < M; ++c) {
            const f64x2 l = e.at(c * (c + 1) / 2 + j);
            f64x2 &dg = e.at(c * (c + 1) / 2 + c);
            dg.x = fma(-l.y, l.y, fma(-l.x, l.x, dg.x));
            for (int i = c + 1; i < M; ++i) {
                const f64x2 pv = e.at(i * (i + 1) / 2 + j);
                f64x2 &r = e.at(i * (i + 1) / 2 + c);
                r = f64x2{fma(-pv.y, l.y, fma(-pv.x, l.x, r.x)), fma(pv.x, l.y, fma(-pv.y, l.x, r.y))};
            }
        }
    }
    const double cnum = (double)M / (1.0 + a.delta);
    const f64x2 *st = a.steer + p.kk;
    double *row = p.sums(a, a.part, D);
    for (int d = 0; d < D; ++d) {
        double q = 0.0;
        for (int i = 0; i < M; ++i) {
            f64x2 u = st[((long)d * M + i) * nK];
            for (int c = 0; c < i; ++c) {
                const f64x2 l = e.at(i * (i + 1) / 2 + c), v = e.at(NT + c);
                u = f64x2{fma(l.y, v.y, fma(-l.x, v.x, u.x)), fma(-l.y, v.x, fma(-l.x, v.y, u.y))};
            }
            const double rinv = e.at(i * (i + 1) / 2 + i).x;
            u = f64x2{u.x * rinv, u.y * rinv};
            e.at(NT + i) = u;
            q = fma(u.y, u.y, fma(u.x, u.x, q));
        }
        const double sum = wave_sum64(p.live && ok ? cnum / q : 0.0);
        if (lane == 0) row[d] = sum;
    }
}

// ---- MUSIC --------------------------------------------------------------------------------------------------------------------------
// The Capon kernels' lane per (stream, block, bin) and covariance; then R / tau = V diag(lambda) V^H by doa_eig.hpp's Jacobi sweeps (a fixed
// count: no lane waits for another), the eigenvalues' ranks by comparisons, and per angle nu = 1 / M sum_{noise i} |v_i^H a_d|^2.
//
// MP = 2 x microphone pairs (2, 4, 6, 8).  An odd count's zero partner channel is never formed: row and column MP-1 are zero with -1 on
// the diagonal and a zero steering entry.  No rotation touches them (their pivots are exact zeros), the eigenvalue -1 sorts last, so
// its vector e_{MP-1} is always noise (n_sources <= M - 1 <= MP - 2) and adds |e^H a|^2 = 0.
template <int MP>
__global__ __launch_bounds__(64) void doa_music_kernel(DoaCovArgs a) {
    constexpr int NT = MP * (MP - 1) / 2;
    const CovLane p(a, MP / 2);
    const int lane = threadIdx.x, M = a.n_mics;
    EigRegs<MP> e;
    cov_accumulate<MP>(p.zr, p.k, a.nfft, M, a.frames_per_block, e.Rr, e.Ri, e.Rd);
    double tau = 0.0;
#pragma unroll
    for (int i = 0; i < MP; ++i) tau += e.Rd[i];  // (the pinned row's entry is an exact 0)
    const bool ok = tau > 0.0;
    const double inv = ok ? 1.0 / tau : 0.0;  // tau = 0: the zero matrix, V = I; nu and lambda are forced below
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        e.Rr[t] *= inv;
        e.Ri[t] *= inv;
    }
#pragma unroll
    for (int i = 0; i < MP; ++i) e.Rd[i] = i < M ? e.Rd[i] * inv : -1.0;
    jacobi_eig<MP>(e, MP, jacobi_sweeps(MP));
    int rk[MP];
    double wgt[MP];  // 1: column i of V spans noise
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        rk[i] = eig_rank<MP>(e, MP, i);
        wgt[i] = rk[i] >= a.n_sources ? 1.0 : 0.0;
    }
    // the profile: slot j takes the eigenvalue of rank j; a wavefront's 64 values per slot in one fixed butterfly, lane j keeps slot j
    double keep = 0.0;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < MP; ++i) v = rk[i] == j ? fmax(e.Rd[i], 0.0) : v;
        const double sum = wave_sum64(p.live && ok ? v : 0.0);
        if (lane == j) keep = sum;
    }
    if (lane < M) p.sums(a, a.epart, M)[lane] = keep;

    walk_angles<MP>(a, p, [&](double (&ur)[MP], double (&ui)[MP]) {
        double q = 0.0;
#pragma unroll
        for (int i = 0; i < MP; ++i) {  // y = v_i^H a = sum_m conj(V_mi) a_m
            double yr = 0.0, yi = 0.0;
#pragma unroll
            for (int m = 0; m < MP; ++m) {
                yr = fma(e.Vi[m * MP + i], ui[m], fma(e.Vr[m * MP + i], ur[m], yr));
                yi = fma(-e.Vi[m * MP + i], ur[m], fma(e.Vr[m * MP + i], ui[m], yi));
            }
            q = fma(wgt[i], fma(yi, yi, yr * yr), q);
        }
        const double quot = q / (double)M;  // formed on every lane: the choices below are selects, not a branch round the products
        const double nu = ok ? quot : 1.0;
        return p.live ? nu : 0.0;
    });
}

// More than 8 microphones: doa_eig.hpp's solver runs on the work space through EigMem; at NT + i per column (noise weight, rank).
__global__ __launch_bounds__(64) void doa_music_ws_kernel(DoaCovArgs a) {
    const int lane = threadIdx.x, M = a.n_mics, D = a.n_angles, nK = a.n_bins;
    const CovLane p(a, (M + 1) / 2);
    EigMem e(a);
    const int NT = e.NT;
    cov_accumulate(e, p.zr, p.k, a.nfft, a.frames_per_block);
    double tau = 0.0;
    for (int i = 0; i < M; ++i) tau += e.diag(i);
    const bool ok = tau > 0.0;
    const double inv = ok ? 1.0 / tau : 0.0;
    for (int t = 0; t < NT; ++t) {
        f64x2 &r = e.at(t);
        r = f64x2{r.x * inv, r.y * inv};
    }
    jacobi_eig<0>(e, M, jacobi_sweeps(M));
    for (int i = 0; i < M; ++i) {
        const int r = eig_rank<0>(e, M, i);
        e.at(NT + i) = f64x2{r >= a.n_sources ? 1.0 : 0.0, (double)r};
    }
    double *erow = p.sums(a, a.epart, M);
    for (int j = 0; j < M; ++j) {
        double v = 0.0;
        for (int i = 0; i < M; ++i)
            if ((int)e.at(NT + i).y == j) v = fmax(e.diag(i), 0.0);
        const double sum = wave_sum64(p.live && ok ? v : 0.0);
        if (lane == 0) erow[j] = sum;
    }
    const f64x2 *st = a.steer + p.kk;
    double *row = p.sums(a, a.part, D);
    for (int d = 0; d < D; ++d) {
        double q = 0.0;
        for (int i = 0; i < M; ++i) {
            double yr = 0.0, yi = 0.0;
            for (int m = 0; m < M; ++m) {
                const EigC v = e.vec(m, i);
                const f64x2 u = st[((long)d * M + m) * nK];
                yr = fma(v.im, u.y, fma(v.re, u.x, yr));
                yi = fma(-v.im, u.x, fma(v.re, u.y, yi));
            }
            q = fma(e.at(NT + i).x, fma(yi, yi, yr * yr), q);
        }
        const double nu = ok ? q / (double)M : 1.0;
        const double sum = wave_sum64(p.live ? nu : 0.0);
        if (lane == 0) row[d] = sum;
    }
}

// the register kernel of the method at one compile-time size
template <int MP>
void launch_cov_regs(const DoaCovArgs &a, bool music, dim3 grid, hipStream_t s) {
    if (music) BF_LAUNCH(doa_music_kernel<MP>, grid, dim3(64), 0, s, a);
    else BF_LAUNCH(doa_capon_kernel<MP>, grid, dim3(64), 0, s, a);
}

}  // namespace

hipError_t launch_doa_cov_table(const f64x2 *src, f64x2 *dst, int n_bins, int n_mics, int n_angles, hipStream_t s) {
    const long n = (long)n_bins * n_mics * n_angles;
    const long blocks = (n + kDoaBlock - 1) / kDoaBlock;
    BF_LAUNCH(capon_table_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kDoaBlock), 0, s, src, dst, n_bins, n_mics, n_angles);
    return hipGetLastError();
}

hipError_t launch_doa_cov(const DoaCovArgs &a, const DoaPlan &p, hipStream_t s) {
    const bool music = p.method == kDoaMusic;
    if ((!music && p.method != kDoaCapon) || a.n_blocks < 1 || a.n_blocks > p.chunk_blocks || a.n_segments != p.segments)
        return hipErrorInvalidValue;
    if (music && (!a.epart || a.n_sources < 1 || a.n_sources > a.n_mics - 1)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.n_blocks * p.segments), p.grid_y);
    switch (p.mp) {
        case 2: launch_cov_regs<2>(a, music, grid, s); break;
        case 4: launch_cov_regs<4>(a, music, grid, s); break;
        case 6: launch_cov_regs<6>(a, music, grid, s); break;
        case 8: launch_cov_regs<8>(a, music, grid, s); break;
        default:
            if (p.path != DoaPath::kWorkspace || !a.ws) return hipErrorInvalidValue;
            if (music) BF_LAUNCH(doa_music_ws_kernel, grid, dim3(64), 0, s, a);
            else BF_LAUNCH(doa_capon_ws_kernel, grid, dim3(64), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_doa_hop_flags(const float *x, const float *hist, unsigned *flags, long n_frames, long mic_stride, long stream_stride_x,
                                int n_streams, int n_mics, int hop, int layout, hipStream_t s) {
    BF_LAUNCH(doa_hop_flags_kernel, dim3((unsigned)(n_frames + 1), (unsigned)n_streams), dim3(kDoaBlock), 0, s, x, hist, flags, n_frames,
              mic_stride, stream_stride_x, n_mics, hop, layout);
    return hipGetLastError();
}

hipError_t launch_doa_map(const DoaMapArgs &a, const DoaPlan &p, hipStream_t s) {
    if (p.path != DoaPath::kFrameTiles || a.n_frames < 1 || a.n_frames > p.chunk_frames || a.n_mics < 1 || a.n_mics > 32) return hipErrorInvalidValue;
    const long n_ft = (a.n_frames + kDoaTileFrames - 1) / kDoaTileFrames, n_at = (a.n_angles + kDoaTileAngles - 1) / kDoaTileAngles;
    const dim3 grid((unsigned)(n_ft * n_at), p.grid_y, p.grid_z);
    switch (p.mp) {
        case 2: BF_LAUNCH(doa_map_kernel<2>, grid, dim3(kDoaBlock), 0, s, a); break;
        case 4: BF_LAUNCH(doa_map_kernel<4>, grid, dim3(kDoaBlock), 0, s, a); break;
        case 8: BF_LAUNCH(doa_map_kernel<8>, grid, dim3(kDoaBlock), 0, s, a); break;
        case 16: BF_LAUNCH(doa_map_kernel<16>, grid, dim3(kDoaBlock), 0, s, a); break;
        default: BF_LAUNCH(doa_map_kernel<0>, grid, dim3(kDoaBlock), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_doa_reduce(const DoaReduceArgs &a, hipStream_t s) {
    BF_LAUNCH(doa_reduce_kernel, dim3((unsigned)a.n_blocks, (unsigned)a.n_streams), dim3(kDoaBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_track_from_peaks(const TrackFromPeaksArgs &a, int n_streams, hipStream_t s) {
    BF_LAUNCH(track_from_peaks_kernel, dim3((unsigned)n_streams), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_doa_pick(const DoaPickArgs &a, hipStream_t s) {
    if (a.n_rows < 1 || a.n_angles < 1 || a.n_angles > 64 * kPickSlots || a.k < 1 || a.k > kPickMax) return hipErrorInvalidValue;
    const long cap = 1L << 20;  // a wavefront walks rows r, r + grid, ... beyond this many
    BF_LAUNCH(doa_pick_kernel, dim3((unsigned)(a.n_rows < cap ? a.n_rows : cap)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ctrack_from_picks(const CtrackFromPicksArgs &a, int n_streams, hipStream_t s) {
    if (a.n_cols < 1 || a.n_cols > kPickMax || a.k < 1 || a.k > kPickMax) return hipErrorInvalidValue;
    BF_LAUNCH(ctrack_from_picks_kernel, dim3((unsigned)n_streams), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ctrack_assign(const CtrackAssignArgs &a, int n_streams, hipStream_t s) {
    if (a.n_cols < 1 || a.n_cols > kAssignMax || a.k < 1 || a.k > kAssignMax || a.n_angles < 1 || a.n_blocks < 1 || n_streams < 1)
        return hipErrorInvalidValue;
    BF_LAUNCH(ctrack_assign_kernel, dim3((unsigned)n_streams), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace bf
