// cov_kernels.hip -- mvdr / lcmv: sliding per-bin covariance + Cholesky-based constrained solve, four mappings of a problem
// onto lanes (thread-per-problem, row-per-lane over LDS, cyclic rows over DPP quads, row-per-lane over DPP rows).
#include "launch_trace.hpp"
#include "bins_common.hpp"

namespace bf {
namespace BF_NTAG {

namespace {

// ======================================================================================
//                     mvdr / lcmv: covariance, Cholesky solve, constraints
// ======================================================================================
// One group of MP lanes per (stream, bin) problem, lane i <-> microphone i; the group walks a
// tile of consecutive frames so the sample covariance of the previous P frames
//   R = past_ffts[j] * past_ffts[j]^H                     (mvdr.cpp:87, lcmv.cpp:112)
// is slid by one rank-1 update and one downdate per frame (recomputed from scratch at the tile
// start).  The reference inverts R o whiteR with PartialPivLU and forms
//   mvdr:  w = R^-1 a / (a^H R^-1 a),   y = w^H x                     (mvdr.cpp:88-94)
//   lcmv:  W = R^-1 C (C^H R^-1 C)^-1,  y = W(:,0)^H x                (lcmv.cpp:113-119)
// R o whiteR is Hermitian positive definite whenever every mic has history energy, so with
// R = L L^H, U = L^-1 [C | x]:   G = U_C^H U_C,  g = U_C^H u_x,  y = (G^-1 g)_0
// (mvdr is the KP1 = 1 case: y = u_a^H u_x / u_a^H u_a).  Lane i owns row i of the
// factorisation; columns are exchanged through LDS (one wavefront executes its LDS operations
// in order, so only compiler barriers separate the phases).  A zero covariance (frame 0 of a
// cold start) yields 0 * inf = NaN, the same NaN frame the reference emits.
// ---- mvdr fast path: one thread per (stream, tile, in-band problem), whole problem in registers -------------
// For M <= 8 the lower triangle of R (36 complex) and of its working copy fit the 512-entry register file of a
// wavefront that has a SIMD to itself (fp64 FMA issues every 4 cycles, so one wavefront per SIMD already keeps the
// fp64 pipe busy).  No LDS exchange, no idle lanes.  Same maths as mvdr_lcmv_kernel with KP1 = 1:
//   R o whiteR = L L^H,  u = L^-1 a,  v = L^-1 x,  y = u^H v / u^H u.
// Lanes enumerate (time tile, problem) pairs of ONE output stream, problem fastest, over the problems that need a solve
// only: k = 0 is problem 0 (y = X_0, mvdr.cpp:76), then the in-band problems (FastPlan).  Out-of-band problems (34 % of
// the rows at the launch-file band) occupy no lane at all, and the host picks the tile length so that the wavefronts
// fill the chip's 4 x CUs slots a whole number of times (65 536 frames, 340 problems, 256 CUs: 1 020 wavefronts of 342 frames
// = one round, where one wavefront per (128-frame tile, 64 consecutive problems) took three; chain_geom.hpp, pinned by the CPU suite).
// MP = 2 x microphone pairs (2, 4, 6, 8): an odd count's last pair has a zero partner channel, whose row is pinned to the
// identity (its spectrum is the transform's ~1e-16 rounding residue, not an exact zero).
// (FastPlan itself: chain_plan.hpp; chain_geom.hpp fills it)

// one row of 64 stored elements, global -> LDS (lane l's 12 or 16 bytes land at row + 16 l)
template <bool Z128>
__device__ __forceinline__ void lds_dma(const char *g, void *l) {
    if constexpr (Z128)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g, (__attribute__((address_space(3))) void *)l, 16, 0, 0);
    else
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g, (__attribute__((address_space(3))) void *)l, 12, 0, 0);
}

template <int KM>
struct GramIdx {  // entries of the Hermitian upper triangle of G followed by g
    static constexpr int NG = KM * (KM + 1) / 2;
    static constexpr int NE = NG + KM;
};

#define BF_COV_TRACK 0
#define BF_COV_ROWS 0
#define BF_COV_NAME(n_) n_##_kernel
#include "cov_kernels_body.hpp"
#undef BF_COV_TRACK
#undef BF_COV_NAME
#define BF_COV_TRACK 1
#define BF_COV_NAME(n_) n_##_track_kernel
#include "cov_kernels_body.hpp"
#undef BF_COV_TRACK
#undef BF_COV_NAME
#undef BF_COV_ROWS
// the lane kernel's twins that store every beam of lcmv (bf_config.lcmv_out_beams): mvdr_fast_rows_kernel, mvdr_fast_track_rows_kernel
#define BF_COV_ROWS 1
#define BF_COV_TRACK 0
#define BF_COV_NAME(n_) n_##_rows_kernel
#include "cov_kernels_body.hpp"
#undef BF_COV_TRACK
#undef BF_COV_NAME
#define BF_COV_TRACK 1
#define BF_COV_NAME(n_) n_##_track_rows_kernel
#include "cov_kernels_body.hpp"
#undef BF_COV_TRACK
#undef BF_COV_NAME
#undef BF_COV_ROWS

// ---- 16-lane DPP row helpers (row_newbcast exchange) of cov2d_kernel below; round 2's one-problem-per-row kernel is gone (EXPERIMENTS.md) ----------
// Same row-per-lane factorisation as mvdr_lcmv_kernel<16, KM>, but a problem occupies exactly one DPP row, so the
// pivot, the scaled column and the right-hand sides travel by `v_mov_b32_dpp row_newbcast:n` (lane n of every row to
// the whole row, one instruction per dword, VALU latency) instead of an LDS write -> s_waitcnt -> read round trip per
// column, and the Gram sums are row reductions (quad_perm xor 1/2, row_half_mirror, row_mirror).  No LDS at all.
// DPP note: every pattern in this file (quad_perm, row_newbcast, row mirrors) reads a valid source lane for every destination
// lane, so the `old` operand is dead.  With bound_ctrl = false hipcc still materialises it (v_mov_b32 old, 0 in front of every
// v_mov_b32_dpp: 812 + 812 instructions in the lcmv-16 solve block = 44 % of it); bound_ctrl = true drops the initialisation.
// (row_newbcast is the one DPP control gfx950 encodes for 64-bit operands: one v_mov_b64_dpp per double instead of two v_mov_b32_dpp)
template <int N>
__device__ __forceinline__ double rowbc(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + N, 0xF, 0xF, true);
}
template <int N>
__device__ __forceinline__ cd rowbc(cd v) { return cd{rowbc<N>(v.x), rowbc<N>(v.y)}; }
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double row_sum(double v) {  // every lane of the 16-lane row gets the row total
    v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_d<0x141>(v);  // row_half_mirror
    v += dpp_d<0x140>(v);  // row_mirror
    return v;
}
template <int C, int MP>
struct RowStep {  // compile-time loops over the broadcast source lane
    template <typename F>
    static __device__ __forceinline__ void run(F &&f) {
        f(std::integral_constant<int, C>{});
        RowStep<C + 1, MP>::run(f);
    }
};
template <int MP>
struct RowStep<MP, MP> {
    template <typename F>
    static __device__ __forceinline__ void run(F &&) {}
};

// ---- lcmv / mvdr, 9..16 microphones: 2-D cyclic 4 x 4 lanes per problem -------------------------------------------------
// One problem (stream, bin) per 16-lane DPP row (as round 2's row-per-lane kernel had it), but the lanes form a 4 x 4 grid (p = lane >> 2,
// q = lane & 3 inside the row) and matrix entry (i, c) lives in lane (i mod 4, c mod 4) at local index (i / 4, c / 4):
// every lane owns a 4 x 4 block of R and of the working copy (its lower triangle + diagonal: 10 entries), so
//   * the triangular trailing update keeps all 16 lanes busy until the last 4 x 4 block (the row-per-lane kernel idles half
//     of them on average: 1 020 fp64 instructions per wavefront-frame where 455 would do),
//   * a lane carries 10 + 10 matrix entries and 4 x 2 right-hand-side entries instead of 16 + 16 + 5: ~130 VGPRs, four
//     wavefronts per SIMD instead of two.
// Exchange per elimination step jj (column jj = 4 bj + qj):
//   pivot            lane (qj, qj)        -> whole row        DPP row_newbcast
//   scaled column    lanes (p, qj)        -> their quad       DPP quad_perm broadcast          Lrow[a] = L(4a+p, jj)
//   its transpose    lane (q, p)          -> lane (p, q)      ds_bpermute, fixed address       Lcol[b] = L(4b+q, jj)
//   right-hand side  lane (qj, q)         -> lanes (., q)     ds_bpermute                      u = b(jj, col) / L(jj, jj)
// Right-hand-side column r belongs to the lanes with q = r mod 4 (slot r / 4): constraints 0..3 in slot 0, the frame's x in
// slot 1 of the q = 0 lanes.  Rows that are already final (i <= jj) are switched off by zeroing their Lrow entry, so the
// updates run unconditionally.  Maths as everywhere in this file: R o whiteR = L L^H, U = L^-1 [C | x], G = U_C^H U_C,
// g = U_C^H u_x, y = (G^-1 g)_0.
template <int SRC>
__device__ __forceinline__ double quadbc(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), SRC * 0x55, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), SRC * 0x55, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
template <int SRC>
__device__ __forceinline__ cd quadbc(cd v) { return cd{quadbc<SRC>(v.x), quadbc<SRC>(v.y)}; }
__device__ __forceinline__ double bperm_d(int addr, double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_ds_bpermute(addr, (int)(b & 0xffffffffLL));
    const int hi = __builtin_amdgcn_ds_bpermute(addr, (int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ cd bperm_c(int addr, cd v) { return cd{bperm_d(addr, v.x), bperm_d(addr, v.y)}; }
// sum over the four quads of a 16-lane row (same q): row_ror 4 and 8
__device__ __forceinline__ double quads_sum(double v) {
    v += dpp_d<0x124>(v);  // row_ror:4
    v += dpp_d<0x128>(v);  // row_ror:8
    return v;
}
// local lower triangle (a >= b) of a 4 x 4 block, row-major
__device__ constexpr int LT(int a, int b) { return a * (a + 1) / 2 + b; }

// cov2d_kernel<KM, WPS, Z128> and its twin that stores every beam (lcmv_out_beams; cov2d_kernel_body.hpp): textual inclusion, so that
// the one-row kernel keeps its name in the launch trace and its instructions
#define BF_COV_ROWS 0
#define BF_COV2D_NAME cov2d_kernel
#include "cov2d_kernel_body.hpp"
#undef BF_COV_ROWS
#undef BF_COV2D_NAME
#define BF_COV_ROWS 1
#define BF_COV2D_NAME cov2d_rows_kernel
#include "cov2d_kernel_body.hpp"
#undef BF_COV_ROWS
#undef BF_COV2D_NAME

}  // namespace

// tiles, grids, the FastPlan and the zero-fill of the batch: ChainPlan::geom (chain_geom.hpp)
hipError_t launch_mvdr_lcmv(const ChainPlan &p, const BinsArgs &a, hipStream_t s) {
    const BinsGeom &g = p.geom.bins;
    const int tile = g.tile, tps = g.tps;
    // lcmv with bf_config.lcmv_out_beams > 1: every kernel stores p.rows rows per stream (Yh = [stream][rows][frame][kYhStride]).  The lane kernel
    // and cov2d_kernel have twins for it, instantiated for two columns and more: a batch without interferers runs the next larger one,
    // whose padding column is the identity (row 0 then equals the one-row kernel's to rounding, not bit for bit).  The group kernel counts at run time
    const bool rows = p.rows > 1;
    if (a.gss_rows != p.rows || (rows && a.cfg.algo != BF_LCMV)) return hipErrorInvalidValue;
    if (p.bins == ChainBins::kMvdrLcmv) {  // a group of MP lanes per problem, padding rows / columns are identity
        const dim3 grid(g.gx, g.gy);
#define BF_LAUNCH_ML(MP_, KM_)                                                                                               \
    do {                                                                                                                     \
        if (p.ctrack) BF_LAUNCH((mvdr_lcmv_track_kernel<MP_, KM_>), grid, dim3(256), 0, s, a, tile, tps);                    \
        else BF_LAUNCH((mvdr_lcmv_kernel<MP_, KM_>), grid, dim3(256), 0, s, a, tile, tps);                                   \
    } while (0)
        if (p.km == 1) {
            if (p.mp == 4) BF_LAUNCH_ML(4, 1); else if (p.mp == 8) BF_LAUNCH_ML(8, 1); else if (p.mp == 16) BF_LAUNCH_ML(16, 1); else BF_LAUNCH_ML(32, 1);
        } else if (p.km == 4) {
            if (p.mp == 4) BF_LAUNCH_ML(4, 4); else if (p.mp == 8) BF_LAUNCH_ML(8, 4); else if (p.mp == 16) BF_LAUNCH_ML(16, 4); else BF_LAUNCH_ML(32, 4);
        } else if (p.km == 8) {
            if (p.mp == 8) BF_LAUNCH_ML(8, 8); else if (p.mp == 16) BF_LAUNCH_ML(16, 8); else BF_LAUNCH_ML(32, 8);
        } else {
            if (p.mp == 16) BF_LAUNCH_ML(16, 16); else BF_LAUNCH_ML(32, 16);
        }
#undef BF_LAUNCH_ML
        return hipGetLastError();
    }
    // 9..16 microphones, up to 3 interferers: 2-D cyclic 4 x 4 lanes per problem.  Wavefronts per SIMD: with constraint columns (lcmv) the
    // three-wavefront build spills 30 registers per lane and the spill traffic alone is 6 GB per 32 768 frames of 16 microphones: two
    // wavefronts at 211 registers are 7 % faster; without constraints (mvdr) three wavefronts win by 12 %
    if (p.bins == ChainBins::kCov2d) {
        const dim3 grid(g.cov2d_grid);  // (unit, problem group) -> XCD-aware order in the kernel
        if (rows) {
            if (p.z48) BF_LAUNCH((cov2d_rows_kernel<4, 2, false>), grid, dim3(256), 0, s, a, tile, tps);
            else BF_LAUNCH((cov2d_rows_kernel<4, 2, true>), grid, dim3(256), 0, s, a, tile, tps);
        } else if (p.km == 1) {
            if (p.z48) BF_LAUNCH((cov2d_kernel<1, 3, false>), grid, dim3(256), 0, s, a, tile, tps);
            else BF_LAUNCH((cov2d_kernel<1, 3, true>), grid, dim3(256), 0, s, a, tile, tps);
        } else {
            if (p.z48) BF_LAUNCH((cov2d_kernel<4, 2, false>), grid, dim3(256), 0, s, a, tile, tps);
            else BF_LAUNCH((cov2d_kernel<4, 2, true>), grid, dim3(256), 0, s, a, tile, tps);
        }
        return hipGetLastError();
    }
    // kMvdrFast: one lane per (tile, problem that needs a solve); the rows nobody solves but the backward transform reads are zeroed first
    const FastPlan &fp = g.fp;
    const int km = g.fast_km;  // columns of the instantiation that runs
    if (g.zero == ChainZero::kF64Rows)
        (void)hipMemsetAsync(a.Yh, 0, (size_t)a.n_streams * p.rows * a.n_frames * kYhStride * sizeof(f64x2), s);
    else if (g.zero == ChainZero::kF32Rows)
        (void)hipMemsetAsync(a.Yh, 0, (size_t)a.n_streams * p.rows * a.n_frames * kYhStride * sizeof(f32x2), s);
    const dim3 grid(g.fast_grid);
#define BF_FAST_GO(MP_, KC_)                                                                                         \
    do {                                                                                                             \
        if (p.ctrack) {                                                                                              \
            if (p.z48) BF_LAUNCH((mvdr_fast_track_kernel<MP_, KC_, false>), grid, dim3(64), 0, s, a, fp);            \
            else BF_LAUNCH((mvdr_fast_track_kernel<MP_, KC_, true>), grid, dim3(64), 0, s, a, fp);                   \
        } else if (p.z48) BF_LAUNCH((mvdr_fast_kernel<MP_, KC_, false>), grid, dim3(64), 0, s, a, fp);               \
        else BF_LAUNCH((mvdr_fast_kernel<MP_, KC_, true>), grid, dim3(64), 0, s, a, fp);                             \
    } while (0)
#define BF_FAST_ROWS(MP_, KC_)                                                                                       \
    do {                                                                                                             \
        if (p.ctrack) {                                                                                              \
            if (p.z48) BF_LAUNCH((mvdr_fast_track_rows_kernel<MP_, KC_, false>), grid, dim3(64), 0, s, a, fp);       \
            else BF_LAUNCH((mvdr_fast_track_rows_kernel<MP_, KC_, true>), grid, dim3(64), 0, s, a, fp);              \
        } else if (p.z48) BF_LAUNCH((mvdr_fast_rows_kernel<MP_, KC_, false>), grid, dim3(64), 0, s, a, fp);          \
        else BF_LAUNCH((mvdr_fast_rows_kernel<MP_, KC_, true>), grid, dim3(64), 0, s, a, fp);                        \
    } while (0)
    if (rows) {
        if (km == 2) {
            if (p.mp == 2) BF_FAST_ROWS(2, 2); else if (p.mp == 4) BF_FAST_ROWS(4, 2); else if (p.mp == 6) BF_FAST_ROWS(6, 2); else BF_FAST_ROWS(8, 2);
        } else if (km == 3) {
            BF_FAST_ROWS(8, 3);
        } else {
            if (p.mp == 4) BF_FAST_ROWS(4, 4); else if (p.mp == 6) BF_FAST_ROWS(6, 4); else BF_FAST_ROWS(8, 4);
        }
    } else if (p.km == 1) {  // mvdr; lcmv without interferers = mvdr except problem 0
        if (p.mp == 2) BF_FAST_GO(2, 1); else if (p.mp == 4) BF_FAST_GO(4, 1); else if (p.mp == 6) BF_FAST_GO(6, 1); else BF_FAST_GO(8, 1);
    } else if (p.km == 2) {
        if (p.mp == 2) BF_FAST_GO(2, 2); else if (p.mp == 4) BF_FAST_GO(4, 2); else if (p.mp == 6) BF_FAST_GO(6, 2); else BF_FAST_GO(8, 2);
    } else if (p.km == 3) {
        BF_FAST_GO(8, 3);
    } else {
        if (p.mp == 4) BF_FAST_GO(4, 4); else if (p.mp == 6) BF_FAST_GO(6, 4); else BF_FAST_GO(8, 4);
    }
#undef BF_FAST_GO
#undef BF_FAST_ROWS
    return hipGetLastError();
}

}  // namespace BF_NTAG
}  // namespace bf
