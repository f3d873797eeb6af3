// das_f64_plan.hpp -- what one batch of das in double launches (das_f64_w64.hip), host arithmetic: which kernel serves it (das_f64_decide,
// below) and the work queue of das_f64_pair_kernel: how a batch is cut into CHUNKS of consecutive frame pairs and where chunk k lies.
// Plain C++ (the CPU suite checks it through tests/host_emul: the decision against every das (double) row of docs/DISPATCH.md, random
// shapes and both switches; every plan must tile every stream exactly once, start every chunk on an even frame, stay inside the table and
// inside the 10-bit fields of the kernel's work word).
//
// Per stream: nb = blocks per stream (n_cus / n_streams, at least 1).  The first level gives every block one long chunk (81 % of its equal
// share: consecutive pairs on one CU share their input hop through L1 / L2 and hand over their output hop through LDS flags), the following
// levels halve what is left, the last ones are chunks of 4 and 2 pairs.  A chunk edge costs one input hop read twice and two atomic adds per
// output sample, so the small chunks are kept to the last ~12 % of the batch.  Level-major order over all streams: the table starts with
// every block's long chunk and ends with the small ones that level the finishing times.
// env = BF_DAS_F64_SCHED: "0" = one level of equal chunks (the static runs of round 4); "88,16,8,4,2" = explicit chunk sizes in pairs.
#pragma once

#include <cstdlib>
#include <cstring>

#include "../../include/bfcore.h"

#if defined(__HIPCC__)
#define BF_PLAN_HD __host__ __device__ inline
#else
#define BF_PLAN_HD inline
#endif

namespace bf {

constexpr int kChunkEnd = 0xFFFFF;       // chunk field of the kernel's work word: the table is exhausted
constexpr int kMaxChunkPairs = 1000;     // pairs per chunk (10 bits, and up to 8 draws past the end before the word is replaced)
constexpr int kSchedMaxChunks = 16384;   // rows of the chunk table
// the kernel's device workspace: the draw counter on a line of its own, then the table, one row {stream, first frame, frames, 0} per chunk
constexpr size_t kSchedCounterBytes = 256, kSchedRowBytes = 16;
constexpr size_t das_f64_sched_ws_bytes() { return kSchedCounterBytes + kSchedMaxChunks * kSchedRowBytes; }
// what the decision needs of the kernels' shape (das_f64_w64.hip asserts each against its own constant): samples per hop (the kernels are
// built for N = 1024), wavefronts per block (one step of the microphone-pair kernel's block is 8 frames), hop slots of a block's ring
constexpr int kDasF64Hop = 512, kDasF64Waves = 8, kDasF64RingSlots = 40;

// The pairing rule of the frame-pair kernels (das_f64_w64.hip das_f64_pair_body; tests/host_emul restates it).  m0, m1, m2: the bit
// patterns of the largest |sample| (float) of hops t - 1, t, t + 1 over the microphones that are transformed; frame t is hops t - 1, t and
// frame t + 1 hops t, t + 1.  The two frames share their transforms only if all three maxima are finite (biased exponent below 0xFF) and
// their exponents are at most kDasPairExpSpan apart; hops of exact zeros pair with other such hops only.
// Why the hops and not the frames, and why 4 and not the 20 of istft_w64_kernel (stft_istft.hip): a shared transform leaves about 1e-16 of
// its LOUDEST hop in every sample of both frames, and which neighbour a frame is paired with -- or whether it goes alone, as under
// bf_process_hop -- depends on how a stream is cut into batches.  The float store of a sample s flips where that error reaches the
// distance to a rounding boundary, on average with probability error / ulp(s) ~ 1e-16 R / 6e-8 for a hop a factor R below the loudest:
// 1e-6 R per hop of 512 samples.  R = 2^20 flips samples in every such hop (seen: tests/test_dynamics_gpu.py, the 2^-20 stretch cut at an
// odd frame -- also in the faint half of a frame that straddles the transition and is itself as loud as its partner, which is why frame
// maxima do not do); R <= 2^5 keeps it at 3e-5 per hop at most, 1e-6 per hop on level audio.  So two cuts of one stream give the same
// bytes only STATISTICALLY: about one differing last bit in 10^5 ... 10^6 hops.  No span makes that zero while frames are paired at all;
// the span bounds the rate.  (A frame that goes alone in both cuts is the same bytes in both.)
constexpr int kDasPairExpSpan = 4;
BF_PLAN_HD bool das_f64_may_pair(unsigned m0, unsigned m1, unsigned m2) {
    const int e0 = (int)(m0 >> 23), e1 = (int)(m1 >> 23), e2 = (int)(m2 >> 23);
    const int hi = e0 > e1 ? (e0 > e2 ? e0 : e2) : (e1 > e2 ? e1 : e2), lo = e0 < e1 ? (e0 < e2 ? e0 : e2) : (e1 < e2 ? e1 : e2);
    return hi < 0xFF && hi - lo <= kDasPairExpSpan;
}

struct DasSchedPlan {
    int n_levels;
    int cnt[8], size[8];   // chunks per stream / pairs per chunk of each level
    int n_chunks;          // over all streams
    int grid;              // persistent blocks
};

// chunk k of the table: level-major, inside a level stream-major; the last chunk of a stream may be shorter (and end on a lone frame)
BF_PLAN_HD void das_f64_chunk(const DasSchedPlan &p, long n_frames, int n_streams, int k, int *stream, long *t0, long *n) {
    int lvl = 0, kk = k;
    long pair0 = 0;  // pairs of a stream in front of level lvl
    while (lvl < p.n_levels - 1 && kk >= p.cnt[lvl] * n_streams) {
        kk -= p.cnt[lvl] * n_streams;
        pair0 += (long)p.cnt[lvl] * p.size[lvl];
        ++lvl;
    }
    const int s = kk / p.cnt[lvl], j = kk - s * p.cnt[lvl];
    *stream = s;
    *t0 = 2 * (pair0 + (long)j * p.size[lvl]);
    long len = 2L * p.size[lvl];
    if (*t0 + len > n_frames) len = n_frames - *t0;
    *n = len;
}

inline DasSchedPlan das_f64_plan(long n_frames, int n_streams, int n_cus, const char *env) {
    DasSchedPlan p{};
    const long pairs = (n_frames + 1) / 2;
    long nb = (long)n_cus / n_streams;
    if (nb < 1) nb = 1;
    int sizes[8], n_sizes = 0;
    const long share = (pairs + nb - 1) / nb;  // pairs per block if they were dealt out evenly
    if (env && strchr(env, ',')) {
        const char *c = env;
        while (*c && n_sizes < 8) {
            sizes[n_sizes++] = atoi(c);
            c = strchr(c, ',');
            if (!c) break;
            ++c;
        }
    } else if (!(env && atoi(env) == 0) && share >= 48) {
        long front = (share * 13 / 16) & ~7L;             // 81 % of the share in long chunks, a multiple of 8 pairs
        long rest = share - front;
        while (front > kMaxChunkPairs && n_sizes < 3) {    // (a chunk holds at most kMaxChunkPairs pairs: very long batches get several)
            sizes[n_sizes++] = kMaxChunkPairs;
            front -= kMaxChunkPairs;
        }
        if (front > kMaxChunkPairs) { rest += front - kMaxChunkPairs; front = kMaxChunkPairs; }
        sizes[n_sizes++] = (int)front;
        while (n_sizes < 6 && rest >= 24) {                // the rest in chunks that halve it level by level: 8 at the headline size
            long sz = (rest / 2) & ~7L;
            if (sz > kMaxChunkPairs) sz = kMaxChunkPairs;
            sizes[n_sizes++] = (int)sz;
            rest -= sz;
        }
        if (rest >= 12) { sizes[n_sizes++] = 4; rest -= 4; }
        sizes[n_sizes++] = 2;
    }
    if (n_sizes == 0) {  // equal chunks
        long sz = ((share + 7) / 8) * 8;
        if (sz > kMaxChunkPairs) sz = kMaxChunkPairs & ~7;
        sizes[n_sizes++] = (int)sz;
    }
    long left = pairs;
    for (int i = 0; i < n_sizes && left > 0; ++i) {
        int sz = sizes[i] < 1 ? 1 : (sizes[i] > kMaxChunkPairs ? kMaxChunkPairs : sizes[i]);
        long cnt = (i == n_sizes - 1) ? (left + sz - 1) / sz : nb;
        if (cnt * sz > left) cnt = (left + sz - 1) / sz;
        p.size[p.n_levels] = sz;
        p.cnt[p.n_levels] = (int)cnt;
        ++p.n_levels;
        left -= cnt * sz;
    }
    long total = 0;
    for (int i = 0; i < p.n_levels; ++i) total += (long)p.cnt[i] * n_streams;
    if (total > kSchedMaxChunks || total >= kChunkEnd) {  // too fine for the table: one level of the largest chunks that fit
        long sz = kMaxChunkPairs & ~7;
        p.n_levels = 1;
        p.size[0] = (int)sz;
        p.cnt[0] = (int)((pairs + sz - 1) / sz);
        total = (long)p.cnt[0] * n_streams;
    }
    p.n_chunks = (int)total;
    p.grid = (int)(total < n_cus ? total : n_cus);
    return p;
}

// What one batch launches: das_f64_decide settles it ONCE from the batch's shape, on the host and without touching the device;
// enqueue_das_f64 (das_f64_w64.hip) carries it out.
enum class DasF64Path {
    kChain,      // none of the kernels here: the STFT -> per-bin -> ISTFT chain serves the batch
    kFramePair,  // das_f64_pair_kernel on planar input
    kRing,       // das_f64_ring_kernel: [sample][mic] input with 2, 4 or 8 microphones, transposed hop by hop into the blocks' rings
    kTranspose,  // interleaved_to_planar_kernel (batch, carried hop) + das_f64_pair_kernel: [sample][mic] input otherwise
    kMicPair,    // das_f64_w64_kernel<1>: [sample][mic] input with one microphone or a non-unit weight row 0
};
struct DasF64Launch {
    DasF64Path path;
    DasSchedPlan plan;                  // frame-pair kernels: the chunk plan
    long run_frames, runs_per_stream;   // microphone-pair kernel: its static runs
    size_t scratch_bytes;               // device scratch of enqueue_das_f64: the blocks' hop rings (kRing), the planar batch + carried hop (kTranspose)
    bool writes_hist;                   // the kernel stores the carried hop into DasF64Args::hist_out itself (no copy behind it)
};
// One batch, as values.  mic0_unit, n_tr: the steering summary (geometry.hpp das_f64_slots); tables: the frame-pair kernels' gains and
// work-queue workspace exist.  das_il_ring, das_f64_sched: the switches BF_DAS_IL_RING and BF_DAS_F64_SCHED (switches.hpp; null = unset).
struct DasF64Shape {
    int layout, n_mics, n_streams, n_cus;
    long n_frames;
    bool mic0_unit, tables;
    int n_tr, das_il_ring;
    const char *das_f64_sched;
};

// Which kernel serves a batch (docs/DISPATCH.md).  The frame-pair kernels -- das_f64_pair_kernel on planar input; on [sample][mic] input
// das_f64_ring_kernel at 2, 4 or 8 microphones (the ring's transposition addresses by shifts; das_il_ring = 0: never) and the
// transposition in front of das_f64_pair_kernel otherwise -- never transform microphone 0: they need the reference's unit weight row
// there (das.cpp:33-38, always true for das on a handle that started cold), a second microphone, and a batch their work queue can
// hold.  [sample][mic] input without the first two: the microphone-pair kernel das_f64_w64_kernel<1>.  Anything else: the chain.
// (The transposition moves tiles of 256 samples.  A batch is n_frames hops and the carried hop is one, 512 samples each, so the tile
// always divides both: no frame count is turned away for it.)
inline DasF64Launch das_f64_decide(const DasF64Shape &c) {
    DasF64Launch d{};  // the chain
    if (c.n_mics > 8) return d;  // the gain tables fill the LDS
    if (!(c.tables && c.mic0_unit && c.n_mics >= 2 && c.n_tr >= 1)) {
        if (c.layout == BF_PLANAR) return d;
        // frames per run: a multiple of one step of the block (8 frames), about one run per CU
        const long runs = c.n_cus > c.n_streams ? c.n_cus / c.n_streams : 1;
        d.path = DasF64Path::kMicPair;
        d.run_frames = ((c.n_frames + runs - 1) / runs + kDasF64Waves - 1) / kDasF64Waves * kDasF64Waves;
        d.runs_per_stream = (c.n_frames + d.run_frames - 1) / d.run_frames;
        return d;
    }
    if ((long)c.n_streams * ((c.n_frames + 1) / 2) >= (1L << 31)) return d;
    d.plan = das_f64_plan(c.n_frames, c.n_streams, c.n_cus, c.das_f64_sched);
    if (d.plan.n_chunks < 1 || d.plan.n_chunks > kSchedMaxChunks) return d;  // (more streams than the table has rows)
    const bool ring = c.das_il_ring != 0 && (c.n_mics == 2 || c.n_mics == 4 || c.n_mics == 8);
    d.path = c.layout == BF_PLANAR ? DasF64Path::kFramePair : ring ? DasF64Path::kRing : DasF64Path::kTranspose;
    d.writes_hist = c.layout == BF_PLANAR;
    // scratch: one ring per CU, whatever the plan's grid; the transposition: the batch and the carried hop, planar
    const size_t hop_elems = (size_t)c.n_mics * kDasF64Hop;
    d.scratch_bytes = sizeof(float) * (c.layout == BF_PLANAR ? 0 : ring ? c.n_cus * kDasF64RingSlots * hop_elems : c.n_streams * hop_elems * (c.n_frames + 1));
    return d;
}

}  // namespace bf
