// doa_assign.hpp -- the rule of bf_ctrack_assign_device (include/bfcore.h) for one stream and one block, serial and over plain arrays:
// which pick continues which talker's column, which columns coast or are freed, and where a new talker is born.  This is the one place
// the rule is written down in C++; ctrack_assign_kernel (doa_kernels.hip) does the same steps with a wavefront and is compared with it
// to the byte.  Plain C++: no HIP in front of the guard, the CPU suite compiles it with g++ the way it compiles doa_pick.hpp.
#pragma once

#include <cstdint>

#include "doa_pick.hpp"

namespace bf {

constexpr int kAssignStateInts = 4;     // BF_ASSIGN_STATE_INTS: {idx, hits, misses, out} per slot
constexpr int kAssignMax = 16;          // the most slots (BF_MAX_INTERF + 1) and the most candidates (BF_DOA_MAX_PICKS)
constexpr int32_t kAssignCap = 1 << 30;  // hits and misses stop counting here

BF_PICK_HD inline int32_t assign_count_up(int32_t v) { return v < kAssignCap ? v + 1 : kAssignCap; }  // min(v + 1, 2^30), no overflow

// Steps 1 to 6 of the contract.  picks: [k] of this block; map_row: [n_angles] of this block or null; state: [n_cols][4], read and
// written; active: [n_cols] or null.  1 <= k, n_cols <= kAssignMax.  A pick is checked against n_angles before it is used as an index,
// a state value is only ever used as an index (into angles) when it is one of 0 .. n_angles-1.
BF_PICK_HD inline void assign_block(const int32_t *picks, const double *map_row, const double *angles, int n_angles, int k, double min_peak,
                                    double gate_deg, int min_hits, int max_coast, int n_cols, int32_t *state, int32_t *active) {
    // 1. candidates
    int32_t cand[kAssignMax];
    int n_cand = 0;
    const int32_t p0 = picks[0];
    if (p0 >= 0 && p0 < n_angles && (map_row == nullptr || !(map_row[p0] < min_peak)))
        for (int j = 0; j < k; ++j)
            if (picks[j] >= 0 && picks[j] < n_angles) cand[n_cand++] = picks[j];
    // 2. match: the distances once, then the closest pair within the gate until there is none
    bool live[kAssignMax], slot_hit[kAssignMax], cand_hit[kAssignMax];
    double d[kAssignMax][kAssignMax];
    for (int c = 0; c < n_cols; ++c) {
        const int32_t idx = state[c * kAssignStateInts];
        live[c] = idx >= 0 && idx < n_angles;
        slot_hit[c] = false;
        if (live[c])
            for (int j = 0; j < n_cand; ++j) d[c][j] = pick_sep(angles[idx], angles[cand[j]]);
    }
    for (int j = 0; j < n_cand; ++j) cand_hit[j] = false;
    for (;;) {
        int bc = -1, bj = -1;
        for (int c = 0; c < n_cols; ++c) {  // ascending c, then ascending j, and a strict <: ties go to the lowest c, then the lowest j
            if (!live[c] || slot_hit[c]) continue;
            for (int j = 0; j < n_cand; ++j)
                if (!cand_hit[j] && d[c][j] <= gate_deg && (bc < 0 || d[c][j] < d[bc][bj])) {  // a NaN is never <= the gate
                    bc = c;
                    bj = j;
                }
        }
        if (bc < 0) break;
        // 3. a matched slot moves to its pick
        int32_t *st = state + bc * kAssignStateInts;
        st[0] = cand[bj];
        st[1] = assign_count_up(st[1]);
        st[2] = 0;
        slot_hit[bc] = cand_hit[bj] = true;
    }
    // 4. an unmatched live slot: a tentative one is freed, a confirmed one coasts for up to max_coast blocks
    for (int c = 0; c < n_cols; ++c) {
        if (!live[c] || slot_hit[c]) continue;
        int32_t *st = state + c * kAssignStateInts;
        if (st[1] < min_hits) st[0] = -1;
        else {
            st[2] = assign_count_up(st[2]);
            if (st[2] > max_coast) st[0] = -1;
        }
    }
    // 5. births: an unmatched candidate takes the lowest free slot, or is dropped
    for (int j = 0; j < n_cand; ++j) {
        if (cand_hit[j]) continue;
        for (int c = 0; c < n_cols; ++c) {
            int32_t *st = state + c * kAssignStateInts;
            if (st[0] >= 0 && st[0] < n_angles) continue;
            st[0] = cand[j];
            st[1] = 1;
            st[2] = 0;
            slot_hit[c] = true;
            break;
        }
    }
    // 6. out follows a confirmed live slot; active: heard in this block and confirmed
    for (int c = 0; c < n_cols; ++c) {
        int32_t *st = state + c * kAssignStateInts;
        const bool confirmed = st[0] >= 0 && st[0] < n_angles && st[1] >= min_hits;
        if (confirmed) st[3] = st[0];
        if (active) active[c] = slot_hit[c] && confirmed ? 1 : 0;
    }
}

// Step 7 around assign_block for one stream: every frame of block b gets `out` as it stood after block b - latency, the `out` of the
// entry state where there is no such block.  picks [n_blocks][k], map [n_blocks][n_angles] or null, track
// [n_blocks * frames_per_block][n_cols], active [n_blocks][n_cols] or null.  The host's counterpart of the kernel's block loop.
inline void assign_stream(const int32_t *picks, const double *map, const double *angles, int n_angles, int k, long n_blocks,
                          int frames_per_block, int latency, double min_peak, double gate_deg, int min_hits, int max_coast, int n_cols,
                          int32_t *state, int32_t *track, int32_t *active) {
    const long W = frames_per_block, WC = W * n_cols;
    for (long b = 0; b < n_blocks && b < latency; ++b)
        for (long i = 0; i < WC; ++i) track[b * WC + i] = state[(i % n_cols) * kAssignStateInts + 3];
    for (long b = 0; b < n_blocks; ++b) {
        assign_block(picks + b * k, map ? map + b * n_angles : nullptr, angles, n_angles, k, min_peak, gate_deg, min_hits, max_coast, n_cols,
                     state, active ? active + b * n_cols : nullptr);
        if (b + latency < n_blocks)
            for (long i = 0; i < WC; ++i) track[(b + latency) * WC + i] = state[(i % n_cols) * kAssignStateInts + 3];
    }
}

}  // namespace bf
