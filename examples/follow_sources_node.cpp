// follow_sources_node.cpp -- an lcmv node that follows the sources a Capon (or MUSIC) map shows, with the whole loop on the device.
//
//   follow_sources_node <beamform_config.yaml> <in.wav> <out.wav> <frames_per_block> <angle_lo> <angle_hi> <angle_step>
//                       [k=2] [min_sep_deg=30] [rel_floor=0] [min_peak=0] [freq_lo=100] [freq_hi=16000] [beams=1] [capon|music[:n]]
//                       [identity [gate_deg=20]]
//
// The config's look direction (initial_angle) and its interferers (angle_interf<k>) are where the node starts; the candidate grid is
// angle_lo, angle_lo + angle_step, ... below angle_hi (degrees).  Per block of frames_per_block periods the strongest peak of the
// Capon map becomes the look direction and the next strongest, at least min_sep_deg away, the interferers, in force from the next
// block on (one block of latency, as an external localiser has).  Four enqueues on one stream and no host synchronisation in between:
//   bf_doa_process_device -> bf_doa_pick_device -> bf_ctrack_from_picks_device -> bf_process_batch_device_ctracked
// Picks and maps come back once, at the end: one line per publishing block on stdout,
//   "<block> <theta_deg> <interferer_deg> ..."
// and the output as rosjack's write_file option writes it: mono PCM16 (rosjack.cpp:189-210, 404-409).
// beams = R > 1 (bf_config.lcmv_out_beams): one signal per constraint column -- row r follows column r of the track (0: the look
// direction, r: interferer r) with nulls on the others -- written to <out.wav>.<r>.wav, one file per row, instead of <out.wav>.
// music[:n]: the MUSIC map instead of the Capon map, with a signal subspace of n dimensions (bf_doa_set_sources; default k, at most
// n_mics - 1).
// identity [gate_deg]: bf_ctrack_assign_device in the third place instead of bf_ctrack_from_picks_device -- a column of the track (and
// with beams > 1 a row of the output) is one talker, not a loudness rank: it follows the pick within gate_deg of where its talker was
// last heard, holds through pauses (min_hits 2, max_coast 8), and a new talker gets a free column.  After the publications one line per
// column on stdout, "column <c> <last_angle_deg or -> <share of blocks in which its talker was heard>".
// in.wav: a multichannel WAV file (its first n_mics channels, its sample rate).  Trailing periods that do not fill a block are dropped.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/bfcore.h"

#define CK(call)                                                                        \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                  \
            return 1;                                                                   \
        }                                                                               \
    } while (0)
#define BF(call)                                                                        \
    do {                                                                                \
        int rc_ = (call);                                                               \
        if (rc_ != BF_OK) {                                                             \
            fprintf(stderr, "%s: %s (%s)\n", #call, bf_strerror(rc_), bf_last_error(nullptr)); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 8) {
        fprintf(stderr,
                "usage: %s <config.yaml> <in.wav> <out.wav> <frames_per_block> <angle_lo> <angle_hi> <angle_step> [k=2] [min_sep_deg=30] "
                "[rel_floor=0] [min_peak=0] [freq_lo=100] [freq_hi=16000] [beams=1] [capon|music[:n]] [identity [gate_deg=20]]\n",
                argv[0]);
        return 2;
    }
    bf_config cfg;
    if (bf_config_init(&cfg, BF_LCMV) != BF_OK || bf_config_load_yaml(&cfg, argv[1]) != BF_OK) {
        fprintf(stderr, "bad config %s\n", argv[1]);
        return 2;
    }
    const int W = atoi(argv[4]);
    const double lo = atof(argv[5]), hi = atof(argv[6]), step = atof(argv[7]);
    const int k = argc > 8 ? atoi(argv[8]) : 2;
    const double min_sep = argc > 9 ? atof(argv[9]) : 30.0, rel_floor = argc > 10 ? atof(argv[10]) : 0.0;
    const double min_peak = argc > 11 ? atof(argv[11]) : 0.0;
    const double freq_lo = argc > 12 ? atof(argv[12]) : 100.0, freq_hi = argc > 13 ? atof(argv[13]) : 16000.0;
    const int beams = argc > 14 ? atoi(argv[14]) : 1;
    if (beams > 1) cfg.lcmv_out_beams = beams;
    const char *method = "capon";
    bool identity = false;
    double gate = 20.0;
    for (int i = 15; i < argc; ++i) {
        if (strcmp(argv[i], "identity") != 0) {
            method = argv[i];
            continue;
        }
        identity = true;
        if (i + 1 < argc) {  // a number behind it is the gate
            char *end = nullptr;
            const double v = strtod(argv[i + 1], &end);
            if (end != argv[i + 1] && *end == '\0') {
                gate = v;
                ++i;
            }
        }
    }
    const bool music = strncmp(method, "music", 5) == 0 && (method[5] == '\0' || method[5] == ':');
    if (!music && strcmp(method, "capon") != 0) {
        fprintf(stderr, "bad method %s (capon, music or music:<n>)\n", method);
        return 2;
    }
    if (W < 1 || beams < 1 || !(step > 0) || !(hi > lo) || (hi - lo) / step > BF_DOA_MAX_ANGLES) {
        fprintf(stderr, "bad block length or grid\n");
        return 2;
    }
    std::vector<double> grid((size_t)std::ceil((hi - lo) / step));
    for (size_t i = 0; i < grid.size(); ++i) grid[i] = lo + (double)i * step;
    const int A = (int)grid.size(), M = cfg.n_mics, H = cfg.hop, n_cols = cfg.n_interf + 1;

    float *planar = nullptr;
    int ch = 0, rate = (int)cfg.sample_rate;
    size_t n = 0;
    const int rc = bf_wav_read(argv[2], &planar, &ch, &n, &rate);
    if (rc != BF_OK || ch < M) {
        fprintf(stderr, "cannot read %s (%s)\n", argv[2], bf_strerror(rc));
        bf_wav_free(planar);
        return 2;
    }
    cfg.sample_rate = rate;
    const size_t nb = n / ((size_t)H * W), frames = nb * W, len = frames * (size_t)H;
    std::vector<float> x((size_t)M * len), y((size_t)beams * len);  // y: [beams][len]
    for (int m = 0; m < M; ++m) memcpy(&x[(size_t)m * len], planar + (size_t)m * n, len * sizeof(float));  // the first n_mics channels
    bf_wav_free(planar);

    bf_handle *node = nullptr;
    bf_doa *doa = nullptr;
    BF(bf_create(&cfg, &node));
    BF(bf_ctrack_set_angles(node, grid.data(), A));
    BF(bf_doa_create(&cfg, grid.data(), A, freq_lo, freq_hi, W, &doa));
    BF(bf_doa_set_method(doa, music ? BF_DOA_MUSIC : BF_DOA_CAPON));
    if (music) {
        const int n_src = method[5] == ':' ? atoi(method + 6) : (k < M - 1 ? k : M - 1);
        BF(bf_doa_set_sources(doa, n_src));  // refuses what is outside 1 .. n_mics - 1
    }

    std::vector<double> maps(nb * A);
    std::vector<int32_t> picks(nb * k), carry(n_cols, -1);
    std::vector<int32_t> state((size_t)n_cols * BF_ASSIGN_STATE_INTS, -1), active(identity ? nb * n_cols : 0);  // identity only
    if (nb) {
        hipStream_t s;
        float *x_dev, *y_dev;
        double *map_dev, *grid_dev;
        int32_t *picks_dev, *carry_dev, *track_dev, *state_dev = nullptr, *active_dev = nullptr;
        CK(hipStreamCreate(&s));
        CK(hipMalloc((void **)&x_dev, x.size() * sizeof(float)));
        CK(hipMalloc((void **)&y_dev, y.size() * sizeof(float)));
        CK(hipMalloc((void **)&map_dev, maps.size() * sizeof(double)));
        CK(hipMalloc((void **)&grid_dev, grid.size() * sizeof(double)));
        CK(hipMalloc((void **)&picks_dev, picks.size() * sizeof(int32_t)));
        CK(hipMalloc((void **)&carry_dev, carry.size() * sizeof(int32_t)));
        CK(hipMalloc((void **)&track_dev, frames * n_cols * sizeof(int32_t)));
        CK(hipMemcpyAsync(x_dev, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(grid_dev, grid.data(), grid.size() * sizeof(double), hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(carry_dev, carry.data(), carry.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (identity) {
            CK(hipMalloc((void **)&state_dev, state.size() * sizeof(int32_t)));
            CK(hipMalloc((void **)&active_dev, active.size() * sizeof(int32_t)));
            CK(hipMemcpyAsync(state_dev, state.data(), state.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        }
        // the loop
        BF(bf_doa_process_device(doa, x_dev, frames, map_dev, nullptr, s));
        BF(bf_doa_pick_device(map_dev, grid_dev, A, 1, nb, k, min_sep, rel_floor, picks_dev, s));
        if (identity)
            BF(bf_ctrack_assign_device(picks_dev, map_dev, grid_dev, A, k, 1, nb, W, 1, min_peak, gate, 2, 8, n_cols, state_dev, track_dev,
                                       active_dev, s));
        else BF(bf_ctrack_from_picks_device(picks_dev, map_dev, A, k, 1, nb, W, 1, min_peak, n_cols, carry_dev, track_dev, s));
        BF(bf_process_batch_device_ctracked(node, x_dev, frames, y_dev, nullptr, track_dev, n_cols, s));
        CK(hipMemcpyAsync(y.data(), y_dev, y.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(maps.data(), map_dev, maps.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(picks.data(), picks_dev, picks.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (identity) {
            CK(hipMemcpyAsync(state.data(), state_dev, state.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            CK(hipMemcpyAsync(active.data(), active_dev, active.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        CK(hipStreamSynchronize(s));
        for (void *p : {(void *)x_dev, (void *)y_dev, (void *)map_dev, (void *)grid_dev, (void *)picks_dev, (void *)carry_dev, (void *)track_dev,
                        (void *)state_dev, (void *)active_dev})
            (void)hipFree(p);
        (void)hipStreamDestroy(s);
    }
    bf_doa_destroy(doa);
    bf_destroy(node);

    size_t n_pub = 0;
    for (size_t b = 0; b < nb; ++b) {
        const int32_t *p = &picks[b * k];
        if (p[0] < 0 || p[0] >= A || maps[b * A + p[0]] < min_peak) continue;
        printf("%zu %.17g", b, grid[p[0]]);
        for (int j = 1; j < k; ++j)
            if (p[j] >= 0 && p[j] < A) printf(" %.17g", grid[p[j]]);
        printf("\n");
        ++n_pub;
    }
    for (int c = 0; identity && c < n_cols; ++c) {  // where every column's talker was last heard, and how often it was
        const int32_t last = state[(size_t)c * BF_ASSIGN_STATE_INTS + 3];
        size_t heard = 0;
        for (size_t b = 0; b < nb; ++b) heard += active[b * n_cols + c] != 0;
        if (last >= 0 && last < A) printf("column %d %.17g %.6f\n", c, grid[last], nb ? (double)heard / (double)nb : 0.0);
        else printf("column %d - %.6f\n", c, nb ? (double)heard / (double)nb : 0.0);
    }
    for (int r = 0; r < beams; ++r) {
        char name[4096];
        if (beams > 1) snprintf(name, sizeof(name), "%s.%d.wav", argv[3], r);
        else snprintf(name, sizeof(name), "%s", argv[3]);
        bf_wav_writer *w = nullptr;
        if (bf_wav_writer_open(name, (int)cfg.sample_rate, &w) != BF_OK) {
            fprintf(stderr, "cannot write %s\n", name);
            return 2;
        }
        for (size_t t = 0; t < frames; ++t) bf_wav_writer_write(w, &y[(size_t)r * len + t * (size_t)H], (size_t)H);  // one sf_write_float per callback
        bf_wav_writer_close(w);
    }
    fprintf(stderr, "lcmv: %zu callbacks in blocks of %d, %d mics, %d interferers, %d angles, %zu publications -> %s\n", frames, W, M,
            cfg.n_interf, A, n_pub, argv[3]);
    return 0;
}
