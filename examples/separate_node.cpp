// separate_node.cpp -- geometric source separation with every source written out: one WAV per separated source.
//
//   separate_node <beamform_config.yaml> <in.wav|in.f32> <out_prefix> [n_sources] [postfilter]
//
// The reference's gss node computes all separated sources every frame and publishes the first (gss.cpp:120-121).  Here the
// config's look direction (initial_angle) and its interferers (angle_interf<k>) are the sources; n_sources (default: the yaml's
// gss_out_sources, else 1 + interferers) of them are written to <out_prefix>0.wav (the look direction), <out_prefix>1.wav
// (angle_interf1), ... as rosjack's write_file option writes its one stream: mono PCM16 (rosjack.cpp:189-210, 404-409).
// A trailing `postfilter` (or the yaml's gss_postfilter: 1) runs the multi-source post-filter over the separated sources before they are
// written (bf_config.gss_postfilter: stationary noise, the leak of the other sources and reverberation come off each magnitude).
// in.f32: planar float32 [n_mics][n_samples]; in.wav: a multichannel WAV file (its first n_mics channels, its sample rate).
// The whole file is one batch (bf_process_batch); a trailing partial period is dropped, as JACK would never deliver it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/bfcore.h"

static bool ends_with(const char *s, const char *suf) {
    const size_t a = strlen(s), b = strlen(suf);
    return a >= b && !strcmp(s + a - b, suf);
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <config.yaml> <in.wav|in.f32> <out_prefix> [n_sources] [postfilter]\n", argv[0]);
        return 2;
    }
    bf_config cfg;
    if (bf_config_init(&cfg, BF_GSS) != BF_OK || bf_config_load_yaml(&cfg, argv[1]) != BF_OK) {
        fprintf(stderr, "bad config %s\n", argv[1]);
        return 2;
    }
    if (argc > 4 && !strcmp(argv[argc - 1], "postfilter")) {
        cfg.gss_postfilter = 1;
        --argc;
    }
    if (argc > 4) cfg.gss_out_sources = atoi(argv[4]);
    if (cfg.gss_out_sources < 1) cfg.gss_out_sources = cfg.n_interf + 1;
    const int R = cfg.gss_out_sources, M = cfg.n_mics;
    float *planar = nullptr;
    int ch = 0, rate = (int)cfg.sample_rate;
    size_t n = 0;
    const bool wav = ends_with(argv[2], ".wav");
    int rc = wav ? bf_wav_read(argv[2], &planar, &ch, &n, &rate) : bf_planar_f32_read(argv[2], M, &planar, &n);
    if (rc != BF_OK || (wav && ch < M)) {
        fprintf(stderr, "cannot read %s (%s)\n", argv[2], bf_strerror(rc));
        bf_wav_free(planar);
        return 2;
    }
    if (wav) cfg.sample_rate = rate;
    const size_t frames = n / (size_t)cfg.hop, len = frames * (size_t)cfg.hop;
    std::vector<float> x((size_t)M * len), y((size_t)R * len);
    for (int m = 0; m < M; ++m) memcpy(&x[(size_t)m * len], planar + (size_t)m * n, len * sizeof(float));  // the first n_mics channels
    bf_wav_free(planar);
    bf_handle *h = nullptr;
    rc = bf_create(&cfg, &h);
    if (rc == BF_OK && frames) rc = bf_process_batch(h, x.data(), frames, y.data());  // y = [source][frames * hop]
    if (rc != BF_OK) {
        fprintf(stderr, "gss: %s (%s)\n", bf_strerror(rc), bf_last_error(h));
        bf_destroy(h);
        return 1;
    }
    bf_destroy(h);
    for (int r = 0; r < R; ++r) {
        const std::string path = std::string(argv[3]) + std::to_string(r) + ".wav";
        bf_wav_writer *w = nullptr;
        if (bf_wav_writer_open(path.c_str(), (int)cfg.sample_rate, &w) != BF_OK) {
            fprintf(stderr, "cannot write %s\n", path.c_str());
            return 2;
        }
        for (size_t k = 0; k < frames; ++k)  // one sf_write_float per callback, as the reference writes its stream
            bf_wav_writer_write(w, &y[(size_t)r * len + k * (size_t)cfg.hop], (size_t)cfg.hop);
        bf_wav_writer_close(w);
    }
    fprintf(stderr, "gss: %zu callbacks, %d mics, %d interferers, %d sources%s -> %s0..%d.wav\n", frames, M, cfg.n_interf, R,
            cfg.gss_postfilter ? ", post-filtered" : "", argv[3], R - 1);
    return 0;
}
