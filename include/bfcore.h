/*
 * bfcore.h -- C ABI of the MI355X beamforming core (libbfcore.so).
 *
 * Drop-in boundary for the per-callback hot path of balkce/beamform:
 *   STFT (sqrt-Hann, 50 % hop) -> per-bin complex weighting -> ISTFT + overlap-add
 * as driven by every node's jack_callback (das, mvdr, lcmv, gss, phase, phasempf).
 * Plain C types only; device buffers are raw HIP device pointers.
 *
 * Each entry point names the reference interface it replaces (file:line relative
 * to the reference root).  All functions return 0 on success or a negative
 * BF_E* code; nothing here exits the process, prints, or keeps global state
 * (the reference keeps everything in file-scope globals, util.h:24-50).
 *
 * There is NO CPU fallback: bf_create fails with BF_ENODEV when no HIP device is
 * usable.
 */
#ifndef BFCORE_H
#define BFCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BF_MAX_MICS 32
#define BF_MAX_INTERF 15 /* beamform_config.yaml:43-57 lists angle_interf1..15 */

/* Which node's apply_weights() runs between the STFT and the ISTFT. */
enum bf_algo {
    BF_DAS = 0,      /* das.cpp:47-70 */
    BF_MVDR = 1,     /* mvdr.cpp:62-115 */
    BF_LCMV = 2,     /* lcmv.cpp:88-140 */
    BF_GSS = 3,      /* gss.cpp:96-156 */
    BF_PHASE = 4,    /* phase.cpp:70-134 */
    BF_PHASEMPF = 5, /* phasempf.cpp:193-302 + :331-334 */
    BF_GSC = 7,      /* gsc.cpp:54-197: per-microphone phase alignment (STFT -> conj(w_m) -> ISTFT, do_overlap_bymic) followed by
                        the sample-serial float32 NLMS sidelobe canceller; uses the gsc_* fields */
    BF_MCRA = 6      /* mcra.cpp:64-155: single-channel MCRA noise subtraction (channel 0 only; uses mcra_*, out_amp,
                        out_only_noise) */
};

enum bf_error {
    BF_OK = 0,
    BF_EINVAL = -22,   /* bad argument / inconsistent config */
    BF_ENOMEM = -12,   /* host or device allocation failed */
    BF_ENODEV = -19,   /* no usable HIP device (no CPU fallback exists) */
    BF_ENOSYS = -38,   /* algorithm/variant not built into this library */
    BF_EIO = -5,       /* HIP runtime error; see bf_last_error() */
    BF_ENOENT = -2     /* config file not found */
};

/* How bf_process_batch* lays out multichannel input. */
enum bf_layout {
    BF_PLANAR = 0,      /* [stream][mic][sample]  -- what JACK hands the callback (rosjack.cpp:538-547) */
    BF_INTERLEAVED = 1  /* [stream][sample][mic]  -- interleaved frame buffer.  das in double (BF_DAS_F64, period 512): with 2, 4 or 8 microphones
                           the kernel transposes hop by hop into per-block rings (160 MB of device scratch on a 256-CU chip, allocated on first
                           use, kept); with 3, 5, 6 or 7 the batch is transposed on the device into a planar scratch of the batch's size in front
                           of the planar kernel; every other node reads the layout directly */
};

/* Arithmetic of the das node.  The reference computes in std::complex<double> end to end (das.cpp:16-24,47-70): BF_DAS_F64 is the
 * default (bf_config_init) and what the bench headline measures.  Other algorithms always compute in double. */
enum bf_das_impl {
    BF_DAS_FUSED_F32 = 0, /* opt-in: one fused kernel in fp32 arithmetic (narrower than the reference's; 1.5e-7 from it on signals of
                             even level, inside the 1e-5 bar; beside silence, faint stretches or NaN: the G-frame contract at
                             bf_process_batch); also the only das path with register-resident kernels at JACK periods other than 512 and with
                             look directions that share their forward transforms */
    BF_DAS_F64 = 1        /* default: double arithmetic like das.cpp.  Period 512, <= 8 microphones, one look direction, no spectrum
                             dump: ONE launch of the frame-pair kernel (das_f64_pair_kernel on planar input; on [sample][mic] input
                             das_f64_ring_kernel for 2, 4 or 8 microphones, a transposition in front of das_f64_pair_kernel otherwise).
                             The frame-pair kernel needs a second microphone and the reference's unit weight row 0: without them
                             [sample][mic] input takes the microphone-pair kernel das_f64_w64_kernel, still one launch, and planar
                             input the chain.  Anything else runs that chain, STFT -> per-bin kernel -> ISTFT, which can dump the
                             full N-bin spectrum */
};

/* Arithmetic of what lies between the transforms (every node computes its per-bin stage in double).
 * BF_PRECISION_REFERENCE (bf_config_init's default): nothing is narrower than the reference's std::complex<double>: spectra cross HBM as
 * complex doubles, the backward transform runs in double (mvdr.cpp:76-115 between fftw_execute(x_forward) and fftw_execute(y_inverse)).
 * BF_PRECISION_MIXED (opt-in, throughput): mvdr / lcmv park their spectra as 12-byte elements (36-bit mantissa: < 1e-10 on the solved
 * spectrum at cond(R) = 3e4) and every node whose per-bin stage can emit float rows runs the backward transform in fp32 (1.1e-7 on the
 * output instead of bit-identity with the double path).  Both are inside the 1e-5 parity bar; only REFERENCE is the reference's arithmetic. */
enum bf_precision {
    BF_PRECISION_REFERENCE = 0,
    BF_PRECISION_MIXED = 1
};

/*
 * Everything a node reads from the ROS parameter server
 * (handle_params util.h:52-134 + each node's *_handle_params) plus the two
 * JACK-server facts rosjack_create() records (rosjack.cpp:131-134).
 * bf_config_init() fills the launch-file values.
 */
typedef struct bf_config {
    int algo;                      /* enum bf_algo */
    int n_mics;                    /* number_of_microphones (util.h:122) */
    int hop;                       /* rosjack_window_size = the JACK period (rosjack.cpp:131); fft_win = 2*hop (util.h:261).
                                      Any power of two from 64 to 4096 (what jackd -p accepts in that range).  512 is the tuned
                                      shape (in-register FFT-1024 kernels); 64 ... 256 and 1024 run on the same register-resident
                                      machinery (several short frames per transform, or two FFT-1024 per long frame) for das
                                      (with the BF_DAS_FUSED_F32 opt-in: one fused fp32 kernel) and for the fp64 bin pipeline of das in double and of every other node;
                                      2048 and 4096 on LDS-staged transforms (radix-4 autosort; radix-2 in place at 4096) */
    double sample_rate;            /* rosjack_sample_rate */
    double mic_x[BF_MAX_MICS];     /* RAW mic<i>.x / .y from beamform_config.yaml (util.h:82-92) */
    double mic_y[BF_MAX_MICS];
    double theta;                  /* initial_angle, degrees (util.h:68-73) */
    int n_interf;                  /* number of angle_interf<k> with |angle| <= 180 (util.h:101-113) */
    double interf_angle[BF_MAX_INTERF];
    int verbose;
    /* mvdr / lcmv / gss */
    int past_windows;              /* mvdr.cpp:151-157 */
    double freq_mag_threshold;     /* mvdr.cpp:159-164 */
    double freq_max, freq_min;     /* mvdr.cpp:166-178 */
    double out_amp;                /* mvdr.cpp:180-185 (also phasempf.cpp:448-453) */
    double interf_angle_threshold; /* lcmv.cpp:212-217 */
    double mu, lambda_;            /* gss.cpp:219-231 */
    /* phase */
    double min_phase;              /* phase.cpp:169-175, phasempf.cpp:359-365 */
    double mag_mult, mag_threshold;/* phase.cpp:177-189 */
    /* phasempf */
    double min_mag;                /* phasempf.cpp:367-372 */
    int smooth_size;               /* phasempf.cpp:374-383 */
    double mcra_alphaS, mcra_alphaD, mcra_alphaD2, mcra_delta; /* phasempf.cpp:385-411 */
    int mcra_L;                    /* phasempf.cpp:413-418 */
    double mpf_alphaS, mpf_eta, mpf_rev_gamma, mpf_rev_delta;  /* phasempf.cpp:420-446 */
    double noise_floor;            /* phasempf.cpp:455-460 */
    int out_only_noise, out_only_mcra; /* phasempf.cpp:462-474 */
    /* build-specific (no reference counterpart) */
    int device;                    /* HIP device ordinal */
    int n_streams;                 /* independent audio streams per batch (each = one reference node's state) */
    int layout;                    /* enum bf_layout for bf_process_batch* input */
    int das_impl;                  /* enum bf_das_impl; bf_config_init: BF_DAS_F64 (the reference's arithmetic) */
    int precision;                 /* enum bf_precision; bf_config_init: BF_PRECISION_REFERENCE */
    int n_dirs;                    /* look directions evaluated per input stream from the SAME samples (0/1 = one, the
                                      reference node).  Output stream index = stream * n_dirs + dir.  Every node except mcra
                                      (no look direction) and gsc; gss / phasempf keep their recursive state per beam.
                                      das (fp32, planar input, <= 8 microphones): from 6 directions on the forward transforms
                                      of a frame are computed once and shared by the beams (das.cpp:51-63 transforms once).
                                      SURVEY 8(e) "look directions" / 8(f) row 4 */
    /* gsc (gsc.cpp:199-256, launch/gsc.launch:6-11); write_mu is file I/O and not part of the path */
    int gsc_use_vad;
    double gsc_vad_threshold, gsc_mu0, gsc_mu_max;
    int gsc_filter_size;           /* 1..256 */
    /* (new fields are appended: a caller built against an older header that zeroes the struct keeps its meaning) */
    int gss_out_sources;           /* gss: separated sources emitted per beam, R (0/1 = one, the reference node; up to BF_MAX_INTERF + 1).
                                      gss.cpp computes this_yf = sep_matrix[j] * in_fft.col(j) every frame and keeps this_yf(0) alone
                                      ("outputting only the first source of interest", gss.cpp:120-121); with R > 1 each beam (input
                                      stream x look direction) yields R output streams, index (stream * n_dirs + dir) * R + r, and
                                      row r is this_yf(r): in band with the gate open (sep_matrix[j] x)(r) for r < 1 + interferers;
                                      gate closed 0.01 X_0 for r = 0 and 0 above (gss.cpp:139-141); out of band, and for r beyond the
                                      current source count, 0.  Every row takes row 0's backward transform, window, out_amp and
                                      overlap-add (gss.cpp:148-155), each with its own tail.  R is fixed at create;
                                      bf_set_interference may change the source count underneath: a row that stops existing goes
                                      silent once its tail has been added, a row that starts existing begins from the
                                      re-initialised sep_matrix = weights^H like every other (gss.cpp:90-93).  Wherever this header
                                      counts output streams as n_streams * n_dirs (y, spectrum_dev, bf_stream_rms, bf_process_hop,
                                      the state blob's tails), read n_streams * n_dirs * R.  Row 0 is the R = 1 node's output bit
                                      for bit; R = 1 runs the very kernels it always ran.  Above 1 with another algo: BF_EINVAL */
    int gss_postfilter;            /* gss: the multi-source post-filter of Valin et al. 2007 over the separated sources (0 = off, the
                                      default and the reference node; 1 = on; anything else, or non-zero with another algo:
                                      BF_EINVAL).  With R = max(1, gss_out_sources) rows per beam and S_t = 1 + interferers sources
                                      in force at frame t, every row r < min(S_t, R) is replaced, bin by bin, by the output of the
                                      reference's MPF block (phasempf.cpp:140-191, 254-295: MCRA noise + leak of the other sources +
                                      reverberation, taken off the magnitude) fed with
                                        soi  = Y_r[t]                                  (the row as gss stores it with the filter off)
                                        int2 = sum over r' != r, r' < min(S_t, R), of |Y_r'[t][j]|^2, in ascending r'
                                      and soi2[0] = int2[0] = 0.  Every quirk of that block is kept as phasempf has it (0.75 soi2 at
                                      bins 1 and N-1, Sf[0] = |soi[0]|, kq = 1 - rev_gamma / rev_delta, the alphaD2 / alphaD pair,
                                      output bin 0 = 0, out_only_noise, out_only_mcra).  One difference: out_amp is NOT applied
                                      inside the filter -- the magnitude is |soi| - Lambda, or noise_floor when that is negative --
                                      and gss's backward path applies out_amp as on every row.  Rows r >= min(S_t, R) are not
                                      touched in frame t: they stay exact zeros and their state does not advance.  Parameters: the
                                      mcra_*, mpf_*, noise_floor, out_only_noise and out_only_mcra fields above (bf_config_init:
                                      phasempf.launch's values).  State: every output row has its own seven vectors and its own
                                      current_L / first_L pair (phasempf's per-stream layout); it carries across frames, batches and
                                      bf_process_hop calls, is NOT restarted by bf_set_theta or bf_set_interference (those restart
                                      sep_matrix; the noise estimate is about the room), is zeroed by bf_reset and travels in the
                                      state blob, which a handle without the filter refuses (and the other way round).  The
                                      spectrum dump shows the filtered rows; R = 1 filters row 0 with int2 = 0 */
    int lcmv_out_beams;            /* lcmv: beams emitted per input stream and look direction, R (0/1 = one, the reference node; up to
                                      BF_MAX_INTERF + 1).  lcmv.cpp:116 forms W = R^-1 C (C^H R^-1 C)^-1 and keeps W.col(0)
                                      (lcmv.cpp:119); column c of W is the beam that looks at constraint column c with unit gain and
                                      puts nulls on every other column.  With R > 1 each beam yields R output streams, index
                                      (stream * n_dirs + dir) * R + r, and with S_t = 1 + interferers columns in force at frame t
                                        row r < S_t   is, frame by frame, the output of the reference's node with `angle` and
                                                      interference_angles[r-1] exchanged and the same past frames (W(C P) = W(C) P for
                                                      a column permutation P): out of band 0; gate closed 0.01 X_0 on EVERY such row
                                                      (lcmv.cpp:121 -- unlike gss, whose rows >= 1 are 0 behind a closed gate);
                                                      microphone 0's entry of each column as the handle has it (quirk Q3 on all columns
                                                      alike); the frames the reference turns into NaN (cold start, singular R) are
                                                      non-finite on the row; out_amp, window and overlap-add as row 0, own tail
                                        row r >= S_t  exact zeros in the spectrum; in time exact zeros once its tail has been added.
                                      R is fixed at create; a structural bf_set_interference may change S between batches: a row
                                      that starts to exist simply starts (there is no recursive state to restart).  In a
                                      column-tracked batch (bf_process_batch_device_ctracked) row r of a frame looks at whatever
                                      angle column r of that frame's track names: follow K + 1 talkers, get K + 1 signals.
                                      Wherever this header counts output streams as n_streams * n_dirs, or says "read n_streams *
                                      n_dirs * R" for gss (y, spectrum_dev, bf_stream_rms, the [n_dirs][R][nframes] of
                                      bf_process_hop, the state blob), the same holds here.  The state blob holds one overlap-add
                                      tail per output row and nothing else new; a blob is accepted only by a handle with the same
                                      R.  Row 0 is the R = 1 node's output (bit for bit with at least one interferer in force;
                                      without any, to rounding); R = 1 runs the very kernels it always ran.  Above 1 with another
                                      algo, negative, above BF_MAX_INTERF + 1, or above 1 together with gss_out_sources > 1:
                                      BF_EINVAL.  bf_shard_run with R > 1: BF_EINVAL (its feed buffer is one stream) */
} bf_config;
#define BF_MAX_DIRS 64

typedef struct bf_handle bf_handle;

/* Library identification / diagnostics. */
const char *bf_version(void);
const char *bf_strerror(int code);
/* Last HIP/runtime error text recorded on this handle (or globally when h==NULL). */
const char *bf_last_error(const bf_handle *h);
/* Number of HIP devices visible; <= 0 means the product cannot run. */
int bf_device_count(void);

/* Launch-file defaults for `algo` and the uncommented geometry of
 * beamform_config.yaml:15-17 (aira3).  Replaces the getParam fallbacks. */
int bf_config_init(bf_config *cfg, int algo);
/* Parse a beamform_config.yaml-style file (util.h:61-113 keys: verbose,
 * initial_angle, mic<i>: {id,x,y[,z]}, angle_interf<k>) plus the flat
 * per-node keys the launch files set (past_windows, freq_max, ...). */
int bf_config_load_yaml(bf_config *cfg, const char *path);
/* Same parser on an in-memory string. */
int bf_config_parse_yaml(bf_config *cfg, const char *text);

/* main(): prepare_overlap_and_add + buffer/plan allocation + update_weights(true)
 * (das.cpp:119-140 and the same block in every node). */
int bf_create(const bf_config *cfg, bf_handle **out);
void bf_destroy(bf_handle *h);

/* theta_roscallback: angle = msg->data; update_weights() (das.cpp:94-99).
 * Thread-safe against a concurrent bf_process_*: takes effect at the next
 * hop/batch (the reference updates in place with no lock). */
int bf_set_theta(bf_handle *h, double degrees);
/* Look-direction batch: direction `dir` (0 <= dir < n_dirs) of every input stream gets its own /theta;
 * bf_set_theta() is bf_set_theta_dir(h, 0, deg).  bf_set_thetas sets directions 0..n-1 with one table rebuild.
 * Every direction starts at bf_config.theta. */
int bf_set_theta_dir(bf_handle *h, int dir, double degrees);
int bf_set_thetas(bf_handle *h, const double *degrees, int n);
/* Root-mean-square of each output stream of a batch that is resident on the device (y as written by
 * bf_process_batch_device): rms_host[n_streams * n_dirs].  This is the quantity the reference's theta controllers
 * steer on (scripts/energy2theta.py:23-27 get_energy_from_list), so "publish theta, wait, measure" becomes
 * "evaluate n_dirs candidates in one batch and pick". */
int bf_stream_rms(bf_handle *h, const float *y_dev, size_t n_frames, double *rms_host, void *hip_stream);

/* ---- direction-of-arrival maps: a source for /theta (SRP-PHAT over das's own beams) ---------------------------------------------
 * The reference steers only when something publishes /theta (README "The direction of interest ... can be changed on-the-fly by
 * writing to the topic /theta"); its publishers are the gradient scripts (scripts/energy2theta*.py).  bf_doa is a stream operator on
 * the same multichannel input as a bf_handle that returns, per block of W frames, the PHAT-weighted steered response power of every
 * candidate angle (Valin et al. 2007) and the index of the best one.
 *   Frames: frame t of a stream is [hop t-1 | hop t] times the periodic sqrt-Hann window; hop -1 is zeros after create / reset and the
 *   previous call's last hop otherwise (util.h:272-302, as in every node).  X_m(k) = forward DFT of microphone m's windowed frame (N = 2 hop).
 *   PHAT:  X^_m(k) = X_m(k) / |X_m(k)| when |X_m(k)| > eps, else 0 (eps: bf_doa_set_phat_floor, default 1e-10).
 *   Band:  K = the bins k in 1 .. N/2-1 with freq_lo <= f_k <= freq_hi, f_k the frequency vector das steers with (quirk Q1 included:
 *          f_{N/2-1} = sample_rate / 2).  An empty K is BF_EINVAL.
 *   Weights: w_m(theta, k) is exactly das's update_weights(ini = true) column for angle theta (das.cpp:27-45: microphone 0's row is 1,
 *          the reference's delay formula): the angle of a peak is the value to pass to bf_set_theta of a das handle (das applies conj(w)).
 *   Map:   P[s][b][d] = 1 / (W |K| M^2) * sum_{t in block b} sum_{k in K} | sum_m conj(w_m(theta_d, k)) X^_{s,m,t}(k) |^2, in [0, 1].
 *   Peak:  peak[s][b] = argmax_d P[s][b][d], the lowest d on ties.
 * Arithmetic is in double from the spectra to the map.  Map and peak bytes do not depend on how a stream is cut into calls (at block
 * boundaries), on the internal chunking, or on the launch: every sum has one fixed order.  A microphone whose windowed frame is exactly
 * zero contributes X^ = 0 in every bin.  No guarantee: a bin with |X| within rounding of eps may land on either side (the spectra of two
 * microphones share one complex transform: a microphone 2^-40 below its pair partner keeps only its leading bits); on a linear array
 * theta and its mirror image through the array axis have the same map value (front/back ambiguity), so the lower index wins the peak.
 * Scratch: about 256 MiB per handle for spectra and partial sums (allocated on the first batch, kept), plus the steering table
 * (angles x |K| x M complex doubles, at most 512 MiB: larger is BF_EINVAL).  One batch at a time per handle. */
#define BF_DOA_MAX_ANGLES 1024
typedef struct bf_doa bf_doa;
/* cfg: reads n_mics (2..BF_MAX_MICS), mic_x/mic_y, hop, sample_rate, n_streams, layout, device; ignores algo and the node parameters.
 * Bad arguments are BF_EINVAL, checked before any device work; without a HIP device BF_ENODEV. */
int bf_doa_create(const bf_config *cfg, const double *angles_deg, int n_angles, double freq_lo, double freq_hi,
                  int frames_per_block, bf_doa **out);
int bf_doa_set_phat_floor(bf_doa *d, double eps);            /* >= 0; default 1e-10 */
/* ---- the Capon (MVDR) map: the handle's second method --------------------------------------------------------------------------------
 * SRP-PHAT localises one source: with 8 or fewer microphones the strongest source's sidelobes outrank the weaker sources.  The Capon
 * spectrum (Capon 1969) keeps them apart; its peaks feed bf_set_theta and bf_set_interference (controllers.follow_sources).
 *   Frames, X_m(k), the band K and the weights w_m(theta, k) are exactly those above (microphone 0's row is 1).  There is no PHAT
 *   normalisation and the PHAT floor is ignored.
 *   Covariance: R_{s,b}(k) = sum_{t in block b, ascending} X_{s,t}(k) X_{s,t}(k)^H (M x M), tau = trace R.
 *   Response: tau > 0:  R~ = R / tau + (delta / M) I,  c_d(k) = M / ((1 + delta) a_d^H R~^-1 a_d),  a_d = w(theta_d, k);  else c_d(k) = 0.
 *           delta: the diagonal loading (bf_doa_set_loading, default 1e-3).
 *   Map:   P[s][b][d] = 1 / |K| * sum_{k in K} c_d(k), in [0, 1]: c <= (1 + delta / M) / (1 + delta), reached by one frame X = a_d.
 *   Peak:  peak[s][b] = argmax_d P[s][b][d], the lowest d on ties.
 * Arithmetic is in double.  Map and peak bytes do not depend on how a stream is cut into calls (at block boundaries), on the internal
 * chunking, or on the launch: every sum has one fixed order.  Any frames_per_block >= 1 is valid: with W < M the covariance is
 * rank-deficient and the loading makes it definite.  A silent microphone needs no special case: its row of R is zero (or the packed
 * transform's 1e-16 residue of its pair partner).  No guarantee for non-finite input or for a subnormal tau.  All of 2 .. BF_MAX_MICS
 * microphones work; up to 8 the covariance and its factor stay in registers, above 8 they live in device memory (correct, not tuned;
 * its work space is part of the 256 MiB scratch).  A second steering table (the same size, bins innermost) is built when the method is
 * first selected.
 * Both setters take effect at the next bf_doa_process* call (one batch at a time per handle, as ever).  The history hop belongs to the
 * stream, not to the method: switching mid-stream continues the stream.  A handle that never calls them is the SRP-PHAT handle above. */
enum bf_doa_method { BF_DOA_SRP_PHAT = 0, BF_DOA_CAPON = 1, BF_DOA_MUSIC = 2 };
int bf_doa_set_method(bf_doa *d, int method);                /* default BF_DOA_SRP_PHAT; BF_EINVAL: NULL handle, unknown method */
int bf_doa_set_loading(bf_doa *d, double delta);             /* Capon's diagonal loading; default 1e-3; BF_EINVAL unless finite and 0 < delta <= 1 */
/* ---- the MUSIC map and the eigenvalue profile: the handle's third method ---------------------------------------------------------------
 * The Capon map's resolution is set by its loading and by how well a block's covariance is estimated, and nothing above says how many
 * sources a block holds.  MUSIC (Schmidt 1986) answers both from the eigendecomposition of the covariance the Capon map already forms:
 * the noise subspace gives a map whose peaks do not broaden with a loading, the eigenvalues show the number of sources
 * (controllers.count_sources).  Every consumer of a map (bf_doa_pick_device, bf_ctrack_from_picks_device, the follow_* loops) works on it.
 *   Frames, X_m(k), the band K and the steering columns a_d = w(theta_d, k) are exactly those above (microphone 0's row is 1, so
 *   a_d^H a_d = M).  There is no PHAT normalisation and no loading; the PHAT floor and the loading are ignored.
 *   Covariance: R_{s,b}(k) = sum_{t in block b, ascending} X X^H and tau = trace R, accumulated exactly as in Capon.
 *   tau > 0:  R^ = R / tau = sum_i lambda_i v_i v_i^H, lambda_1 >= ... >= lambda_M, v_i orthonormal;
 *             nu_d(k) = (1 / M) sum_{i > n} |v_i^H a_d|^2, n = bf_doa_set_sources (default 1).  This is the noise-subspace form, not
 *             1 - (the signal part), which would cancel where the map peaks.
 *   tau = 0:  nu_d(k) = 1 and every lambda_i(k) = 0.
 *   Map:   P[s][b][d] = mu / (mu + (1 / |K|) sum_{k in K} nu_d(k)), in (0, 1]; P = 1: a_d lies in the signal subspace in every bin.
 *          The order of the angles in a row is that of the classical incoherent wideband MUSIC spectrum 1 / sum_k a^H E_n E_n^H a for
 *          every mu; mu (bf_doa_set_music_floor, default 1e-2) only sets the contrast that rel_floor and min_peak see.
 *   Peak:  peak[s][b] = argmax_d P[s][b][d], the lowest d on ties.
 *   Profile: E[s][b][i] = (1 / |K|) sum_{k in K} lambda_i(k), i = 0 .. M-1, descending; each entry in [0, 1], a row sums to at most 1
 *          (to 1 where no bin of the block has tau = 0).
 * Arithmetic is in double throughout.  Every sum has one fixed order: map, peak and profile bytes do not depend on how a stream is cut
 * into calls (at block boundaries), on the internal chunking, or on the launch.  The eigendecomposition is a cyclic Jacobi iteration
 * with a fixed number of sweeps (beamform_amd/csrc/doa_eig.hpp: 8 up to 8 microphones, 11 above), so its bytes depend on the matrix
 * alone.  No guarantee where lambda_n - lambda_{n+1} is within 1e-6 of lambda_1: the cut between the subspaces is not defined there
 * (the profile still holds); none for non-finite input or for a subnormal tau.  Any frames_per_block >= 1 is valid (with W < n the
 * covariance has fewer than n nonzero eigenvalues: that is the clause above).  All of 2 .. BF_MAX_MICS microphones
 * work.  Up to 8 the covariance triangle and the eigenvectors stay in registers, one wavefront per SIMD (keeping the eigenvectors in LDS
 * instead would let two wavefronts share a compute unit where the registers let four: DESIGN.md); above 8 they live in device memory
 * (correct, not tuned; the work space is part of the 256 MiB scratch).  MUSIC shares Capon's second steering table.
 * Both setters take effect at the next bf_doa_process* call, are ignored by the other methods, and survive a method switch. */
int bf_doa_set_sources(bf_doa *d, int n_sources);            /* the signal subspace's dimension; default 1; BF_EINVAL unless 1 <= n_sources <= n_mics - 1 */
int bf_doa_set_music_floor(bf_doa *d, double mu);            /* default 1e-2; BF_EINVAL unless finite and 0 < mu <= 1 */
/* n_frames: a multiple of frames_per_block (else BF_EINVAL), 0 is a no-op.  x: as bf_process_batch_device reads it (cfg.layout).
 * map: [n_streams][n_frames/W][n_angles] double, peak: [n_streams][n_frames/W] int32; either may be NULL, not both.
 * Enqueued on hip_stream, no host sync.  HIP errors: BF_EIO, text in bf_last_error(NULL). */
int bf_doa_process_device(bf_doa *d, const float *x_dev, size_t n_frames, double *map_dev, int32_t *peak_dev, void *hip_stream);
/* The same on host buffers (staged through the device; returns when the results are in map_host / peak_host). */
int bf_doa_process(bf_doa *d, const float *x_host, size_t n_frames, double *map_host, int32_t *peak_host);
/* The two calls above plus the eigenvalue profile of the MUSIC method, eig: [n_streams][n_frames/W][n_mics] double.  Any of map, peak
 * and eig may be NULL, not all three (BF_EINVAL); a non-NULL eig on a handle whose method is not BF_DOA_MUSIC is BF_EINVAL.  With
 * eig = NULL they are the calls above for every method; those, on a MUSIC handle, write the map and the peak only. */
int bf_doa_process_device_eig(bf_doa *d, const float *x_dev, size_t n_frames, double *map_dev, int32_t *peak_dev, double *eig_dev,
                              void *hip_stream);
int bf_doa_process_eig(bf_doa *d, const float *x_host, size_t n_frames, double *map_host, int32_t *peak_host, double *eig_host);
int bf_doa_reset(bf_doa *d);                                  /* cold start: history hop zeroed (host-synchronous) */
void bf_doa_destroy(bf_doa *d);
/* interf_theta_roscallback (lcmv.cpp:258-309, gss.cpp:288-339): id is 1-based.  id <= current count updates that
 * interferer (and removes it when it lands within interf_angle_threshold of another one); id > count appends a
 * new interferer unless it is that close to an existing one.  As in the reference, a structural change rebuilds
 * the weight matrices zeroed and re-runs update_weights() without ini, so the reference-mic row is 0 afterwards
 * (quirk Q3).  Up to BF_MAX_INTERF interferers.  With more constraints than microphones (K + 1 > n_mics) the constraint
 * Gram matrix is singular and the reference's inverse() returns rounding noise: no parity is claimed there.
 * Takes effect at the next hop/batch. */
int bf_set_interference(bf_handle *h, unsigned id, double degrees);
/* Current number of interferers (interference_angles.size()). */
int bf_n_interferers(bf_handle *h);

/* Page-locked host memory for the host-buffer entry points: bf_process_batch copies from / to pageable memory at
 * about 30 GB/s (the runtime stages it), from / to these buffers at the PCIe rate (~55 GB/s) -- 34 vs 22 ms per
 * 65 536-frame 8-microphone batch.  No reference counterpart (JACK owns the reference's buffers). */
void *bf_host_alloc(size_t bytes);
void bf_host_free(void *p);

/* jack_callback body: do_overlap(in, out, nframes, apply_weights)
 * (das.cpp:72-92, util.h:289-314).  in = n_mics pointers to nframes float32
 * (host memory, as input_from_rosjack returns), out = nframes float32 (host).
 * nframes must equal cfg.hop.  Single-stream handles only; with n_dirs > 1 `out` receives [n_dirs][nframes], with gss_out_sources = R > 1
 * [n_dirs][R][nframes]. */
int bf_process_hop(bf_handle *h, const float *const *in, float *out, uint32_t nframes);

/* n_frames consecutive callbacks per stream in one call, host buffers.
 * x: layout per cfg.layout with n_frames*hop samples per mic;
 * y: [n_streams][n_frames*hop].  State carries over to the next call exactly
 * as consecutive callbacks would.
 * What is promised about silence, faint stretches and non-finite samples (tests/dynamics_cases.py states both contracts):
 *   The default precision -- das in double and every fp64 node -- per OUTPUT HOP, not per signal: no sample is non-zero where the
 *   reference writes an exact zero; every other finite hop is within 1e-5 of the reference on its own norm; the non-finite hops are
 *   the reference's (in the memoryless nodes, das and phase, a NaN or Inf sample in input hop h reaches hops h, h + 1, h + 2 and no
 *   others; the recursive nodes stay non-finite from there on, as the reference does).
 *   Rounding across cuts: the das kernels that take several frames of a batch through one transform (das in double: two; fp32 das at
 *   periods below 512: 1024 / (2 hop)) choose the frames by their position in the batch, so the same stream cut differently agrees to
 *   the last bits of the float output, not bit for bit.  For das in double the pairing rule below bounds how often a last bit
 *   differs: about 1e-6 per output hop on audio of even level, 3e-5 per hop at most next to a change of level -- one sample in 10^5 to
 *   10^6 hops; statistically, not a guarantee.  The frame-pair kernels (das in double, planar or [sample][mic] input)
 *   take frames t and t + 1 through one transform only if neither holds a non-finite sample and the largest magnitudes of their three
 *   hops are within 2^4 of each other (das_f64_plan.hpp das_f64_may_pair); otherwise each frame goes alone, at three times the cost for
 *   that pair.  The backward transform pairs two frames only if both are finite and within 2^20 of each other, and never behind das.
 *   Not covered: a faint but non-zero MICROPHONE beside loud ones.  Two microphones share a forward transform and the packed
 *   spectrum's storage, so a microphone more than about 2^20 below its partner loses its own low bits.
 *   BF_DAS_FUSED_F32 (fp32 opt-in): G frames may share a transform, G = 1024 / (2 hop) at periods below 512 and 2 otherwise, and the
 *   rounding error is 1e-7 of the LOUDEST of them.  So: |y - reference| <= 1e-5 of the largest reference magnitude within G + 1 hops
 *   on either side; exact zeros where the reference has them and every input hop within G + 1 hops is zero; the non-finite hops
 *   contain the reference's and lie within that set widened by G hops each way.  Its frames are chosen by their position in the
 *   batch, so the same stream cut differently agrees to the last bits of the float output, not bit for bit.
 *   An all-zero microphone: das and gsc keep the strict contract; mcra reads channel 0 only.  phase and phasempf take arg(+-0 +- 0i)
 *   of the dead channel -- the reference's own answer hangs on the signs of its FFT library's zeros -- and mvdr, lcmv and gss invert a
 *   singular covariance: no parity claim there.  phase, phasempf and gss run and stay finite where the reference does; for mvdr and lcmv
 *   the reference is NaN from frame 0 on, so nothing is promised, or tested, beyond that the node runs.  The same holds for phasempf
 *   on frames that are all zeros in every microphone (its output there is 1e-6 of the signal, not zero).
 * gss: from 57 streams on a batch runs one lane per (stream, bin) problem
 * (sums over the microphones as one FMA chain), below that a group of lanes per problem (pairwise sums): the demixing recursion of a
 * stream rounds differently in a small and in a large batch, 1e-16 per step on a state with long memory -- the same stream alone and
 * inside a 64-stream batch agrees to ~1e-12 on the spectrum (float output: equal but for rare last-bit flips), not bit for bit. */
int bf_process_batch(bf_handle *h, const float *x_host, size_t n_frames, float *y_host);

/* Same, buffers already resident in HBM; enqueued on `hip_stream`
 * (a hipStream_t, NULL = default stream) without host synchronisation.
 * spectrum_dev (nullable): receives y_fft per frame as double2
 * [n_streams][n_frames][2*hop] (see DESIGN.md for the DAS fused variant).  With look directions / gss_out_sources the leading
 * axis of y and of spectrum_dev is the output stream, (stream * n_dirs + dir) * R + r. */
int bf_process_batch_device(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev,
                            void *spectrum_dev, void *hip_stream);

/* Steering / constraint matrices as the reference's update_weights builds them:
 * [2*hop][n_mics][n_interf+1] complex double (re,im). */
int bf_get_weights(bf_handle *h, double *w_host);

/* Checkpoint of all per-stream state (ring hop, OLA tail, covariance history,
 * GSS demixing matrices, MCRA/MPF vectors, smoothing tail).  The reference has
 * no counterpart (state lives in process globals).  A blob is accepted only by a handle of the same shape, gss_out_sources
 * and gss_postfilter included (one overlap-add tail per output stream; with the post-filter its state per output row). */
size_t bf_state_size(const bf_handle *h);
int bf_get_state(bf_handle *h, void *blob_host, size_t size);
int bf_set_state(bf_handle *h, const void *blob_host, size_t size);
/* Back to the reference's cold start (zeroed rings/tails/history; prepare_overlap_and_add, util.h:272-286).  Host-synchronous:
 * waits for the device before and after. */
int bf_reset(bf_handle *h);
/* The same, enqueued on `hip_stream` without host synchronisation: ordered against the batches the caller runs on that
 * stream (what a per-step cold start in a stream-driven loop needs: beamform_amd/shard.py run_shard, bf_shard_run). */
int bf_reset_async(bf_handle *h, void *hip_stream);

/* ---- frame-range sharding of one long stream across processes (one per GPU) -- SURVEY 8(e) ---------------------------------
 * The reference runs one node per process on one stream (das.cpp:101-145); frames are independent except for the overlap-add
 * neighbour (util.h:301-302) and mvdr / lcmv's covariance of the previous P frames (mvdr.cpp:87,100-101), so a rank that owns
 * the output hops [lo, hi) feeds a COLD node with `lead` hop (seeds the ring buffer, util.h:272-277) + `warm` recomputed frames
 * (output dropped) + its owned frames and needs no data-path collective; the one collective is the final gather of the
 * owned hops (RCCL over xGMI: examples/shard_node.cpp calls it directly, beamform_amd/shard.py through torch.distributed). */
/* bf_process_batch_device on a column range of a longer planar buffer: microphone m starts at x_dev + m * mic_stride
 * (samples), so one resident slice can be walked in pieces without copies (state carries from piece to piece as always). */
int bf_process_batch_device_strided(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *hip_stream,
                                    long mic_stride);
typedef struct bf_shard {
    long long lo, hi; /* output hops this rank owns */
    int warm;         /* frames recomputed in front of lo (clipped at the stream start) */
    int lead;         /* hops fed in front of the first recomputed frame (0 at the stream start) */
} bf_shard;
/* Frames in front of its first frame a shard must recompute: 1 (das, phase), past_windows + 1 (mvdr, lcmv);
 * -1 for the nodes that recurse over frames or samples (gss, phasempf, mcra, gsc): those shard by stream only. */
int bf_shard_halo(const bf_config *cfg);
/* Contiguous, near-equal frame ranges; rank 0 starts from the true stream state (no warm-up, no lead). */
int bf_shard_plan(size_t n_frames, int world, int rank, int halo, bf_shard *out);
long long bf_shard_first_feed(const bf_shard *s); /* first hop of the global stream fed to the rank's cold node: lo - warm - lead */
long long bf_shard_n_feed(const bf_shard *s);     /* hops fed: lead + warm + owned */
long long bf_shard_n_drop(const bf_shard *s);     /* output hops in front of the owned range that are discarded: warm + lead */
/* One rank's step: cold start + the fed hops, enqueued on `hip_stream` without host synchronisation.  x_feed_dev holds hops
 * [first_feed, hi) of the global stream in the handle's layout, y_feed_dev n_feed * hop floats; the owned hops start at
 * element n_drop * hop of y_feed_dev.  One input stream, one look direction, one output row: lcmv with lcmv_out_beams > 1 is
 * BF_EINVAL (y_feed_dev is one stream). */
int bf_shard_run(bf_handle *h, const float *x_feed_dev, const bf_shard *shard, float *y_feed_dev, void *hip_stream);

/* Timing hook for bench.py: runs bf_process_batch_device `iters` times between
 * two hipEvents recorded on `hip_stream` (mean ms per call -> *ms_per_call) and,
 * when ms_kernel != NULL, brackets every launch of the dominant kernel with its
 * own event pair on the same stream (mean ms per launch -> *ms_kernel). */
int bf_time_batch_device(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *hip_stream,
                         int iters, float *ms_per_call, float *ms_kernel);
/* The same per-launch event pairs around the launches the CALLER issues between begin and end (bench.py takes its
 * roofline duration from the very launches its step time covers).  end: mean ms per launch, number of launches. */
int bf_kernel_timing_begin(bf_handle *h);
int bf_kernel_timing_end(bf_handle *h, float *ms_mean, int *n_launches);
/* Launch trace (diagnostics; no counterpart in the reference): the names of the kernels the CALLING THREAD launches through this library
 * between begin and end, in launch order, '\n'-separated, spelled as rocprofv3 spells them (demangled, no parameter list, e.g.
 * "bf::das_f64_pair_kernel", "bf::n1024::stft_kernel<0, true>").  end returns the length of the full list (snprintf convention: the
 * list is truncated to cap - 1 bytes) or a negative error when no trace is open.  tools/dispatch_table.py prints DESIGN.md's
 * dispatch table from it; bench.py prints a `traffic` figure only beside the kernels the counter file was taken on. */
int bf_trace_begin(void);
long bf_trace_end(char *buf, size_t cap);

/* ---- rosjack output stage, file half, and the batch front-end ----------------------------------------
 * rosjack.cpp:189-210: sf_open(audio_file_path, SFM_WRITE, {WAV | PCM_16, 1 channel, JACK or resampled rate});
 * rosjack.cpp:404-409: sf_write_float(audio_file, write_file_buffer, data_length) once per callback; closed with the node.
 * libsndfile (1.0.28 on the reference's Ubuntu 20.04) is neither vendored in the reference nor installed here; its header
 * layout and its float -> short rule on this call path (lrintf(x * 32767.0f), no clipping: beyond +-1.0 it wraps) are
 * restated in csrc/wavio.cpp.  Host functions: no HIP device needed. */
typedef struct bf_wav_writer bf_wav_writer;
int bf_wav_writer_open(const char *path, int sample_rate, bf_wav_writer **out);        /* sf_open(..., SFM_WRITE, ...) */
int bf_wav_writer_write(bf_wav_writer *w, const float *samples, size_t n);             /* sf_write_float */
int bf_wav_writer_write_pcm16(bf_wav_writer *w, const int16_t *pcm, size_t n);         /* samples already converted (device) */
int bf_wav_writer_close(bf_wav_writer *w);                                             /* sf_close: patches the lengths */
/* The sample rule of sf_write_float on a PCM_16 file, on the host and on a batch resident in HBM (16-byte aligned buffers). */
void bf_float_to_pcm16(const float *src, int16_t *dst, size_t n);
int bf_float_to_pcm16_device(const float *src_dev, int16_t *dst_dev, size_t n, void *hip_stream);
/* Front-end: a WAV file (PCM 16/24/32 or float32, any channel count; sf_read_float's scaling) or a raw planar float32 file
 * -> planar float32 [channel][sample], the BF_PLANAR layout of bf_process_batch.  Release with bf_wav_free. */
int bf_wav_read(const char *path, float **planar, int *n_channels, size_t *n_samples, int *sample_rate);
int bf_planar_f32_read(const char *path, int n_channels, float **planar, size_t *n_samples);
void bf_wav_free(float *planar);

/* ---- rosjack output stage, sample-rate half ----------------------------------------------------------------------------------
 * rosjack.cpp:159-184: samplerate_conv = src_new(SRC_SINC_FASTEST, 1, ..), src_ratio = ros_output_sample_rate / rosjack_sample_rate,
 * refused when src_is_valid_ratio fails; rosjack.cpp:311-338 (convert_to_sample_rate): one src_process per JACK period with
 * end_of_input = 0, the generated samples queued and emitted one period at a time (:340-349).  bf_resampler_* is that converter
 * as a stream operator on the GPU: every call takes the next piece of the mono stream and returns the output samples that
 * have become available (an output exists once bf_resampler_latency input samples beyond its position have been seen; what
 * libsamplerate holds back in the same way).  Results do not depend on how the stream is cut into calls.
 * libsamplerate (un-vendored; 0.1.9 on the reference's Ubuntu 20.04) is not in this image: csrc/resample.hip restates
 * src_sinc.c's mono converter; the built-in coefficient table is a Kaiser-windowed sinc of SINC_FASTEST's geometry, NOT
 * libsamplerate's fastest_coeffs.h (parity unpinned) -- bf_resampler_set_table installs any table of that form, e.g. the
 * original one.
 * Two ways of driving it (bf_resampler_set_mode):
 *   BF_RS_STREAM (default)  every input sample is consumed and every output sample returned (bf_resampler_process*): the
 *                           mathematically complete conversion of the stream, independent of how it is cut into calls;
 *   BF_RS_ROSJACK           the stage exactly as rosjack runs it, one bf_resampler_callback* per JACK period: src_process may
 *                           return at most one period of output (output_frames = rosjack_window_size, rosjack.cpp:176-183), a
 *                           period is copied into the converter only when input_frames == 0 and DROPPED otherwise (:311-338),
 *                           libsamplerate pulls input in lazily (src_sinc.c prepare_data), and a block is published only when a
 *                           full period of output is queued, at most one per callback, the tail never (:340-349, :416-436).
 *                           With out_rate > in_rate the reference therefore loses whole periods (16 -> 48 kHz keeps about every
 *                           third one); with out_rate <= in_rate the two modes differ only in the blocking of the output.
 *                           examples/file_node: trailing argument "rosjack". */
typedef struct bf_resampler bf_resampler;
int bf_resampler_create(int in_rate, int out_rate, bf_resampler **out);               /* src_new + src_ratio; BF_EINVAL outside 1/256..256 */
int bf_resampler_set_table(bf_resampler *r, const float *coeffs, int n_coeffs, int index_inc); /* half table incl. 2 guard entries; resets */
enum bf_resampler_mode { BF_RS_STREAM = 0, BF_RS_ROSJACK = 1 };
int bf_resampler_set_mode(bf_resampler *r, int mode, int period);                     /* period = rosjack_window_size (BF_RS_ROSJACK); resets */
/* BF_RS_ROSJACK: one output_to_rosjack(data_out, period).  *emitted = 1 when a block of `period` samples was published into
 * `block`, *accepted = 0 when the reference would have dropped this period.  Device or host buffers of `period` floats. */
int bf_resampler_callback_device(bf_resampler *r, const float *period_dev, float *block_dev, int *emitted, int *accepted, void *hip_stream);
int bf_resampler_callback(bf_resampler *r, const float *period, float *block, int *emitted, int *accepted);
int bf_resampler_reset(bf_resampler *r);                                              /* src_reset */
size_t bf_resampler_out_count(bf_resampler *r, size_t n_in);                          /* outputs the next call with n_in samples yields */
int bf_resampler_latency(bf_resampler *r);                                            /* look-ahead in input samples */
int bf_resampler_process_device(bf_resampler *r, const float *in_dev, size_t n_in, float *out_dev, size_t out_cap, size_t *n_out,
                                void *hip_stream);                                    /* src_process on buffers resident in HBM */
int bf_resampler_process(bf_resampler *r, const float *in, size_t n_in, float *out, size_t out_cap, size_t *n_out); /* host buffers */
void bf_resampler_destroy(bf_resampler *r);                                           /* src_delete */
int bf_resampler_default_table(float *dst, int cap, int *index_inc);                  /* copy of the built-in table; returns its length */

/* ---- steering tracks: a look angle per frame inside one batch --------------------------------------------------------------------
 * In the reference a /theta message lands between two JACK callbacks, so the look angle can change at every frame (das.cpp:94-99,
 * SURVEY 3.3); bf_set_theta takes effect at the next batch, which freezes a batch on one angle.  A steering track lifts that: the handle
 * holds one steering table per CANDIDATE angle, and a device array names, for every (stream, frame) of a batch, which of them weights
 * that frame.
 *   Semantics: frame t of stream s is weighted exactly as the reference's callback t is with /theta = angles[track[s][t]] in force,
 *   i.e. as if that angle had been set between callbacks t-1 and t.  theta_roscallback only rewrites the weight rows of these nodes, so
 *   everything else -- the history hop (frame t is [hop t-1 | hop t] as always), the overlap-add tail, phasempf's recursive state and
 *   smoother -- carries across frames and across calls exactly as in an untracked batch.
 *   Index rule: track[s][t] in 0 .. n_angles-1 selects that table; ANY other value (negative, >= n_angles) selects the handle's own
 *   /theta table, the one an untracked batch uses.  A bad index is never read through; -1 is the way to say "nothing published yet".
 *   Supported: BF_DAS with BF_DAS_F64, BF_PHASE, BF_PHASEMPF, one look direction (n_dirs <= 1); any n_streams, both layouts, every
 *   period, both precisions.  Every other handle answers BF_ENOSYS (gss re-initialises its demixing matrices on every /theta,
 *   gss.cpp:90-93; the fp32 das kernels are not built for tracks; mvdr / lcmv have entry points of their own, bf_ctrack_* below).
 *   Kernels: period 512 with <= 8 microphones keeps STFT and per-bin stage in one launch (the spectra never leave the CU); every other
 *   shape runs STFT -> per-bin kernel -> ISTFT.  das in double never takes its one-launch frame-pair kernel for a tracked batch (two
 *   frames share a transform there), so an untracked batch is the faster way to run a constant angle.
 * A handle that never installs angles runs the kernels it always ran. */
#define BF_TRACK_MAX_ANGLES 1024   /* = BF_DOA_MAX_ANGLES: a bf_doa peak index is a track index */
/* Installs the candidate angles (degrees): table a holds the bytes bf_set_theta with angles_deg[a] would leave in the handle's table (the
 * same host code, microphone 0's row as it stands).  n_angles = 0 drops the tables.  HOST-SYNCHRONOUS: waits until the device has
 * finished everything enqueued before it, then installs the new tables for the batches that begin afterwards.  Thread-safe against a
 * concurrent bf_process_* on the handle, like bf_set_theta: the handle's mutex guards the switch, and a tracked batch that another
 * thread has begun keeps the tables it began with -- they are retired, not freed, until the NEXT bf_track_set_angles (or bf_destroy),
 * so up to two sets of tables are resident.  The tables are input, not state: no part of bf_state_size / the state blob.
 * BF_EINVAL: a non-finite angle, n_angles outside 0 .. BF_TRACK_MAX_ANGLES, tables (n_angles x n_mics x 2 hop complex doubles) above
 * 512 MiB.  BF_ENOSYS: a handle without tracks (above). */
int bf_track_set_angles(bf_handle *h, const double *angles_deg, int n_angles);
/* bf_process_batch_device with a track: track_dev is [n_streams][n_frames] int32 on the device, read by the kernels (it must stay
 * valid until hip_stream has passed the batch).  Tracked and untracked calls may alternate on one handle; the handle's own theta is
 * not changed.  BF_EINVAL: no angles installed, track_dev NULL, n_dirs > 1.  BF_ENOSYS: a handle without tracks. */
int bf_process_batch_device_tracked(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *spectrum_dev,
                                    const int32_t *track_dev, void *hip_stream);
/* From direction-of-arrival peaks to a track, on the device (no handle; one small launch on hip_stream, no host synchronisation).
 * peak_dev: [n_streams][n_blocks] as bf_doa_process_device writes it; map_dev: [n_streams][n_blocks][n_angles], may be NULL when
 * min_peak <= 0.  Block b PUBLISHES peak[s][b] when map[s][b][peak[s][b]] >= min_peak (not below it: a NaN publishes, as
 * controllers.DoaTheta does); with a NULL map every block publishes; with a map, a peak outside 0 .. n_angles-1 is not looked up and
 * does not publish.  Every frame of block b gets the index published by the latest block b' <= b - latency_blocks that published; if
 * there is none, carry[s] as it was on entry.  On exit carry[s] is the index a block n_blocks would get, so that consecutive calls
 * continue one stream (exactly for latency_blocks <= 1: carry is one index, a longer latency forgets what the last
 * latency_blocks - 1 blocks of the previous call published).  Start with carry = -1: "the handle's theta".  latency_blocks = 1 is an
 * external localiser's one block of latency (controllers.follow_doa).  track_dev: [n_streams][n_blocks * frames_per_block].
 * BF_EINVAL, checked before any device work: n_angles < 1, n_streams < 1, frames_per_block < 1, latency_blocks < 0, NULL peak / carry /
 * track, NULL map with min_peak > 0. */
int bf_track_from_peaks_device(const int32_t *peak_dev, const double *map_dev, int n_angles, int n_streams, size_t n_blocks,
                               int frames_per_block, int latency_blocks, double min_peak, int32_t *carry_dev, int32_t *track_dev,
                               void *hip_stream);

/* ---- column tracks: mvdr and lcmv, an angle per frame AND per constraint column ----------------------------------------------------
 * mvdr's theta_roscallback only rewrites its steering vector (mvdr.cpp:41-60, 139-143) and lcmv's update_weights() rebuilds every
 * constraint column from `angle` and `interference_angles` (lcmv.cpp:44-86); neither touches past_ffts.  So a steering vector per frame
 * is the reference's semantics for these nodes too.  They get entry points of their own (bf_track_* keeps answering BF_ENOSYS on them)
 * because an lcmv track carries one index per constraint column, not one per frame.
 *   Track layout: track_dev is [n_streams][n_frames][n_cols] int32 on the device, n_cols from 1 to 1 + bf_n_interferers(h) at the time
 *   of the call (mvdr: 1 only).  Column 0 is the look direction, column c >= 1 is interferer c (the 1-based id of bf_set_interference).
 *   Semantics: frame t of stream s is processed exactly as the reference's callback t is with angle = angles[track[s][t][0]] and
 *   interference_angles[c-1] = angles[track[s][t][c]] in force and update_weights() (without `ini`) run after the assignment.  The
 *   interferer COUNT does not change inside a batch, and the callback's proximity rule (lcmv.cpp:264-279: an interferer that comes within
 *   interf_angle_threshold of another is removed) is NOT applied: where two columns of one frame lie that close the reference would
 *   have dropped one, and no parity is claimed there.
 *   Index rule, per column: 0 .. n_angles-1 selects that angle's table; ANY other value selects the handle's own column c (what an
 *   untracked batch uses).  Columns >= n_cols are always the handle's own.  A bad index is never read through.
 *   Microphone 0: whatever the index, the entry of microphone 0 in column c is the handle's own column c's entry -- 1 after create, 0
 *   after a structural interferer change (quirk Q3, lcmv.cpp:50-56, 243-252).  The kernels read it from the handle's table at every
 *   frame, so a structural bf_set_interference after bf_ctrack_set_angles leaves nothing stale behind.
 *   State: the history hop, the covariance history of the previous past_windows frames, the overlap-add tail and out_amp carry across
 *   frames and calls exactly as in an untracked batch; tracked and untracked calls may alternate on one handle.
 *   Supported: BF_MVDR and BF_LCMV, n_dirs <= 1, any n_streams, both layouts, both precisions, every period, up to 32 microphones and
 *   the handle's current column count, with or without spectrum_dev.
 *   Kernels: up to 8 microphones (and the columns mvdr_fast_kernel takes) run mvdr_fast_track_kernel -- for mvdr without the
 *   register-resident steering vector of the untracked kernel, the columns are re-read per frame as lcmv's always were.  Everything
 *   else, 9 .. 16 microphones included, runs mvdr_lcmv_track_kernel, the group kernel's twin: cov2d_kernel has no twin, so those shapes
 *   are correct but not tuned.  BF_MVDR_TILE and BF_MVDR_GROUP act as on untracked batches.  An untracked batch is the faster way to
 *   run constant angles. */
/* bf_track_set_angles for these handles, with its rules: host-synchronous, thread-safe beside a batch being enqueued, the replaced tables
 * retired until the next install, the tables no part of the state blob.  One table per candidate angle serves every column
 * (calculate_interf_delays is calculate_delays with another angle, util.h:136-188).  BF_ENOSYS: any algorithm but mvdr / lcmv.
 * BF_EINVAL: NULL handle, n_dirs > 1, a non-finite angle, n_angles outside 0 .. BF_TRACK_MAX_ANGLES, tables above 512 MiB. */
int bf_ctrack_set_angles(bf_handle *h, const double *angles_deg, int n_angles);
/* One batch with a column track (it must stay valid until hip_stream has passed the batch).  Checked before any device work:
 * BF_ENOSYS: any algorithm but mvdr / lcmv.  BF_EINVAL: NULL handle, x, y or track; no angles installed; n_cols < 1 or above the
 * current column count; n_dirs > 1. */
int bf_process_batch_device_ctracked(bf_handle *h, const float *x_dev, size_t n_frames, float *y_dev, void *spectrum_dev,
                                     const int32_t *track_dev, int n_cols, void *hip_stream);

/* ---- multi-source picks and their column track, on the device ------------------------------------------------------------------------
 * The device half of controllers.pick_sources / DoaSources / sources_track: with these two a caller closes the multi-source loop in
 * four enqueues on one stream and no host synchronisation -- bf_doa_process_device (the Capon map), bf_doa_pick_device,
 * bf_ctrack_from_picks_device, bf_process_batch_device_ctracked (controllers.follow_sources_device, examples/follow_sources_node.cpp).
 * Neither takes a handle; each is one small launch on hip_stream.  bf_ctrack_from_picks_device's columns are loudness ranks (pick j in
 * column j); bf_ctrack_assign_device, the third call below, takes its place where a column has to stay with one talker. */
#define BF_DOA_MAX_PICKS 16   /* = BF_MAX_INTERF + 1: a look direction and every interferer */
/* The k strongest separated peaks of every map row.  map_dev: [n_streams][n_blocks][n_angles] as bf_doa_process_device writes it;
 * angles_dev: [n_angles] doubles ON THE DEVICE, the candidate grid in degrees (any order, any range); picks_dev:
 * [n_streams][n_blocks][k] int32, strongest first, unused places -1.  Per row:
 *   1. m = the row's maximum, floor = rel_floor * m; every angle is free.
 *   2. For j = 0 .. k-1: d = the free index with the largest value, the lowest index on ties.  Stop if nothing is free or
 *      row[d] < floor.  Otherwise picks[j] = d, d is no longer free, and every free i with sep(angles[i], angles[d]) < min_sep_deg
 *      is no longer free.
 *   3. sep(a, b):  t = (a - b) + 180.0;  r = fmod(t, 360.0);  if r < 0 then r += 360.0;  the result is |r - 180.0| -- every step in
 *      double and in exactly this order.  Each step is an exact or a correctly rounded IEEE operation, so the device, the host
 *      (beamform_amd/csrc/doa_pick.hpp) and numpy's % agree bit for bit.
 * For rows without NaN the picks are exactly those of controllers.pick_sources (a value of -inf, which its masking cannot tell from
 * a suppressed angle, is outside this claim too; maps are in [0, 1]).  A row holding a NaN is outside the contract: the kernel still
 * terminates and writes nothing but -1 or an index in 0 .. n_angles-1.  Rows are independent (one wavefront each, registers only):
 * the bytes do not depend on the launch.
 * BF_EINVAL, checked before any device work: n_angles outside 1 .. BF_DOA_MAX_ANGLES, n_streams < 1, k outside 1 .. BF_DOA_MAX_PICKS,
 * a non-finite or negative min_sep_deg, a non-finite rel_floor, a NULL pointer.  n_blocks = 0 is BF_OK and launches nothing. */
int bf_doa_pick_device(const double *map_dev, const double *angles_dev, int n_angles, int n_streams, size_t n_blocks, int k,
                       double min_sep_deg, double rel_floor, int32_t *picks_dev, void *hip_stream);
/* From picks to a column track: controllers.sources_track with a DoaSources controller, stated per column.
 * picks_dev: [n_streams][n_blocks][k]; map_dev: [n_streams][n_blocks][n_angles], may be NULL when min_peak <= 0; carry_dev:
 * [n_streams][n_cols] int32, in and out; track_dev: [n_streams][n_blocks * frames_per_block][n_cols], the layout
 * bf_process_batch_device_ctracked reads.
 *   Publishing: block b publishes when p0 = picks[s][b][0] is in 0 .. n_angles-1 and the map is NULL or map[s][b][p0] is not below
 *   min_peak (a NaN publishes, as controllers.DoaSources and bf_track_from_peaks_device have it).
 *   Column updates: a publishing block updates column c, 0 <= c < min(n_cols, k), when picks[s][b][c] is in 0 .. n_angles-1.  A column
 *   the publication does not mention keeps its value, columns >= k are never updated, picks beyond n_cols are dropped.
 *   Frames: every frame of block b gets, per column, the value of the latest update of that column by a block b' <= b - latency_blocks;
 *   if there is none, carry[s][c] as it was on entry.
 *   Carry: on exit carry[s][c] is what a block n_blocks would get, so that consecutive calls continue one stream -- exactly for
 *   latency_blocks <= 1 (carry is one index per column: a longer latency forgets what the last latency_blocks - 1 blocks of the
 *   previous call published).  Start with -1 everywhere: "the handle's own column".
 * A pick outside the map neither publishes nor updates and is never read through; a value read from carry is copied as it stands and
 * never used as an index.  The track holds the picks themselves: indices into the grid the picker was given, which is the grid to
 * install with bf_ctrack_set_angles.
 * BF_EINVAL, checked before any device work: n_angles < 1, k outside 1 .. BF_DOA_MAX_PICKS, n_streams < 1, frames_per_block < 1,
 * latency_blocks < 0, n_cols outside 1 .. BF_MAX_INTERF + 1, NULL picks / carry / track, NULL map with min_peak > 0.  n_blocks = 0 is
 * BF_OK (carry stays). */
int bf_ctrack_from_picks_device(const int32_t *picks_dev, const double *map_dev, int n_angles, int k, int n_streams, size_t n_blocks,
                                int frames_per_block, int latency_blocks, double min_peak, int n_cols, int32_t *carry_dev,
                                int32_t *track_dev, void *hip_stream);
/* From picks to a column track in which a column is a TALKER.  bf_ctrack_from_picks_device above puts pick j into column j, and picks
 * are ordered by strength: its columns are loudness ranks, and they swap whenever another talker becomes the loudest.  This builder
 * associates the picks of every block with the columns instead: a column follows the pick nearest to where its talker was last heard,
 * holds through pauses, and a new talker gets a free column.  No handle, one small launch on hip_stream, one wavefront per stream,
 * serial over the blocks; it stands in the third place of the four-enqueue loop (controllers.follow_talkers_device).
 * picks_dev: [n_streams][n_blocks][k]; map_dev: [n_streams][n_blocks][n_angles], may be NULL when min_peak <= 0; angles_dev:
 * [n_angles] doubles ON THE DEVICE, the picker's grid; track_dev: [n_streams][n_blocks * frames_per_block][n_cols], the layout
 * bf_process_batch_device_ctracked reads; active_dev: [n_streams][n_blocks][n_cols] int32, may be NULL; state_dev:
 * [n_streams][n_cols][BF_ASSIGN_STATE_INTS] int32, read and written: per slot (column) {idx, hits, misses, out}.
 *   A slot is LIVE iff idx is in 0 .. n_angles-1; otherwise it is free and its hits and misses are ignored.  A state filled with -1 is a
 *   cold start.
 * Per stream, for each block b in ascending order:
 *   1. Candidates.  The block publishes by the rule of bf_ctrack_from_picks_device: p0 = picks[s][b][0] is in 0 .. n_angles-1 and the
 *      map is NULL or map[s][b][p0] is not below min_peak (a NaN publishes).  If it publishes, the candidates are the picks[s][b][j],
 *      j < k, that are in 0 .. n_angles-1, in order of j; otherwise there are none.  Duplicate picks in a row are ordinary candidates.
 *   2. Match.  Among the live slots and the candidates, repeat until no pair qualifies: take the unmatched pair (slot c, candidate j)
 *      with the smallest d = sep(angles[idx_c], angles[p_j]) for which d <= gate_deg holds; ties go to the lowest c, then the lowest
 *      j.  sep is the picker's circular distance (step 3 of bf_doa_pick_device, beamform_amd/csrc/doa_pick.hpp), the same function
 *      to the bit; idx_c is the slot's index as the block found it.  A NaN distance never matches.
 *   3. A matched slot: idx = p_j, hits = min(hits + 1, 2^30), misses = 0.
 *   4. An unmatched live slot: with hits < min_hits it is tentative and is freed (idx = -1).  Otherwise misses = min(misses + 1, 2^30),
 *      and the slot is freed when misses > max_coast.
 *   5. Births.  Each unmatched candidate, in order of j, takes the lowest free slot c < n_cols -- slots freed in step 4 of this block
 *      count as free -- with idx = p_j, hits = 1, misses = 0.  With no free slot the candidate is dropped.  A newborn talker may land
 *      in column 0, the look direction, once column 0's talker has been freed.
 *   6. Out.  For every live slot with hits >= min_hits: out = idx.  Any other out stays as it was: a freed column keeps pointing where
 *      its talker was last heard.  active[s][b][c] = 1 iff slot c was matched or born in this block and has hits >= min_hits, else 0;
 *      active is not delayed.
 *   7. Frames.  Every frame of block b gets, per column, out as it stood after block b - latency_blocks; if there is no such block, out
 *      as it was on entry.
 * On exit the state is the state after the last block, so that consecutive calls continue one stream -- exactly for
 * latency_blocks <= 1 (out is one index per column: a longer latency forgets what the last latency_blocks - 1 blocks of the previous
 * call left in out).  The rule for one block in plain C++: beamform_amd/csrc/doa_assign.hpp; in numpy: controllers.assign_sources.
 * A pick outside the map is neither a candidate nor ever read through.  A value read from the state is copied as it stands and never
 * used as an index, but for an idx that has been checked against n_angles.  Streams do not see each other and a stream's blocks are
 * walked in order by one wavefront: the bytes do not depend on the launch.
 * BF_EINVAL, checked before any device work: n_angles outside 1 .. BF_DOA_MAX_ANGLES, k outside 1 .. BF_DOA_MAX_PICKS, n_streams < 1,
 * frames_per_block < 1, latency_blocks < 0, n_cols outside 1 .. BF_MAX_INTERF + 1, a non-finite or negative gate_deg, min_hits < 1,
 * max_coast < 0, NULL picks / angles / state / track, NULL map with min_peak > 0.  n_blocks = 0 is BF_OK and launches nothing (the
 * state stays). */
#define BF_ASSIGN_STATE_INTS 4
int bf_ctrack_assign_device(const int32_t *picks_dev, const double *map_dev, const double *angles_dev, int n_angles, int k,
                            int n_streams, size_t n_blocks, int frames_per_block, int latency_blocks, double min_peak,
                            double gate_deg, int min_hits, int max_coast, int n_cols,
                            int32_t *state_dev, int32_t *track_dev, int32_t *active_dev, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* BFCORE_H */
