"""Node parameters off their launch-file values: the cases shared by tests/test_params_cpu.py (are the cases worth running?) and
tests/test_params_gpu.py (parity on the device).  The launch values of beamform_amd/params.py hide mistakes -- twin defaults
(mcra_alphaS == mcra_alphaD, mpf_rev_delta == 1, lambda_ == 0, out_amp == 1), a minimum search that never decides anything at
mcra_delta = 0.001, one covariance window length, one smoothing length, one sample rate -- so every case here moves them.

A case is (name, algo, M, interf, hop, F, layout, streams, precision, over, env, kernels, seed, cuts, named, extra):
  over     make_params overrides
  env      switches read once per process: a case with an `env` runs in a fresh child process, cases with the same `env` share one
  kernels  what one batch of the case must launch, written down here from docs/DISPATCH.md and the comments of chain_plan.hpp and NOT
           computed by the code under test (a name matches when a traced kernel contains it); test_params_cpu.py holds chain_decide to
           it, test_params_gpu.py the launch trace
  cuts     frame boundaries (0, ..., F) of the same stream fed in several batches, besides the single batch
  named    the keys of `over` the case is named for: test_params_cpu.py shows that each one, put back to its launch value alone,
           moves the oracle's output by at least 1e-3 (100 times the parity bar)
  extra    how the batch is driven: track (a steering / column track), dirs (look directions), rows (gss_out_sources), pf
           (gss_postfilter), f32 (the fp32 das opt-in), per_hop (one callback at a time), checkpoint (state saved after that many
           frames and restored into a fresh handle), offset (output through a pointer that is 4- but not 16-byte aligned)
Every case stays at or below 8192 samples per stream, except the 64-stream ones (12 frames or fewer).

The figures behind each case are measured on the oracle alone by test_params_cpu.py (`python tests/test_params_cpu.py` prints them);
FIGURES at the end of this file quotes them: per named key the relative L2 distance of the oracle's output from the same case with
that key at its launch value (and, for the twins, with the two values swapped), `o2o` the distance between the two restatements of
the oracle (C++ and numpy, different FFTs), `busy` the share of in-band bins of the subtraction nodes that are neither zero nor on
noise_floor.
"""
from collections import namedtuple

import numpy as np

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene

PLANAR, INTERLEAVED = 0, 1       # bf_layout
REF, MIXED = 0, 1                # bf_precision
GROUP = {"BF_MVDR_GROUP": "1"}
LANE = {"BF_GSS_GROUP": "0"}

Case = namedtuple("Case", "name algo M interf hop F layout streams precision over env kernels seed cuts named extra")

#: the twins: pairs whose launch values coincide (or whose reads sit side by side): swapping the two values must show as well
TWINS = (("mcra_alphaS", "mcra_alphaD"), ("mcra_alphaD", "mcra_alphaD2"), ("mpf_alphaS", "mcra_alphaS"))

# ---- the parameter sets ------------------------------------------------------------------------------------------------------------
# alphaD2 sits below 1 - alphaD on purpose: otherwise the noise estimate settles above the signal power, `lambda > soi2` always holds and
# mcra_delta / mcra_alphaS / the minimum search decide nothing.  The reverberation pair stays mild (k = 1 - gamma / delta = 0.02, and positive
# when either goes back to its launch value) and the phase threshold wide: with a stronger pair (0.6 / 2.0) and 20 degrees
# Lambda exceeded |soi| in 99 % of the bins and the output was noise_floor nearly everywhere
MPF = dict(mcra_alphaS=0.6, mcra_alphaD=0.4, mcra_alphaD2=0.2, mcra_delta=1.5, mcra_L=4, mpf_alphaS=0.5, mpf_eta=0.1, mpf_rev_gamma=0.93,
           mpf_rev_delta=0.95, min_phase=45.0, min_mag=0.2, smooth_size=5, out_amp=1.7, noise_floor=0.05)
MCRA = dict(mcra_alphaS=0.8, mcra_alphaD=0.3, mcra_alphaD2=0.9, mcra_delta=2.0, mcra_L=6, out_amp=1.7)
#: the gss post-filter reads the recursion's keys only (no phase decision, no smoother)
GPF = {k: v for k, v in MPF.items() if k not in ("min_phase", "min_mag", "smooth_size", "out_amp")}
PHASE = dict(min_phase=25.0, mag_mult=0.3, mag_threshold=5e-4)
GSS = dict(mu=0.01, lambda_=5.0, out_amp=0.3, freq_mag_threshold=0.01, freq_min=300.0, freq_max=7000.0)
GSS5 = dict(GSS, mu=0.003)          # five interferers: at mu = 0.01 the update diverges once freq_mag_threshold goes back to 0.001
PW = dict(out_amp=0.6, freq_mag_threshold=0.01)

K2, K5 = (-60.0, 90.0), (-60.0, 90.0, 150.0, -120.0, 45.0)
DIR_ANGLES = [20.0, -35.0, 110.0]          # steering tracks and look directions of phase / phasempf (tests/test_track_gpu.py)
TRACK_EVERY = 3                            # a new angle every three frames


def _n(hop, *names):
    return [f"n{2 * hop}::{k}" for k in names]


CASES = []


def _add(name, algo, M, hop, F, kernels, named, interf=(), layout=PLANAR, streams=1, precision=REF, env=None, seed=None, cuts=None,
         extra=None, **over):
    assert name not in [c.name for c in CASES], name
    assert F * hop <= 8192 or (streams == 64 and F <= 12), name
    assert set(named) <= set(over), (name, set(named) - set(over))
    assert cuts is None or (cuts[0] == 0 and cuts[-1] == F and list(cuts) == sorted(set(cuts))), name
    CASES.append(Case(name, algo, M, tuple(interf), hop, F, layout, streams, precision, dict(over), dict(env or {}), list(kernels),
                      7000 + len(CASES) if seed is None else seed, cuts, tuple(named), dict(extra or {})))


# ==== 1. the MCRA / MPF recursion, every implementation ===============================================================================
_MPF_KEYS = tuple(MPF)
_add("mpf-m8", "phasempf", 8, 512, 16, _n(512, "stft_bins_w64_kernel<0, 8, 5>", "fused_tail_kernel<8, 5>", "mpf_recursion_kernel", "smooth4_kernel<5>"),
     _MPF_KEYS, **MPF)
_add("mpf-m16", "phasempf", 16, 512, 16, _n(512, "stft_kernel<0, false>", "mpf_mask_kernel<16>", "mpf_recursion_kernel", "smooth4_kernel<5>"),
     _MPF_KEYS, **MPF)
_add("mpf-s64", "phasempf", 8, 512, 11, _n(512, "fused_tail_kernel<8, 5>", "mpf_rec_istft_kernel", "smooth4_kernel<5>"), _MPF_KEYS, streams=64,
     cuts=(0, 1, 3, 6, 11), **MPF)
_add("mpf-track-m8", "phasempf", 8, 512, 16, _n(512, "stft_bins_w64_track_kernel<0, 8, 5>", "fused_tail_track_kernel<8, 5>", "mpf_recursion_kernel"),
     _MPF_KEYS, extra=dict(track=1), **MPF)
_add("mpf-track-m16", "phasempf", 16, 512, 16, _n(512, "mpf_mask_track_kernel<16>", "mpf_recursion_kernel"), _MPF_KEYS, extra=dict(track=1), **MPF)
_add("mpf-mixed", "phasempf", 8, 512, 16, _n(512, "fused_tail_kernel<8, 5>", "mpf_recursion_kernel", "istft32_kernel", "smooth4_kernel<5>"), _MPF_KEYS,
     precision=MIXED, **MPF)
_add("mpf-noise", "phasempf", 8, 512, 16, _n(512, "fused_tail_kernel<8, 5>", "mpf_recursion_kernel"),
     [k for k in MPF if k != "noise_floor"], out_only_noise=1, **MPF)        # Lambda itself is the output: nothing is floored
_add("mpf-mcra", "phasempf", 8, 512, 16, _n(512, "fused_tail_kernel<8, 5>", "mpf_recursion_kernel"),
     [k for k in MPF if not k.startswith("mpf_")], out_only_mcra=1, **MPF)   # |soi| - sqrt(lambda): the MPF terms are not in the output
_add("mpf-hop64", "phasempf", 8, 64, 128, _n(64, "stft_bins_small_kernel<0, 8, 5>", "fused_tail_kernel<8, 5>", "mpf_recursion_kernel", "smooth4_kernel<5>"),
     _MPF_KEYS, **MPF)
_add("mpf-hop2048", "phasempf", 8, 2048, 4, _n(2048, "stft_generic_kernel<0>", "mpf_mask_kernel<8>", "mpf_recursion_kernel", "smooth4_kernel<5>"),
     _MPF_KEYS, **dict(MPF, mcra_L=0))    # four frames: the minimum search restarts at every frame
_MCRA_KEYS = tuple(MCRA)
_add("mcra-m2", "mcra", 2, 512, 16, _n(512, "stft_kernel<0, false>", "mcra_node_kernel"), _MCRA_KEYS, **MCRA)
_add("mcra-m2-il", "mcra", 2, 512, 16, _n(512, "stft_kernel<1, false>", "mcra_node_kernel"), _MCRA_KEYS, layout=INTERLEAVED, **MCRA)
_add("mcra-m2-hop128", "mcra", 2, 128, 64, _n(128, "stft_small_kernel<0, false>", "mcra_node_kernel"), _MCRA_KEYS,
     **dict(MCRA, mcra_alphaD2=0.6))   # (64 frames at alphaD2 = 0.9: the estimate settles at 7 times the power and 94 % of the bins are zero)
_add("mcra-m2-noise", "mcra", 2, 512, 16, _n(512, "mcra_node_kernel"), _MCRA_KEYS, out_only_noise=1, **MCRA)
_add("gpf-r3", "gss", 8, 512, 16, _n(512, "gss_kernel_all<8, 4>", "gss_postfilter_kernel<4>"), tuple(GPF), interf=K2,
     extra=dict(rows=3, pf=1), **GPF)
_add("gpf-r3-lane", "gss", 8, 512, 12, _n(512, "gss_lane_kernel_all<8, 4>", "gss_postfilter_kernel<4>"), tuple(GPF), interf=K2, streams=64,
     extra=dict(rows=3, pf=1), **GPF)

# ==== 2. phase ========================================================================================================================
_PH = tuple(PHASE)
_add("phase-m8", "phase", 8, 512, 16, _n(512, "stft_bins_w64_kernel<0, 8, 4>", "fused_tail_kernel<8, 4>"), _PH, **PHASE)
_add("phase-m16", "phase", 16, 512, 16, _n(512, "stft_kernel<0, false>", "pointwise_bins_kernel<16, 4>"), _PH, **PHASE)
_add("phase-m8-d3", "phase", 8, 512, 16, _n(512, "stft_kernel<0, false>", "pointwise_bins_kernel<8, 4>"), _PH, extra=dict(dirs=3), **PHASE)
_add("phase-track", "phase", 8, 512, 16, _n(512, "stft_bins_w64_track_kernel<0, 8, 4>", "fused_tail_track_kernel<8, 4>"), _PH, extra=dict(track=1),
     **PHASE)
_add("phase-hop128", "phase", 8, 128, 64, _n(128, "stft_bins_small_kernel<0, 8, 4>", "fused_tail_kernel<8, 4>"), _PH, **PHASE)
_add("phase-mixed", "phase", 8, 512, 16, _n(512, "fused_tail_kernel<8, 4>", "istft32_kernel"), _PH, precision=MIXED, **PHASE)

# ==== 3. gss ==========================================================================================================================
_GS = tuple(GSS)
_add("gss-k2", "gss", 8, 512, 16, _n(512, "gss_kernel<8, 4>"), _GS, interf=K2, **GSS)
_add("gss-k5", "gss", 8, 512, 16, _n(512, "gss_kernel<8, 8>"), _GS, interf=K5, **GSS5)
_add("gss-k2-rows", "gss", 8, 512, 16, _n(512, "gss_kernel_all<8, 4>"), _GS, interf=K2, extra=dict(rows=3), **GSS)
_add("gss-k5-rows", "gss", 8, 512, 16, _n(512, "gss_kernel_all<8, 8>"), _GS, interf=K5, extra=dict(rows=6), **GSS5)
_add("gss-k2-lane", "gss", 8, 512, 16, _n(512, "gss_lane_kernel<8, 4>"), _GS, interf=K2, env=LANE, **GSS)
# (five interferers never reach the lane kernel: beyond three chain_decide takes the group kernel's next larger instantiation whatever
# the switch says; one interferer runs the lane kernel's same instantiation with columns to spare)
_add("gss-k1-lane", "gss", 8, 512, 16, _n(512, "gss_lane_kernel<8, 4>"), _GS, interf=(-60.0,), env=LANE, **GSS)
_add("gss-k2-lane-rows", "gss", 8, 512, 16, _n(512, "gss_lane_kernel_all<8, 4>"), _GS, interf=K2, env=LANE, extra=dict(rows=3), **GSS)
_add("gss-k1-lane-rows", "gss", 8, 512, 16, _n(512, "gss_lane_kernel_all<8, 4>"), _GS, interf=(-60.0,), env=LANE, extra=dict(rows=2), **GSS)

# ==== 4. past_windows =================================================================================================================
# name -> (algo, M, interferers, per-bin kernel by precision, env, extra); z128 = "true" at reference precision, "false" at mixed
_PW_SHAPES = {
    "fast8": ("mvdr", 8, (), "mvdr_fast_kernel<8, 1, %s>", None, None),
    "fast4k1": ("lcmv", 4, (-60.0,), "mvdr_fast_kernel<4, 2, %s>", None, None),
    "fast8k2": ("lcmv", 8, K2, "mvdr_fast_kernel<8, 3, %s>", None, None),
    "fast6": ("mvdr", 6, (), "mvdr_fast_kernel<6, 1, %s>", None, None),
    "cov12": ("mvdr", 12, (), "cov2d_kernel<1, 3, %s>", None, None),
    "cov12k2": ("lcmv", 12, K2, "cov2d_kernel<4, 2, %s>", None, None),
    "group8": ("mvdr", 8, (), "mvdr_lcmv_kernel<8, 1>", GROUP, None),
    "group8k5": ("lcmv", 8, K5, "mvdr_lcmv_kernel<8, 8>", GROUP, None),
    "track8": ("mvdr", 8, (), "mvdr_fast_track_kernel<8, 1, %s>", None, dict(track=1)),
}
_PW_NAMED = ("past_windows", "out_amp", "freq_mag_threshold")


def _pw(name, shape, P, hop, F, precision, env=None, seed=None, cuts=None, extra=None, named=_PW_NAMED):
    algo, M, interf, kern, shape_env, shape_extra = _PW_SHAPES[shape]
    kern = kern % ("false" if precision == MIXED else "true") if "%s" in kern else kern
    front = f"{'stft_small_kernel' if hop < 512 else 'stft_kernel'}<0, {'true' if precision == MIXED else 'false'}>"   # mixed: z48 spectra
    _add(name, algo, M, hop, F, _n(hop, front, kern), named, interf=interf, precision=precision, env={**(shape_env or {}), **(env or {})},
         seed=seed, cuts=cuts, extra={**(shape_extra or {}), **(extra or {})}, past_windows=P, **PW)


# every kernel at every window length, both precisions; the two precisions of a shape share their scene (and their oracle run)
for _i, _shape in enumerate(_PW_SHAPES):
    for _P in (1, 2, 3, 11, 64):
        _hop, _F = (64, 100) if _P == 64 else (512, 16)       # P = 64: the tile the plan picks by itself at F = 100
        for _prec in (REF, MIXED):
            _pw(f"pw{_P}-{_shape}-{'mixed' if _prec else 'ref'}", _shape, _P, _hop, _F, _prec, seed=7500 + 10 * _i + _P)
# P = 1, 2, 3: the leaving frame is, or sits next to, a slot of the ring of new frames -- tile lengths 1, 2, P and P + 1
for _P in (1, 2, 3):
    for _tile in sorted({1, 2, _P, _P + 1}):
        for _prec in (REF, MIXED):
            _pw(f"pw{_P}-tile{_tile}-{'mixed' if _prec else 'ref'}", "fast8", _P, 512, 16, _prec, env={"BF_MVDR_TILE": str(_tile)}, seed=7600 + _P)
            if _prec == REF:
                _pw(f"pw{_P}-tile{_tile}-k2", "fast8k2", _P, 512, 16, _prec, env={"BF_MVDR_TILE": str(_tile)}, seed=7610 + _P)
# P = 64, the limit: fewer frames than the window, exactly the window, one more
for _F in (3, 64, 65):
    for _shape in ("fast8", "cov12"):
        # (three frames never fill a window of ten either: F = 3 is about the warm-up alone and is not named for past_windows)
        _pw(f"pw64-{_shape}-f{_F}", _shape, 64, 64, _F, REF, seed=7700 + _F, named=_PW_NAMED[1:] if _F == 3 else _PW_NAMED)
# cuts shorter than the window; a checkpoint inside it
_pw("pw11-fast8-cuts", "fast8", 11, 256, 27, REF, cuts=(0, 1, 2, 5, 15, 27))
_pw("pw11-cov12-cuts", "cov12", 11, 256, 27, REF, cuts=(0, 1, 2, 5, 15, 27))
_pw("pw3-fast8-checkpoint", "fast8", 3, 512, 16, REF, cuts=(0, 2, 16), extra=dict(checkpoint=2))
_pw("pw3-cov12k2-checkpoint", "cov12k2", 3, 512, 16, REF, cuts=(0, 2, 16), extra=dict(checkpoint=2))

# ==== 5. smooth_size ==================================================================================================================
for _sz in (1, 2, 4, 5, 6, 8):
    _add(f"smooth{_sz}", "phasempf", 8, 512, 16, _n(512, "mpf_recursion_kernel", f"smooth4_kernel<{_sz}>", "smooth_state_kernel"), ("smooth_size",),
         smooth_size=_sz)
for _sz in (9, 33, 64):
    _add(f"smooth{_sz}", "phasempf", 8, 512, 16, _n(512, "mpf_recursion_kernel", "smooth_kernel", "smooth_state_kernel"), ("smooth_size",), smooth_size=_sz)
# the output pointer 4- but not 16-byte aligned: smooth4_kernel stores float4, so size 3 runs smooth_kernel (the C ABI accepts the pointer)
_add("smooth3-offset", "phasempf", 8, 512, 16, _n(512, "mpf_recursion_kernel", "smooth_kernel", "smooth_state_kernel"), (), extra=dict(offset=1),
     smooth_size=3)
# the 64-entry state is the whole previous batch
_add("smooth64-hop64", "phasempf", 8, 64, 128, _n(64, "mpf_recursion_kernel", "smooth_kernel", "smooth_state_kernel"), ("smooth_size",),
     extra=dict(per_hop=1), smooth_size=64, mpf_eta=0.05, mpf_rev_gamma=0.99)   # (the milder Lambda keeps more than a tenth of the bins off noise_floor)

# ==== 6. sample_rate ==================================================================================================================
_SR = ("sample_rate",)
for _sr in (16000.0, 44100.0):
    _t = f"sr{int(_sr)}"
    _add(f"{_t}-das", "das", 8, 512, 16, ["das_f64_sched_kernel", "das_f64_pair_kernel"], _SR, sample_rate=_sr)
    _add(f"{_t}-das-il", "das", 8, 512, 16, ["das_f64_sched_kernel", "das_f64_ring_kernel"], _SR, layout=INTERLEAVED, sample_rate=_sr)
    _add(f"{_t}-das-f32", "das", 8, 512, 16, ["das_fused_kernel<0, 4, 4, 1>"], _SR, extra=dict(f32=1), sample_rate=_sr)
    _add(f"{_t}-das-f32-hop256", "das", 8, 256, 32, ["das_fused_kernel<0, 4, 4, 2>"], _SR, extra=dict(f32=1), sample_rate=_sr)
    # 16 kHz: freq_max = 16000 lies above every bin, the Nyquist problems N/2 and N/2 + 1 (quirk Q1) are in band and the band rows of the
    # backward transform give way to the full spectrum
    _add(f"{_t}-mvdr", "mvdr", 8, 512, 16, _n(512, "stft_kernel<0, false>", "mvdr_fast_kernel<8, 1, true>",
                                             "istft_w64_kernel<false>" if _sr == 16000.0 else "istft_w64_kernel<true>"), _SR, sample_rate=_sr)
    _add(f"{_t}-lcmv12", "lcmv", 12, 512, 16, _n(512, "stft_kernel<0, false>", "cov2d_kernel<4, 2, true>"), _SR, interf=K2, sample_rate=_sr)
    _add(f"{_t}-gss", "gss", 8, 512, 16, _n(512, "gss_kernel<8, 4>"), _SR, interf=K2, sample_rate=_sr)
    # (phase at its launch values never takes the phase decision on these scenes: mag / N stays below mag_threshold = 0.05 in every bin)
    _add(f"{_t}-phase", "phase", 8, 512, 16, _n(512, "fused_tail_kernel<8, 4>"), _SR, sample_rate=_sr, **PHASE)
    _add(f"{_t}-phasempf", "phasempf", 8, 512, 16, _n(512, "fused_tail_kernel<8, 5>", "mpf_recursion_kernel"), _SR, sample_rate=_sr)
    _add(f"{_t}-gsc", "gsc", 8, 512, 16, _n(512, "gsc_align_kernel", "gsc_nlms_mw_kernel<8, 1, 2>"), _SR, sample_rate=_sr)

BY_NAME = {c.name: c for c in CASES}
ENVS = []                                  # the distinct non-empty environments, in order of appearance: one child process each
for _c in CASES:
    if _c.env and _c.env not in ENVS:
        ENVS.append(_c.env)


def env_id(env):
    return "-".join(f"{k[3:].lower()}{v}" for k, v in sorted(env.items()))


def params(c, **over):
    return make_params(c.algo, n_mics=c.M, interf=c.interf, hop=c.hop, theta=20.0, **{**c.over, **over})


def scene(c):
    """x [streams][M][F * hop] float32, planar (the GPU tests transpose it for a [sample][mic] handle), at the case's sample rate; the gss
    rows cases have no silent tail (tests/gss_sources_cases.py: behind a closed gate the rows r >= 1 are exact zeros)."""
    sr = c.over.get("sample_rate", 48000.0)
    kw = dict(silent_frac=0.0) if c.extra.get("rows") else {}
    return np.stack([make_scene(c.M, c.F, hop=c.hop, sr=sr, seed=c.seed + 100 * s, **kw) for s in range(c.streams)])


def compared_streams(c):
    return (0, 1, 31, c.streams - 1) if c.streams > 4 else tuple(range(c.streams))


def track_of(c):
    """The steering track [F] (phase / phasempf: an index into DIR_ANGLES every TRACK_EVERY frames, -1 = the handle's theta) or the
    column track [F, 1] (mvdr: tests/ctrack_cases.py's busy track over its MVDR_ANGLES)."""
    if c.algo == "mvdr":
        import ctrack_cases as cc
        return cc.mvdr_track(c.F, 7)
    return np.repeat(np.array([0, 2, 1, -1, 2, 0, 1, 2, 0] * 8, np.int32), TRACK_EVERY)[:c.F]


def oracle_key(c):
    """Cases with the same key share one oracle run (the two precisions and the tile lengths of a shape)."""
    return (c.algo, c.M, c.interf, c.hop, c.F, c.streams, tuple(sorted(c.over.items())), c.seed, tuple(sorted(c.extra.items())))


def reference(c, stream=0, **over):
    """The oracle's output for one stream of the case (with `over` on top of the case's parameters) -> (y [rows, F * hop] float32,
    Y [rows, F, N] complex128 or None for gsc); rows = look directions or gss's separated sources, 1 otherwise.  A tracked case drives
    the oracle hop by hop with the control calls of its track (tests/track_ref.py, tests/ctrack_ref.py); gss rows come from
    tests/gss_sources_ref.py and, post-filtered, tests/gss_postfilter_ref.py."""
    import oracle
    p = params(c, **over)
    x = scene(c)[stream]
    e = c.extra
    if e.get("rows"):
        from gss_sources_ref import gss_sources
        y, Y = gss_sources(p, x, [(c.F, oracle.OracleNode(p).weights())], e["rows"])
        if e.get("pf"):
            from gss_postfilter_cases import filtered
            y, Y = filtered(p, Y, len(c.interf) + 1)
        return np.asarray(y), np.asarray(Y)
    if e.get("track"):
        if c.algo == "mvdr":
            import ctrack_cases as cc
            import ctrack_ref
            y, Y, _ = ctrack_ref.oracle_ctracked(p, x, cc.MVDR_ANGLES, track_of(c), p["theta"])
        else:
            import track_ref
            y, Y = track_ref.oracle_tracked(p, x, DIR_ANGLES, track_of(c), p["theta"])
        return y[None], Y[None]
    if e.get("dirs"):
        outs = [oracle.OracleNode(dict(p, theta=th)).process(x, want_spectrum=True) for th in DIR_ANGLES[:e["dirs"]]]
        return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    y, Y = oracle.OracleNode(p).process(x, want_spectrum=c.algo != "gsc")
    return y[None], (None if Y is None else Y[None])


#: what `python tests/test_params_cpu.py` printed for this table (one line per oracle run; the two precisions and the tile lengths of a
#: shape share theirs): key = relative L2 of the oracle's output from the case with that key at its launch value, a<->b = with the twins'
#: values swapped, o2o = C++ oracle against its numpy restatement, busy = share of in-band bins off zero / noise_floor
FIGURES = """
mpf-m8: mcra_alphaS 1.5e-01 mcra_alphaD 5.6e-01 mcra_alphaD2 7.3e-01 mcra_delta 9.7e-02 mcra_L 7.7e-01 mpf_alphaS 9.5e-03 mpf_eta 6.7e-02
    mpf_rev_gamma 2.4e-01 mpf_rev_delta 3.9e-01 min_phase 4.7e-01 min_mag 4.0e-02 smooth_size 7.9e-01 out_amp 4.7e-01 noise_floor 9.0e-03
    mcra_alphaS<->mcra_alphaD 1.7e-01 mcra_alphaD<->mcra_alphaD2 1.8e-01 mpf_alphaS<->mcra_alphaS 7.5e-02 o2o 1e-15 busy 0.33
mpf-m16: mcra_alphaS 1.9e-01 mcra_alphaD 5.6e-01 mcra_alphaD2 7.0e-01 mcra_delta 7.2e-02 mcra_L 7.4e-01 mpf_alphaS 1.0e-02 mpf_eta 7.1e-02
    mpf_rev_gamma 2.3e-01 mpf_rev_delta 3.8e-01 min_phase 5.0e-01 min_mag 4.5e-02 smooth_size 8.2e-01 out_amp 4.7e-01 noise_floor 9.5e-03
    mcra_alphaS<->mcra_alphaD 1.5e-01 mcra_alphaD<->mcra_alphaD2 1.5e-01 mpf_alphaS<->mcra_alphaS 4.9e-02 o2o 8e-16 busy 0.31
mpf-s64: mcra_alphaS 4.1e-02 mcra_alphaD 6.5e-01 mcra_alphaD2 6.6e-01 mcra_delta 3.4e-02 mcra_L 6.7e-01 mpf_alphaS 7.4e-03 mpf_eta 6.4e-02
    mpf_rev_gamma 2.0e-01 mpf_rev_delta 3.3e-01 min_phase 4.6e-01 min_mag 3.4e-02 smooth_size 8.1e-01 out_amp 4.7e-01 noise_floor 9.3e-03
    mcra_alphaS<->mcra_alphaD 1.7e-01 mcra_alphaD<->mcra_alphaD2 2.1e-01 mpf_alphaS<->mcra_alphaS 1.5e-02 o2o 8e-16 busy 0.35
mpf-track-m8: mcra_alphaS 9.9e-02 mcra_alphaD 4.8e-01 mcra_alphaD2 5.4e-01 mcra_delta 3.2e-03 mcra_L 7.4e-01 mpf_alphaS 1.6e-02 mpf_eta
    8.3e-02 mpf_rev_gamma 2.2e-01 mpf_rev_delta 3.6e-01 min_phase 5.1e-01 min_mag 3.1e-02 smooth_size 6.8e-01 out_amp 4.7e-01 noise_floor
    1.5e-02 mcra_alphaS<->mcra_alphaD 1.1e-01 mcra_alphaD<->mcra_alphaD2 8.1e-02 mpf_alphaS<->mcra_alphaS 8.6e-03 busy 0.15
mpf-track-m16: mcra_alphaS 1.3e-01 mcra_alphaD 5.8e-01 mcra_alphaD2 5.6e-01 mcra_delta 4.4e-02 mcra_L 7.0e-01 mpf_alphaS 2.1e-02 mpf_eta
    9.7e-02 mpf_rev_gamma 2.4e-01 mpf_rev_delta 3.9e-01 min_phase 5.6e-01 min_mag 3.5e-02 smooth_size 8.3e-01 out_amp 4.7e-01 noise_floor
    2.0e-02 mcra_alphaS<->mcra_alphaD 1.4e-01 mcra_alphaD<->mcra_alphaD2 8.5e-02 mpf_alphaS<->mcra_alphaS 1.1e-02 busy 0.14
mpf-mixed: mcra_alphaS 1.7e-01 mcra_alphaD 5.8e-01 mcra_alphaD2 7.1e-01 mcra_delta 7.6e-02 mcra_L 7.5e-01 mpf_alphaS 9.3e-03 mpf_eta 6.7e-02
    mpf_rev_gamma 2.4e-01 mpf_rev_delta 4.0e-01 min_phase 4.7e-01 min_mag 5.3e-02 smooth_size 7.9e-01 out_amp 4.7e-01 noise_floor 8.5e-03
    mcra_alphaS<->mcra_alphaD 1.7e-01 mcra_alphaD<->mcra_alphaD2 1.6e-01 mpf_alphaS<->mcra_alphaS 6.4e-02 o2o 9e-16 busy 0.33
mpf-noise: mcra_alphaS 1.1e-01 mcra_alphaD 3.9e-01 mcra_alphaD2 1.6e+00 mcra_delta 4.7e-02 mcra_L 4.8e-01 mpf_alphaS 1.8e-02 mpf_eta 1.3e-01
    mpf_rev_gamma 2.4e-01 mpf_rev_delta 4.1e-01 min_phase 1.7e-01 min_mag 4.5e-02 smooth_size 8.1e-01 out_amp 4.7e-01
    mcra_alphaS<->mcra_alphaD 1.1e-01 mcra_alphaD<->mcra_alphaD2 1.9e-01 mpf_alphaS<->mcra_alphaS 3.3e-02 o2o 2e-15
mpf-mcra: mcra_alphaS 1.9e-01 mcra_alphaD 5.1e-01 mcra_alphaD2 7.5e-01 mcra_delta 8.4e-02 mcra_L 7.5e-01 min_phase 4.2e-01 min_mag 9.9e-02
    smooth_size 8.1e-01 out_amp 4.7e-01 noise_floor 3.5e-03 mcra_alphaS<->mcra_alphaD 1.5e-01 mcra_alphaD<->mcra_alphaD2 1.7e-01 o2o 7e-16
    busy 0.80
mpf-hop64: mcra_alphaS 6.6e-01 mcra_alphaD 2.0e-01 mcra_alphaD2 9.0e-01 mcra_delta 8.6e-02 mcra_L 5.6e-01 mpf_alphaS 1.3e-02 mpf_eta 7.5e-02
    mpf_rev_gamma 2.8e-01 mpf_rev_delta 5.9e-01 min_phase 5.6e-01 min_mag 5.1e-02 smooth_size 8.5e-01 out_amp 4.7e-01 noise_floor 3.3e-02
    mcra_alphaS<->mcra_alphaD 9.2e-02 mcra_alphaD<->mcra_alphaD2 5.6e-02 mpf_alphaS<->mcra_alphaS 6.7e-02 o2o 2e-14 busy 0.26
mpf-hop2048: mcra_alphaS 1.4e-01 mcra_alphaD 1.9e-01 mcra_alphaD2 1.3e-02 mcra_delta 2.3e-01 mcra_L 6.3e-01 mpf_alphaS 4.6e-03 mpf_eta
    4.9e-02 mpf_rev_gamma 1.2e-01 mpf_rev_delta 1.8e-01 min_phase 5.2e-01 min_mag 2.2e-02 smooth_size 8.4e-01 out_amp 4.7e-01 noise_floor
    3.2e-03 mcra_alphaS<->mcra_alphaD 8.7e-02 mcra_alphaD<->mcra_alphaD2 4.6e-02 mpf_alphaS<->mcra_alphaS 4.6e-02 o2o 6e-16 busy 0.37
mcra-m2: mcra_alphaS 1.2e-02 mcra_alphaD 2.6e+00 mcra_alphaD2 1.3e-01 mcra_delta 1.3e-02 mcra_L 2.6e-01 out_amp 1.1e+00
    mcra_alphaS<->mcra_alphaD 1.2e+00 mcra_alphaD<->mcra_alphaD2 2.9e+00 o2o 2e-14 busy 0.21
mcra-m2-il: mcra_alphaS 1.5e-02 mcra_alphaD 2.7e+00 mcra_alphaD2 1.4e-01 mcra_delta 2.4e-02 mcra_L 2.7e-01 out_amp 1.1e+00
    mcra_alphaS<->mcra_alphaD 1.3e+00 mcra_alphaD<->mcra_alphaD2 3.0e+00 o2o 9e-15 busy 0.22
mcra-m2-hop128: mcra_alphaS 5.5e-01 mcra_alphaD 3.5e+00 mcra_alphaD2 8.2e-01 mcra_delta 2.4e+00 mcra_L 7.9e-01 out_amp 1.1e+00
    mcra_alphaS<->mcra_alphaD 2.9e+00 mcra_alphaD<->mcra_alphaD2 1.5e+00 o2o 4e-15 busy 0.17
mcra-m2-noise: mcra_alphaS 6.7e-03 mcra_alphaD 7.5e-01 mcra_alphaD2 2.1e-01 mcra_delta 4.5e-03 mcra_L 1.2e-01 out_amp 1.1e+00
    mcra_alphaS<->mcra_alphaD 5.1e-01 mcra_alphaD<->mcra_alphaD2 8.3e-01 o2o 1e-15
gpf-r3: mcra_alphaS 2.1e-01 mcra_alphaD 9.0e-01 mcra_alphaD2 7.7e-01 mcra_delta 1.5e-01 mcra_L 7.0e-01 mpf_alphaS 5.3e-02 mpf_eta 2.9e-01
    mpf_rev_gamma 3.5e-01 mpf_rev_delta 5.3e-01 noise_floor 4.6e-03 mcra_alphaS<->mcra_alphaD 2.6e-01 mcra_alphaD<->mcra_alphaD2 2.4e-01
    mpf_alphaS<->mcra_alphaS 9.1e-02 busy 0.50
gpf-r3-lane: mcra_alphaS 1.2e-01 mcra_alphaD 9.8e-01 mcra_alphaD2 7.1e-01 mcra_delta 8.0e-02 mcra_L 6.6e-01 mpf_alphaS 5.6e-02 mpf_eta
    2.9e-01 mpf_rev_gamma 3.3e-01 mpf_rev_delta 4.9e-01 noise_floor 4.3e-03 mcra_alphaS<->mcra_alphaD 2.6e-01 mcra_alphaD<->mcra_alphaD2
    2.6e-01 mpf_alphaS<->mcra_alphaS 6.0e-02 busy 0.55
phase-m8: min_phase 5.4e-01 mag_mult 2.8e-01 mag_threshold 5.8e-01 o2o 6e-16
phase-m16: min_phase 5.4e-01 mag_mult 2.8e-01 mag_threshold 5.7e-01 o2o 7e-16
phase-m8-d3: min_phase 4.4e-01 mag_mult 4.5e-01 mag_threshold 4.7e-01
phase-track: min_phase 4.5e-01 mag_mult 4.3e-01 mag_threshold 4.8e-01
phase-hop128: min_phase 5.3e-01 mag_mult 2.9e-01 mag_threshold 5.6e-01 o2o 9e-16
phase-mixed: min_phase 5.4e-01 mag_mult 2.8e-01 mag_threshold 5.7e-01 o2o 6e-16
gss-k2: mu 1.9e-01 lambda_ 2.2e-02 out_amp 6.7e-01 freq_mag_threshold 1.6e+00 freq_min 2.4e-01 freq_max 1.2e+00 o2o 5e-16
gss-k5: mu 1.6e-01 lambda_ 5.3e-03 out_amp 6.7e-01 freq_mag_threshold 1.5e+00 freq_min 3.4e-01 freq_max 1.1e+00 o2o 6e-16
gss-k2-rows: mu 2.8e-01 lambda_ 2.4e-02 out_amp 6.7e-01 freq_mag_threshold 1.9e+00 freq_min 3.8e-01 freq_max 1.3e+00 o2o 5e-16
gss-k5-rows: mu 2.8e-01 lambda_ 8.7e-03 out_amp 6.7e-01 freq_mag_threshold 1.8e+00 freq_min 2.7e-01 freq_max 1.1e+00 o2o 5e-16
gss-k2-lane: mu 1.8e-01 lambda_ 2.1e-02 out_amp 6.7e-01 freq_mag_threshold 1.5e+00 freq_min 2.0e-01 freq_max 1.1e+00 o2o 5e-16
gss-k1-lane: mu 7.9e-02 lambda_ 3.4e-02 out_amp 6.7e-01 freq_mag_threshold 1.6e+00 freq_min 9.8e-02 freq_max 9.2e-01 o2o 5e-16
gss-k2-lane-rows: mu 2.9e-01 lambda_ 2.3e-02 out_amp 6.7e-01 freq_mag_threshold 1.5e+00 freq_min 2.6e-01 freq_max 9.1e-01 o2o 6e-16
gss-k1-lane-rows: mu 1.6e-01 lambda_ 2.8e-02 out_amp 6.7e-01 freq_mag_threshold 1.8e+00 freq_min 2.3e-01 freq_max 1.2e+00 o2o 6e-16
pw1-fast8-ref: past_windows 6.8e-01 out_amp 6.7e-01 freq_mag_threshold 3.5e+00 o2o 9e-14
pw2-fast8-ref: past_windows 6.7e-01 out_amp 6.7e-01 freq_mag_threshold 4.7e+00 o2o 2e-13
pw3-fast8-ref: past_windows 6.9e-01 out_amp 6.7e-01 freq_mag_threshold 4.6e+00 o2o 1e-13
pw11-fast8-ref: past_windows 1.1e-01 out_amp 6.7e-01 freq_mag_threshold 4.3e+00 o2o 1e-13
pw64-fast8-ref: past_windows 7.0e-01 out_amp 6.7e-01 freq_mag_threshold 1.4e-01 o2o 1e-13
pw1-fast4k1-ref: past_windows 6.9e-01 out_amp 6.7e-01 freq_mag_threshold 3.8e+00 o2o 5e-13
pw2-fast4k1-ref: past_windows 7.1e-01 out_amp 6.7e-01 freq_mag_threshold 4.0e+00 o2o 6e-14
pw3-fast4k1-ref: past_windows 3.9e-01 out_amp 6.7e-01 freq_mag_threshold 4.0e+00 o2o 1e-13
pw11-fast4k1-ref: past_windows 4.2e-02 out_amp 6.7e-01 freq_mag_threshold 3.4e+00 o2o 6e-14
pw64-fast4k1-ref: past_windows 3.0e-01 out_amp 6.7e-01 freq_mag_threshold 1.6e-01 o2o 9e-14
pw1-fast8k2-ref: past_windows 7.1e-01 out_amp 6.7e-01 freq_mag_threshold 4.3e+00 o2o 2e-13
pw2-fast8k2-ref: past_windows 5.4e-01 out_amp 6.7e-01 freq_mag_threshold 3.6e+00 o2o 1e-13
pw3-fast8k2-ref: past_windows 4.5e-01 out_amp 6.7e-01 freq_mag_threshold 4.0e+00 o2o 2e-13
pw11-fast8k2-ref: past_windows 6.3e-02 out_amp 6.7e-01 freq_mag_threshold 3.6e+00 o2o 1e-13
pw64-fast8k2-ref: past_windows 4.8e-01 out_amp 6.7e-01 freq_mag_threshold 1.5e-01 o2o 1e-13
pw1-fast6-ref: past_windows 5.7e-01 out_amp 6.7e-01 freq_mag_threshold 3.3e+00 o2o 1e-13
pw2-fast6-ref: past_windows 6.9e-01 out_amp 6.7e-01 freq_mag_threshold 3.8e+00 o2o 2e-13
pw3-fast6-ref: past_windows 6.8e-01 out_amp 6.7e-01 freq_mag_threshold 4.2e+00 o2o 1e-13
pw11-fast6-ref: past_windows 7.3e-02 out_amp 6.7e-01 freq_mag_threshold 4.4e+00 o2o 9e-14
pw64-fast6-ref: past_windows 5.9e-01 out_amp 6.7e-01 freq_mag_threshold 1.4e-01 o2o 1e-13
pw1-cov12-ref: past_windows 6.9e-01 out_amp 6.7e-01 freq_mag_threshold 3.8e+00 o2o 1e-13
pw2-cov12-ref: past_windows 7.7e-01 out_amp 6.7e-01 freq_mag_threshold 4.3e+00 o2o 2e-13
pw3-cov12-ref: past_windows 6.6e-01 out_amp 6.7e-01 freq_mag_threshold 4.5e+00 o2o 1e-13
pw11-cov12-ref: past_windows 5.6e-02 out_amp 6.7e-01 freq_mag_threshold 4.2e+00 o2o 2e-13
pw64-cov12-ref: past_windows 9.2e-01 out_amp 6.7e-01 freq_mag_threshold 1.7e-01 o2o 2e-13
pw1-cov12k2-ref: past_windows 6.1e-01 out_amp 6.7e-01 freq_mag_threshold 3.9e+00 o2o 1e-13
pw2-cov12k2-ref: past_windows 4.4e-01 out_amp 6.7e-01 freq_mag_threshold 4.1e+00 o2o 2e-13
pw3-cov12k2-ref: past_windows 3.7e-01 out_amp 6.7e-01 freq_mag_threshold 4.0e+00 o2o 1e-13
pw11-cov12k2-ref: past_windows 6.5e-02 out_amp 6.7e-01 freq_mag_threshold 3.6e+00 o2o 2e-13
pw64-cov12k2-ref: past_windows 6.8e-01 out_amp 6.7e-01 freq_mag_threshold 1.6e-01 o2o 2e-13
pw1-group8-ref: past_windows 6.4e-01 out_amp 6.7e-01 freq_mag_threshold 3.3e+00 o2o 1e-13
pw2-group8-ref: past_windows 6.1e-01 out_amp 6.7e-01 freq_mag_threshold 3.9e+00 o2o 1e-13
pw3-group8-ref: past_windows 6.7e-01 out_amp 6.7e-01 freq_mag_threshold 4.3e+00 o2o 8e-14
pw11-group8-ref: past_windows 5.9e-02 out_amp 6.7e-01 freq_mag_threshold 3.6e+00 o2o 1e-13
pw64-group8-ref: past_windows 7.0e-01 out_amp 6.7e-01 freq_mag_threshold 1.7e-01 o2o 1e-13
pw1-group8k5-ref: past_windows 2.9e-01 out_amp 6.7e-01 freq_mag_threshold 2.9e+00 o2o 4e-11
pw2-group8k5-ref: past_windows 6.1e-01 out_amp 6.7e-01 freq_mag_threshold 3.9e+00 o2o 2e-11
pw3-group8k5-ref: past_windows 1.6e-01 out_amp 6.7e-01 freq_mag_threshold 4.3e+00 o2o 9e-13
pw11-group8k5-ref: past_windows 1.8e-02 out_amp 6.7e-01 freq_mag_threshold 2.5e+00 o2o 4e-12
pw64-group8k5-ref: past_windows 2.3e-01 out_amp 6.7e-01 freq_mag_threshold 1.7e-01 o2o 8e-12
pw1-track8-ref: past_windows 7.6e-01 out_amp 6.7e-01 freq_mag_threshold 3.0e+00
pw2-track8-ref: past_windows 6.3e-01 out_amp 6.7e-01 freq_mag_threshold 3.7e+00
pw3-track8-ref: past_windows 6.9e-01 out_amp 6.7e-01 freq_mag_threshold 4.7e+00
pw11-track8-ref: past_windows 5.5e-02 out_amp 6.7e-01 freq_mag_threshold 3.6e+00
pw64-track8-ref: past_windows 7.3e-01 out_amp 6.7e-01 freq_mag_threshold 1.8e-01
pw1-tile1-ref: past_windows 6.1e-01 out_amp 6.7e-01 freq_mag_threshold 3.3e+00 o2o 1e-13
pw1-tile1-k2: past_windows 6.0e-01 out_amp 6.7e-01 freq_mag_threshold 4.6e+00 o2o 8e-14
pw2-tile1-ref: past_windows 6.9e-01 out_amp 6.7e-01 freq_mag_threshold 3.7e+00 o2o 2e-13
pw2-tile1-k2: past_windows 4.4e-01 out_amp 6.7e-01 freq_mag_threshold 4.3e+00 o2o 1e-13
pw3-tile1-ref: past_windows 7.0e-01 out_amp 6.7e-01 freq_mag_threshold 4.4e+00 o2o 1e-13
pw3-tile1-k2: past_windows 3.8e-01 out_amp 6.7e-01 freq_mag_threshold 4.0e+00 o2o 1e-13
pw64-fast8-f3: out_amp 6.7e-01 freq_mag_threshold 2.1e-01 o2o 1e-13
pw64-cov12-f3: out_amp 6.7e-01 freq_mag_threshold 2.7e-01 o2o 2e-13
pw64-fast8-f64: past_windows 6.2e-01 out_amp 6.7e-01 freq_mag_threshold 1.7e-01 o2o 1e-13
pw64-cov12-f64: past_windows 8.2e-01 out_amp 6.7e-01 freq_mag_threshold 1.8e-01 o2o 2e-13
pw64-fast8-f65: past_windows 6.3e-01 out_amp 6.7e-01 freq_mag_threshold 1.8e-01 o2o 1e-13
pw64-cov12-f65: past_windows 8.4e-01 out_amp 6.7e-01 freq_mag_threshold 2.1e-01 o2o 2e-13
pw11-fast8-cuts: past_windows 1.5e-01 out_amp 6.7e-01 freq_mag_threshold 1.4e+00 o2o 1e-13
pw11-cov12-cuts: past_windows 1.7e-01 out_amp 6.7e-01 freq_mag_threshold 1.3e+00 o2o 1e-13
pw3-fast8-checkpoint: past_windows 6.8e-01 out_amp 6.7e-01 freq_mag_threshold 4.1e+00 o2o 1e-13
pw3-cov12k2-checkpoint: past_windows 3.3e-01 out_amp 6.7e-01 freq_mag_threshold 3.8e+00 o2o 2e-13
smooth1: smooth_size 8.2e-01 o2o 2e-15 busy 0.15
smooth2: smooth_size 5.2e-01 o2o 9e-15 busy 0.16
smooth4: smooth_size 5.2e-01 o2o 4e-15 busy 0.16
smooth5: smooth_size 7.5e-01 o2o 8e-16 busy 0.16
smooth6: smooth_size 9.4e-01 o2o 1e-15 busy 0.16
smooth8: smooth_size 1.2e+00 o2o 2e-15 busy 0.15
smooth9: smooth_size 1.2e+00 o2o 1e-15 busy 0.15
smooth33: smooth_size 2.8e+00 o2o 1e-15 busy 0.15
smooth64: smooth_size 3.4e+00 o2o 2e-15 busy 0.16
smooth3-offset: o2o 1e-15 busy 0.16
smooth64-hop64: smooth_size 5.1e+00 o2o 8e-15 busy 0.11
sr16000-das: sample_rate 1.0e+00 o2o 4e-16
sr16000-das-il: sample_rate 1.0e+00 o2o 4e-16
sr16000-das-f32: sample_rate 1.0e+00 o2o 4e-16
sr16000-das-f32-hop256: sample_rate 1.0e+00 o2o 4e-16
sr16000-mvdr: sample_rate 1.0e+00 o2o 1e-13
sr16000-lcmv12: sample_rate 1.0e+00 o2o 2e-13
sr16000-gss: sample_rate 9.9e-01 o2o 4e-16
sr16000-phase: sample_rate 5.9e-01 o2o 6e-16
sr16000-phasempf: sample_rate 1.0e+00 o2o 3e-15 busy 0.19
sr16000-gsc: sample_rate 1.0e+00 o2o 0e+00
sr44100-das: sample_rate 8.8e-01 o2o 4e-16
sr44100-das-il: sample_rate 8.9e-01 o2o 4e-16
sr44100-das-f32: sample_rate 8.9e-01 o2o 4e-16
sr44100-das-f32-hop256: sample_rate 8.9e-01 o2o 4e-16
sr44100-mvdr: sample_rate 9.7e-01 o2o 1e-13
sr44100-lcmv12: sample_rate 9.9e-01 o2o 2e-13
sr44100-gss: sample_rate 8.3e-01 o2o 4e-16
sr44100-phase: sample_rate 5.5e-01 o2o 1e-15
sr44100-phasempf: sample_rate 8.3e-01 o2o 9e-16 busy 0.17
sr44100-gsc: sample_rate 9.0e-01 o2o 0e+00
"""
