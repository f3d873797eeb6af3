"""gss's multi-source post-filter (bf_config.gss_postfilter): what can be checked without a GPU -- the numpy reference of the GPU tests
against the phasempf oracle, the sensitivity of the filter to the rounding of its inputs on the shapes those tests use, and the host
side (config, yaml, argument checks, launch plan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from chain_plan_util import ALGO, PLAN, SHAPE, SHAPE_DEFAULTS, chain_kernels, chain_plan
from conftest import rel_l2
from gss_postfilter_cases import PF_CASES, filtered, pf_base, pf_params, pf_ref, pf_rows, sem_pf_ref
from gss_postfilter_ref import postfilter
from gss_sources_cases import CASES, SEM, case_ref, case_streams, sem_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 1e-7    # the suite's floor for two roundings of the same inputs, per-frame relative L2 (tests/test_gss_sources_cpu.py)
QUIET = 1e-6    # no filtered row r < S may have a frame this far below row 0's


# ---- the reference against the phasempf oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [{}, {"out_only_noise": 1}, {"out_only_mcra": 1}], ids=["full", "only_noise", "only_mcra"])
def test_row0_of_two_rows_is_phasempf_bit_for_bit(over):
    """phasempf feeds the very block with its phase mask and the mask's negative: postfilter on (soi, inter) with S = 2 gives a row 0
    equal to oracle.np_oracle.phasempf_bins bit for bit (out_amp = 1; mcra_L = 5: the search window resets at frames 6 and 11)."""
    from beamform_amd.params import make_params
    from beamform_amd.synth import make_scene
    from oracle import np_oracle
    M, F = 8, 12
    p = make_params("phasempf", n_mics=M, theta=20.0, out_amp=1.0, mcra_L=5, **over)
    X = np_oracle.stft(p, make_scene(M, F, seed=77))
    w = np_oracle.steering(p, p["theta"])
    N = X.shape[2]
    thr = p["min_phase"] * np.pi / 180
    rows = np.zeros((2, F, N), np.complex128)
    for t in range(F):   # np_oracle.phasempf_bins lines 207-216
        x = X[t]
        mag = np.abs(x).sum(axis=0) / M
        pha = np.angle(x[0])
        aligned = np.angle(np.conj(w) * x)
        dmean = np_oracle._pair_phase_mean(aligned.T)
        is_soi = dmean < thr
        msoi = np.where(is_soi, mag, mag * p["min_mag"])
        mint = np.where(is_soi, mag * p["min_mag"], mag)
        soi = msoi * np.cos(pha) + 1j * (msoi * np.sin(pha))
        inter = mint * np.cos(pha) + 1j * (mint * np.sin(pha))
        soi[0] = x[0, 0]; inter[0] = x[0, 0]
        rows[0, t], rows[1, t] = soi, inter
    want = np_oracle.phasempf_bins(p, X, w)
    got = postfilter(p, rows, 2)
    assert want.any() and np.array_equal(got[0], want)
    assert np.array_equal(postfilter(p, rows, np.full(F, 2))[0], want)


def test_rows_beyond_the_source_count_are_left_alone():
    """S_t per frame: a row that does not exist yet is neither filtered nor does its state advance -- when it appears it starts cold."""
    p = pf_params("g8")
    _, Y = case_ref("g8")
    F = Y.shape[1]
    S_t = np.array([2] * 10 + [3] * (F - 10))
    out = postfilter(p, Y, S_t)
    assert np.array_equal(out[2, :10], Y[2, :10])
    cold = postfilter(p, Y[:, 10:], 3)                       # row 2 from a cold start at frame 10 ...
    warm = postfilter(p, Y, 3)
    rows01 = postfilter(p, Y[:2], 2)                         # ... while rows 0 and 1 saw two sources before it
    assert np.array_equal(out[:2, :10], rows01[:, :10])
    assert not np.array_equal(out[2, 10:], warm[2, 10:])
    # row 2's block sees the same soi and int2 from frame 10 on, from a zeroed state: the cold run's row 2
    assert np.array_equal(out[2, 10:], cold[2])


# ---- a condition on the inputs ------------------------------------------------------------------------------------------------------------
def _sensitivity(Ya, Yb, rows_frames):
    for r, t0, t1 in rows_frames:
        for t in range(t0, t1):
            n0, nr = np.linalg.norm(Ya[0, t]), np.linalg.norm(Ya[r, t])
            assert nr >= QUIET * n0, (r, t, nr, n0)
            e = rel_l2(Yb[r, t], Ya[r, t])
            assert e < FLOOR, (r, t, e)


@pytest.mark.parametrize("name", list(PF_CASES))
def test_the_filter_does_not_amplify_the_rounding_of_its_inputs(name):
    """A condition on the INPUTS: on every case the GPU tests use, feeding the filter with the rows of gss_sources summed serially
    or pairwise over the microphones moves no frame of a filtered row r < S by 1e-7 (no threshold of the block -- the noise update,
    the floor -- flips on a bin that matters), and no filtered row has a frame below 1e-6 of row 0's norm.  So 1e-5 per row on the
    GPU is a statement about the kernels."""
    base = pf_base(name)
    S = min(len(CASES[base]["interf"]) + 1, pf_rows(name))
    F = CASES[base]["F"]
    for s in case_streams(base):
        _, Ya = pf_ref(name, s, "serial")
        _, Yb = pf_ref(name, s, "pairwise")
        _sensitivity(Ya, Yb, [(r, 0, F) for r in range(S)])
        _, Y = pf_ref(name, s)
        _sensitivity(Y, Ya, [(r, 0, F) for r in range(S)])


@pytest.mark.parametrize("retarget", [True, False])
def test_the_stream_semantics_case_is_as_insensitive(retarget):
    cuts, F = SEM["cuts"], SEM["F"]
    _, Ya = sem_pf_ref(None, retarget, "serial")
    _, Yb = sem_pf_ref(None, retarget, "pairwise")
    _sensitivity(Ya, Yb, [(0, 0, F), (1, 0, F), (2, cuts[3], F)])
    _, Y = sem_ref(None, retarget)
    assert np.array_equal(sem_pf_ref(None, retarget)[1][2, :cuts[3]], Y[2, :cuts[3]]) and not Y[2, :cuts[3]].any()


def _floor_share(p, Yf_row, Y_row):
    """share of the in-band non-zero input bins of a row that end on noise_floor"""
    live = Y_row != 0
    live[:, 0] = False
    return float((np.abs(np.abs(Yf_row[live]) - p["noise_floor"]) < 1e-15).mean())


def test_most_of_row0_is_not_on_the_noise_floor():
    """A filter that floored (nearly) everything would make every check of Lambda vacuous: at the launch values fewer than 0.9 of row
    0's in-band bins end on noise_floor, at the milder set fewer than 0.5."""
    _, Y = case_ref("g8")
    for name, bar in (("g8", 0.9), ("g8_mild", 0.5)):
        p = pf_params(name)
        share = _floor_share(p, pf_ref(name)[1][0], Y[0])
        print(f"{name}: share of row 0 on the noise floor {share:.3f}")
        assert share < bar, (name, share)
    p = {**pf_params("g8"), "mcra_L": 50}     # the launch values with phasempf.launch's own window length
    share = _floor_share(p, filtered(p, Y, 3)[1][0], Y[0])
    print(f"g8, mcra_L = 50: share of row 0 on the noise floor {share:.3f}")
    assert share < 0.9, share


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
def test_config_field_yaml_key_and_argument_checks():
    from beamform_amd import capi
    from beamform_amd.params import make_params
    lib = capi.load()
    c = capi.BfConfig()
    c.gss_postfilter = 7
    assert lib.bf_config_init(C.byref(c), 3) == 0 and c.gss_postfilter == 0
    assert lib.bf_config_parse_yaml(C.byref(c), b"mu: 0.002\ngss_postfilter: 1\n") == 0
    assert c.gss_postfilter == 1 and c.mu == 0.002 and c.gss_out_sources == 0
    assert make_params("gss")["gss_postfilter"] == 0
    assert capi.config_from_params(make_params("gss", gss_postfilter=1)).gss_postfilter == 1
    assert capi.config_from_params(make_params("gss"), gss_postfilter=1).gss_postfilter == 1
    assert capi.config_from_params(make_params("gss")).gss_postfilter == 0
    # bad values are BF_EINVAL, checked with the other argument checks: before any device work, so also without a device
    h = C.c_void_p()
    for algo, v in (("gss", 2), ("gss", -1), ("das", 1), ("lcmv", 1), ("phasempf", 1)):
        cfg = capi.config_from_params(make_params(algo, n_mics=8))
        cfg.gss_postfilter = v
        assert lib.bf_create(C.byref(cfg), C.byref(h)) == -22, (algo, v)
        assert b"gss_postfilter" in lib.bf_last_error(None)
    for algo, v in (("gss", 0), ("gss", 1), ("das", 0)):      # accepted: the next check (or the device) answers
        cfg = capi.config_from_params(make_params(algo, n_mics=8))
        cfg.gss_postfilter = v
        rc = lib.bf_create(C.byref(cfg), C.byref(h))
        assert rc in (0, -19), (algo, v, rc)
        if rc == 0:
            lib.bf_destroy(h)
    cfg = capi.config_from_params(make_params("gss", n_mics=8))
    cfg.gss_postfilter = 1
    assert lib.bf_shard_halo(C.byref(cfg)) == -1


@pytest.fixture(scope="module")
def pf_lib(emul_lib):
    so = os.path.join(ROOT, "tests", "host_emul", "libemul_gss_pf.so")
    src = os.path.join(ROOT, "tests", "host_emul", "emul_gss_pf.cpp")
    hdr = os.path.join(ROOT, "beamform_amd", "csrc", "chain_plan.hpp")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.emul_chain_plan_pf.restype = None
    lib.emul_chain_plan_pf.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def _plan_pf(lib, rows, pf, **shape):
    s = {**SHAPE_DEFAULTS, **shape}
    vin = (C.c_long * len(SHAPE))(*[int(s[k]) for k in SHAPE])
    out = (C.c_long * (len(PLAN) + 3))()
    lib.emul_chain_plan_pf(vin, rows, pf, out)
    return dict(zip(PLAN + ("rows", "postfilter", "post_rp"), out))


def test_chain_plan_flags_the_filter_and_changes_nothing_else(emul_lib, pf_lib):
    """Field 0: the plan of today in every member.  Field 1: the same kernels, template arguments and sizes in front of the filter
    (it works in place: Yh does not grow), the filter flagged with the rows padded to a power of two.  Other nodes ignore the field."""
    rng = np.random.default_rng(6)
    for i in range(200):
        hop = int(2 ** rng.integers(6, 13))
        N = 2 * hop
        shape = dict(algo=ALGO["gss"], n_fft=N, layout=int(rng.integers(0, 2)), n_mics=int(rng.integers(1, 33)), n_streams=int(rng.integers(1, 301)),
                     n_dirs=int(rng.integers(1, 4)), kp1=int(rng.integers(1, 17)), precision=int(rng.integers(0, 2)), dump=bool(rng.integers(0, 2)),
                     n_frames=int(rng.integers(1, 200)), n_cus=int(rng.integers(1, 305)))
        base = chain_plan(emul_lib, **shape)
        R = int(rng.integers(0, 17))
        off = _plan_pf(pf_lib, R, 0, **shape)
        assert off.pop("postfilter") == 0 and off.pop("post_rp") == 0
        rows = off.pop("rows")
        assert rows == max(R, 1)
        if R <= 1:
            assert off == base, shape
        on = _plan_pf(pf_lib, R, 1, **shape)
        assert on.pop("postfilter") == 1
        rp = on.pop("post_rp")
        assert rp in (1, 2, 4, 8, 16) and rp >= max(R, 1) and (rp == 1 or rp // 2 < max(R, 1)), (R, rp)
        assert on.pop("rows") == rows and on == off, shape                       # every other member, sizes included
        assert chain_kernels(on, N) == chain_kernels(base, N)
    for algo in ("das", "mvdr", "lcmv", "phase", "phasempf", "mcra", "gsc"):
        shape = dict(algo=ALGO[algo], n_fft=1024, n_mics=8, n_streams=3, n_frames=20, n_cus=256, band_yh_lo=3, band_yh_hi=341)
        d = _plan_pf(pf_lib, 1, 1, **shape)
        assert d.pop("postfilter") == 0 and d.pop("post_rp") == 0 and d.pop("rows") == 1 and d == chain_plan(emul_lib, **shape), algo


def test_the_silent_tail_case_is_as_insensitive():
    """The scene with a silent tail (tests/test_gss_postfilter_gpu.py): rows 1 and 2 behind the closed gate are exact zeros in both
    roundings and come out on noise_floor in both."""
    from gss_postfilter_cases import SILENT, silent_ref
    F = SILENT["F"]
    _, Ya = silent_ref("serial")
    _, Yb = silent_ref("pairwise")
    _sensitivity(Ya, Yb, [(r, 0, F) for r in range(3)])
    _sensitivity(silent_ref()[1], Ya, [(r, 0, F) for r in range(3)])
