"""CPU suite (no GPU): host-side logic of the product -- the kernels' algebra run through the CPU
emulation harness, the C ABI surface, the YAML reader, and the loud failure without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene
from conftest import ROOT, rel_l2

P = C.c_void_p


def _ptr(a):
    return a.ctypes.data_as(P)


def test_emulated_fft32_and_fft1024(emul_lib):
    rng = np.random.default_rng(0)
    for dit in (0, 1):
        for d in (-1, 1):
            x = rng.standard_normal(32) + 1j * rng.standard_normal(32)
            o = np.empty(32, np.complex128)
            emul_lib.emul_fft32(_ptr(x), _ptr(o), d, dit)
            ref = np.fft.fft(x) if d < 0 else np.fft.ifft(x) * 32
            assert rel_l2(o, ref) < 1e-14
    for use_float, tol in ((0, 1e-14), (1, 5e-7)):
        for d in (-1, 1):
            x = rng.standard_normal(1024) + 1j * rng.standard_normal(1024)
            o = np.empty(1024, np.complex128)
            emul_lib.emul_fft1024(_ptr(x), _ptr(o), d, use_float)
            ref = np.fft.fft(x) if d < 0 else np.fft.ifft(x) * 1024
            assert rel_l2(o, ref) < tol


def test_emulated_small_and_split_transforms(emul_lib):
    """fft_small.hpp (N = 32 x NL: 1024 / N frames side by side through one transpose plane, an NL-point second pass per frame -- the transforms of
    stft_small_kernel / istft_small_kernel) and the radix-2 steps around FFT-1024 that istft_split_kernel / stft_bins_split_kernel use at N = 2048,
    instantiated on the CPU against numpy: index maps, twiddles, the one-transform backward path of a real frame."""
    rng = np.random.default_rng(7)
    for n in (512, 256, 128):
        g = 1024 // n
        for d in (-1, 1):
            x = rng.standard_normal((g, n)) + 1j * rng.standard_normal((g, n))
            o = np.empty((g, n), np.complex128)
            assert emul_lib.emul_fft_small(n, _ptr(x), _ptr(o), d) == 0
            ref = np.fft.fft(x, axis=1) if d < 0 else np.fft.ifft(x, axis=1) * n
            assert rel_l2(o, ref) < 1e-14
    x = rng.standard_normal(2048) + 1j * rng.standard_normal(2048)
    o = np.empty(2048, np.complex128)
    emul_lib.emul_fft2048_split(_ptr(x), _ptr(o), -1)
    assert rel_l2(o, np.fft.fft(x)) < 1e-14
    yr = rng.standard_normal(2048)           # backward: the spectrum of a real frame comes back from ONE complex FFT-1024
    Y = np.fft.fft(yr)
    back = np.empty(2048)
    emul_lib.emul_fft2048_split(_ptr(Y), _ptr(back), 1)
    assert rel_l2(back, yr * 2048) < 1e-14


def test_emulated_fft2048_on_a_full_wavefront(emul_lib):
    """N = 2048 = 32 registers x 64 lanes (das_fused_wave2048_kernel): the two-half transpose plane read as one 64-column transform and the
    radix-2 stage between the halves of the wavefront, both directions, against numpy."""
    rng = np.random.default_rng(11)
    for use_float, tol in ((0, 1e-14), (1, 5e-7)):
        for d in (-1, 1):
            x = rng.standard_normal(2048) + 1j * rng.standard_normal(2048)
            o = np.empty(2048, np.complex128)
            emul_lib.emul_fft2048_wave(_ptr(x), _ptr(o), d, use_float)
            ref = np.fft.fft(x) if d < 0 else np.fft.ifft(x) * 2048
            assert rel_l2(o, ref) < tol


def test_emulated_fft1024_w64(emul_lib):
    """64-lane x 16-point three-pass factorisation (fft1024_w64.hpp): index maps and twiddles."""
    rng = np.random.default_rng(1)
    for use_float, tol in ((0, 1e-14), (1, 5e-7)):
        for d in (-1, 1):
            x = rng.standard_normal(1024) + 1j * rng.standard_normal(1024)
            o = np.empty(1024, np.complex128)
            emul_lib.emul_fft1024_w64(_ptr(x), _ptr(o), d, use_float)
            ref = np.fft.fft(x) if d < 0 else np.fft.ifft(x) * 1024
            assert rel_l2(o, ref) < tol
    for d in (-1, 1):  # the fp64 kernel's exchange: segments rotated by 4 b columns, the shift absorbed by the tw2' table
        x = rng.standard_normal(1024) + 1j * rng.standard_normal(1024)
        o = np.empty(1024, np.complex128)
        emul_lib.emul_fft1024_w64_rot(_ptr(x), _ptr(o), d)
        ref = np.fft.fft(x) if d < 0 else np.fft.ifft(x) * 1024
        assert rel_l2(o, ref) < 1e-14


@pytest.mark.parametrize("M,theta", [(8, 20.0), (4, 0.0), (3, -75.0), (16, 135.0), (1, 0.0)])
def test_emulated_fused_das_matches_oracle(emul_lib, M, theta):
    """Pair packing + Hermitian-part gains + unpaired inverse, in fp32 exactly as the kernel does it."""
    import oracle
    F = 10
    p = make_params("das", n_mics=M, theta=theta)
    x = make_scene(M, F, seed=31 + M)
    y_ref, _ = oracle.OracleNode(p).process(x)
    y = np.empty(F * 512, np.float32)
    mx = np.array([m[0] for m in p["mics"]])
    my = np.array([m[1] for m in p["mics"]])
    emul_lib.emul_das_fused(M, 512, C.c_double(48000.0), _ptr(mx), _ptr(my), C.c_double(theta), _ptr(x), C.c_long(F), _ptr(y))
    assert rel_l2(y, y_ref) < 1e-6


@pytest.mark.parametrize("M,theta,F", [(8, 20.0, 9), (5, -110.0, 6), (1, 0.0, 3)])
def test_emulated_frame_pair_das_matches_oracle(emul_lib, M, theta, F):
    """das_f64_pair_kernel's formulation on the CPU with the kernel's own gain table and addressing (geometry.hpp das_mic_gains_w64_f64:
    bins 0 .. 512 in rows of 65, mirror bins read from row (3 - g, 3 - k3) column 64 - lane and conjugated): two frames of a microphone per
    transform, real / imaginary part of ONE backward transform = the two frames.  Odd frame counts end on a lone frame."""
    import oracle
    p = make_params("das", n_mics=M, theta=theta)
    x = make_scene(M, F, seed=77 + M)
    y_ref, _ = oracle.OracleNode(p).process(x)
    y = np.empty(F * 512, np.float32)
    mx = np.array([m[0] for m in p["mics"]])
    my = np.array([m[1] for m in p["mics"]])
    emul_lib.emul_das_pair_f64(M, C.c_double(48000.0), _ptr(mx), _ptr(my), C.c_double(theta), _ptr(x), C.c_long(F), _ptr(y))
    assert rel_l2(y, y_ref) < 2e-7   # double arithmetic up to the float stores


@pytest.mark.parametrize("hop,M,F", [(256, 8, 11), (128, 3, 14), (64, 6, 21)])
def test_emulated_frame_interleaving_das_matches_oracle(emul_lib, hop, M, F):
    """das_fused_small_kernel's formulation on the CPU: 1024 / N consecutive frames interleaved into one 1024-point sequence, the N-point
    pair gains repeated (geometry.hpp das_pair_gains_interleaved) -- the N-point chain of every frame is the 1024-point chain of the
    interleaved sequence.  Frame counts that are not multiples of the group size end on a partial group."""
    import oracle
    p = make_params("das", n_mics=M, theta=40.0, hop=hop)
    x = make_scene(M, F, hop=hop, seed=5 + hop)
    y_ref, _ = oracle.OracleNode(p).process(x)
    y = np.empty(F * hop, np.float32)
    mx = np.array([m[0] for m in p["mics"]])
    my = np.array([m[1] for m in p["mics"]])
    emul_lib.emul_das_small(M, hop, C.c_double(48000.0), _ptr(mx), _ptr(my), C.c_double(40.0), _ptr(x), C.c_long(F), _ptr(y))
    assert rel_l2(y, y_ref) < 1e-6   # fp32 gain table


def test_host_geometry_matches_oracle(emul_lib):
    import oracle
    p = make_params("das", n_mics=8, theta=57.0)
    node = oracle.OracleNode(p)
    f = np.empty(1024)
    emul_lib.emul_freqs(1024, C.c_double(48000.0), _ptr(f))
    assert np.array_equal(f, node.freqs())
    h = np.empty(1024)
    emul_lib.emul_hann(1024, _ptr(h))
    assert np.array_equal(h, node.hann())
    mx = np.array([m[0] for m in p["mics"]])
    my = np.array([m[1] for m in p["mics"]])
    tau = np.empty(8)
    emul_lib.emul_delays(8, _ptr(mx), _ptr(my), C.c_double(57.0), _ptr(tau))
    assert np.array_equal(tau, node.delays())


def test_library_exports_every_declared_symbol():
    from beamform_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "bfcore.h")).read()
    declared = set(re.findall(r"\b(bf_[a-z_0-9]+)\s*\(", header))
    assert declared == set(capi.EXPORTS), declared ^ set(capi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert b"bfcore" in lib.bf_version()


def test_config_defaults_are_the_launch_file_values():
    from beamform_amd import capi
    lib = capi.load()
    c = capi.BfConfig()
    assert lib.bf_config_init(C.byref(c), 1) == 0       # mvdr.launch:6-10
    assert (c.past_windows, c.freq_mag_threshold, c.freq_max, c.freq_min, c.out_amp) == (10, 0.001, 16000.0, 100.0, 1.0)
    assert (c.n_mics, c.hop, c.sample_rate) == (3, 512, 48000.0)   # aira3, beamform_config.yaml:15-17
    assert (c.mic_x[2], c.mic_y[2]) == (-0.156, -0.090)
    assert lib.bf_config_init(C.byref(c), 5) == 0       # phasempf.launch
    assert (c.min_phase, c.min_mag, c.smooth_size, c.mcra_L, c.out_amp) == (30.0, 0.05, 3, 50, 2.5)
    assert lib.bf_config_init(C.byref(c), 3) == 0       # gss.launch
    assert (c.out_amp, c.mu, c.lambda_) == (0.1, 0.001, 0.0)
    assert lib.bf_config_init(C.byref(c), 4) == 0       # phase: fallbacks of phase.cpp:180,187 (Q14)
    assert (c.min_phase, c.mag_mult, c.mag_threshold) == (10.0, 0.1, 0.05)
    assert lib.bf_config_init(C.byref(c), 9) != 0


YAML = b"""verbose: true
initial_angle: 12.5

#aira3
#mic0: {id: 0, x:  9.000, y:  9.000}
mic0:  {id:  0, x:  0.158, y:  0.115, z:  0.000}
mic1:  {id:  1, x:  0.158, y: -0.115, z:  0.000}
mic2:  {id:  2, x: -0.045, y:  0.000, z:  0.000}
mic3:  {id:  3, x: -0.050, y: -0.188, z:  0.000}
mic5:  {id:  5, x: 1, y: 1}

angle_interf1:  -60.0
angle_interf2:  90
angle_interf3:  181.0
angle_interf4:  10.0
past_windows: 12
freq_max: 8000
MCRA_L: 20
lambda: 0.5
write_file_path: ''
"""


def test_yaml_reader_follows_handle_params():
    """util.h:82-113: mics consumed until the first missing index, interferers until the first |angle| > 180."""
    from beamform_amd import capi
    lib = capi.load()
    c = capi.BfConfig()
    lib.bf_config_init(C.byref(c), 2)
    assert lib.bf_config_parse_yaml(C.byref(c), YAML) == 0
    assert c.theta == 12.5 and c.verbose == 1
    assert c.n_mics == 4 and (c.mic_x[3], c.mic_y[3]) == (-0.050, -0.188)      # mic4 missing -> mic5 ignored
    assert c.n_interf == 2 and (c.interf_angle[0], c.interf_angle[1]) == (-60.0, 90.0)
    assert (c.past_windows, c.freq_max, c.mcra_L, c.lambda_) == (12, 8000.0, 20, 0.5)
    path = os.path.join(ROOT, "tests", "golden", "_tmp_cfg.yaml")
    with open(path, "wb") as f:
        f.write(YAML)
    try:
        c2 = capi.BfConfig()
        lib.bf_config_init(C.byref(c2), 0)
        assert lib.bf_config_load_yaml(C.byref(c2), path.encode()) == 0 and c2.n_mics == 4
        assert lib.bf_config_load_yaml(C.byref(c2), b"/nonexistent.yaml") == -2
    finally:
        os.remove(path)


#: every parameter key of the launch files -> its bf_config field; the second table: the spellings the mcra node reads (mcra.cpp:180-217)
YAML_KEYS = {
    "initial_angle": "theta", "past_windows": "past_windows", "freq_mag_threshold": "freq_mag_threshold", "freq_max": "freq_max",
    "freq_min": "freq_min", "out_amp": "out_amp", "interf_angle_threshold": "interf_angle_threshold", "mu": "mu", "lambda": "lambda_",
    "min_phase": "min_phase", "mag_mult": "mag_mult", "mag_threshold": "mag_threshold", "min_mag": "min_mag", "smooth_size": "smooth_size",
    "MCRA_alphaS": "mcra_alphaS", "MCRA_alphaD": "mcra_alphaD", "MCRA_alphaD2": "mcra_alphaD2", "MCRA_delta": "mcra_delta", "MCRA_L": "mcra_L",
    "MPF_alphaS": "mpf_alphaS", "MPF_eta": "mpf_eta", "MPF_rev_gamma": "mpf_rev_gamma", "MPF_rev_delta": "mpf_rev_delta",
    "noise_floor": "noise_floor", "out_only_noise": "out_only_noise", "out_only_mcra": "out_only_mcra",
    "use_vad": "gsc_use_vad", "vad_threshold": "gsc_vad_threshold", "mu0": "gsc_mu0", "mu_max": "gsc_mu_max", "filter_size": "gsc_filter_size",
    "rosjack_window_size": "hop", "rosjack_sample_rate": "sample_rate", "gss_out_sources": "gss_out_sources", "gss_postfilter": "gss_postfilter",
}
YAML_KEYS_MCRA = {"alphaS": "mcra_alphaS", "alphaD": "mcra_alphaD", "alphaD2": "mcra_alphaD2", "delta": "mcra_delta", "L": "mcra_L"}


def test_yaml_reader_puts_every_key_into_its_own_field():
    """Every key gets a value no other key has (integers, so that the int fields keep theirs): a reader that stores one twin into the
    other's field -- alphaS / alphaD, MCRA_alphaS / MPF_alphaS, mu / mu0 -- or drops a key shows.  Both spellings of the MCRA keys."""
    from beamform_amd import capi
    lib = capi.load()
    source = open(os.path.join(ROOT, "beamform_amd", "csrc", "config.cpp")).read()
    fields = {n for n, _ in capi.BfConfig._fields_}
    for algo, table, first in ((5, YAML_KEYS, 101), (6, {**YAML_KEYS, **YAML_KEYS_MCRA}, 301)):
        assert set(table.values()) <= fields
        for spelled in ((YAML_KEYS,) if algo == 5 else (YAML_KEYS, YAML_KEYS_MCRA)):   # one spelling at a time: the two write the same field
            want = {key: first + 2 * i for i, key in enumerate(spelled)}
            assert len(set(want.values())) == len(want)
            c = capi.BfConfig()
            assert lib.bf_config_init(C.byref(c), algo) == 0
            before = {f: getattr(c, f) for f in set(table.values())}
            text = "".join(f"{key}: {v}\n" for key, v in want.items()).encode()
            assert lib.bf_config_parse_yaml(C.byref(c), text) == 0
            for key, v in want.items():
                assert getattr(c, spelled[key]) == v, (algo, key, spelled[key], getattr(c, spelled[key]))
            for f in set(table.values()) - set(spelled.values()):   # and nothing else moved
                assert getattr(c, f) == before[f], f
    # the unprefixed spellings belong to the mcra node alone
    c = capi.BfConfig()
    lib.bf_config_init(C.byref(c), 5)
    assert lib.bf_config_parse_yaml(C.byref(c), b"alphaS: 0.5\nL: 7\n") == 0 and (c.mcra_alphaS, c.mcra_L) == (0.95, 50)
    # the table above is the reader's whole key list
    read = set(re.findall(r'key == "([A-Za-z_0-9]+)"', source)) | set(re.findall(r"BF_KEY_[DI]\(([a-z_0-9]+)\)", source)) - {"name"}
    assert read - {"verbose"} == set(YAML_KEYS) | set(YAML_KEYS_MCRA), read ^ (set(YAML_KEYS) | set(YAML_KEYS_MCRA))


def test_create_fails_loudly_without_gpu_or_with_bad_config():
    import torch
    from beamform_amd import capi
    lib = capi.load()
    c = capi.config_from_params(make_params("das", n_mics=8))
    h = C.c_void_p()
    if not torch.cuda.is_available():
        assert lib.bf_device_count() <= 0
        assert lib.bf_create(C.byref(c), C.byref(h)) == -19           # BF_ENODEV: no CPU fallback
        assert b"no CPU fallback" in lib.bf_last_error(None)
        with pytest.raises(capi.BfError):
            capi.Beamformer(make_params("das", n_mics=8))
    c.hop = 384
    assert lib.bf_create(C.byref(c), C.byref(h)) in (-38, -19)        # not a power-of-two JACK period (or no device)
    c.hop, c.n_mics = 512, 0
    assert lib.bf_create(C.byref(c), C.byref(h)) == -22
    assert lib.bf_create(None, C.byref(h)) == -22
    assert lib.bf_strerror(-19).startswith(b"no usable HIP device")


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: no product source may reference it."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "beamform_amd")):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dirpath, fn), errors="ignore").read()
                if re.search(r"^\s*(import|from)\s+oracle|liboracle|bf_oracle|np_oracle", txt, re.M):
                    bad.append(fn)
    assert not bad, bad


def test_das_f64_chunk_plan_tiles_every_stream(emul_lib):
    """The work queue of das_f64_pair_kernel (csrc/das_f64_plan.hpp, the host arithmetic das_f64_sched_kernel runs per chunk): for any
    batch shape and plan the chunks must tile every stream exactly once, start on even frames (so that WHICH frames share a transform
    never depends on the plan), hold at most 1000 pairs (the 10-bit fields of the kernel's work word), fit the table, and come longest
    first inside a stream's level order."""
    import ctypes as C
    rng = np.random.default_rng(5)
    shapes = [(65536, 1, 256), (65537, 1, 256), (1, 1, 256), (2, 1, 256), (7, 3, 256), (256, 256, 256), (300, 5, 256), (1_000_000, 1, 256),
              (4_000_000, 1, 256), (20_000, 300, 256), (2049, 1, 256), (16400, 1, 256), (33, 2, 304), (100_000, 7, 64)]
    shapes += [(int(rng.integers(1, 300_000)), int(rng.integers(1, 40)), int(rng.choice([64, 256, 304]))) for _ in range(40)]
    cap = 16384
    st, t0, n = (C.c_int * cap)(), (C.c_long * cap)(), (C.c_long * cap)()
    grid = C.c_int()
    emul_lib.emul_das_plan.restype = C.c_int
    emul_lib.emul_das_plan.argtypes = [C.c_long, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for env in (b"", b"0", b"5,3,1", b"104,8,4,2", b"40,7,5,3", b"1"):
        for F, S, cus in shapes:
            k = emul_lib.emul_das_plan(F, S, cus, env, cap, st, t0, n, C.byref(grid))
            assert 0 < k <= cap, (F, S, cus, env, k)
            assert 1 <= grid.value <= min(k, cus)
            seen = {s: [] for s in range(S)}
            for i in range(k):
                assert 0 <= st[i] < S and n[i] >= 1 and t0[i] % 2 == 0 and (n[i] + 1) // 2 <= 1000, (F, S, env, i, st[i], t0[i], n[i])
                seen[st[i]].append((t0[i], n[i]))
            for s in range(S):
                pos = 0
                for a, b in sorted(seen[s]):
                    assert a == pos, (F, S, env, s, a, pos)      # no gap, no overlap
                    assert b % 2 == 0 or a + b == F               # only a stream's last chunk ends on a lone frame
                    pos = a + b
                assert pos == F, (F, S, env, s, pos)
            if env == b"" and k > grid.value:   # level-major order: the table starts with one long chunk per block-share of every stream
                first = [n[i] for i in range(min(grid.value, k))]
                assert min(first) >= max(n[i] for i in range(k - 1, k)), (F, S)


def test_bench_tables_in_the_docs_match_their_records():
    """BASELINE.md section 4 and README.md carry ONE generated table of measured figures each (tools/bench_tables.py): regenerated from
    the records the table itself names (the driver's BENCH_rNN.json, this build's profiles/rNN_*bench*.json) it must come out the same
    text, i.e. no figure in it was typed or edited by hand."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_tables.py"), "--check"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- the launch decision of fused fp32 das (csrc/das_fused_plan.hpp through emul_das_fused_plan) ---------------------------------------
K_REGS, K_IL4, K_IL8, K_WAVE2048, K_DIRS, K_GEN = range(6)   # DasFusedKernel's order
DEFAULT_SWITCHES = dict(das_interleave=1, das_split2048=3, das_shared_dirs=6)   # switches.hpp


def _das_fused_plan(lib, hop, layout, mics, streams, dirs, dump, F, cus, das_interleave=1, das_split2048=3, das_shared_dirs=6):
    out = (C.c_long * 9)()
    lib.emul_das_fused_plan.restype = None
    lib.emul_das_fused_plan.argtypes = [C.c_int] * 6 + [C.c_long] + [C.c_int] * 4 + [C.c_void_p]
    lib.emul_das_fused_plan(hop, layout, mics, streams, dirs, int(dump), F, cus, das_interleave, das_split2048, das_shared_dirs, out)
    keys = ("kernel", "npl", "unr", "group", "fpc", "cps", "blocks", "zero_run_heads", "group_tables")
    return dict(zip(keys, out))


def test_das_fused_decision_names_the_kernels_of_the_dispatch_table(emul_lib):
    """Every das (fp32) row of docs/DISPATCH.md (traced on a GPU: 96 frames, one stream, 256 CUs, default switches): the host decision
    must name the row's first kernel -- for das_fused_kernel<L, NPL, UNR, R> the same four integers, for das_fused_gen_kernel<N> the
    transform the engine asks for (N = 2 * period), for das_fused_wave2048_kernel<L> the layout."""
    rows = []
    for line in open(os.path.join(ROOT, "docs", "DISPATCH.md")):
        c = [f.strip() for f in line.strip().strip("|").split("|")]
        if len(c) == 7 and c[0] == "das (fp32)":
            rows.append(c)
    assert len(rows) >= 14   # seven periods, and at period 512 seven more layouts / microphone counts / direction counts / a dump
    for _, period, layout, mics, dirs, dump, kernels in rows:
        hop, lay, M, D = int(period), {"planar": 0, "[sample][mic]": 1}[layout], int(mics), int(dirs)
        d = _das_fused_plan(emul_lib, hop, lay, M, 1, D, dump == "yes", 96, 256)
        first = kernels.strip("`").split(" + ")[0]
        name, _, targs = first.partition("<")
        targs = [int(t) for t in targs.rstrip(">").split(",")] if targs else []
        if name == "das_fused_kernel":
            assert (d["kernel"], [lay, d["npl"], d["unr"], d["group"]]) == (K_REGS, targs), (first, d)
        elif name == "das_fused_gen_kernel":
            assert (d["kernel"], [2 * hop]) == (K_GEN, targs), (first, d)
        elif name == "das_fused_wave2048_kernel":
            assert (d["kernel"], [lay]) == (K_WAVE2048, targs), (first, d)
        else:
            assert d["kernel"] == {"das_fused_il_kernel": K_IL4, "das_fused_il8_kernel": K_IL8, "das_fused_dirs_kernel": K_DIRS}[name], (first, d)


def test_das_fused_decision_covers_every_stream_within_the_run_budget(emul_lib):
    """A few hundred random shapes at the default switches: the runs tile a stream (no empty run, none past the end), stay within the
    budget of blocks in flight (n_cus; the LDS-staged kernels 8 / 6 / 3 / 1 per CU at N <= 512 / 1024 / 2048 / above), keep the chosen
    kernel's multiple of frames, and every kernel appears only for the shapes it is built for.  A spectrum dump never selects the
    wavefront-per-frame kernel, the shared-transform kernel or group mode, none of which writes one.  (The two 16-byte-load kernels
    of [sample][mic] input do write it and take such batches today -- tests/test_fused_bins_gpu.py runs one -- so for them the
    dump must NOT change the choice.)"""
    rng = np.random.default_rng(20)
    fixed_F = [1, 2, 15, 16, 17, 96, 97, 65_536, 1_000_003]
    shapes = []
    for i in range(400):
        F = fixed_F[i % len(fixed_F)] if i % 2 == 0 else int(rng.integers(1, 300_000))
        shapes.append((int(2 ** rng.integers(6, 13)), int(rng.integers(0, 2)), int(rng.integers(1, 25)), int(rng.integers(1, 41)),
                       int(rng.integers(1, 17)), bool(rng.integers(0, 2)), F, int(rng.choice([64, 256, 304]))))
    # the corners a random draw may miss: the eligibility edges of every kernel
    shapes += [(512, 1, m, 1, 1, dump, 96, 256) for m in (4, 8) for dump in (False, True)]
    shapes += [(512, 0, m, 2, dd, False, 97, 256) for m in (8, 9) for dd in (5, 6, 16)]
    seen = set()
    for hop, lay, M, S, D, dump, F, cus in shapes:
        d = _das_fused_plan(emul_lib, hop, lay, M, S, D, dump, F, cus)
        k, fpc, cps, ctx = d["kernel"], d["fpc"], d["cps"], ((hop, lay, M, S, D, dump, F, cus), d)
        seen.add(k)
        N = 2 * hop
        group_mode = k == K_REGS and hop < 512
        budget = cus * ((8 if N <= 512 else 6 if N <= 1024 else 3 if N <= 2048 else 1) if k == K_GEN else 1)
        streams = S if k == K_DIRS else S * D
        assert cps >= 1 and (cps - 1) * fpc < F <= cps * fpc, ctx
        assert cps <= max(1, budget // streams), ctx
        multiple = 16 * d["group"] if k in (K_REGS, K_IL4, K_IL8, K_DIRS) else 8 if k == K_WAVE2048 else 1
        assert fpc % multiple == 0, ctx
        assert d["group"] == (1024 // N if group_mode else 1) and d["group_tables"] == group_mode, ctx
        assert d["blocks"] == cps * streams, ctx
        assert d["zero_run_heads"] == (cps > 1 and k != K_GEN), ctx
        # who may appear where
        shared_ok = hop == 512 and lay == 0 and M <= 8 and not dump and D >= DEFAULT_SWITCHES["das_shared_dirs"]
        assert (k == K_DIRS) == shared_ok, ctx
        assert (k == K_IL4) == (hop == 512 and lay == 1 and M == 4) and (k == K_IL8) == (hop == 512 and lay == 1 and M == 8), ctx
        assert (k == K_WAVE2048) == (hop == 1024 and not dump), ctx
        assert group_mode == (hop < 512 and not dump), ctx
        assert (k == K_GEN) == (hop != 512 and k not in (K_WAVE2048, K_REGS)), ctx
        if dump:
            assert k not in (K_WAVE2048, K_DIRS) and not group_mode, ctx
        if k == K_REGS:
            np_ = (M + 1) // 2
            assert d["npl"] == (np_ if np_ <= 2 else 4 if np_ <= 4 else 0) and d["unr"] == (np_ if lay == 0 and np_ <= 4 else 0), ctx
    assert seen == set(range(6))


def test_das_fused_switches_route_to_the_cross_check_kernels(emul_lib):
    """BF_DAS_INTERLEAVE=0 / BF_DAS_SPLIT2048=0: the LDS-staged kernel instead of group mode / the wavefront-per-frame kernel;
    BF_DAS_SHARED_DIRS=0: the per-direction kernel; each leaves the other shapes alone."""
    shapes = [(hop, lay, 8, 2, 8, 97, 256) for hop in (64, 128, 256, 512, 1024, 2048) for lay in (0, 1)]
    for hop, lay, M, S, D, F, cus in shapes:
        base = _das_fused_plan(emul_lib, hop, lay, M, S, D, False, F, cus)
        for name in DEFAULT_SWITCHES:
            off = _das_fused_plan(emul_lib, hop, lay, M, S, D, False, F, cus, **{**DEFAULT_SWITCHES, name: 0})
            hit = {"das_interleave": hop < 512, "das_split2048": hop == 1024, "das_shared_dirs": hop == 512 and lay == 0}[name]
            if not hit:
                assert off == base, (name, hop, lay)
            elif name == "das_shared_dirs":
                assert base["kernel"] == K_DIRS and (off["kernel"], off["npl"], off["unr"], off["group"]) == (K_REGS, 4, 4, 1), (hop, lay, off)
                assert off["blocks"] == off["cps"] * S * D and base["blocks"] == base["cps"] * S
            else:
                assert base["kernel"] == (K_REGS if hop < 512 else K_WAVE2048) and off["kernel"] == K_GEN, (name, hop, lay, off)
                assert not off["group_tables"] and off["group"] == 1 and not off["zero_run_heads"]
    # the threshold itself: BF_DAS_SHARED_DIRS = the smallest direction count that shares the transforms
    for thr, dirs, want in ((6, 5, K_REGS), (6, 6, K_DIRS), (2, 2, K_DIRS), (9, 8, K_REGS), (-1, 8, K_REGS)):
        assert _das_fused_plan(emul_lib, 512, 0, 8, 1, dirs, False, 96, 256, das_shared_dirs=thr)["kernel"] == want, (thr, dirs)


# ---- the launch plan of the STFT -> per-bin -> ISTFT chain (csrc/chain_plan.hpp through emul_chain_plan) ---------------------------------
from chain_plan_util import (ALGO, CHAIN_SWITCHES, NODES, chain_kernels, chain_plan, dispatch_rows, row_plan)   # noqa: E402


def test_chain_plan_names_the_kernels_of_the_dispatch_table(emul_lib):
    """Every chain row of docs/DISPATCH.md (traced on a GPU: 96 frames, 256 CUs, default switches, make_params' defaults, 1 or 64 streams):
    the plan's kernel list, formatted as the table prints it, equals the row exactly and in order.  Left out, and nothing else: fused fp32
    das, the one-launch das in double (das_f64_*), and shapes the node refuses."""
    compared, skipped = 0, []
    for row in dispatch_rows():
        node, kernels = row[0], row[6]
        if node == "das (fp32)" or kernels.startswith("das_f64_") or kernels.startswith("(refused:"):
            skipped.append(row)
            continue
        d, nfft = row_plan(emul_lib, row, 96, 256)
        assert " + ".join(chain_kernels(d, nfft)) == kernels, (row, d)
        compared += 1
    assert compared >= 80, compared
    assert all(r[0] == "das (fp32)" or r[6].startswith(("das_f64_", "(refused:")) for r in skipped)
    assert compared + len(skipped) == len(dispatch_rows())


def test_chain_plan_is_consistent_on_random_shapes(emul_lib):
    """Seeded random shapes over all eight nodes, every hop, 1-32 microphones (gsc <= 16), 1-16 columns, both precisions, dump on / off,
    1-300 streams, 1-304 CUs: the template arguments cover the shape, every kernel appears only where it is built for, and the workspace
    sizes are the pipeline's expressions (written out here on their own)."""
    rng = np.random.default_rng(23)
    seen = set()
    for i in range(480):
        algo = NODES[i % 8]
        a = ALGO[algo]
        hop = int(2 ** rng.integers(6, 13))
        N = 2 * hop
        M = int(rng.integers(1, 17 if algo == "gsc" else 33))
        kp1 = int(rng.integers(1, 17)) if algo in ("lcmv", "gss") else 1
        mixed, dump = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        S, cus, F = int(rng.integers(1, 301)), int(rng.integers(1, 305)), int(rng.integers(1, 200))
        dirs = int(rng.integers(1, 5)) if algo != "gsc" and i % 3 == 0 else 1
        fs, sz, P = int(rng.integers(1, 257)), int(rng.integers(1, 65)), int(rng.integers(1, 65))
        blo = int(rng.integers(1, 40))
        bhi = int(rng.integers(blo, N // 2 - 2))
        al = bool(rng.integers(0, 4))
        d = chain_plan(emul_lib, algo=a, n_fft=N, layout=int(rng.integers(0, 2)), n_mics=M, n_streams=S, n_dirs=dirs, kp1=kp1, past_windows=P,
                       precision=int(mixed), dump=dump, n_frames=F, n_cus=cus, gsc_filter_size=fs, smooth_size=sz, band_yh_lo=blo, band_yh_hi=bhi,
                       aligned16=al)
        ctx = ((algo, hop, M, kp1, mixed, dump, S, cus, F, dirs, fs, sz, P, al), d)
        names = chain_kernels(d, N)
        seen.update(n.split("::")[1].split("<")[0] for n in names)
        cov, gsc, mpf = algo in ("mvdr", "lcmv"), algo == "gsc", algo == "phasempf"
        D = M if gsc else dirs
        So, MF = S * D, (1 if algo == "mcra" else M)
        # template arguments cover the shape
        bins = d["bins"]
        if bins == 6:
            assert 8 < M <= 16, ctx      # cov2d_kernel: 4 x 4 lanes per problem, no MP argument
        elif algo not in ("mcra", "gsc"):
            assert d["mp"] >= M, ctx
        if algo in ("mvdr", "lcmv", "gss"):
            assert d["km"] >= kp1, ctx
        if gsc:
            if d["tail"] == 5:
                assert d["t0"] * d["t1"] >= M - 1 and 64 * d["t2"] >= fs, ctx      # (filter sizes stop at 256 = 64 * 4)
            else:
                assert d["t0"] >= M - 1 and 64 * d["t1"] >= fs, ctx
        # who may appear where
        is32 = d["istft"] == 2
        assert is32 == bool(d["yh32"] or d["mpf32"]), ctx
        if is32:
            assert N == 1024 and mixed and not dump and not gsc, ctx
        assert bool(d["z48"]) == (cov and mixed), ctx
        rec_istft = d["rec"] == 2
        if rec_istft:
            assert d["istft"] == 0 and not d["mpf32"] and mpf and N == 1024 and not dump and So * 4 >= cus, ctx
        else:
            assert d["istft"] != 0, ctx
        assert (d["rec"] != 0) == mpf, ctx
        if d["band_rows"] or (d["yh_lo"], d["yh_hi"]) != (0, N // 2 + 1):
            assert cov and not dump and N == 1024 and (d["yh_lo"], d["yh_hi"]) == (blo, bhi), ctx
        if d["fused"]:
            assert algo in ("das", "phase", "phasempf") and M <= 8 and dirs == 1 and N <= 2048 and bins == 0, ctx
        else:
            assert bins != 0, ctx
        assert bool(d["expand"]) == (dump and not gsc), ctx
        assert (d["tail"] in (1, 2)) == mpf and (d["tail"] in (3, 4, 5)) == gsc, ctx
        if d["tail"] == 1:
            assert al and 1 <= sz <= 8 and d["t0"] == sz, ctx
        # workspace sizes: the expressions of BinPipelineImpl::run_chain
        NP, YS, zsz = (MF + 1) // 2, N // 2 + 4, (12 if cov and mixed else 16)
        FT = (P if cov else 0) + F
        z = S * F * 2 * 8 * 16 if d["fused"] else (S * FT + (512 if cov else 0)) * NP * N * zsz
        assert d["z_bytes"] == z, ctx
        assert d["yh_bytes"] == So * F * YS * (16 + (8 if mpf else 0)), ctx
        assert d["yraw_elems"] == (So * F * hop if mpf or gsc else 0), ctx
        assert d["frames_elems"] == (So * F * N if N != 1024 else 0), ctx
    assert {"stft_kernel", "stft_small_kernel", "stft_wave2048_kernel", "stft_generic_kernel", "stft_bins_w64_kernel", "stft_bins_small_kernel",
            "stft_bins_split_kernel", "pointwise_bins_kernel", "mpf_mask_kernel", "mcra_node_kernel", "gsc_align_kernel", "mvdr_fast_kernel",
            "cov2d_kernel", "mvdr_lcmv_kernel", "gss_kernel", "gss_lane_kernel", "mpf_recursion_kernel", "mpf_rec_istft_kernel",
            "istft_w64_kernel", "istft32_kernel", "istft_small_kernel", "istft_split_kernel", "istft_generic_kernel", "smooth4_kernel",
            "smooth_kernel", "gsc_nlms_par_kernel", "gsc_nlms_mw_kernel", "expand_spectrum_kernel"} <= seen, seen


def test_chain_switches_route_as_documented(emul_lib):
    """Each switch away from its default: BF_FUSED_BINS=0 no fused front; BF_STFT_SMALL=0 / BF_STFT_SPLIT=0 the generic
    STFT and ISTFT at their sizes and no effect on the fused front; BF_MVDR_GROUP=1 only mvdr_lcmv_kernel; BF_GSS_GROUP 0 / 1 the lane /
    the group kernel; BF_GSC_SERIAL=1 gsc_nlms_kernel."""
    def names(algo, hop=512, M=8, kp1=1, S=1, **sw):
        d = chain_plan(emul_lib, algo=ALGO[algo], n_fft=2 * hop, n_mics=M, n_streams=S, kp1=kp1, n_frames=96, n_cus=256, band_yh_lo=3, band_yh_hi=341, **sw)
        return [n.split("::")[1] for n in chain_kernels(d, 2 * hop)], d
    for hop in (64, 128, 256, 512, 1024):
        for algo in ("das", "phase", "phasempf"):
            on, d_on = names(algo, hop)
            off, d_off = names(algo, hop, fused_bins=0)
            assert d_on["fused"] and on[0].startswith("stft_bins_") and not d_off["fused"], (hop, algo)
            assert not any("stft_bins_" in n or "fused_tail" in n for n in off), (hop, algo, off)
            assert d_off["z_bytes"] == 96 * 4 * 2 * hop * 16    # the packed spectra of four microphone pairs
    for hop, sw in ((64, "stft_small"), (128, "stft_small"), (256, "stft_small"), (1024, "stft_split")):
        base, _ = names("mvdr", hop)
        off, _ = names("mvdr", hop, **{sw: 0})
        assert base[0].startswith("stft_small_kernel" if hop < 512 else "stft_wave2048_kernel") and base[-1] == ("istft_small_kernel" if hop < 512 else "istft_split_kernel")
        assert off[0] == "stft_generic_kernel<0>" and off[-2:] == ["istft_generic_kernel", "ola_generic_kernel"], (hop, off)
        assert names("phase", hop, **{sw: 0})[0][0] == names("phase", hop)[0][0]              # the fused front has no generic twin ...
        assert names("phase", hop, **{sw: 0})[0][-2:] == ["istft_generic_kernel", "ola_generic_kernel"]   # ... its backward transform has
        other = "stft_split" if sw == "stft_small" else "stft_small"
        assert names("mvdr", hop, **{other: 0})[0] == base                                    # the other sizes' switch leaves this one alone
    assert names("mvdr", 512, stft_small=0, stft_split=0)[0] == names("mvdr", 512)[0]
    for algo, kp1 in (("mvdr", 1), ("lcmv", 3)):
        for M in (2, 3, 8, 12, 16, 24):
            assert names(algo, 512, M, kp1, mvdr_group=1)[0][1].startswith("mvdr_lcmv_kernel<"), (algo, M)
    assert names("mvdr", 512, 8)[0][1].startswith("mvdr_fast_kernel<") and names("mvdr", 512, 12)[0][1].startswith("cov2d_kernel<")
    for S in (1, 64):
        assert names("gss", 512, 8, 3, S, gss_group=0)[0][1] == "gss_lane_kernel<8, 4>"
        assert names("gss", 512, 8, 3, S, gss_group=1)[0][1] == "gss_kernel<8, 4>"
    assert names("gss", 512, 8, 3, 1)[0][1] == "gss_kernel<8, 4>" and names("gss", 512, 8, 3, 64)[0][1] == "gss_lane_kernel<8, 4>"
    assert names("gss", 512, 12, 3, 64, gss_group=0)[0][1] == "gss_kernel<16, 4>"             # the lane kernel is built for up to 8 microphones
    for M, want in ((2, "gsc_nlms_kernel<1, 2>"), (8, "gsc_nlms_kernel<7, 2>"), (16, "gsc_nlms_kernel<15, 2>")):
        assert names("gsc", 512, M, gsc_serial=1)[0][-1] == want, M
    assert names("gsc", 512, 2)[0][-1] == "gsc_nlms_par_kernel<1, 2>" and names("gsc", 512, 8)[0][-1] == "gsc_nlms_mw_kernel<8, 1, 2>"
    assert set(CHAIN_SWITCHES) == {"fused_bins", "stft_small", "stft_split", "mvdr_group", "gss_group", "gsc_serial"}


# ---- the launch decision of das in double (csrc/das_f64_plan.hpp das_f64_decide, csrc/geometry.hpp das_f64_slots) ------------------------
from das_f64_plan_util import (FRAME_PAIR_PATHS, das_f64_decide, das_f64_kernels, das_f64_slots, das_plan_levels, params_decide)   # noqa: E402

DAS_F64_ONE_LAUNCH_ROWS = {("planar", 8): "das_f64_sched_kernel + das_f64_pair_kernel",
                           ("[sample][mic]", 8): "das_f64_sched_kernel + das_f64_ring_kernel",
                           ("planar", 3): "das_f64_sched_kernel + das_f64_pair_kernel"}


def test_das_f64_decision_names_the_kernels_of_the_dispatch_table(emul_lib):
    """Every das (double) row of docs/DISPATCH.md (traced on a GPU: 96 frames, one stream, 256 CUs, default switches) that reaches
    das_f64_decide -- a spectrum dump and several look directions never do: the decision names the row's kernels, or the chain where the
    row lists chain kernels.  mic0_unit and n_tr come from das_f64_slots on the row's geometry, as on a cold handle."""
    one_launch, chained = {}, 0
    for _, period, layout, mics, dirs, dump, kernels in (r for r in dispatch_rows() if r[0] == "das (double)"):
        if dump == "yes" or int(dirs) > 1:
            continue
        M = int(mics)
        over = {"mics": [(0.2, 0.0)] * M} if M > 16 else {}
        p = make_params("das", n_mics=M, hop=int(period), **over)
        d = params_decide(emul_lib, p, 96, 256, layout={"planar": 0, "[sample][mic]": 1}[layout])
        if kernels.startswith("das_f64_"):
            assert int(period) == 512 and " + ".join(das_f64_kernels(d)) == kernels, (period, layout, mics, d)
            one_launch[(layout, M)] = kernels
        else:
            assert d["path"] == "chain", (period, layout, mics, d)
            chained += 1
    assert one_launch == DAS_F64_ONE_LAUNCH_ROWS, one_launch
    assert chained >= 8    # the six other periods, 16 and 24 microphones


def _das_f64_shapes():
    """(layout, M, S, F, cus, mic0_unit, n_tr, tables): seeded random shapes and the corners of every branch."""
    rng = np.random.default_rng(29)
    fixed_F = [1, 2, 3, 5, 96, 97, 65_536, 1_000_003]
    shapes = []
    for i in range(400):
        M = int(rng.integers(1, 11))
        F = fixed_F[i % len(fixed_F)] if i % 2 == 0 else int(rng.integers(1, 300_000))
        S = int(rng.integers(1, 41)) if i % 5 else int(rng.integers(200, 20_000))
        n_tr = max(0, M - 1 - int(rng.integers(0, 2))) if i % 7 else 0
        shapes.append((int(rng.integers(0, 2)), M, S, F, int(rng.choice([64, 256, 304])), bool(i % 11), n_tr, bool(i % 13)))
    for lay in (0, 1):
        for M in (1, 2, 8, 9):
            for F in (1, 2, 3, 65_536):
                shapes.append((lay, M, 1, F, 256, True, M - 1, True))
        for M in (2, 3, 4, 5, 6, 7, 8):
            shapes += [(lay, M, 300, 7, 256, True, M - 1, True),            # more streams than CUs
                       (lay, M, 65_536, 65_536, 256, True, M - 1, True),    # 2^31 pairs exactly
                       (lay, M, 65_536, 65_534, 256, True, M - 1, True),    # one pair per stream fewer: the plan, then the table's limit
                       (lay, M, 16_384, 2, 256, True, M - 1, True),         # the table's last row
                       (lay, M, 16_385, 2, 256, True, M - 1, True),         # one stream past it
                       (lay, M, 1, 96, 256, True, M - 1, False),            # tables = false
                       (lay, M, 1, 96, 256, False, M - 1, True),            # mic0_unit = false
                       (lay, M, 1, 96, 256, True, 0, True)]                 # n_tr = 0
    return shapes


def _das_f64_expected_path(lay, M, S, F, unit, n_tr, tables, ring_switch, n_chunks):
    """The issue's table of who serves what, written out on its own."""
    if M > 8:
        return "chain"
    if not (tables and unit and M >= 2 and n_tr >= 1):
        return "chain" if lay == 0 else "mic_pair"
    if S * ((F + 1) // 2) >= 2 ** 31 or not 1 <= n_chunks <= 16384:
        return "chain"
    return "frame_pair" if lay == 0 else "ring" if M in (2, 4, 8) and ring_switch else "transpose"


def test_das_f64_decision_is_consistent_on_random_shapes(emul_lib):
    """A few hundred shapes at the default switches: every path appears exactly where it is built for, the microphone-pair kernel's runs
    tile a stream within the budget of blocks, the scratch sizes are enqueue_das_f64's, and the frame-pair paths carry das_f64_plan's own
    value.  The transposition serves every frame count from 1 on: the branch that once turned batches away for its 256-sample tiles could
    never be taken (a hop is 512 samples)."""
    seen = set()
    for lay, M, S, F, cus, unit, n_tr, tables in _das_f64_shapes():
        d = das_f64_decide(emul_lib, lay, M, S, F, cus, unit, n_tr, tables)
        ctx = ((lay, M, S, F, cus, unit, n_tr, tables), d)
        pairs_fit = S * ((F + 1) // 2) < 2 ** 31
        plan = das_plan_levels(emul_lib, F, S, cus) if pairs_fit else None
        path = d["path"]
        seen.add(path)
        assert path == _das_f64_expected_path(lay, M, S, F, unit, n_tr, tables, 1, plan["n_chunks"] if plan else 0), ctx
        assert d["writes_hist"] == (path == "frame_pair"), ctx
        if path == "mic_pair":
            rf, runs = d["run_frames"], d["runs_per_stream"]
            assert rf % 8 == 0 and (runs - 1) * rf < F <= runs * rf and runs <= max(1, cus // S), ctx
        else:
            assert (d["run_frames"], d["runs_per_stream"]) == (0, 0), ctx
        want_scratch = {"ring": 4 * cus * 40 * M * 512, "transpose": 4 * S * M * 512 * (F + 1)}.get(path, 0)
        assert d["scratch_bytes"] == want_scratch, ctx
        if path in FRAME_PAIR_PATHS:
            assert d["plan"] == plan and 1 <= plan["n_chunks"] <= 16384, ctx
        elif not pairs_fit:
            assert not any(d["plan"].values()), ctx      # 2^31 pairs are turned away before the plan's int arithmetic sees them
    assert seen == {"chain", "frame_pair", "ring", "transpose", "mic_pair"}
    for M in (3, 5, 6, 7):       # the transposition takes every frame count
        for F in list(range(1, 20)) + [255, 256, 257, 65_535]:
            assert das_f64_decide(emul_lib, 1, M, 1, F, 256)["path"] == "transpose", (M, F)


def test_das_f64_switches_change_only_what_they_name(emul_lib):
    """BF_DAS_IL_RING=0 turns every ring batch into a transposition (with the transposition's scratch) and touches nothing else;
    BF_DAS_F64_SCHED changes only the chunk plan, and that plan is das_f64_plan's for the same string."""
    ring_seen = plans_differ = 0
    for lay, M, S, F, cus, unit, n_tr, tables in _das_f64_shapes():
        base = das_f64_decide(emul_lib, lay, M, S, F, cus, unit, n_tr, tables)
        off = das_f64_decide(emul_lib, lay, M, S, F, cus, unit, n_tr, tables, das_il_ring=0)
        if base["path"] == "ring":
            ring_seen += 1
            assert off == {**base, "path": "transpose", "scratch_bytes": 4 * S * M * 512 * (F + 1)}, (lay, M, S, F, off)
        else:
            assert off == base, (lay, M, S, F, off)
        for sched in (b"0", b"5,3,1", b"104,8,4,2", b"1"):
            d = das_f64_decide(emul_lib, lay, M, S, F, cus, unit, n_tr, tables, sched=sched)
            assert {**d, "plan": None} == {**base, "plan": None}, (lay, M, S, F, sched, d)
            if d["path"] in FRAME_PAIR_PATHS:
                assert d["plan"] == das_plan_levels(emul_lib, F, S, cus, sched), (lay, M, S, F, sched)
                plans_differ += d["plan"] != base["plan"]
    assert ring_seen >= 30 and plans_differ >= 100


def test_das_f64_slots_merge_identical_rows_and_know_row_0(emul_lib):
    """geometry.hpp das_f64_slots, what BinPipelineImpl::upload_steering hands the frame-pair kernels: is row 0 identically 1, the first pair
    of microphones past 0 whose weight rows coincide (slot 0 + extra_mic), the others in ascending order."""
    def check(mics, theta, **kw):
        sl = das_f64_slots(emul_lib, mics, theta, **kw)
        named = sl["slot_mic"][:sl["n_tr"]] + ([sl["extra_mic"]] if sl["extra_mic"] >= 0 else [])
        assert sorted(named) == list(range(1, len(mics))), (mics, theta, sl)     # every microphone past 0 exactly once
        return sl
    bench = make_params("das", n_mics=8)["mics"]      # aira16's first eight: microphones 1 and 7 share (x, y)
    for theta in (0.0, 20.0, -75.0, 135.0, 180.0, 33.3):
        sl = check(bench, theta)
        assert (sl["mic0_unit"], sl["n_tr"], sl["extra_mic"], sl["slot_mic"][:6]) == (True, 6, 7, [1, 2, 3, 4, 5, 6]), (theta, sl)
        z = check(bench, theta, zero_row0=True)         # quirk Q3: row 0 left at zero -- not a unit row, the walk is the same
        assert not z["mic0_unit"] and {**z, "mic0_unit": True} == sl, (theta, z)
    for M in (2, 3, 5, 7):                              # no coinciding (x, y): everyone past 0 in ascending order
        sl = check(make_params("das", n_mics=M)["mics"], 20.0)
        assert (sl["mic0_unit"], sl["n_tr"], sl["extra_mic"], sl["slot_mic"][:M - 1]) == (True, M - 1, -1, list(range(1, M))), (M, sl)
    # A uniform linear array at broadside, every delay equal: the FIRST pair is (1, 2).  The rows must coincide bit for bit, which rounding
    # denies a horizontal line (cos(90 degrees) is 6e-17 times each distance); a vertical line has it exactly, the reference drops z.
    line = [(0.05, 0.12)] * 6
    sl = check(line, 40.0)
    assert (sl["n_tr"], sl["extra_mic"], sl["slot_mic"][:4]) == (4, 2, [1, 3, 4, 5]), sl
    one = check([(0.1, 0.2)], 10.0)
    assert (one["mic0_unit"], one["n_tr"], one["extra_mic"]) == (True, 0, -1), one
    two = check([(0.1, 0.2), (-0.1, 0.0)], 10.0)
    assert (two["n_tr"], two["extra_mic"], two["slot_mic"][0]) == (1, -1, 1), two
