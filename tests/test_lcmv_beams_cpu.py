"""lcmv with one beam per constraint column (bf_config.lcmv_out_beams): what can be checked without a GPU -- the permutation identity that
makes the swapped oracle the yardstick of every row (tests/lcmv_beams_cases.py), and the host side (config, argument checks, launch
plan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from chain_plan_util import ALGO, PLAN, SHAPE, SHAPE_DEFAULTS, chain_kernels, chain_plan
from conftest import rel_l2
from lcmv_beams_cases import CASES, case_params, case_scene, row_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = 1e-7   # per frame and row: two orders inside the 1e-5 the GPU tests spend
#: (M, K, hop) = (8, 2, 512), (16, 3, 512), (5, 1, 64), (4, 3, 512), (8, 5, 512).  Worst per-frame relative L2 on these scenes: 1.7e-13,
#: 2.6e-13, 1.3e-13, 7.3e-11, 3.2e-10 (on the scenes the identity was first measured with: 1.2e-13, 2.6e-13, 1.0e-13, 4.0e-11, 1.1e-8)
SHAPES = ["l8k2", "c16k3", "m5k1h64", "m4k3", "g8k5"]


def lcmv_all_columns(p, X, Cm):
    """oracle.np_oracle.mvdr_lcmv_bins (lcmv.cpp:102-130) keeping every column of W: -> Y [S, F, N], Y[c] = (W^H x)_c in band with the gate
    open, 0.01 X_0 on every row behind a closed gate (lcmv.cpp:121), 0 out of band."""
    from oracle import np_oracle
    F, M, N = X.shape
    S, P = Cm.shape[2], p["past_windows"]
    f = np.abs(np_oracle.freq_vector(N, p["sample_rate"]))
    inb = (f >= p["freq_min"]) & (f <= p["freq_max"])
    Y = np.zeros((S, F, N), np.complex128)
    white = np.ones((M, M)) + 0.001 * np.eye(M)
    hist = np.zeros((N, M, P), np.complex128)
    for t in range(F):
        x = X[t]
        mag = np.abs(x).sum(axis=0) / (M * N)
        for j in np.flatnonzero(inb):
            if mag[j] > p["freq_mag_threshold"]:
                R = (hist[j] @ hist[j].conj().T) * white
                with np.errstate(all="ignore"):
                    try:
                        Ri = np.linalg.inv(R)
                        W = (Ri @ Cm[j]) @ np.linalg.inv(Cm[j].conj().T @ Ri @ Cm[j])
                    except np.linalg.LinAlgError:
                        W = np.full((M, S), np.nan + 0j)
                    Y[:, t, j] = W.conj().T @ x[:, j]
            else:
                Y[:, t, j] = 0.01 * x[0, j]
            hist[j, :, :-1] = hist[j, :, 1:]
            hist[j, :, -1] = x[:, j]
    return Y


@pytest.mark.parametrize("name", SHAPES)
def test_column_c_of_W_is_the_node_with_swapped_angles(name):
    """W (C P) = W(C) P: every column of the numpy restatement against the oracle with `angle` and interferer r exchanged, per frame and
    row inside 1e-7; the reference is non-finite on frame 0 only (the inverse of a zero covariance) and every row carries signal."""
    import oracle
    from oracle import np_oracle
    c, p = CASES[name], case_params(name)
    x = case_scene(name)
    Y = lcmv_all_columns(p, np_oracle.stft(p, x), oracle.OracleNode(p).weights())
    assert Y.shape[0] == c["K"] + 1
    norms = []
    for r in range(c["K"] + 1):
        _, Y_ref = row_ref(name, r)
        fin = np.isfinite(Y_ref).all(axis=1)
        assert list(np.flatnonzero(~fin)) == [0], (r, np.flatnonzero(~fin))
        assert not np.isfinite(Y[r, 0]).all()
        worst = max(rel_l2(Y[r, t], Y_ref[t]) for t in range(1, c["F"]))
        print(f"{name} row {r}: {worst:.2e}")
        assert worst < IDENTITY, (r, worst)
        norms.append(np.linalg.norm(Y_ref[1:]))
    assert min(norms) > 0.05 * norms[0], norms


def test_swapped_weights_are_the_columns_permuted():
    import oracle
    for name in ("l8k2", "g8k5"):
        W0 = oracle.OracleNode(case_params(name)).weights()
        for r in range(1, CASES[name]["K"] + 1):
            Wr = oracle.OracleNode(case_params(name, swap=r)).weights()
            perm = list(range(W0.shape[2]))
            perm[0], perm[r] = r, 0
            assert np.array_equal(Wr, W0[:, :, perm]), (name, r)


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
def test_config_field_and_argument_checks():
    from beamform_amd import capi
    from beamform_amd.params import make_params
    lib = capi.load()
    c = capi.BfConfig()
    c.lcmv_out_beams = 7
    assert lib.bf_config_init(C.byref(c), 2) == 0 and c.lcmv_out_beams == 0
    assert C.sizeof(capi.BfConfig) >= capi.BfConfig.lcmv_out_beams.offset + 4
    assert make_params("lcmv")["lcmv_out_beams"] == 0
    assert capi.config_from_params(make_params("lcmv", lcmv_out_beams=4)).lcmv_out_beams == 4
    assert capi.config_from_params(make_params("lcmv"), lcmv_out_beams=2).lcmv_out_beams == 2
    # bad values are BF_EINVAL, checked with the other argument checks: before any device work, so also without a device
    h = C.c_void_p()
    for algo, r in (("lcmv", -1), ("lcmv", capi.BF_MAX_INTERF + 2), ("gss", 2), ("das", 3), ("mvdr", 2)):
        cfg = capi.config_from_params(make_params(algo, n_mics=8))
        cfg.lcmv_out_beams = r
        assert lib.bf_create(C.byref(cfg), C.byref(h)) == -22, (algo, r)
        assert b"lcmv_out_beams" in lib.bf_last_error(None)
    for algo in ("lcmv", "gss"):     # both row counts above one exclude each other, whatever the node
        cfg = capi.config_from_params(make_params(algo, n_mics=8))
        cfg.lcmv_out_beams = cfg.gss_out_sources = 2
        assert lib.bf_create(C.byref(cfg), C.byref(h)) == -22, algo
    for algo, r in (("lcmv", 0), ("lcmv", 1), ("lcmv", 2), ("lcmv", 16), ("gss", 1), ("das", 0)):   # accepted: the next check (or the device) answers
        cfg = capi.config_from_params(make_params(algo, n_mics=8, interf=(-60.0,) if algo != "das" else ()))
        cfg.lcmv_out_beams = r
        rc = lib.bf_create(C.byref(cfg), C.byref(h))
        assert rc in (0, -19), (algo, r, rc)
        if rc == 0:
            lib.bf_destroy(h)


@pytest.fixture(scope="module")
def rows_lib(emul_lib):
    so = os.path.join(ROOT, "tests", "host_emul", "libemul_lcmv_rows.so")
    src = os.path.join(ROOT, "tests", "host_emul", "emul_lcmv_rows.cpp")
    hdr = os.path.join(ROOT, "beamform_amd", "csrc", "chain_plan.hpp")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.emul_chain_plan_lcmv_rows.restype = None
    lib.emul_chain_plan_lcmv_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def _plan_rows(lib, rows, **shape):
    s = {**SHAPE_DEFAULTS, **shape}
    vin = (C.c_long * len(SHAPE))(*[int(s[k]) for k in SHAPE])
    out = (C.c_long * (len(PLAN) + 1))()
    lib.emul_chain_plan_lcmv_rows(vin, rows, out)
    return dict(zip(PLAN + ("rows",), out))


def test_chain_plan_carries_the_row_count(emul_lib, rows_lib):
    """A shape written without the field, R = 0 and R = 1: the plan of today in every member.  R > 1: the same kernels and template
    arguments -- the twins are picked by the launcher from ChainPlan::rows -- and R times the rows behind the per-bin stage; the packed
    spectra in front of it do not grow.  Every other node ignores the field."""
    rng = np.random.default_rng(11)
    for i in range(200):
        hop = int(2 ** rng.integers(6, 13))
        N = 2 * hop
        shape = dict(algo=ALGO["lcmv"], n_fft=N, layout=int(rng.integers(0, 2)), n_mics=int(rng.integers(1, 33)), n_streams=int(rng.integers(1, 40)),
                     n_dirs=int(rng.integers(1, 4)), kp1=int(rng.integers(1, 17)), precision=int(rng.integers(0, 2)), dump=bool(rng.integers(0, 2)),
                     n_frames=int(rng.integers(1, 200)), n_cus=int(rng.integers(1, 305)), band_yh_lo=3, band_yh_hi=N // 3,
                     mvdr_group=int(rng.integers(0, 2)))
        base = chain_plan(emul_lib, **shape)
        for r in (-1, 0, 1):
            d = _plan_rows(rows_lib, r, **shape)
            assert d.pop("rows") == 1 and d == base, (shape, r)
        R = int(rng.integers(2, 17))
        d = _plan_rows(rows_lib, R, **shape)
        assert d["rows"] == R
        assert chain_kernels(d, N) == chain_kernels(base, N), shape
        So, F = shape["n_streams"] * shape["n_dirs"], shape["n_frames"]
        assert d["yh_bytes"] == R * base["yh_bytes"] == So * R * F * (N // 2 + 4) * 16
        assert d["frames_elems"] == R * base["frames_elems"] == (So * R * F * N if N != 1024 else 0)
        assert d["z_bytes"] == base["z_bytes"] and d["yraw_elems"] == 0
        for k in PLAN:
            if k not in ("yh_bytes", "frames_elems"):
                assert d[k] == base[k], (k, shape)
    for algo in ("das", "mvdr", "gss", "phase", "phasempf", "mcra", "gsc"):
        shape = dict(algo=ALGO[algo], n_fft=1024, n_mics=8, n_streams=3, n_frames=20, n_cus=256, band_yh_lo=3, band_yh_hi=341)
        d = _plan_rows(rows_lib, 5, **shape)
        assert d.pop("rows") == 1 and d == chain_plan(emul_lib, **shape), algo
