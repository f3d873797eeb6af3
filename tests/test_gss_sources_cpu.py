"""gss with every separated source (bf_config.gss_out_sources): what can be checked without a GPU -- the numpy reference of the GPU
tests against the two oracles, the rounding floor of the shapes those tests use, and the host side (config, yaml, argument checks,
launch plan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from chain_plan_util import ALGO, PLAN, SHAPE, SHAPE_DEFAULTS, chain_kernels, chain_plan
from conftest import rel_l2
from gss_sources_cases import (CASES, SEM, case_params, case_ref, case_scene, case_streams, sem_params, sem_ref, sem_scene, sem_segments)
from gss_sources_ref import gss_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5      # the suite's bar against the oracle (tests/test_pipeline_gpu.py TOL_SPECTRUM / TOL_TIME)
FLOOR = 1e-7    # two summation orders of the same recursion, per frame
QUIET = 1e-6    # no row r < S may have a frame this far below row 0's


def _frames_close(Y, Y_ref, tol):
    return max(rel_l2(Y[t], Y_ref[t]) for t in range(Y_ref.shape[0]))


@pytest.mark.parametrize("name", list(CASES))
def test_row0_of_the_reference_is_the_oracles_output(name):
    """Row 0 equals oracle.np_oracle.process bit for bit (same constraint matrices, same expressions) and is within 1e-5 of
    oracle.OracleNode on every compared stream; rows r >= S are exact zeros."""
    import oracle
    from oracle import np_oracle
    c, p = CASES[name], case_params(name)
    x = case_scene(name, 0)
    y_np, Y_np = np_oracle.process(p, x)
    y, Y = gss_sources(p, x, [(c["F"], np_oracle.constraint_matrices(p, p["theta"]))], c["R"])
    assert np.array_equal(Y[0], Y_np) and np.array_equal(y[0], y_np)
    S = len(c["interf"]) + 1
    for s in case_streams(name):
        y, Y = case_ref(name, s)
        y_o, Y_o = oracle.OracleNode(p).process(case_scene(name, s), want_spectrum=True)
        assert np.isfinite(Y).all() and np.isfinite(Y_o).all()
        assert _frames_close(Y[0], Y_o, TOL) < TOL
        assert rel_l2(y[0], y_o) < TOL
        assert not Y[S:].any() and not y[S:].any()


def test_row0_follows_the_oracle_through_theta_and_interferer_changes():
    """The segments of the stream-semantics case, constraint matrices from the oracle's own control calls (quirk Q3 included)."""
    import oracle
    node = oracle.OracleNode(sem_params())
    x, cuts, H = sem_scene(), SEM["cuts"], 512
    ys, Ys = [], []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if i == 2:
            node.set_theta(SEM["theta1"])
        if i == 3:
            assert node.set_interference(2, SEM["new_interf"]) == 2
        y, Y = node.process(np.ascontiguousarray(x[:, a * H:b * H]), want_spectrum=True)
        ys.append(y)
        Ys.append(Y)
    y_o, Y_o = np.concatenate(ys), np.concatenate(Ys)
    y, Y = sem_ref()
    assert _frames_close(Y[0], Y_o, TOL) < TOL and rel_l2(y[0], y_o) < TOL
    assert not Y[2, :cuts[3]].any() and Y[2, cuts[3]:].any()      # the third source exists from the fourth piece on
    assert [C is not None for _, C in sem_segments()] == [True, False, True, True]


def _floor(Ya, Yb, rows_frames):
    for r, t0, t1 in rows_frames:
        for t in range(t0, t1):
            n0, nr = np.linalg.norm(Ya[0, t]), np.linalg.norm(Ya[r, t])
            assert nr >= QUIET * n0, (r, t, nr, n0)
            e = rel_l2(Yb[r, t], Ya[r, t])
            assert e < FLOOR, (r, t, e)


@pytest.mark.parametrize("name", list(CASES))
def test_rounding_floor_of_the_gpu_shapes(name):
    """A condition on the INPUTS: on every shape the GPU tests use, summing over the microphones serially or pairwise moves no
    frame of any row r < S by 1e-7, and no such row has a frame below 1e-6 of row 0's norm -- so 1e-5 per row on the GPU is a
    statement about the kernels, not about the scene."""
    c = CASES[name]
    S = min(len(c["interf"]) + 1, c["R"])
    for s in case_streams(name):
        _, Ya = case_ref(name, s, "serial")
        _, Yb = case_ref(name, s, "pairwise")
        _floor(Ya, Yb, [(r, 0, c["F"]) for r in range(S)])
        _, Y = case_ref(name, s)
        _floor(Y, Ya, [(r, 0, c["F"]) for r in range(S)])     # ... and the bin-by-bin loop is the same recursion


@pytest.mark.parametrize("retarget", [True, False])
def test_rounding_floor_of_the_stream_semantics_case(retarget):
    cuts, F = SEM["cuts"], SEM["F"]
    _, Ya = sem_ref(None, retarget, "serial")
    _, Yb = sem_ref(None, retarget, "pairwise")
    _floor(Ya, Yb, [(0, 0, F), (1, 0, F), (2, cuts[3], F)])


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
def test_config_field_yaml_key_and_argument_checks():
    from beamform_amd import capi
    from beamform_amd.params import make_params
    lib = capi.load()
    c = capi.BfConfig()
    c.gss_out_sources = 7
    assert lib.bf_config_init(C.byref(c), 3) == 0 and c.gss_out_sources == 0
    assert lib.bf_config_parse_yaml(C.byref(c), b"mu: 0.002\ngss_out_sources: 3\n") == 0
    assert c.gss_out_sources == 3 and c.mu == 0.002
    assert make_params("gss")["gss_out_sources"] == 0
    assert capi.config_from_params(make_params("gss", gss_out_sources=4)).gss_out_sources == 4
    assert capi.config_from_params(make_params("gss"), gss_out_sources=2).gss_out_sources == 2
    # bad values are BF_EINVAL, checked with the other argument checks: before any device work, so also without a device
    h = C.c_void_p()
    for algo, r in (("gss", -1), ("gss", capi.BF_MAX_INTERF + 2), ("lcmv", 2), ("das", 3), ("mvdr", 16)):
        cfg = capi.config_from_params(make_params(algo, n_mics=8))
        cfg.gss_out_sources = r
        assert lib.bf_create(C.byref(cfg), C.byref(h)) == -22, (algo, r)
        assert b"gss_out_sources" in lib.bf_last_error(None)
    for algo, r in (("gss", 0), ("gss", 1), ("gss", 16), ("lcmv", 1), ("das", 0)):      # accepted: the next check (or the device) answers
        cfg = capi.config_from_params(make_params(algo, n_mics=8))
        cfg.gss_out_sources = r
        rc = lib.bf_create(C.byref(cfg), C.byref(h))
        assert rc in (0, -19), (algo, r, rc)
        if rc == 0:
            lib.bf_destroy(h)
    cfg = capi.config_from_params(make_params("gss", n_mics=8))
    assert lib.bf_shard_halo(C.byref(cfg)) == -1
    cfg.gss_out_sources = 3
    assert lib.bf_shard_halo(C.byref(cfg)) == -1


@pytest.fixture(scope="module")
def rows_lib(emul_lib):
    so = os.path.join(ROOT, "tests", "host_emul", "libemul_gss_rows.so")
    src = os.path.join(ROOT, "tests", "host_emul", "emul_gss_rows.cpp")
    hdr = os.path.join(ROOT, "beamform_amd", "csrc", "chain_plan.hpp")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.emul_chain_plan_rows.restype = None
    lib.emul_chain_plan_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def _plan_rows(lib, rows, **shape):
    s = {**SHAPE_DEFAULTS, **shape}
    vin = (C.c_long * len(SHAPE))(*[int(s[k]) for k in SHAPE])
    out = (C.c_long * (len(PLAN) + 1))()
    lib.emul_chain_plan_rows(vin, rows, out)
    return dict(zip(PLAN + ("rows",), out))


def test_chain_plan_carries_the_row_count(emul_lib, rows_lib):
    """R = 0 / 1: the plan of today in every member (tests/chain_plan_util.py's chain_plan, which knows nothing of rows).  R > 1: the
    same kernels and template arguments -- the all-rows variants are picked by the launcher from ChainPlan::rows -- and R times the
    rows behind the per-bin stage (Yh, the generic sizes' frames); the packed spectra in front of it do not grow."""
    rng = np.random.default_rng(5)
    for i in range(200):
        hop = int(2 ** rng.integers(6, 13))
        N = 2 * hop
        shape = dict(algo=ALGO["gss"], n_fft=N, layout=int(rng.integers(0, 2)), n_mics=int(rng.integers(1, 33)), n_streams=int(rng.integers(1, 301)),
                     n_dirs=int(rng.integers(1, 4)), kp1=int(rng.integers(1, 17)), precision=int(rng.integers(0, 2)), dump=bool(rng.integers(0, 2)),
                     n_frames=int(rng.integers(1, 200)), n_cus=int(rng.integers(1, 305)))
        base = chain_plan(emul_lib, **shape)
        for r in (0, 1):
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
        for k in ("front", "bins", "mp", "km", "istft", "expand", "yh32", "yh_lo", "yh_hi", "band_rows", "fused"):
            assert d[k] == base[k], (k, shape)
    # the lane kernel's threshold counts beams, not rows (a lane owns a whole problem, whatever it stores)
    for R in (1, 3):
        for S, bins in ((56, 8), (57, 9)):
            d = _plan_rows(rows_lib, R, algo=ALGO["gss"], n_fft=1024, n_mics=8, n_streams=S, kp1=3, n_frames=96, n_cus=256)
            assert d["bins"] == bins, (R, S)
    # every other node ignores the field
    for algo in ("das", "mvdr", "lcmv", "phase", "phasempf", "mcra", "gsc"):
        shape = dict(algo=ALGO[algo], n_fft=1024, n_mics=8, n_streams=3, n_frames=20, n_cus=256, band_yh_lo=3, band_yh_hi=341)
        d = _plan_rows(rows_lib, 5, **shape)
        assert d.pop("rows") == 1 and d == chain_plan(emul_lib, **shape), algo
