"""Direction-of-arrival maps (bf_doa_*): the float64 restatement, the C ABI's argument checks, and the physical expectations the GPU
tests (test_doa_gpu.py) rely on, established here on the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402

from beamform_amd.params import AIRA16_XY, make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

SR = 48000.0
GRID = np.arange(-180.0, 180.0)  # 360 angles, 1 degree


def _ang_err(a, b):
    return np.abs((np.asarray(a) - b + 180.0) % 360.0 - 180.0)


def test_restatement_matches_naive_loops():
    rng = np.random.default_rng(3)
    mics = AIRA16_XY[:3]
    x = rng.standard_normal((3, 4 * 16)).astype(np.float32)
    x[2, :20] = 0.0  # a silent stretch: bins of exactly zero
    angles = [-90.0, 0.0, 45.0, 170.0]
    P, pk = doa_ref.doa_map(x, mics, 16, SR, angles, 3000.0, 24000.0, 2)
    Pn = doa_ref.doa_map_naive(x, mics, 16, SR, angles, 3000.0, 24000.0, 2)
    assert np.allclose(P, Pn, rtol=1e-12, atol=1e-14)
    assert np.array_equal(pk, np.argmax(Pn, axis=1))
    assert np.all(P >= 0) and np.all(P <= 1 + 1e-12)


def test_band_uses_quirk_q1():
    # f[N/2-1] = sr/2: a band ending at the Nyquist frequency includes bin N/2-1 (and nothing else above 23.9 kHz)
    assert doa_ref.band_bins(1024, SR, 23950.0, 24000.0).tolist() == [511]
    assert doa_ref.band_bins(1024, SR, 100.0, 16000.0)[[0, -1]].tolist() == [3, 341]


def test_symbols_exported():
    from beamform_amd import capi
    lib = capi.load()
    for s in ("bf_doa_create", "bf_doa_set_phat_floor", "bf_doa_process_device", "bf_doa_process", "bf_doa_reset", "bf_doa_destroy"):
        assert s in capi.EXPORTS and hasattr(lib, s), s


def _create(cfg, angles, lo, hi, W):
    from beamform_amd import capi
    lib = capi.load()
    h = C.c_void_p()
    a = np.ascontiguousarray(angles, np.float64)
    ap = a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
    rc = lib.bf_doa_create(C.byref(cfg), ap, int(a.size), lo, hi, W, C.byref(h))
    if rc == 0:
        lib.bf_doa_destroy(h)
    return rc


def test_create_checks_arguments_with_or_without_gpu():
    import torch
    from beamform_amd import capi
    lib = capi.load()
    cfg = capi.config_from_params(make_params("das", n_mics=8))
    EINVAL, ENODEV = -22, -19
    assert _create(cfg, GRID, 100.0, 16000.0, 0) == EINVAL                  # W = 0
    assert _create(cfg, [], 100.0, 16000.0, 16) == EINVAL                   # D = 0
    assert _create(cfg, np.zeros(1025), 100.0, 16000.0, 16) == EINVAL       # D > BF_DOA_MAX_ANGLES
    assert _create(cfg, GRID, 10.0, 20.0, 16) == EINVAL                     # no bin in the band (bin width 46.9 Hz)
    assert _create(cfg, GRID, 16000.0, 100.0, 16) == EINVAL                 # inverted band
    c1 = capi.config_from_params(make_params("das", n_mics=8))
    c1.n_mics = 1
    assert _create(c1, GRID, 100.0, 16000.0, 16) == EINVAL                  # M = 1
    c2 = capi.config_from_params(make_params("das", n_mics=8))
    c2.hop = 384
    assert _create(c2, GRID, 100.0, 16000.0, 16) == EINVAL                  # not a JACK period
    c3 = capi.config_from_params(make_params("das", n_mics=16, mics=AIRA16_XY[:16]))
    c3.hop = 4096
    assert _create(c3, np.zeros(1024), 0.0, 24000.0, 1) == EINVAL           # 4095 x 16 x 1024 complex doubles > 512 MiB
    h = C.c_void_p()
    assert lib.bf_doa_create(None, np.zeros(1).ctypes.data_as(C.POINTER(C.c_double)), 1, 0.0, 1e4, 1, C.byref(h)) == EINVAL
    assert lib.bf_doa_process(None, None, 0, None, None) == EINVAL
    assert lib.bf_doa_set_phat_floor(None, 1e-10) == EINVAL
    assert lib.bf_doa_reset(None) == EINVAL
    lib.bf_doa_destroy(None)
    if not torch.cuda.is_available():
        assert lib.bf_device_count() <= 0
        assert _create(cfg, GRID, 100.0, 16000.0, 16) == ENODEV
        assert b"no CPU fallback" in lib.bf_last_error(None)
        with pytest.raises(capi.BfError):
            capi.Doa(make_params("das", n_mics=8), GRID, 100.0, 16000.0, 16)
    else:
        assert _create(cfg, GRID, 100.0, 16000.0, 16) == 0


# ---- the scenes of test_doa_gpu.py, checked on the restatement --------------------------------------------------------------------
def test_localisation_expectation_on_restatement():
    """One source + sensor noise, 8 aira16 microphones, 1 degree grid, W = 16: the peak is within 2 degrees in every block; with
    the default interferers the global peak stays at the target."""
    mics = AIRA16_XY[:8]
    for th in (-150.0, -60.0, 20.0, 90.0):
        x = make_scene(8, 64, 512, SR, seed=11, theta_s=th, interferers=())
        P, pk = doa_ref.doa_map(x, mics, 512, SR, GRID, 100.0, 16000.0, 16)
        assert np.all(_ang_err(GRID[pk], th) <= 2.0), (th, GRID[pk])
        x = make_scene(8, 64, 512, SR, seed=12, theta_s=th)
        P, _ = doa_ref.doa_map(x, mics, 512, SR, GRID, 100.0, 16000.0, 64)
        assert _ang_err(GRID[np.argmax(P[0])], th) <= 2.0, th


def test_closed_loop_expectation_on_restatement():
    """The source jumps from 20 to -60 degrees halfway: the block peaks settle within 2 degrees of -60 within one block."""
    x = _jump_scene()
    P, pk = doa_ref.doa_map(x, AIRA16_XY[:8], 512, SR, GRID, 100.0, 16000.0, 16)
    nb = len(pk)
    assert np.all(_ang_err(GRID[pk[:nb // 2]], 20.0) <= 2.0)
    assert np.all(_ang_err(GRID[pk[nb // 2:]], -60.0) <= 2.0)


def _jump_scene():
    a = make_scene(8, 64, 512, SR, seed=21, theta_s=20.0, interferers=(), silent_frac=0.0)
    b = make_scene(8, 64, 512, SR, seed=22, theta_s=-60.0, interferers=(), silent_frac=0.0)
    return np.concatenate([a, b], axis=1)


def test_silent_microphone_expectation_on_restatement():
    """A digitally silent microphone beside loud ones contributes nothing: the map equals 1/M^2 * (the map of the other M-1
    microphones' sum scaled to M-1 channels), checked here as: its X^ is 0 in every bin, so P <= ((M-1)/M)^2."""
    x = make_scene(8, 32, 512, SR, seed=5, interferers=()) * np.float32(1000.0)
    x[3] = 0.0
    P, _ = doa_ref.doa_map(x, AIRA16_XY[:8], 512, SR, GRID, 100.0, 16000.0, 8)
    assert P.max() <= (7.0 / 8.0) ** 2 + 1e-12
    assert P.max() > 0.5 * (7.0 / 8.0) ** 2
