"""MUSIC direction-of-arrival maps and eigenvalue profiles on the GPU (bf_doa_set_method(BF_DOA_MUSIC)): against the float64 restatement
(tests/doa_music_ref.py), independence of how a stream is cut, switching among the three methods on one handle, silent and all-zero
input, the device entry point and the refusals, two-source localisation with the source count, and the device loop that consumes the
maps (follow_sources_device).

Tolerance of the maps: 1e-9 relative L2, the project's bar for maps (test_doa_gpu.py).  The noise projector moves by about
1e-16 / gap under rounding, and test_doa_music_cpu.py holds every case below to gap >= 1e-5 (3.7e-3 is the smallest found), so about
1e-13 is expected.  The profile: 1e-12 absolute (eigenvalues of a trace-normalised matrix move by a few 1e-16)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_music_ref as ref  # noqa: E402

from beamform_amd.params import AIRA16_XY, make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 48000.0
GRID = np.arange(-180.0, 180.0)
GRID2 = np.arange(-180.0, 180.0, 2.0)
BF_EINVAL = -22


def _doa(M, hop, angles, lo, hi, W, n_streams=1, layout=0, method="music", n=None, mu=None):
    from beamform_amd.capi import Doa
    p = make_params("das", n_mics=M, hop=hop, mics=ref.geometry(M))
    d = Doa(p, angles, lo, hi, W, n_streams=n_streams, layout=layout)
    if method is not None:
        d.set_method(method)
    if n is not None:
        d.set_sources(n)
    if mu is not None:
        d.set_music_floor(mu)
    return d


def _ang_err(a, b):
    return np.abs((np.asarray(a) - b + 180.0) % 360.0 - 180.0)


def _check_against_ref(P, pk, E, Pr, Er, what=""):
    """test_doa_gpu.py's two rules for the map and the peak, and the profile's absolute bar."""
    err = np.linalg.norm(P - Pr) / np.linalg.norm(Pr)
    eerr = np.max(np.abs(E - Er))
    print(what, "relative L2 of the map:", err, " profile, max abs:", eerr)
    assert err <= 1e-9, err
    srt = np.sort(Pr, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-9 * srt[:, -1] if Pr.shape[1] > 1 else np.ones(len(Pr), bool)
    assert np.array_equal(pk[clear], np.argmax(Pr, axis=1)[clear])
    assert eerr <= 1e-12, eerr


def two_source_scene(F=32):
    """20 degrees at 0.2 plus -60 degrees at 0.05 (test_doa_music_cpu.py): frames of hop 512, 8 microphones."""
    return make_scene(8, F, 512, SR, seed=41, theta_s=20.0, interferers=(-60.0,), sigma_s=0.2, sigma_i=0.05, silent_frac=0.0)


# ---- 1. map, peak and profile against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,hop,D,W,layout,S,band,n", ref.GPU_CASES)
def test_map_peak_and_profile_match_restatement(M, hop, D, W, layout, S, band, n):
    F = ref.GPU_FRAMES
    angles = ref.gpu_case_angles(D)
    xs = [ref.gpu_case_scene(M, hop, s) for s in range(S)]
    doa = _doa(M, hop, angles, band[0], band[1], W, n_streams=S, layout=layout, n=n)
    x = np.stack([xx.T if layout == 1 else xx for xx in xs])
    P, pk, E = doa.process(x, eig=True)
    doa.close()
    P, pk, E = (P[None], pk[None], E[None]) if S == 1 else (P, pk, E)
    assert P.shape == (S, F // W, D) and pk.shape == (S, F // W) and E.shape == (S, F // W, M)
    assert np.all(P > 0) and np.all(P <= 1.0)
    assert np.all(E >= 0) and np.all(E <= 1.0) and np.all(np.diff(E, axis=2) <= 0)
    for s in range(S):
        Pr, _, Er, gap = ref.music_map(xs[s], ref.geometry(M), hop, SR, angles, band[0], band[1], W, n)
        assert gap >= 1e-5
        _check_against_ref(P[s], pk[s], E[s], Pr, Er, "M=%d stream %d (gap %.1e):" % (M, s, gap))


# ---- 2. cuts, chunks and launches --------------------------------------------------------------------------------------------------------
def test_cuts_chunks_and_launches_give_equal_bytes():
    M, hop, W = 8, 512, 8
    angles = np.arange(-180.0, 180.0, 5.0)
    x = make_scene(M, 8192, hop, SR, seed=7)  # 8192 frames: more than one internal chunk of spectra (about 4 000 frames)
    doa = _doa(M, hop, angles, 100.0, 16000.0, W, n=2)
    P1, k1, E1 = doa.process(x, eig=True)
    doa.reset()
    parts = [doa.process(x[:, i * 1024 * hop:(i + 1) * 1024 * hop], eig=True) for i in range(8)]
    assert P1.tobytes() == np.concatenate([p for p, _, _ in parts]).tobytes()
    assert k1.tobytes() == np.concatenate([k for _, k, _ in parts]).tobytes()
    assert E1.tobytes() == np.concatenate([e for _, _, e in parts]).tobytes()
    doa.reset()
    cuts = [0, 8, 24, 64, 72, 200, 1024]  # calls of W * q frames
    parts = [doa.process(x[:, a * hop:b * hop], eig=True) for a, b in zip(cuts[:-1], cuts[1:])]
    assert P1[:128].tobytes() == np.concatenate([p for p, _, _ in parts]).tobytes()
    assert k1[:128].tobytes() == np.concatenate([k for _, k, _ in parts]).tobytes()
    assert E1[:128].tobytes() == np.concatenate([e for _, _, e in parts]).tobytes()
    doa.reset()
    P2, k2, E2 = doa.process(x, eig=True)   # a second launch, and reset = the cold start
    assert P1.tobytes() == P2.tobytes() and k1.tobytes() == k2.tobytes() and E1.tobytes() == E2.tobytes()
    doa.reset()
    P3, k3 = doa.process(x[:, :256 * hop])  # without the profile: the same map
    assert P3.tobytes() == P1[:32].tobytes() and k3.tobytes() == k1[:32].tobytes()
    Pr, _, Er, _ = ref.music_map(x[:, :256 * hop], AIRA16_XY[:M], hop, SR, angles, 100.0, 16000.0, W, 2)
    _check_against_ref(P1[:32], k1[:32], E1[:32], Pr, Er)
    doa.close()


# ---- 3. switching among the three methods on one handle ------------------------------------------------------------------------------------
def test_method_switching_on_one_handle():
    M, hop, W = 8, 512, 8
    x = make_scene(M, 32, hop, SR, seed=13)
    doa = _doa(M, hop, GRID2, 100.0, 16000.0, W, method=None)
    Ps1, ks1 = doa.process(x)       # the default: SRP-PHAT
    doa.reset()
    doa.set_method("capon")
    Pc1, kc1 = doa.process(x)
    doa.reset()
    doa.set_sources(2)              # ignored by the other methods, kept across the switches
    doa.set_music_floor(0.05)
    Pc1b, _ = doa.process(x)
    assert Pc1b.tobytes() == Pc1.tobytes()
    doa.reset()
    doa.set_method("music")
    Pm, km, Em = doa.process(x, eig=True)
    doa.reset()
    doa.set_method("srp_phat")
    Ps2, ks2 = doa.process(x)
    doa.reset()
    doa.set_method("capon")
    Pc2, kc2 = doa.process(x)
    doa.reset()
    assert Ps1.tobytes() == Ps2.tobytes() and ks1.tobytes() == ks2.tobytes()
    assert Pc1.tobytes() == Pc2.tobytes() and kc1.tobytes() == kc2.tobytes()
    fresh = _doa(M, hop, GRID2, 100.0, 16000.0, W, n=2, mu=0.05)
    Pf, kf, Ef = fresh.process(x, eig=True)
    assert Pm.tobytes() == Pf.tobytes() and km.tobytes() == kf.tobytes() and Em.tobytes() == Ef.tobytes()
    assert Pm.tobytes() != Ps1.tobytes() and Pm.tobytes() != Pc1.tobytes()
    # the setters take effect at the next call, and only there
    fresh.reset()
    fresh.set_sources(1)
    P1, _, E1 = fresh.process(x, eig=True)
    assert P1.tobytes() != Pf.tobytes() and E1.tobytes() == Ef.tobytes()   # the profile does not depend on n
    fresh.reset()
    fresh.set_sources(2)
    fresh.set_music_floor(1e-2)
    Pmu, kmu, _ = fresh.process(x, eig=True)
    fresh.close()
    assert Pmu.tobytes() != Pf.tobytes() and np.array_equal(kmu, kf)   # mu moves the contrast, not the peak
    Pr, _, Er, _ = ref.music_map(x, AIRA16_XY[:M], hop, SR, GRID2, 100.0, 16000.0, W, 2, 0.05)
    _check_against_ref(Pm, km, Em, Pr, Er)
    doa.set_method("music")         # the switched handle still carries n = 2 and mu = 0.05
    Pm2, _ = doa.process(x)
    doa.close()
    assert Pm2.tobytes() == Pm.tobytes()


# ---- 4. silent microphone, all-zero input ------------------------------------------------------------------------------------------------
def test_silent_microphone():
    M, hop, W = 8, 512, 8
    x = make_scene(M, 32, hop, SR, seed=5, interferers=())
    x[3] = 0.0
    doa = _doa(M, hop, GRID, 100.0, 16000.0, W)
    P, k, E = doa.process(x, eig=True)
    doa.close()
    assert np.all(np.isfinite(P)) and np.all(P > 0) and np.all(P <= 1.0)
    Pr, _, Er, gap = ref.music_map(x, AIRA16_XY[:M], hop, SR, GRID, 100.0, 16000.0, W, 1)
    print("gap with a silent microphone:", gap)
    _check_against_ref(P, k, E, Pr, Er)


def test_all_zero_input():
    M, hop, W = 8, 512, 8
    for mu in (1e-2, 0.3):
        doa = _doa(M, hop, GRID, 100.0, 16000.0, W, mu=mu)
        P, k, E = doa.process(np.zeros((M, 16 * hop), np.float32), eig=True)
        doa.close()
        assert P.shape == (2, 360) and np.all(P == np.float64(mu) / (np.float64(mu) + 1.0))
        assert k.tolist() == [0, 0]
        assert E.shape == (2, M) and not E.any() and not np.signbit(E).any()


# ---- 5. the device entry point and the refusals ------------------------------------------------------------------------------------------
def test_device_entry_and_refusals():
    import torch
    from beamform_amd import capi
    from beamform_amd.capi import BfError
    M, hop, W, F = 8, 512, 4, 16
    x = make_scene(M, F, hop, SR, seed=9)
    doa = _doa(M, hop, GRID, 100.0, 16000.0, W, n=2)
    P, k, E = doa.process(x, eig=True)
    doa.reset()
    xd = torch.from_numpy(x).cuda()
    md = torch.full((F // W, 360), float("nan"), dtype=torch.float64, device="cuda")
    kd = torch.full((F // W,), -1, dtype=torch.int32, device="cuda")
    ed = torch.full((F // W, M), float("nan"), dtype=torch.float64, device="cuda")
    doa.process_device(xd.data_ptr(), F, md.data_ptr(), kd.data_ptr(), eig_ptr=ed.data_ptr())
    torch.cuda.synchronize()
    assert md.cpu().numpy().tobytes() == P.tobytes() and np.array_equal(kd.cpu().numpy(), k) and ed.cpu().numpy().tobytes() == E.tobytes()
    doa.reset()
    ed.fill_(float("nan"))
    doa.process_device(xd.data_ptr(), F, eig_ptr=ed.data_ptr())   # the profile alone
    torch.cuda.synchronize()
    assert ed.cpu().numpy().tobytes() == E.tobytes()
    doa.reset()
    md.fill_(float("nan"))
    doa.process_device(xd.data_ptr(), F, md.data_ptr(), kd.data_ptr())   # the existing call on a MUSIC handle: map and peak
    torch.cuda.synchronize()
    assert md.cpu().numpy().tobytes() == P.tobytes()

    def still_works():
        doa.reset()
        P2, k2, E2 = doa.process(x, eig=True)
        assert P2.tobytes() == P.tobytes() and k2.tobytes() == k.tobytes() and E2.tobytes() == E.tobytes()

    for bad in (0, M, -1, M + 5):
        with pytest.raises(BfError) as e:
            doa.set_sources(bad)
        assert e.value.code == BF_EINVAL
    still_works()
    for bad in (0.0, -1e-3, 1.5, float("nan"), float("inf")):
        with pytest.raises(BfError) as e:
            doa.set_music_floor(bad)
        assert e.value.code == BF_EINVAL
    still_works()
    doa.set_sources(M - 1)   # the ends of the ranges are inside
    doa.set_music_floor(1.0)
    doa.set_sources(2)
    doa.set_music_floor(1e-2)
    lib, h = capi.load(), doa._h
    assert lib.bf_doa_process_device_eig(h, xd.data_ptr(), F, None, None, None, None) == BF_EINVAL   # all three NULL
    assert lib.bf_doa_process_eig(h, x.ctypes.data, F, None, None, None) == BF_EINVAL
    still_works()
    doa.set_method("capon")
    doa.reset()
    with pytest.raises(BfError) as e:
        doa.process(x, eig=True)
    assert e.value.code == BF_EINVAL
    with pytest.raises(BfError) as e:
        doa.process_device(xd.data_ptr(), F, md.data_ptr(), kd.data_ptr(), eig_ptr=ed.data_ptr())
    assert e.value.code == BF_EINVAL
    doa.set_method("srp_phat")
    with pytest.raises(BfError) as e:
        doa.process(x, eig=True)
    assert e.value.code == BF_EINVAL
    doa.set_method("music")
    still_works()
    doa.close()


# ---- 6. two sources ----------------------------------------------------------------------------------------------------------------------
def test_localises_two_sources_and_counts_them():
    from beamform_amd.controllers import count_sources, pick_sources
    x = two_source_scene()
    doa = _doa(8, 512, GRID2, 100.0, 16000.0, 16, n=2)
    P, _, E = doa.process(x, eig=True)
    doa.close()
    assert P.shape == (2, 180) and E.shape == (2, 8)
    for b in range(2):
        got = GRID2[pick_sources(P[b], GRID2, 2, 15.0)]
        print("block", b, "picks", got, "profile", E[b][:4])
        for src in (20.0, -60.0):
            assert np.min(_ang_err(got, src)) <= 2.0, (b, got)
        assert count_sources(E[b]) == 2
    x1 = make_scene(8, 32, 512, SR, seed=5, interferers=(), silent_frac=0.0)
    doa = _doa(8, 512, GRID2, 100.0, 16000.0, 16)
    _, _, E1 = doa.process(x1, eig=True)
    doa.close()
    assert [count_sources(E1[b]) for b in range(2)] == [1, 1]


# ---- 7. the device loop with a MUSIC handle ----------------------------------------------------------------------------------------------
def test_follow_sources_device_with_a_music_handle():
    """test_picks_gpu.py's scheme: the loop with the picks taken on the device against the loop with the picks taken on the host from the
    same maps -- the same publications, the same track through the same kernels, so the same bytes."""
    from beamform_amd import capi
    from beamform_amd.controllers import DoaSources, follow_sources_device, follow_sources_tracked
    W, K, MIN_SEP = 16, 2, 30.0
    x = two_source_scene(64)
    p = make_params("lcmv", n_mics=8, theta=0.0, interf=[120.0])
    doa = _doa(8, 512, GRID2, 100.0, 16000.0, W, n=2)
    node = capi.Beamformer(p)
    y_host, pub_host = follow_sources_tracked(node, doa, x, W, DoaSources(GRID2, K, MIN_SEP))
    w_host = node.weights()
    node.close()
    doa.reset()
    node = capi.Beamformer(p)
    with capi.launch_trace() as tr:
        y_dev, pub_dev = follow_sources_device(node, doa, x, W, K, MIN_SEP)
    w_dev = node.weights()
    node.close()
    doa.close()
    assert any("doa_music_kernel<8>" in name for name in tr.kernels) and not any("doa_capon" in name for name in tr.kernels), tr.kernels
    assert pub_dev == pub_host and len(pub_dev) == 64 // W and all(len(i) == 1 for _, _, i in pub_dev)
    for _, theta, interf in pub_dev:
        assert _ang_err(theta, 20.0) <= 2.0 and _ang_err(interf[0], -60.0) <= 2.0
    assert np.array_equal(y_dev, y_host, equal_nan=True)
    assert np.array_equal(w_dev, w_host)
