"""Direction-of-arrival maps on the GPU (bf_doa_*): against the float64 restatement (tests/doa_ref.py), independence of how a
stream is cut, the PHAT floor beside a silent microphone, localisation, and the closed loop driving a das node."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402

from beamform_amd.params import AIRA16_XY, make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 48000.0
GRID = np.arange(-180.0, 180.0)
# eight microphones on a circle of radius 0.1 m plus eight on one of 0.2 m (no two coincide; aira16's microphones 1 and 7 do)
RING16 = [(0.1 * np.cos(2 * np.pi * i / 8), 0.1 * np.sin(2 * np.pi * i / 8)) for i in range(8)] + \
         [(0.2 * np.cos(2 * np.pi * (i + 0.5) / 8), 0.2 * np.sin(2 * np.pi * (i + 0.5) / 8)) for i in range(8)]


def _doa(M, hop, angles, lo, hi, W, mics=None, n_streams=1, layout=0):
    from beamform_amd.capi import Doa
    p = make_params("das", n_mics=M, hop=hop, **({"mics": mics} if mics is not None else {}))
    return Doa(p, angles, lo, hi, W, n_streams=n_streams, layout=layout)


def _ang_err(a, b):
    return np.abs((np.asarray(a) - b + 180.0) % 360.0 - 180.0)


def _check_against_ref(P, pk, Pr):
    err = np.linalg.norm(P - Pr) / np.linalg.norm(Pr)
    assert err <= 1e-9, err
    srt = np.sort(Pr, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-9 * srt[:, -1] if Pr.shape[1] > 1 else np.ones(len(Pr), bool)
    assert np.array_equal(pk[clear], np.argmax(Pr, axis=1)[clear])


CASES = [  # M, mics, hop, D, W, layout, streams, band
    (2, None, 128, 72, 1, 0, 1, (100.0, 16000.0)),
    (4, None, 512, 360, 8, 1, 3, (100.0, 16000.0)),
    (8, None, 512, 72, 8, 0, 3, (100.0, 24000.0)),
    (16, None, 2048, 1, 8, 0, 1, (300.0, 8000.0)),
    (8, RING16[:8], 512, 360, 1, 1, 1, (100.0, 16000.0)),
    (16, RING16, 128, 360, 8, 1, 1, (100.0, 16000.0)),
    (16, None, 512, 72, 1, 1, 3, (100.0, 16000.0)),
    (3, None, 2048, 72, 1, 0, 1, (100.0, 16000.0)),
]


@pytest.mark.parametrize("M,mics,hop,D,W,layout,S,band", CASES)
def test_map_matches_restatement(M, mics, hop, D, W, layout, S, band):
    F = 32
    angles = np.linspace(-180.0, 180.0, D, endpoint=False) + 0.25
    geo = list(AIRA16_XY[:M]) if mics is None else mics
    xs = [make_scene(M, F, hop, SR, seed=100 + s, mics=geo, theta_s=-40.0 + 50 * s) for s in range(S)]
    doa = _doa(M, hop, angles, band[0], band[1], W, mics=mics, n_streams=S, layout=layout)
    x = np.stack([xx.T if layout == 1 else xx for xx in xs])
    P, pk = doa.process(x)
    doa.close()
    P, pk = (P[None], pk[None]) if S == 1 else (P, pk)
    assert P.shape == (S, F // W, D) and pk.shape == (S, F // W)
    for s in range(S):
        Pr, _ = doa_ref.doa_map(xs[s], geo, hop, SR, angles, band[0], band[1], W)
        _check_against_ref(P[s], pk[s], Pr)


def test_cuts_chunks_and_launches_give_equal_bytes():
    M, hop, W = 8, 512, 8
    angles = np.arange(-180.0, 180.0, 5.0)
    x = make_scene(M, 8192, hop, SR, seed=7)  # 8192 frames: more than one internal chunk of spectra (about 3 850 frames)
    doa = _doa(M, hop, angles, 100.0, 16000.0, W)
    P1, k1 = doa.process(x)
    doa.reset()
    parts = [doa.process(x[:, i * 1024 * hop:(i + 1) * 1024 * hop]) for i in range(8)]
    assert P1.tobytes() == np.concatenate([p for p, _ in parts]).tobytes()
    assert k1.tobytes() == np.concatenate([k for _, k in parts]).tobytes()
    doa.reset()
    cuts = [0, 8, 24, 64, 72, 200, 1024]  # calls of W * q frames
    parts = [doa.process(x[:, a * hop:b * hop]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert P1[:128].tobytes() == np.concatenate([p for p, _ in parts]).tobytes()
    doa.reset()
    P2, k2 = doa.process(x)
    assert P1.tobytes() == P2.tobytes() and k1.tobytes() == k2.tobytes()  # a second launch, and reset = the cold start
    Pr, _ = doa_ref.doa_map(x[:, :256 * hop], AIRA16_XY[:M], hop, SR, angles, 100.0, 16000.0, W)
    _check_against_ref(P1[:32], k1[:32], Pr)
    doa.close()


def test_device_entry_and_bad_frame_counts():
    import torch
    from beamform_amd.capi import BfError
    M, hop, W = 8, 512, 4
    x = make_scene(M, 16, hop, SR, seed=9)
    doa = _doa(M, hop, GRID, 100.0, 16000.0, W)
    P, k = doa.process(x)
    doa.reset()
    xd = torch.from_numpy(x).cuda()
    md = torch.full((16 // W, 360), float("nan"), dtype=torch.float64, device="cuda")
    kd = torch.full((16 // W,), -1, dtype=torch.int32, device="cuda")
    doa.process_device(xd.data_ptr(), 16, md.data_ptr(), kd.data_ptr())
    torch.cuda.synchronize()
    assert md.cpu().numpy().tobytes() == P.tobytes() and np.array_equal(kd.cpu().numpy(), k)
    with pytest.raises(BfError) as e:
        doa.process(x[:, :6 * hop])  # 6 frames, W = 4
    assert e.value.code == -22
    with pytest.raises(BfError) as e:
        doa.process_device(xd.data_ptr(), 16, 0, 0)  # neither map nor peak
    assert e.value.code == -22
    doa.process_device(xd.data_ptr(), 0, md.data_ptr(), 0)  # 0 frames: a no-op
    doa.close()


def test_silent_microphone_contributes_nothing():
    M, hop, W = 8, 512, 8
    x = make_scene(M, 32, hop, SR, seed=5, interferers=()) * np.float32(1e6)  # packed-pair residue of the partner: ~1e-9 > eps
    x[3] = 0.0
    doa = _doa(M, hop, GRID, 100.0, 16000.0, W)
    P, k = doa.process(x)
    doa.close()
    Pr, _ = doa_ref.doa_map(x, AIRA16_XY[:M], hop, SR, GRID, 100.0, 16000.0, W)
    _check_against_ref(P, k, Pr)
    assert P.max() <= (7.0 / 8.0) ** 2 * (1 + 1e-12)


@pytest.mark.parametrize("theta", [-150.0, -60.0, 20.0, 90.0])
def test_localises_one_source(theta):
    x = make_scene(8, 64, 512, SR, seed=11, theta_s=theta, interferers=())
    doa = _doa(8, 512, GRID, 100.0, 16000.0, 16)
    _, k = doa.process(x)
    doa.close()
    assert np.all(_ang_err(GRID[k], theta) <= 2.0), GRID[k]
    x = make_scene(8, 64, 512, SR, seed=12, theta_s=theta)  # with the default interferers (-60, 90, 150 at half the level)
    doa = _doa(8, 512, GRID, 100.0, 16000.0, 64)
    _, k = doa.process(x)
    doa.close()
    assert _ang_err(GRID[k[0]], theta) <= 2.0


def test_closed_loop_follows_a_jump():
    from beamform_amd.capi import Beamformer
    from beamform_amd.controllers import DoaTheta, follow_doa
    a = make_scene(8, 64, 512, SR, seed=21, theta_s=20.0, interferers=(), silent_frac=0.0)
    b = make_scene(8, 64, 512, SR, seed=22, theta_s=-60.0, interferers=(), silent_frac=0.0)
    x = np.concatenate([a, b], axis=1)
    W = 16
    node = Beamformer(make_params("das", n_mics=8, theta=0.0))
    doa = _doa(8, 512, GRID, 100.0, 16000.0, W)
    y, published = follow_doa(node, doa, x, W, DoaTheta(GRID))
    node.close()
    doa.close()
    Pr, kr = doa_ref.doa_map(x, AIRA16_XY[:8], 512, SR, GRID, 100.0, 16000.0, W)
    assert y.shape == (x.shape[1],) and np.all(np.isfinite(y))
    assert [b for b, _ in published] == list(range(len(kr)))
    assert [t for _, t in published] == [float(GRID[i]) for i in kr]
    half = len(kr) // 2
    assert np.all(_ang_err([t for _, t in published[:half]], 20.0) <= 2.0)
    assert np.all(_ang_err([t for _, t in published[half:]], -60.0) <= 2.0)  # settled in the first block after the jump
