"""Capon (MVDR) direction-of-arrival maps on the GPU (bf_doa_set_method(BF_DOA_CAPON)): against the float64 restatement
(tests/doa_capon_ref.py), independence of how a stream is cut, switching the method on one handle, silent and all-zero input, the
device entry point, two-source localisation, and the loops that consume the maps (follow_doa_device, follow_sources).

Tolerance of the maps: 1e-9 relative L2, the project's bar for maps (test_doa_gpu.py).  The solve amplifies rounding by at most
cond(R~) <= M (1 + delta) / delta, about 3e4 at the default delta = 1e-3, so about 1e-11 is expected; no case loads below 1e-3."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_capon_ref  # noqa: E402

from beamform_amd.params import AIRA16_XY, make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402
from conftest import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

SR = 48000.0
GRID = np.arange(-180.0, 180.0)
GRID2 = np.arange(-180.0, 180.0, 2.0)
# 32 microphones: two rings of 16 (no two coincide)
RING32 = [(0.1 * np.cos(2 * np.pi * i / 16), 0.1 * np.sin(2 * np.pi * i / 16)) for i in range(16)] + \
         [(0.2 * np.cos(2 * np.pi * (i + 0.5) / 16), 0.2 * np.sin(2 * np.pi * (i + 0.5) / 16)) for i in range(16)]


def _geo(M):
    return list(AIRA16_XY[:M]) if M <= 16 else RING32[:M]


def _doa(M, hop, angles, lo, hi, W, n_streams=1, layout=0, method="capon", loading=None):
    from beamform_amd.capi import Doa
    p = make_params("das", n_mics=M, hop=hop, mics=_geo(M))
    d = Doa(p, angles, lo, hi, W, n_streams=n_streams, layout=layout)
    if method is not None:
        d.set_method(method)
    if loading is not None:
        d.set_loading(loading)
    return d


def _ang_err(a, b):
    return np.abs((np.asarray(a) - b + 180.0) % 360.0 - 180.0)


def _check_against_ref(P, pk, Pr):
    """test_doa_gpu.py's two rules."""
    err = np.linalg.norm(P - Pr) / np.linalg.norm(Pr)
    print("relative L2 of the map:", err)
    assert err <= 1e-9, err
    srt = np.sort(Pr, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-9 * srt[:, -1] if Pr.shape[1] > 1 else np.ones(len(Pr), bool)
    assert np.array_equal(pk[clear], np.argmax(Pr, axis=1)[clear])


def two_source_scene(M=8, seed=41):
    """20 degrees at 0.2 plus -60 degrees at 0.05 (test_doa_capon_cpu.py): 32 frames of hop 512."""
    return make_scene(M, 32, 512, SR, seed=seed, theta_s=20.0, interferers=(-60.0,), sigma_s=0.2, sigma_i=0.05, silent_frac=0.0)


@pytest.fixture(scope="module")
def scene41():
    """The seed-41 scene and its restatement map (2 degree grid, W = 16): computed once, never written to."""
    x = two_source_scene()
    Pr, kr = doa_capon_ref.capon_map(x, AIRA16_XY[:8], 512, SR, GRID2, 100.0, 16000.0, 16)
    x.setflags(write=False)
    Pr.setflags(write=False)
    return x, Pr, kr


# ---- 1. the map against the restatement --------------------------------------------------------------------------------------------------
CASES = [  # M, hop, D, W, layout, streams, band, loading
    (2, 128, 72, 1, 0, 1, (100.0, 16000.0), None),
    (3, 512, 72, 8, 1, 3, (100.0, 16000.0), None),      # an odd count: the pinned partner row
    (8, 512, 360, 8, 0, 3, (100.0, 24000.0), None),
    (8, 512, 1, 4, 0, 1, (300.0, 2000.0), None),        # |K| < 64: one partly filled wavefront
    (9, 512, 72, 8, 1, 1, (100.0, 16000.0), None),      # an odd count above 8
    (16, 2048, 72, 8, 0, 1, (300.0, 8000.0), None),
    (32, 128, 8, 16, 0, 1, (100.0, 16000.0), None),
    (6, 512, 72, 4, 0, 1, (100.0, 16000.0), 1e-2),      # another loading (and the 6-row kernel, W < M)
]


@pytest.mark.parametrize("M,hop,D,W,layout,S,band,loading", CASES)
def test_map_matches_restatement(M, hop, D, W, layout, S, band, loading):
    F = 32
    angles = np.linspace(-180.0, 180.0, D, endpoint=False) + 0.25
    geo = _geo(M)
    xs = [make_scene(M, F, hop, SR, seed=100 + s, mics=geo, theta_s=-40.0 + 50 * s) for s in range(S)]
    doa = _doa(M, hop, angles, band[0], band[1], W, n_streams=S, layout=layout, loading=loading)
    x = np.stack([xx.T if layout == 1 else xx for xx in xs])
    P, pk = doa.process(x)
    doa.close()
    P, pk = (P[None], pk[None]) if S == 1 else (P, pk)
    assert P.shape == (S, F // W, D) and pk.shape == (S, F // W)
    assert np.all(P >= 0) and np.all(P <= 1.0)
    for s in range(S):
        Pr, _ = doa_capon_ref.capon_map(xs[s], geo, hop, SR, angles, band[0], band[1], W, **({"delta": loading} if loading else {}))
        _check_against_ref(P[s], pk[s], Pr)


# ---- 2. cuts, chunks and launches --------------------------------------------------------------------------------------------------------
def test_cuts_chunks_and_launches_give_equal_bytes():
    M, hop, W = 8, 512, 8
    angles = np.arange(-180.0, 180.0, 5.0)
    x = make_scene(M, 8192, hop, SR, seed=7)  # 8192 frames: more than one internal chunk of spectra (about 4 000 frames)
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
    Pr, _ = doa_capon_ref.capon_map(x[:, :256 * hop], AIRA16_XY[:M], hop, SR, angles, 100.0, 16000.0, W)
    _check_against_ref(P1[:32], k1[:32], Pr)
    doa.close()


# ---- 3. switching the method on one handle -----------------------------------------------------------------------------------------------
def test_method_switching_on_one_handle():
    M, hop, W = 8, 512, 8
    x = make_scene(M, 32, hop, SR, seed=13)
    doa = _doa(M, hop, GRID2, 100.0, 16000.0, W, method=None)
    Ps1, ks1 = doa.process(x)       # the default: SRP-PHAT
    doa.reset()
    doa.set_method("capon")
    Pc, kc = doa.process(x)
    doa.reset()
    doa.set_method("srp_phat")
    Ps2, ks2 = doa.process(x)
    doa.close()
    assert Ps1.tobytes() == Ps2.tobytes() and ks1.tobytes() == ks2.tobytes()
    fresh = _doa(M, hop, GRID2, 100.0, 16000.0, W)
    Pf, kf = fresh.process(x)
    fresh.close()
    assert Pc.tobytes() == Pf.tobytes() and kc.tobytes() == kf.tobytes()
    assert Pc.tobytes() != Ps1.tobytes()
    never = _doa(M, hop, GRID2, 100.0, 16000.0, W, method=None)   # a handle that never heard of the setters
    Pn, kn = never.process(x)
    never.close()
    assert Pn.tobytes() == Ps1.tobytes() and kn.tobytes() == ks1.tobytes()


# ---- 4. / 5. silent microphone, all-zero input -------------------------------------------------------------------------------------------
def test_silent_microphone():
    M, hop, W = 8, 512, 8
    x = make_scene(M, 32, hop, SR, seed=5, interferers=())
    x[3] = 0.0
    doa = _doa(M, hop, GRID, 100.0, 16000.0, W)
    P, k = doa.process(x)
    doa.close()
    assert np.all(np.isfinite(P)) and np.all(P >= 0) and np.all(P <= 1.0)
    Pr, _ = doa_capon_ref.capon_map(x, AIRA16_XY[:M], hop, SR, GRID, 100.0, 16000.0, W)
    _check_against_ref(P, k, Pr)


def test_all_zero_input_gives_a_zero_map():
    M, hop, W = 8, 512, 8
    doa = _doa(M, hop, GRID, 100.0, 16000.0, W)
    P, k = doa.process(np.zeros((M, 16 * hop), np.float32))
    doa.close()
    assert P.shape == (2, 360) and not P.any() and not np.signbit(P).any()
    assert k.tolist() == [0, 0]


# ---- 6. the device entry point and the setters' refusals ---------------------------------------------------------------------------------
def test_device_entry_and_refusals():
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
        doa.set_method(7)
    assert e.value.code == -22
    with pytest.raises(BfError) as e:
        doa.set_loading(0.0)
    assert e.value.code == -22
    for bad in (-1e-3, 1.5, float("nan"), float("inf")):
        with pytest.raises(BfError):
            doa.set_loading(bad)
    doa.reset()
    P2, k2 = doa.process(x)   # still the Capon handle with the default loading
    doa.close()
    assert P2.tobytes() == P.tobytes() and k2.tobytes() == k.tobytes()


# ---- 7. two sources ----------------------------------------------------------------------------------------------------------------------
def test_localises_two_sources(scene41):
    from beamform_amd.controllers import pick_sources
    x, Pr, _ = scene41
    doa = _doa(8, 512, GRID2, 100.0, 16000.0, 16)
    P, _ = doa.process(x)
    doa.close()
    assert P.shape == (2, 180)
    for b in range(2):
        got = GRID2[pick_sources(P[b], GRID2, 2, 15.0)]
        print("block", b, "picks", got)
        for src in (20.0, -60.0):
            assert np.min(_ang_err(got, src)) <= 2.0, (b, got)


# ---- 8. the peaks through the existing device loop ---------------------------------------------------------------------------------------
def test_follow_doa_device_with_a_capon_handle():
    from beamform_amd.capi import Beamformer
    from beamform_amd.controllers import follow_doa_device
    a = make_scene(8, 64, 512, SR, seed=21, theta_s=20.0, interferers=(), silent_frac=0.0)
    b = make_scene(8, 64, 512, SR, seed=22, theta_s=-60.0, interferers=(), silent_frac=0.0)
    x = np.concatenate([a, b], axis=1)   # test_closed_loop_follows_a_jump's input
    W = 16
    node = Beamformer(make_params("das", n_mics=8, theta=0.0))
    doa = _doa(8, 512, GRID, 100.0, 16000.0, W)
    y, published = follow_doa_device(node, doa, x, W)
    node.close()
    doa.close()
    _, kr = doa_capon_ref.capon_map(x, AIRA16_XY[:8], 512, SR, GRID, 100.0, 16000.0, W)
    assert y.shape == (x.shape[1],) and np.all(np.isfinite(y))
    assert [blk for blk, _ in published] == list(range(len(kr)))
    assert [t for _, t in published] == [float(GRID[i]) for i in kr]
    half = len(kr) // 2
    assert np.all(_ang_err([t for _, t in published[:half]], 20.0) <= 2.0)
    assert np.all(_ang_err([t for _, t in published[half:]], -60.0) <= 2.0)


# ---- 9. follow_sources ---------------------------------------------------------------------------------------------------------------------
class _ReplayDoa:
    """Hands follow_sources the restatement's map rows, block by block."""

    def __init__(self, P):
        self.P, self.b = P, 0

    def process(self, seg):
        self.b += 1
        return self.P[self.b - 1:self.b], None


@pytest.mark.parametrize("algo", ["lcmv", "gss"])
def test_follow_sources(algo, scene41):
    import oracle
    from beamform_amd.capi import Beamformer
    from beamform_amd.controllers import DoaSources, follow_sources, pick_sources
    x, Pr, _ = scene41
    W = 16
    # the restatement's rows have clear margins: at every greedy step the best remaining angle beats the next one by far more than
    # the maps' 1e-9, so the picks on the GPU's rows are the picks on the restatement's
    for row in Pr:
        free = np.ones(len(row), bool)
        for d in pick_sources(row, GRID2, 2, 15.0):
            top = np.sort(row[free])[-2:]
            assert top[1] == row[d] and top[1] - top[0] > 1e-6 * top[1], top
            free &= _ang_err(GRID2, GRID2[d]) >= 15.0
    p = make_params(algo, n_mics=8, theta=0.0, interf=[])
    ref_node = oracle.OracleNode(p)
    y_ref, pub_ref = follow_sources(ref_node, _ReplayDoa(Pr), x, W, DoaSources(GRID2, 2, 15.0))
    node = Beamformer(p)
    doa = _doa(8, 512, GRID2, 100.0, 16000.0, W)
    y, published = follow_sources(node, doa, x, W, DoaSources(GRID2, 2, 15.0))
    node.close()
    doa.close()
    assert published == pub_ref and len(published) == 2
    assert ref_node.S == 2                       # the interferer was appended after block 0
    assert all(len(i) == 1 for _, _, i in published)
    y = np.asarray(y).reshape(-1)
    ok = np.isfinite(y_ref)
    assert y.shape == y_ref.shape and (np.isfinite(y) == ok).all()
    assert np.abs(y_ref[ok][W * 512:]).max() > 1e-3   # block 1, steered and constrained by block 0's publication, has signal
    err = rel_l2(y[ok], y_ref[ok])
    print(algo, "relative L2 against the oracle:", err)
    assert err <= 1e-5, err
