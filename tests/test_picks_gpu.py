"""Multi-source picks and their column track on the GPU (bf_doa_pick_device, bf_ctrack_from_picks_device; include/bfcore.h): both
kernels against their numpy restatements (tests/picks_ref.py, themselves checked against controllers.pick_sources / sources_track in
tests/test_picks_cpu.py) with array_equal, the device loop controllers.follow_sources_device against follow_sources_tracked and the
oracle, and examples/follow_sources_node against the device loop.  The kernels are asserted from a launch trace."""
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrack_cases as cc  # noqa: E402
import ctrack_ref  # noqa: E402
import picks_ref  # noqa: E402

from beamform_amd.params import AIRA16_XY, make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICK, CTRACK = "bf::doa_pick_kernel", "bf::ctrack_from_picks_kernel"


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _pick(torch, md, ad, S, nb, A, k, min_sep, rel_floor):
    """One bf_doa_pick_device call -> (picks [S, nb, k], kernels launched); the output starts as -77, so every place must be written."""
    from beamform_amd import capi
    out = torch.full((S, nb, k), -77, dtype=torch.int32, device="cuda")
    with capi.launch_trace() as tr:
        capi.doa_pick_device(md.data_ptr(), ad.data_ptr(), A, S, nb, k, min_sep, rel_floor, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), tr.kernels


# ---- 1. the picker -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 63, 64, 65, 360, 1024])
def test_picker_equals_its_restatement(A):
    """One lane; the last lane; the second register slot; a ragged last slot; the full 16 slots.  2 streams x 5 blocks of the CPU test's
    row kinds (random, ties, constant, all zero), on a sorted grid that holds -180 and 180 and on the same grid in no order."""
    torch = _torch()
    S, nb = 2, 5
    maps = picks_ref.rows(S * nb, A).reshape(S, nb, A)
    md = torch.from_numpy(maps).cuda()
    grids = picks_ref.grids(A)
    if A > 1:
        assert -180.0 in grids["sorted"] and 180.0 in grids["sorted"]
    n_short = 0
    for name in ("sorted", "unsorted"):
        ad = torch.from_numpy(np.ascontiguousarray(grids[name])).cuda()
        for k, min_sep, rel_floor in picks_ref.PARAMS:
            got, kernels = _pick(torch, md, ad, S, nb, A, k, min_sep, rel_floor)
            assert kernels == [PICK], kernels
            want = picks_ref.pick_all(maps, grids[name], k, min_sep, rel_floor)
            assert np.array_equal(got, want), (name, k, min_sep, rel_floor)
            n_short += int((want == -1).any())
    assert n_short > 0


def test_picker_tie_across_lanes_and_register_slots():
    """Equal maxima at indices 3, 64 + 3 (the same lane, the next register slot) and 7 (another lane): the lowest index wins, then 7,
    then 67."""
    torch = _torch()
    A = 130
    maps = np.random.default_rng(9).random((1, 1, A)) * 0.5
    maps[0, 0, [3, 64 + 3, 7]] = 0.875
    grid = np.linspace(-180.0, 180.0, A, endpoint=False)
    md, ad = torch.from_numpy(maps).cuda(), torch.from_numpy(grid).cuda()
    got, kernels = _pick(torch, md, ad, 1, 1, A, 4, 0.0, 0.0)
    assert kernels == [PICK] and list(got[0, 0, :3]) == [3, 7, 67], got
    assert np.array_equal(got, picks_ref.pick_all(maps, grid, 4, 0.0, 0.0))
    got, _ = _pick(torch, md, ad, 1, 1, A, 1, 30.0, 1.0)
    assert got[0, 0, 0] == 3


def test_picker_with_a_nan_stays_inside_the_row():
    """Outside the contract, but bounded: the kernel ends and writes nothing but -1 or an index of the row."""
    torch = _torch()
    S, nb, A = 2, 5, 130
    maps = picks_ref.rows(S * nb, A, seed=3).reshape(S, nb, A)
    maps[0, 0, 5] = maps[0, 1, 0] = maps[0, 2, A - 1] = maps[1, 0, 64] = np.nan
    maps[0, 3, :] = np.nan
    maps[1, 1, ::2] = np.nan
    md = torch.from_numpy(maps).cuda()
    ad = torch.from_numpy(picks_ref.grids(A)["unsorted"].copy()).cuda()
    for k, min_sep, rel_floor in picks_ref.PARAMS:
        got, kernels = _pick(torch, md, ad, S, nb, A, k, min_sep, rel_floor)
        assert kernels == [PICK]
        assert ((got == -1) | ((got >= 0) & (got < A))).all(), (k, min_sep, rel_floor, got)
        clean = ~np.isnan(maps).any(axis=2)  # and the rows without one are not disturbed
        want = picks_ref.pick_all(maps[clean], picks_ref.grids(A)["unsorted"], k, min_sep, rel_floor)
        assert np.array_equal(got[clean], want)


# ---- 2. the track builder ------------------------------------------------------------------------------------------------------------
def _builder_case(nb, A, k, seed):
    """Two streams with different picks: valid indices, -1 and values >= A (and far beyond) in column 0 and above, and maps of which
    about half clear min_peak = 0.5 at the first pick."""
    rng = np.random.default_rng(seed)
    S = 2
    picks = rng.integers(0, A, (S, nb, k)).astype(np.int32)
    bad = np.array([-1, -1, -5, A, A + 3, 2 ** 30, -2 ** 31], np.int64)
    hit = rng.random((S, nb, k)) < 0.3
    picks[hit] = bad[rng.integers(0, bad.size, int(hit.sum()))].astype(np.int32)
    maps = rng.random((S, nb, A))
    return picks, maps


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_builder_equals_its_restatement(nb):
    """Around the 64-block round of the wavefront.  One call, and for a latency of 0 and 1 block the same stream cut into three calls
    through carry."""
    from beamform_amd import capi
    torch = _torch()
    S, A, min_peak = 2, 9, 0.5
    n_calls = 0
    for k in (1, 3):
        picks, maps = _builder_case(nb, A, k, 700 + 10 * nb + k)
        assert not np.array_equal(picks[0], picks[1])
        pd, md = torch.from_numpy(picks).cuda(), torch.from_numpy(maps).cuda()
        for W in (1, 3):
            for n_cols in (1, 2, 4):
                for latency in (0, 1, 2, nb + 1):
                    for c_in in (-1, "mixed"):
                        c0 = np.full((S, n_cols), -1, np.int32) if c_in == -1 else np.array([[5, -1, 2, 99], [-3, 7, 0, -1]], np.int32)[:, :n_cols].copy()
                        for with_map in (True, False):
                            case = (k, W, n_cols, latency, c_in, with_map)
                            mp = min_peak if with_map else 0.0
                            t_ref, c_ref = picks_ref.from_picks(picks, maps if with_map else None, A, W, latency, mp, n_cols, c0)
                            cuts = [[(0, nb)]]
                            if latency <= 1 and nb >= 3:
                                cuts.append([(0, nb // 3), (nb // 3, nb - 2), (nb - 2, nb)])
                            for parts in cuts:
                                carry = torch.from_numpy(c0.copy()).cuda()
                                trk = torch.full((S, nb * W, n_cols), -77, dtype=torch.int32, device="cuda")
                                with capi.launch_trace() as tr:
                                    for a, b in parts:
                                        pk, mm = pd[:, a:b].contiguous(), md[:, a:b].contiguous()
                                        tt = torch.full((S, (b - a) * W, n_cols), -77, dtype=torch.int32, device="cuda")
                                        capi.ctrack_from_picks_device(pk.data_ptr(), mm.data_ptr() if with_map else 0, A, k, S, b - a, W, latency, mp,
                                                                      n_cols, carry.data_ptr(), tt.data_ptr())
                                        torch.cuda.synchronize()
                                        trk[:, a * W:b * W] = tt
                                assert tr.kernels == [CTRACK] * len(parts), tr.kernels
                                n_calls += len(parts)
                                assert np.array_equal(trk.cpu().numpy(), t_ref), (case, parts)
                                assert np.array_equal(carry.cpu().numpy(), c_ref), (case, parts)
    assert n_calls == (192 + 96 * 3 if nb >= 3 else 192)


def test_builder_cases_do_what_they_are_for():
    """The cases above hold what the issue lists: bad picks in column 0 and above, blocks below min_peak, and tracks in which a column
    keeps its value over a publication that does not mention it."""
    A, k, nb = 9, 3, 130
    picks, maps = _builder_case(nb, A, k, 700 + 10 * nb + k)
    ok = (picks >= 0) & (picks < A)
    assert (~ok[..., 0]).any() and (~ok[..., 1:]).any() and (picks >= A).any() and (picks < 0).any()
    first = np.take_along_axis(maps, np.clip(picks[..., :1], 0, A - 1).astype(np.int64), axis=2)[..., 0]
    pub = ok[..., 0] & ~(first < 0.5)
    assert 0.2 < pub.mean() < 0.8 and (ok[..., 0] & ~pub).any()
    assert (pub & ~ok[..., 1]).any()  # a publication that leaves column 1 as it is
    t, _ = picks_ref.from_picks(picks, maps, A, 1, 1, 0.5, 4, -1)
    assert (t[..., 3] == -1).all() and (t[..., :3] >= 0).any() and (t < A).all()


# ---- 3. the closed loop --------------------------------------------------------------------------------------------------------------
GRID2 = np.arange(-180.0, 180.0, 2.0)
M, W, F, K, MIN_SEP = 8, 8, 64, 2, 30.0
ENQUEUES = ["doa.process_device", "doa_pick_device", "ctrack_from_picks_device", "node.process_device_ctracked"]


def _scene():
    return make_scene(M, F, 512, cc.SR, seed=41, theta_s=20.0, interferers=(-60.0,), sigma_s=0.2, sigma_i=0.05, silent_frac=0.0)


def _recorded(mp, events, owner, name, label):
    fn = getattr(owner, name)

    def wrapper(*a, **kw):
        events.append(label)
        return fn(*a, **kw)
    mp.setattr(owner, name, wrapper)


@pytest.fixture(scope="module")
def loop():
    """Everything the loop tests look at, computed once: follow_sources_tracked and follow_sources_device on fresh nodes, the device
    track of the same maps, and the oracle with sources_track's track in force."""
    from beamform_amd import capi, controllers
    from beamform_amd.controllers import DoaSources, follow_sources_device, follow_sources_tracked, sources_track
    torch = _torch()
    x = _scene()
    p = make_params("lcmv", n_mics=M, theta=0.0, interf=[120.0])
    doa = capi.Doa(make_params("das", n_mics=M), GRID2, 100.0, 16000.0, W)
    doa.set_method("capon")
    r = dict(x=x, p=p)
    node = capi.Beamformer(p)
    r["y_host"], r["pub_host"] = follow_sources_tracked(node, doa, x, W, DoaSources(GRID2, K, MIN_SEP))
    r["w_host"] = node.weights()
    node.close()
    doa.reset()
    node = capi.Beamformer(p)
    events = []  # the loop's enqueues and everything that brings device memory to the host or waits for the device, in order
    with pytest.MonkeyPatch.context() as mp:
        _recorded(mp, events, capi.Doa, "process_device", ENQUEUES[0])
        _recorded(mp, events, capi, "doa_pick_device", ENQUEUES[1])
        _recorded(mp, events, capi, "ctrack_from_picks_device", ENQUEUES[2])
        _recorded(mp, events, capi.Beamformer, "process_device_ctracked", ENQUEUES[3])
        for name in ("cpu", "to", "item", "tolist", "numpy", "__array__"):
            _recorded(mp, events, torch.Tensor, name, "to the host: Tensor." + name)
        _recorded(mp, events, torch.cuda, "synchronize", "torch.cuda.synchronize")
        with capi.launch_trace() as tr:
            r["y_dev"], r["pub_dev"] = follow_sources_device(node, doa, x, W, K, MIN_SEP)
    r["events"], r["kernels"] = events, tr.kernels
    r["w_dev"] = node.weights()
    node.close()
    # the device track of the same maps (they do not depend on how the stream is cut)
    nb = F // W
    doa.reset()
    xd, ad = torch.from_numpy(x).cuda(), torch.from_numpy(GRID2).cuda()
    maps = torch.empty((nb, GRID2.size), dtype=torch.float64, device="cuda")
    picks = torch.full((nb, K), -77, dtype=torch.int32, device="cuda")
    carry = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    track = torch.full((nb * W, 2), -77, dtype=torch.int32, device="cuda")
    doa.process_device(xd.data_ptr(), F, maps.data_ptr(), 0)
    capi.doa_pick_device(maps.data_ptr(), ad.data_ptr(), GRID2.size, 1, nb, K, MIN_SEP, 0.0, picks.data_ptr())
    capi.ctrack_from_picks_device(picks.data_ptr(), maps.data_ptr(), GRID2.size, K, 1, nb, W, 1, 0.0, 2, carry.data_ptr(), track.data_ptr())
    torch.cuda.synchronize()
    doa.close()
    r["maps"], r["track_dev"] = maps.cpu().numpy(), track.cpu().numpy()
    r["track_host"], r["pub_track"] = sources_track(r["maps"], DoaSources(GRID2, K, MIN_SEP), W, 2)
    r["y_ref"], _, _ = ctrack_ref.oracle_ctracked(p, x, GRID2, r["track_host"], 0.0)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def test_device_loop_publishes_what_the_host_loop_publishes(loop):
    assert loop["pub_dev"] == loop["pub_host"] == loop["pub_track"]
    assert len(loop["pub_dev"]) == F // W and all(len(i) == 1 for _, _, i in loop["pub_dev"])
    assert np.array_equal(loop["track_dev"], loop["track_host"])
    assert (loop["track_dev"][:W] == -1).all() and (loop["track_dev"][W:] >= 0).all()
    assert np.array_equal(loop["w_dev"], loop["w_host"])  # the node is left at the last publication, as the host loop leaves it
    assert np.array_equal(loop["y_dev"], loop["y_host"], equal_nan=True)  # the same track through the same kernels


def test_device_loop_output_is_the_oracles(loop):
    cc.check(loop["y_dev"], None, loop["y_ref"], None)


def test_device_loop_is_four_enqueues_and_nothing_comes_back_in_between(loop):
    k = loop["kernels"]
    one = {n: [i for i, name in enumerate(k) if n in name] for n in ("doa_capon_kernel<8>", "doa_reduce_kernel", "doa_pick_kernel",
                                                                      "ctrack_from_picks_kernel", "mvdr_fast_track_kernel<8, 2, true>", "istft")}
    assert all(len(v) == 1 for v in one.values()), k
    assert k[one["doa_pick_kernel"][0]] == PICK and k[one["ctrack_from_picks_kernel"][0]] == CTRACK
    assert not cc.names(k, "mvdr_fast_kernel") and not cc.names(k, "track_from_peaks_kernel"), k
    order = [one[n][0] for n in ("doa_capon_kernel<8>", "doa_reduce_kernel", "doa_pick_kernel", "ctrack_from_picks_kernel",
                                 "mvdr_fast_track_kernel<8, 2, true>")]
    assert order == sorted(order) and order[3] == order[2] + 1, k
    assert cc.names(k[order[2]:], "doa_") == [PICK], k  # every DOA kernel is in front of the picker
    # the host side of the same stretch: from the first enqueue to the last nothing is brought to the host and nothing waits
    ev = loop["events"]
    first, last = ev.index(ENQUEUES[0]), ev.index(ENQUEUES[3])
    assert ev[first:last + 1] == ENQUEUES, ev
    assert any(e.startswith("to the host") for e in ev[last + 1:]), ev  # the recorder sees the copies at the end


# ---- 4. the example --------------------------------------------------------------------------------------------------------------------
def _write_float_wav(path, x, rate):
    """x [channels, n] float32 -> a WAVE_FORMAT_IEEE_FLOAT file: the samples reach the node as they are."""
    ch, n = x.shape
    data = np.ascontiguousarray(x.T).astype("<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_example_is_the_device_loop(loop, tmp_path):
    from beamform_amd import capi
    exe = os.path.join(ROOT, "examples", "follow_sources_node")
    assert os.path.exists(exe), "examples/follow_sources_node is built by `make all` (__graft_entry__.build)"
    lines = ["initial_angle: 0.0", "angle_interf1: 120.0"]
    lines += [f"mic{i}: {{id: {i}, x: {x:.3f}, y: {y:.3f}, z: 0.000}}" for i, (x, y) in enumerate(AIRA16_XY[:M])]
    cfg = tmp_path / "beamform_config.yaml"
    cfg.write_text("\n".join(lines) + "\n")
    _write_float_wav(str(tmp_path / "in.wav"), loop["x"], 48000)
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(cfg), str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(W), "-180", "180", "2",
                          str(K), str(MIN_SEP)], capture_output=True, text=True, timeout=150)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    published = []
    for line in out.stdout.splitlines():
        f = line.split()
        published.append((int(f[0]), float(f[1]), tuple(float(v) for v in f[2:])))
    assert published == loop["pub_dev"]
    with wave.open(str(tmp_path / "out.wav"), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 48000, F * 512)
        got = np.frombuffer(f.readframes(F * 512), "<i2")
    assert np.array_equal(got, capi.float_to_pcm16(loop["y_dev"]))
