"""Talker identities on the GPU (bf_ctrack_assign_device; include/bfcore.h): ctrack_assign_kernel against its numpy restatement
(tests/assign_ref.py, itself checked against doa_assign.hpp and controllers.assign_sources in tests/test_assign_cpu.py) with
array_equal on track, active and state, and the five-segment conversation end to end -- Capon maps, device picks, the new builder and
a column-tracked lcmv batch with a beam per column -- alone and through controllers.follow_talkers_device.  The kernel is asserted
from a launch trace.  Out-of-range picks sit inside buffers of the exact size and are compared with the restatement; nothing here
tries to make a bad index fault."""
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref  # noqa: E402
import picks_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ASSIGN = "bf::ctrack_assign_kernel"


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _device(torch, picks, maps, angles, W, latency, min_peak, gate, min_hits, max_coast, n_cols, state, with_active=True, n_launch=1):
    """assign_ref.assign's signature on the device; every output starts as -77, so every place must be written.
    -> (track, active or None, state), the kernels launched."""
    from beamform_amd import capi
    picks = np.ascontiguousarray(picks, np.int32)
    S, nb, k = picks.shape
    A = np.asarray(angles).size
    pd = torch.from_numpy(picks).cuda()
    md = None if maps is None else torch.from_numpy(np.ascontiguousarray(maps, np.float64)).cuda()
    ad = torch.from_numpy(np.ascontiguousarray(angles, np.float64)).cuda()
    st0 = np.ascontiguousarray(np.broadcast_to(np.asarray(state, np.int32), (S, n_cols, 4)))
    outs = []
    with capi.launch_trace() as tr:
        for _ in range(n_launch):
            sd = torch.from_numpy(st0.copy()).cuda()
            trk = torch.full((S, nb * W, n_cols), -77, dtype=torch.int32, device="cuda")
            act = torch.full((S, nb, n_cols), -77, dtype=torch.int32, device="cuda") if with_active else None
            capi.ctrack_assign_device(pd.data_ptr(), 0 if md is None else md.data_ptr(), ad.data_ptr(), A, k, S, nb, W, latency, min_peak, gate,
                                      min_hits, max_coast, n_cols, sd.data_ptr(), trk.data_ptr(), 0 if act is None else act.data_ptr())
            torch.cuda.synchronize()
            outs.append((trk.cpu().numpy(), None if act is None else act.cpu().numpy(), sd.cpu().numpy()))
    for o in outs[1:]:  # the same bytes on every launch
        assert all(np.array_equal(x, y) for x, y in zip(o, outs[0]) if x is not None)
    return outs[0], tr.kernels


def _check(got, ref, what):
    for x, y, n in zip(got, ref, ("track", "active", "state")):
        if x is not None:
            assert x.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), (what, n)


# ---- 1. the kernel against its restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", assign_ref.A_SET)
def test_kernel_equals_its_restatement(A):
    """The CPU test's sweep (grids, row kinds with -1 holes, out-of-range and repeated picks, k, n_cols, gate, min_hits, max_coast,
    latency, W, nb, with and without a map, cold and garbage states) on 3 streams, every fourth case also on 1, with and without the
    active output, and launched twice."""
    torch = _torch()
    n = 0
    for i, c in enumerate(c for c in assign_ref.sweep() if c["A"] == A):
        for S in (3, 1) if i % 4 == 0 else (3,):
            picks, maps, angles, min_peak, state = assign_ref.case_input(c, S)
            ref = assign_ref.run(assign_ref.assign, c, picks, maps, angles, min_peak, state)
            got, kernels = _device(torch, picks, maps, angles, c["W"], c["latency"], min_peak, c["gate"], c["min_hits"], c["max_coast"],
                                   c["n_cols"], state, with_active=i % 3 != 1, n_launch=2 if i % 5 == 0 else 1)
            assert kernels and set(kernels) == {ASSIGN}, kernels
            _check(got, ref, (c, S))
            n += 1
    assert n == 72 + 18


def test_kernel_on_seventy_streams_and_every_block_count():
    """More streams than one lane group, one wavefront each, with different picks per stream: 70 streams x 1, 2 and 67 blocks (one
    round, a ragged round, 17 rounds of four blocks), talkers that drift, pause and come back."""
    torch = _torch()
    A, k, n_cols, S = 24, 3, 4, 70
    angles = picks_ref.grids(A)["unsorted"]
    for nb in assign_ref.NB_SET:
        picks = assign_ref.slow_rows(S, nb, k, A, 21)
        maps = assign_ref.maps_for(S, nb, A, 21)
        state = assign_ref.garbage_state(S, n_cols, A, 21)
        for with_map, latency in ((True, 1), (False, 0), (True, 3)):
            args = (maps if with_map else None, angles, 2, latency, 0.3 if with_map else 0.0, 20.0, 2, 2, n_cols, state)
            ref = assign_ref.assign(picks, *args)
            got, kernels = _device(torch, picks, *args, n_launch=2)
            assert kernels == [ASSIGN] * 2
            _check(got, ref, (nb, with_map, latency))
            if nb == 67:
                assert ref[1].any() and not np.array_equal(ref[0][0], ref[0][1])


@pytest.mark.parametrize("latency", [0, 1])
def test_split_calls_continue_the_stream(latency):
    torch = _torch()
    A, k, nb, W, n_cols, S = 24, 3, 13, 2, 3, 3
    picks = assign_ref.slow_rows(S, nb, k, A, 11)
    maps = assign_ref.maps_for(S, nb, A, 11)
    angles = picks_ref.grids(A)["unsorted"]
    tail = (angles, W, latency, 0.3, 20.0, 2, 2, n_cols)
    one = assign_ref.assign(picks, maps, *tail, -1)
    for cuts in ((0, 1, nb), (0, 4, 5, nb), (0, 9, nb)):
        state, trk, act = np.full((S, n_cols, 4), -1, np.int32), [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            (t, ac, state), kernels = _device(torch, picks[:, a:b], maps[:, a:b], *tail, state)
            assert kernels == [ASSIGN]
            trk.append(t)
            act.append(ac)
        _check((np.concatenate(trk, axis=1), np.concatenate(act, axis=1), state), one, (latency, cuts))


# ---- 2. the conversation end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """Everything the scene tests look at, computed once: the device's maps and picks, the device track, the column-tracked batch fed
    that track, the same batch fed the restatement's track from the host, and follow_talkers_device on a fresh node."""
    from beamform_amd import capi
    from beamform_amd.controllers import follow_talkers_device
    from beamform_amd.params import make_params
    torch = _torch()
    g, W, M = assign_ref.SCENE_GRID, assign_ref.SCENE_W, assign_ref.SCENE_M
    k, min_sep, rel_floor = assign_ref.SCENE_PICK
    p = assign_ref.SCENE_ASSIGN
    x = assign_ref.scene_audio()
    F = x.shape[1] // 512
    nb, A, n_cols = F // W, g.size, p["n_cols"]
    params = make_params("lcmv", n_mics=M, theta=0.0, interf=[120.0, -120.0])
    doa = capi.Doa(make_params("das", n_mics=M), g, 100.0, 16000.0, W)
    doa.set_method("capon")
    r = dict(nb=nb, F=F, x=x)
    xd, ad = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    maps = torch.empty((nb, A), dtype=torch.float64, device="cuda")
    picks = torch.full((nb, k), -77, dtype=torch.int32, device="cuda")
    state = torch.full((n_cols, 4), -1, dtype=torch.int32, device="cuda")
    track = torch.full((nb * W, n_cols), -77, dtype=torch.int32, device="cuda")
    active = torch.full((nb, n_cols), -77, dtype=torch.int32, device="cuda")
    yd = torch.full((n_cols, F * 512), float("nan"), dtype=torch.float32, device="cuda")
    node = capi.Beamformer(params, lcmv_out_beams=n_cols)
    node.set_ctrack_angles(g)
    with capi.launch_trace() as tr:
        doa.process_device(xd.data_ptr(), F, maps.data_ptr(), 0)
        capi.doa_pick_device(maps.data_ptr(), ad.data_ptr(), A, 1, nb, k, min_sep, rel_floor, picks.data_ptr())
        capi.ctrack_assign_device(picks.data_ptr(), 0, ad.data_ptr(), A, k, 1, nb, W, p["latency"], 0.0, p["gate"], p["min_hits"],
                                  p["max_coast"], n_cols, state.data_ptr(), track.data_ptr(), active.data_ptr())
        node.process_device_ctracked(xd.data_ptr(), F, yd.data_ptr(), track.data_ptr(), n_cols)
    torch.cuda.synchronize()
    node.close()
    r["kernels"] = tr.kernels
    r["picks"], r["track"], r["active"], r["state"], r["y"] = (v.cpu().numpy() for v in (picks, track, active, state, yd))
    # the restatement on the device's own picks, and its track through the same batch from the host
    r["ref"] = assign_ref.assign(r["picks"][None], None, g, W, p["latency"], 0.0, p["gate"], p["min_hits"], p["max_coast"], n_cols, -1)
    node = capi.Beamformer(params, lcmv_out_beams=n_cols)
    node.set_ctrack_angles(g)
    td = torch.from_numpy(np.ascontiguousarray(r["ref"][0][0])).cuda()
    yd.fill_(float("nan"))
    node.process_device_ctracked(xd.data_ptr(), F, yd.data_ptr(), td.data_ptr(), n_cols)
    torch.cuda.synchronize()
    r["y_host_track"] = yd.cpu().numpy()
    node.close()
    doa.reset()
    node = capi.Beamformer(params, lcmv_out_beams=n_cols)
    with capi.launch_trace() as tr:
        r["loop"] = follow_talkers_device(node, doa, x, W, k, min_sep, rel_floor, 0.0, p["gate"], p["min_hits"], p["max_coast"])
    r["loop_kernels"] = tr.kernels
    node.close()
    doa.close()
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def test_scene_device_track_is_the_restatements(scene):
    assert ((scene["picks"] == -1) | ((scene["picks"] >= 0) & (scene["picks"] < assign_ref.SCENE_GRID.size))).all()
    assert np.array_equal(scene["track"], scene["ref"][0][0])
    assert np.array_equal(scene["active"], scene["ref"][1][0])
    assert np.array_equal(scene["state"], scene["ref"][2][0])
    k = scene["kernels"]
    assert k.count(ASSIGN) == 1 and not [n for n in k if "ctrack_from_picks_kernel" in n], k
    assert k.index("bf::doa_pick_kernel") + 1 == k.index(ASSIGN) < len(k) - 1, k   # then the column-tracked batch


def test_scene_columns_stay_with_their_talkers(scene):
    """Column 0 within 5 degrees of 20 and column 1 within 5 degrees of -60 in every block from 2 on -- through the change of the
    loudest talker at block 2, the pause of blocks 4 and 5 and the third talker of blocks 8 and 9."""
    g, W = assign_ref.SCENE_GRID, assign_ref.SCENE_W
    per_block = scene["track"].reshape(scene["nb"], W, -1)
    assert (per_block == per_block[:, :1]).all()
    cols = per_block[2:, 0]
    assert (cols[:, :2] >= 0).all()
    assert (picks_ref.sep(g[cols[:, 0]], 20.0) <= 5.0).all(), g[cols[:, 0]]
    assert (picks_ref.sep(g[cols[:, 1]], -60.0) <= 5.0).all(), g[cols[:, 1]]
    assert (scene["track"][:2 * W] == -1).all()


def test_scene_output_is_the_host_tracks(scene):
    y = scene["y"]
    assert y.shape == (3, scene["F"] * 512) and all(y[r][np.isfinite(y[r])].any() for r in range(3))
    assert np.array_equal(y, scene["y_host_track"], equal_nan=True)


def test_follow_talkers_device_is_the_four_enqueues(scene):
    g, W, nb = assign_ref.SCENE_GRID, assign_ref.SCENE_W, scene["nb"]
    y, columns, active = scene["loop"]
    assert np.array_equal(y, scene["y"], equal_nan=True)
    assert np.array_equal(active, scene["active"]) and active.dtype == np.int32
    outs = assign_ref.outs_of(scene["track"], scene["state"], W)
    assert columns.shape == (nb, 3) and columns.dtype == np.float64
    assert np.array_equal(np.isnan(columns), outs < 0)
    assert np.array_equal(columns[outs >= 0], g[outs[outs >= 0]])
    k = scene["loop_kernels"]
    assert k.count(ASSIGN) == 1 and k.count("bf::doa_pick_kernel") == 1 and not [n for n in k if "ctrack_from_picks_kernel" in n], k
    assert k.index("bf::doa_pick_kernel") + 1 == k.index(ASSIGN)


# ---- 3. the example --------------------------------------------------------------------------------------------------------------------
def _write_float_wav(path, x, rate):
    """x [channels, n] float32 -> a WAVE_FORMAT_IEEE_FLOAT file: the samples reach the node as they are."""
    ch, n = x.shape
    data = np.ascontiguousarray(x.T).astype("<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def test_example_identity_mode_is_the_device_loop(scene, tmp_path):
    """examples/follow_sources_node ... beams=3 capon identity 20: a WAV per talker, and per column its last angle and the share of
    blocks in which it was heard.  The example coasts for 8 blocks where the scene tests coast for 4; no pause of this scene is that long."""
    from beamform_amd import capi
    from beamform_amd.params import AIRA16_XY
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "follow_sources_node")
    assert os.path.exists(exe), "examples/follow_sources_node is built by `make all` (__graft_entry__.build)"
    g, W, M, nb = assign_ref.SCENE_GRID, assign_ref.SCENE_W, assign_ref.SCENE_M, scene["nb"]
    k, min_sep, rel_floor = assign_ref.SCENE_PICK
    ref8 = assign_ref.assign(scene["picks"][None], None, g, W, 1, 0.0, 20.0, 2, 8, 3, -1)
    assert np.array_equal(ref8[0][0], scene["track"]) and np.array_equal(ref8[1][0], scene["active"])
    lines = ["initial_angle: 0.0", "angle_interf1: 120.0", "angle_interf2: -120.0"]
    lines += [f"mic{i}: {{id: {i}, x: {x:.3f}, y: {y:.3f}, z: 0.000}}" for i, (x, y) in enumerate(AIRA16_XY[:M])]
    cfg = tmp_path / "beamform_config.yaml"
    cfg.write_text("\n".join(lines) + "\n")
    _write_float_wav(str(tmp_path / "in.wav"), scene["x"], 48000)
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(cfg), str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(W), "-180", "180", "2",
                          str(k), str(min_sep), str(rel_floor), "0", "100", "16000", "3", "capon", "identity", "20"],
                         capture_output=True, text=True, timeout=150)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    cols = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("column ")]
    last, share = ref8[2][0][:, 3], ref8[1][0].mean(axis=0)
    assert [int(c[1]) for c in cols] == [0, 1, 2]
    assert [float(c[2]) for c in cols] == [float(g[i]) for i in last] == [20.0, -60.0, 110.0]
    assert np.allclose([float(c[3]) for c in cols], share, atol=1e-6) and list(share) == [0.7, 0.7, 0.1]
    for r in range(3):
        with wave.open(str(tmp_path / f"out.wav.{r}.wav"), "rb") as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 48000, scene["F"] * 512)
            got = np.frombuffer(f.readframes(scene["F"] * 512), "<i2")
        assert np.array_equal(got, capi.float_to_pcm16(scene["y"][r]))
