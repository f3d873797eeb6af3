"""lcmv with one beam per constraint column (bf_config.lcmv_out_beams = R): the rows of each beam through the C ABI against the oracle
driven with swapped angles (tests/lcmv_beams_cases.py; the identity behind it: tests/test_lcmv_beams_cpu.py).  Every row is judged on its
own at the suite's 1e-5 per-frame relative L2; the non-finite frames must be the reference's (frame 0 after a cold start, no more); what
the definition makes zero must be exactly zero; row 0 must be the R = 1 handle's bytes, whose trace names the kernels it always named."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from beamform_amd.capi import BF_INTERLEAVED, BF_PRECISION_MIXED, BfError
from lcmv_beams_cases import (CASES, SEM, THETA, TRACK_ANGLES, case_params, case_ref, case_scene, case_track, check_case, check_rows,
                              check_time, run_case, run_dev, run_one_row, sem_params, sem_ref, sem_scene, track_ref)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE = ["l8k2", "l8k3", "l4k1", "l6k3", "l8k1r4"]
LANE_KERNEL = {"l8k2": "<8, 3, true>", "l8k3": "<8, 4, true>", "l4k1": "<4, 2, true>", "l6k3": "<6, 4, true>", "l8k1r4": "<8, 2, true>"}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _bf(p, **kw):
    from beamform_amd.capi import Beamformer
    _torch()
    return Beamformer(p, **kw)


# ---- 1. the three per-bin kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LANE)
def test_lane_kernel_rows(name):
    """mvdr_fast_rows_kernel: one batch, then the same stream as two uneven batches (the deferred last store falls on a batch end)."""
    _torch()
    y, Y, kernels = run_case(name)
    check_case(name, y, Y, kernels, "mvdr_fast_rows_kernel" + LANE_KERNEL[name], "mvdr_fast_kernel" + LANE_KERNEL[name])
    y2, Y2, _ = run_case(name, cuts=(5,))
    check_rows(case_params(name), y2, Y2, *case_ref(name))


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import lcmv_beams_cases as lc
y, Y, kernels = lc.run_case(%(name)r)
lc.check_case(%(name)r, y, Y, kernels, %(twin)r, %(one_row)r)
print("RESULT ok")
"""


def _child(env, name, twin, one_row):
    """The switches are read once per process: the case in a child with the switch set."""
    code = CHILD % dict(root=ROOT, name=name, twin=twin, one_row=one_row)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "RESULT ok" in out.stdout, out.stderr[-3000:]


@pytest.mark.parametrize("name", LANE)
def test_lane_kernel_rows_with_a_tile_that_does_not_divide_the_batch(name):
    """BF_MVDR_TILE = 5 over 12 / 14 / 16 frames: lanes of a wavefront sit in different tiles, the last tile is short."""
    assert CASES[name]["F"] % 5
    _child({"BF_MVDR_TILE": "5"}, name, "mvdr_fast_rows_kernel" + LANE_KERNEL[name], "mvdr_fast_kernel" + LANE_KERNEL[name])


@pytest.mark.parametrize("name,z", [("c16k3", "<4, 2, true>"), ("c9k1", "<4, 2, true>")])
def test_cov2d_kernel_rows(name, z):
    _torch()
    y, Y, kernels = run_case(name)
    check_case(name, y, Y, kernels, "cov2d_rows_kernel" + z, "cov2d_kernel" + z)


@pytest.mark.parametrize("name,k", [("g20k1", "mvdr_lcmv_kernel<32, 4>"), ("g8k5", "mvdr_lcmv_kernel<8, 8>")])
def test_group_kernel_rows(name, k):
    """The group kernel counts its rows at run time: the same kernel with one row and with R."""
    _torch()
    y, Y, kernels = run_case(name)
    check_case(name, y, Y, kernels, k, k)


def test_group_kernel_rows_under_the_switch():
    _child({"BF_MVDR_GROUP": "1"}, "l8k2", "mvdr_lcmv_kernel<8, 4>", "mvdr_lcmv_kernel<8, 4>")


def test_group_kernel_rows_two_microphones_three_columns():
    """K + 1 > M: the constraint Gram matrix is singular and the reference's inverse returns rounding noise or NaN (here it is
    non-finite on every frame but one) -- include/bfcore.h claims no parity there, so there is no oracle to judge the rows by.  What
    stands: the group kernel runs, out of band every row is zero, and row 0 is the R = 1 handle's output bit for bit."""
    _torch()
    name = "g2k2"
    y, Y, kernels = run_case(name)
    assert any("mvdr_lcmv_kernel<4, 4>" in k for k in kernels), kernels
    from lcmv_beams_cases import inband
    assert Y.shape[0] == 3 and not Y[:, :, ~inband(case_params(name))].any()
    y1, Y1, _ = run_one_row(name)
    assert np.array_equal(Y[0], Y1, equal_nan=True) and np.array_equal(y[0], y1, equal_nan=True)


def test_group_kernel_rows_two_microphones_under_the_switch():
    """Two microphones with one interferer on the group kernel: a two-microphone shape the oracle can judge."""
    _child({"BF_MVDR_GROUP": "1"}, "g2k1", "mvdr_lcmv_kernel<4, 4>", "mvdr_lcmv_kernel<4, 4>")


@pytest.mark.parametrize("name,twin", [("l8k0", "mvdr_fast_rows_kernel<8, 2, true>"), ("c12k0", "cov2d_rows_kernel<4, 2, true>"),
                                       ("g20k0", "mvdr_lcmv_kernel<32, 1>")])
def test_rows_without_an_interferer(name, twin):
    """K = 0 on a handle with two rows: the lane kernel and cov2d run their two- / four-column twin with an identity padding column (row
    0 then equals the one-row kernel's to rounding, not bit for bit: judged against the oracle), row 1 is exactly zero.  Then a
    structural bf_set_interference: row 1 starts, from the same history."""
    import oracle
    _torch()
    c, p = CASES[name], case_params(name)
    H, F, cut = c["hop"], c["F"], 6
    x = case_scene(name)
    bf = _bf(p, lcmv_out_beams=2)
    y0, Y0, kernels = run_dev(bf, x[:, :cut * H], cut)
    assert any(twin in k for k in kernels), kernels
    assert bf.set_interference(1, -60.0) == 1
    y1, Y1, _ = run_dev(bf, x[:, cut * H:], F - cut)
    bf.close()
    y, Y = np.concatenate([y0, y1], axis=1), np.concatenate([Y0, Y1], axis=1)
    nodes = [oracle.OracleNode(p), oracle.OracleNode(p)]
    refs = [n.process(x[:, :cut * H], want_spectrum=True) for n in nodes]
    for n in nodes:
        assert n.set_interference(1, -60.0) == 1
    nodes[1].set_theta(-60.0)                                   # row 1: columns 0 and 1 exchanged
    assert nodes[1].set_interference(1, THETA, threshold=0.0) == 1
    refs2 = [n.process(x[:, cut * H:], want_spectrum=True) for n in nodes]
    Y_ref = np.stack([np.concatenate([a[1], b[1]]) for a, b in zip(refs, refs2)])
    Y_ref[1, :cut] = 0
    from oracle import np_oracle
    y_ref = np.stack([np.concatenate([refs[0][0], refs2[0][0]]), np_oracle.istft_ola(p, Y_ref[1], p["out_amp"])])
    assert not Y[1, :cut].any() and not y[1, :cut * H].any() and Y[1, cut:].any()
    check_rows(p, y, Y, y_ref, Y_ref)


@pytest.mark.parametrize("name", ["h64", "h256", "h1024", "h2048", "h4096"])
def test_other_fft_sizes(name):
    _torch()
    N = 2 * CASES[name]["hop"]
    y, Y, kernels = run_case(name)
    check_case(name, y, Y, kernels, f"n{N}::mvdr_fast_rows_kernel<4, 2, true>", f"n{N}::mvdr_fast_kernel<4, 2, true>")


# ---- 2. formats ------------------------------------------------------------------------------------------------------------------------------
def _no_dump(name, rows=True, **kw):
    c = CASES[name]
    bf = _bf(case_params(name), **({"lcmv_out_beams": c["R"]} if rows else {}), **kw)
    y, _, kernels = run_dev(bf, case_scene(name), c["F"], dump=False)
    bf.close()
    return y, kernels


@pytest.mark.parametrize("name", ["l8k2", "c16k3", "g8k5", "l8k1r4"])
def test_band_limited_rows_without_the_dump(name):
    """Without the spectrum dump the rows in front of the backward transform are band-limited: judged on time, every row."""
    y, kernels = _no_dump(name)
    assert any("istft_w64_kernel<true>" in k for k in kernels) and not any("expand_spectrum" in k for k in kernels), kernels
    check_time(y, case_ref(name)[0], left_out=2 * 512)
    y1, k1 = _no_dump(name, rows=False)
    assert not any("_rows_kernel" in k for k in k1) and np.array_equal(y[0], y1[0], equal_nan=True)


@pytest.mark.parametrize("name,twin", [("l8k2", "mvdr_fast_rows_kernel<8, 3, false>"), ("c16k3", "cov2d_rows_kernel<4, 2, false>"),
                                       ("g8k5", "mvdr_lcmv_kernel<8, 8>")])
def test_mixed_precision_rows(name, twin):
    """BF_PRECISION_MIXED: z48 spectra, f32x2 band-limited rows, the fp32 backward transform; judged on time."""
    y, kernels = _no_dump(name, precision=BF_PRECISION_MIXED)
    assert any(twin in k for k in kernels) and any("istft32_kernel" in k for k in kernels), kernels
    check_time(y, case_ref(name)[0], left_out=2 * 512)


def test_interleaved_input():
    name = "l8k2"
    c = CASES[name]
    bf = _bf(case_params(name), layout=BF_INTERLEAVED, lcmv_out_beams=c["R"])
    y, Y, _ = run_dev(bf, case_scene(name).T, c["F"])
    bf.close()
    check_rows(case_params(name), y, Y, *case_ref(name))


def test_two_streams_two_directions():
    """Output stream (stream * n_dirs + dir) * R + r."""
    name, theta1 = "l8k2", -100.0
    c, p = CASES[name], case_params(name)
    R, F = c["R"], c["F"]
    bf = _bf(p, n_streams=2, n_dirs=2, lcmv_out_beams=R)
    bf.set_theta_dir(1, theta1)
    assert bf.n_out == 2 * 2 * R
    y, Y, _ = run_dev(bf, np.stack([case_scene(name), case_scene(name, 1)]), F)
    bf.close()
    for s in range(2):
        for d, th in enumerate((None, theta1)):
            o = (s * 2 + d) * R
            check_rows(case_params(name, theta=th), y[o:o + R], Y[o:o + R], *case_ref(name, s, th))


def test_closed_gates_put_the_scaled_reference_microphone_on_every_row():
    """The default scene has a silent stretch: behind a closed gate every row r < S is 0.01 X_0 (lcmv.cpp:121), as the swapped oracle has it."""
    _torch()
    name = "silent"
    y, Y, kernels = run_case(name)
    check_case(name, y, Y, kernels, "mvdr_fast_rows_kernel<8, 3, true>", "mvdr_fast_kernel<8, 3, true>")
    Y_ref = case_ref(name)[1]
    closed = (Y_ref[0, 1:] != 0) & (Y_ref[0, 1:] == Y_ref[1, 1:]) & (Y_ref[0, 1:] == Y_ref[2, 1:])   # (frame, bin) with the gate closed
    assert closed.sum() > 300, "the scene closes the gates of a whole frame at least"
    assert (Y[0, 1:][closed] == Y[1, 1:][closed]).all() and (Y[0, 1:][closed] == Y[2, 1:][closed]).all()


# ---- 3. stream semantics ------------------------------------------------------------------------------------------------------------------
def _sem_controls(bf, i):
    if i == 2:
        bf.set_theta(SEM["theta1"])
    if i == 3:
        assert bf.set_interference(2, SEM["new_interf"]) == 2


def _sem_pieces():
    cuts, x = SEM["cuts"], sem_scene()
    return [(b - a, np.ascontiguousarray(x[:, a * 512:b * 512])) for a, b in zip(cuts[:-1], cuts[1:])]


def test_stream_semantics_across_batches():
    """A batch cut, /theta in front of the third piece, a second interferer in front of the fourth: row 2 is zero before it and live
    after it, microphone 0's zeroed entries (quirk Q3) are on all columns, the tails of all rows carry across the cuts."""
    bf = _bf(sem_params(), lcmv_out_beams=SEM["R"])
    ys, Ys = [], []
    for i, (n, x) in enumerate(_sem_pieces()):
        _sem_controls(bf, i)
        y, Y, _ = run_dev(bf, x, n)
        ys.append(y)
        Ys.append(Y)
    w = bf.weights()
    bf.close()
    assert w.shape[2] == 3 and not w[:, 0, :].any()
    y, Y = np.concatenate(ys, axis=1), np.concatenate(Ys, axis=1)
    check_rows(sem_params(), y, Y, *sem_ref())
    t3 = SEM["cuts"][3]
    assert not Y[2, :t3].any() and Y[2, t3:].any() and not y[2, :t3 * 512].any() and y[2, t3 * 512:].any()


def test_stream_semantics_hop_by_hop():
    """bf_process_hop: out = [R][nframes] per callback."""
    bf = _bf(sem_params(), lcmv_out_beams=SEM["R"])
    x, cuts, out = sem_scene(), SEM["cuts"], []
    for t in range(SEM["F"]):
        if t in cuts[1:-1]:
            _sem_controls(bf, cuts.index(t))
        o = bf.process_hop(x[:, t * 512:(t + 1) * 512])
        assert o.shape == (SEM["R"], 512)
        out.append(o)
    bf.close()
    check_time(np.concatenate(out, axis=1), sem_ref()[0], left_out=2 * 512)


#: bf_state_size of a one-row lcmv handle with 4 microphones, one interferer, hop 512, past_windows 10, one stream -- the parent commit's
#: value (header 32 + control 656 + carried hop 8192 + one tail 2048 + the covariance history 10 * 2 * 1024 * 16)
STATE_BYTES_R1 = 338608


def test_checkpoint_with_rows():
    name = "l4k1"
    c, p, x = CASES[name], case_params(name), case_scene(name)
    R, h = c["R"], 7 * 512
    a = _bf(p, lcmv_out_beams=R)
    a.process(np.ascontiguousarray(x[:, :h]))
    blob = a.get_state()
    ya2 = a.process(np.ascontiguousarray(x[:, h:]))
    b = _bf(p, lcmv_out_beams=R)
    b.process(np.ascontiguousarray(x[:, :3 * 512]))  # scramble b's state first
    b.set_state(blob)
    yb2 = b.process(np.ascontiguousarray(x[:, h:]))
    assert ya2.shape == (R, x.shape[1] - h) and np.isfinite(ya2).all() and np.array_equal(ya2, yb2)
    check_time(ya2, case_ref(name)[0][:, h:])
    one = _bf(p)
    one.process(np.ascontiguousarray(x[:, :h]))
    blob1 = one.get_state()
    print(len(blob1), len(blob))
    assert len(blob1) == STATE_BYTES_R1 and len(blob) == STATE_BYTES_R1 + (R - 1) * 512 * 4
    three = _bf(p, lcmv_out_beams=R + 1)
    for hd, bl in ((b, blob1), (b, blob1 + bytes(len(blob) - len(blob1))), (one, blob), (three, blob)):
        with pytest.raises(BfError):
            hd.set_state(bl)
    one.set_state(blob1)
    for hd in (a, b, one, three):
        hd.close()


def test_stream_rms_counts_every_row():
    torch = _torch()
    name = "l8k2"
    c, p = CASES[name], case_params(name)
    n, F, R = 2, c["F"], c["R"]
    xs = np.stack([case_scene(name), case_scene(name, 1)])
    bf = _bf(p, n_streams=n, n_dirs=2, lcmv_out_beams=R)
    xd = torch.from_numpy(np.ascontiguousarray(xs)).cuda()
    yd = torch.empty((n * 2 * R, (F - 2) * 512), dtype=torch.float32, device="cuda")
    warm = xd[:, :, :2 * 512].contiguous()                # frame 0 of a cold start is NaN, and so are the two hops it is added to
    rest = xd[:, :, 2 * 512:].contiguous()
    bf.process_device(warm.data_ptr(), 2, yd.data_ptr())
    bf.process_device(rest.data_ptr(), F - 2, yd.data_ptr())
    rms = bf.stream_rms(yd.data_ptr(), F - 2)
    y = yd.cpu().numpy().astype(np.float64)
    bf.close()
    assert rms.shape == (n, 2, R)
    want = np.sqrt((y ** 2).mean(axis=1)).reshape(n, 2, R)
    assert np.isfinite(want).all() and np.allclose(rms, want, rtol=1e-12, atol=0) and (want > 0).all()


def test_shard_run_refuses_rows():
    from beamform_amd import capi, shard
    torch = _torch()
    name = "l4k1"
    bf = _bf(case_params(name), lcmv_out_beams=2)

    class CShard(C.Structure):
        _fields_ = [("lo", C.c_longlong), ("hi", C.c_longlong), ("warm", C.c_int), ("lead", C.c_int)]
    L = capi.load()
    L.bf_shard_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CShard), C.c_void_p, C.c_void_p]
    xd = torch.zeros((4, 4 * 512), dtype=torch.float32, device="cuda")
    yd = torch.zeros((2, 4 * 512), dtype=torch.float32, device="cuda")
    assert L.bf_shard_run(bf._h, xd.data_ptr(), C.byref(CShard(0, 4, 0, 0)), yd.data_ptr(), None) == -22
    with pytest.raises(ValueError):
        shard.run_shard(bf, xd.data_ptr(), shard.plan(4, 1, 0, 11), yd.data_ptr())
    bf.close()


# ---- 4. column tracks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,twin", [("t8k2", "mvdr_fast_track_rows_kernel<8, 3, true>"), ("t16k1", "mvdr_lcmv_track_kernel<16, 4>")])
def test_column_tracked_rows(name, twin):
    """Row r of a tracked frame looks at whatever angle column r of that frame's track names: columns 0 and 1 change at different
    frames inside the batch, one index is out of range (the column's own angle)."""
    c, p = CASES[name], case_params(name)
    track = case_track(name)
    assert track.shape == (c["F"], c["K"] + 1) and (track == 99).any()
    bf = _bf(p, lcmv_out_beams=c["R"])
    bf.set_ctrack_angles(TRACK_ANGLES)
    y, Y, kernels = run_dev(bf, case_scene(name), c["F"], track=track)
    bf.close()
    assert any(twin in k for k in kernels), kernels
    refs = [track_ref(name, r) for r in range(c["R"])]
    check_rows(p, y, Y, np.stack([a for a, _ in refs]), np.stack([b for _, b in refs]))
    one = _bf(p)
    one.set_ctrack_angles(TRACK_ANGLES)
    y1, Y1, k1 = run_dev(one, case_scene(name), c["F"], track=track)
    one.close()
    assert not any("_rows_kernel" in k for k in k1), k1
    assert np.array_equal(Y[0], Y1[0], equal_nan=True) and np.array_equal(y[0], y1[0], equal_nan=True)


# ---- 5. the loop ---------------------------------------------------------------------------------------------------------------------------------
def test_follow_sources_device_returns_a_row_per_beam():
    from beamform_amd import capi
    from beamform_amd.controllers import follow_sources_device
    from beamform_amd.params import make_params
    from beamform_amd.synth import make_scene
    _torch()
    M, W, F, K = 8, 8, 32, 2
    grid = np.arange(-180.0, 180.0, 2.0)
    x = make_scene(M, F, 512, 48000.0, seed=41, theta_s=20.0, interferers=(-60.0,), sigma_s=0.2, sigma_i=0.05, silent_frac=0.0)
    p = make_params("lcmv", n_mics=M, theta=0.0, interf=[120.0])
    doa = capi.Doa(make_params("das", n_mics=M), grid, 100.0, 16000.0, W)
    doa.set_method("capon")
    out = []
    for R in (1, 2):
        doa.reset()
        node = capi.Beamformer(p, **({"lcmv_out_beams": R} if R > 1 else {}))
        y, pub = follow_sources_device(node, doa, x, W, K, 30.0)
        node.close()
        out.append((y, pub))
    doa.reset()
    node = capi.Beamformer(p, lcmv_out_beams=2)
    from beamform_amd.controllers import DoaSources, follow_sources_tracked
    yt, pubt = follow_sources_tracked(node, doa, x, W, DoaSources(grid, K, 30.0))
    node.close()
    doa.reset()
    node = capi.Beamformer(p)
    yt1, _ = follow_sources_tracked(node, doa, x, W, DoaSources(grid, K, 30.0))
    node.close()
    assert yt.shape == (2, F * 512) and yt1.shape == (F * 512,) and pubt and np.array_equal(yt[0], yt1, equal_nan=True)
    assert yt[1][np.isfinite(yt[1])].any()
    (y1, pub1), (y2, pub2) = out
    assert y1.shape == (F * 512,) and y2.shape == (2, F * 512) and pub1 == pub2 and pub1
    assert np.array_equal(y2[0], y1, equal_nan=True)
    fin = np.isfinite(y2[1])
    assert (fin == np.isfinite(y1)).all() and y2[1][fin].any() and not np.array_equal(y2[1][fin], y1[fin])
