"""Steering tracks on the GPU (bf_track_*, include/bfcore.h): a look angle per frame inside one batch, against the oracle driven hop by
hop with set_theta in front of every frame whose angle changes (tests/track_ref.py); the kernels are asserted from a launch trace, so no
test can pass on another path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_ref  # noqa: E402

from beamform_amd.params import make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402
from conftest import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_SPECTRUM = 1e-5  # the project's own (tests/test_dirs_gpu.py): per-frame relative L2 on the complex spectrum
TOL_TIME = 1e-5
SR = 48000.0
BF_EINVAL, BF_ENOSYS = -22, -38


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _node(p, **kw):
    """Tracked tests name the das arithmetic themselves."""
    from beamform_amd import capi
    kw.setdefault("das_impl", capi.BF_DAS_F64)
    return capi.Beamformer(p, **kw)


def _dev_x(x, layout):
    """x [S, M, F*H] -> the device tensor in the handle's layout."""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if layout == 1 else x)).cuda()


def run_tracked(bf, x, track, layout=0, spectrum=True):
    """x [S, M, F*H], track [S, F] (None: an untracked batch) -> (y [S, F*H], Y [S, F, N] or None, kernels launched)."""
    from beamform_amd import capi
    torch = _torch()
    S, H = x.shape[0], bf.H
    F = x.shape[2] // H
    xd = _dev_x(x, layout)
    yd = torch.full((S, F * H), float("nan"), dtype=torch.float32, device="cuda")
    Yd = torch.full((S, F, 2 * H, 2), float("nan"), dtype=torch.float64, device="cuda") if spectrum else None
    with capi.launch_trace() as tr:
        if track is None:
            bf.process_device(xd.data_ptr(), F, yd.data_ptr(), Yd.data_ptr() if spectrum else 0)
        else:
            td = torch.from_numpy(np.ascontiguousarray(track, np.int32)).cuda()
            bf.process_device_tracked(xd.data_ptr(), F, yd.data_ptr(), td.data_ptr(), Yd.data_ptr() if spectrum else 0)
    torch.cuda.synchronize()
    Y = Yd.cpu().numpy().view(np.complex128)[..., 0] if spectrum else None
    return yd.cpu().numpy(), Y, tr.kernels


def check(y, Y, y_ref, Y_ref):
    """Per-frame relative L2 on the spectrum, relative L2 on the samples."""
    if Y is not None:
        assert np.isfinite(Y_ref).all() and np.isfinite(Y).all()
        worst = max(rel_l2(Y[t], Y_ref[t]) for t in range(len(Y_ref)))
        print(f"worst per-frame spectrum error {worst:.3e}")
        assert worst < TOL_SPECTRUM, worst
    assert np.isfinite(y).all()
    e = rel_l2(y, y_ref)
    print(f"time-domain error {e:.3e}")
    assert e < TOL_TIME, e


def busy_track(F, A, seed):
    """A new index at every frame; frame 0 and the last frame differ from their neighbours, 0 and A-1 appear, and so do -1 and a value
    >= A (both: the handle's theta)."""
    rng = np.random.default_rng(seed)
    vals = list(range(A)) + [-1, A + 2]
    t = [1, 0, A - 1, -1, A + 2]  # every special value, whatever the seed
    while len(t) < F:
        v = vals[int(rng.integers(len(vals)))]
        if v != t[-1]:
            t.append(v)
    t = np.array(t, np.int32)
    assert all(t[i] != t[i + 1] for i in range(F - 1))
    return t


def _names(kernels, what):
    return [k for k in kernels if what in k]


# ---- 5. das tracked against the oracle ---------------------------------------------------------------------------------------------
DAS_ANGLES = [-90.0, -30.0, 0.0, 20.0, 75.0]
DAS_CASES = [  # M, F, hop, S, layout, the per-bin kernel the trace must name
    (8, 24, 512, 1, 0, "stft_bins_w64_track_kernel<0, 8, 0>"),
    (3, 21, 512, 2, 1, "stft_bins_w64_track_kernel<1, 4, 0>"),
    (16, 18, 512, 1, 0, "pointwise_track_kernel<16, 0>"),
    (4, 40, 64, 1, 0, "pointwise_track_kernel<4, 0>"),
]


@pytest.mark.parametrize("M,F,hop,S,layout,kernel", DAS_CASES)
def test_das_tracked_against_the_oracle(M, F, hop, S, layout, kernel):
    p = make_params("das", n_mics=M, hop=hop, theta=45.0)
    x = np.stack([make_scene(M, F, hop, SR, seed=4100 + 10 * M + s) for s in range(S)])
    track = np.stack([busy_track(F, len(DAS_ANGLES), 7 + s) for s in range(S)])
    assert S == 1 or not np.array_equal(track[0], track[1])
    bf = _node(p, n_streams=S, layout=layout)
    bf.set_track_angles(DAS_ANGLES)
    y, Y, kernels = run_tracked(bf, x, track, layout)
    bf.close()
    assert _names(kernels, kernel), kernels
    if "stft_bins" in kernel:
        assert _names(kernels, "fused_tail_track_kernel") and not _names(kernels, "pointwise"), kernels
    assert not _names(kernels, "das_f64_") and not _names(kernels, "pointwise_bins_kernel") and not _names(kernels, "stft_bins_w64_kernel"), kernels
    for s in range(S):
        y_ref, Y_ref = track_ref.oracle_tracked(p, x[s], DAS_ANGLES, track[s], 45.0)
        check(y[s], Y[s], y_ref, Y_ref)


def test_das_tracked_mixed_precision():
    """BF_PRECISION_MIXED: float rows into the fp32 backward transform (no spectrum dump: the dump keeps the rows in double)."""
    from beamform_amd import capi
    M, F = 8, 24
    p = make_params("das", n_mics=M, theta=45.0)
    x = make_scene(M, F, seed=4180)[None]
    track = busy_track(F, len(DAS_ANGLES), 7)[None]
    bf = _node(p, precision=capi.BF_PRECISION_MIXED)
    bf.set_track_angles(DAS_ANGLES)
    y, _, kernels = run_tracked(bf, x, track, spectrum=False)
    bf.close()
    assert _names(kernels, "stft_bins_w64_track_kernel<0, 8, 0>") and _names(kernels, "istft32_kernel"), kernels
    y_ref, _ = track_ref.oracle_tracked(p, x[0], DAS_ANGLES, track[0], 45.0)
    check(y[0], None, y_ref, None)


# ---- 6. phase and phasempf ---------------------------------------------------------------------------------------------------------
DIR_ANGLES = [20.0, -35.0, 110.0]  # the angles (and the scene) at which test_bin_pipeline_look_directions holds per frame


def test_phase_tracked_a_new_angle_every_frame():
    M, F = 8, 24
    p = make_params("phase", n_mics=M)
    x = make_scene(M, F, seed=1108)[None]
    track = busy_track(F, len(DIR_ANGLES), 11)[None]
    bf = _node(p)
    bf.set_track_angles(DIR_ANGLES)
    y, Y, kernels = run_tracked(bf, x, track)
    bf.close()
    assert _names(kernels, "stft_bins_w64_track_kernel<0, 8, 4>") and _names(kernels, "fused_tail_track_kernel<8, 4>"), kernels
    y_ref, Y_ref = track_ref.oracle_tracked(p, x[0], DIR_ANGLES, track[0], p["theta"])
    check(y[0], Y[0], y_ref, Y_ref)


@pytest.mark.parametrize("M,layout,kernel", [(8, 0, "stft_bins_w64_track_kernel<0, 8, 5>"), (8, 1, "stft_bins_w64_track_kernel<1, 8, 5>"),
                                             (16, 0, "mpf_mask_track_kernel<16>")])
def test_phasempf_tracked_recursion_carries_across_angle_changes(M, layout, kernel):
    """A new angle every 7 frames; the MCRA / MPF recursion and the smoother run through the changes.  M = 8 takes the fused front -- on
    [sample][mic] input the one tracked kernel whose code differs from its twin's (the double-precision redo of the phase decision in two
    halves) -- and M = 16 the unfused chain (mpf_mask_track_kernel)."""
    F = 60
    p = make_params("phasempf", n_mics=M)
    x = make_scene(M, F, seed=1108)[None]
    track = np.repeat(np.array([0, 2, 1, -1, 2, 0, 1, 2, 0], np.int32), 7)[:F][None]
    bf = _node(p, layout=layout)
    bf.set_track_angles(DIR_ANGLES)
    y, Y, kernels = run_tracked(bf, x, track, layout)
    bf.close()
    assert _names(kernels, kernel), kernels
    if M == 8:
        assert _names(kernels, "fused_tail_track_kernel<8, 5>") and not _names(kernels, "mpf_mask"), kernels
    else:
        assert not _names(kernels, "mpf_mask_kernel") and not _names(kernels, "stft_bins"), kernels
    assert _names(kernels, "mpf_rec"), kernels
    y_ref, Y_ref = track_ref.oracle_tracked(p, x[0], DIR_ANGLES, track[0], p["theta"])
    check(y[0], Y[0], y_ref, Y_ref)


# ---- 7. against the look-direction batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["das", "phase"])
def test_tracked_frames_equal_the_look_direction_batch(algo):
    """Frame t of the tracked spectrum against frame t of direction track[t] of an n_dirs = 3 batch on the same input: the same per-bin
    device functions on the spectra of the same samples.  Bit for bit when the two batches share their forward transform; the tracked
    batch of this shape runs the fused front (64-lane transform), the look-direction batch the separate STFT (32 x 32 transform), whose
    roundings differ at 1e-16 of a frame's scale: then 1e-13 relative per frame, four orders above double rounding -- an indexing error
    gives O(1)."""
    M, F = 8, 16
    p = make_params(algo, n_mics=M)
    x = make_scene(M, F, seed=1108)[None]
    track = busy_track(F, 3, 5)[None] % 3  # every index names a table
    bf = _node(p)
    bf.set_track_angles(DIR_ANGLES)
    _, Y, _ = run_tracked(bf, x, track)
    bf.close()
    bd = _node(p, n_dirs=3)
    bd.set_thetas(DIR_ANGLES)
    torch = _torch()
    xd = _dev_x(x, 0)
    yd = torch.empty((3, F * 512), dtype=torch.float32, device="cuda")
    Yd = torch.empty((3, F, 1024, 2), dtype=torch.float64, device="cuda")
    bd.process_device(xd.data_ptr(), F, yd.data_ptr(), Yd.data_ptr())
    torch.cuda.synchronize()
    bd.close()
    Yd = Yd.cpu().numpy().view(np.complex128)[..., 0]
    want = np.stack([Yd[track[0, t], t] for t in range(F)])
    if Y[0].tobytes() == want.tobytes():
        print("tracked spectrum equals the look-direction batch bit for bit")
        return
    worst = max(rel_l2(Y[0, t], want[t]) for t in range(F))
    print(f"tracked vs look-direction batch: worst per-frame relative L2 {worst:.3e}")
    assert worst <= 1e-13, worst


# ---- 8. carry and alternation --------------------------------------------------------------------------------------------------------
def test_one_call_against_two():
    """F = 24 as one tracked call and as 10 + 14: history hop and overlap-add tail carry; the float output agrees to 1e-6 of its scale
    (the header's rule for a stream cut differently)."""
    M, F = 8, 24
    p = make_params("das", n_mics=M, theta=45.0)
    x = make_scene(M, F, seed=4200)[None]
    track = busy_track(F, len(DAS_ANGLES), 3)[None]
    bf = _node(p)
    bf.set_track_angles(DAS_ANGLES)
    y1, _, _ = run_tracked(bf, x, track, spectrum=False)
    bf.reset()
    ya, _, _ = run_tracked(bf, x[:, :, :10 * 512], track[:, :10], spectrum=False)
    yb, _, _ = run_tracked(bf, x[:, :, 10 * 512:], track[:, 10:], spectrum=False)
    bf.close()
    y2 = np.concatenate([ya, yb], axis=1)
    d = float(np.abs(y1 - y2).max()) / float(np.abs(y1).max())
    print(f"one call vs 10 + 14: max difference / scale {d:.3e}")
    assert d <= 1e-6, d


@pytest.mark.parametrize("algo", ["das", "phasempf"])
def test_tracked_then_untracked_on_one_handle(algo):
    M, F = 8, 24
    p = make_params(algo, n_mics=M, theta=45.0)
    x = make_scene(M, F, seed=4300)[None]
    angles = DAS_ANGLES
    track = busy_track(12, len(angles), 9)
    bf = _node(p)
    bf.set_track_angles(angles)
    ya, Ya, ka = run_tracked(bf, x[:, :, :12 * 512], track[None])
    yb, Yb, kb = run_tracked(bf, x[:, :, 12 * 512:], None)
    bf.close()
    assert _names(ka, "_track_kernel") and not _names(kb, "_track_kernel"), (ka, kb)
    full = np.concatenate([track, np.full(12, -1, np.int32)])  # the second half: the angle held at the handle's theta
    y_ref, Y_ref = track_ref.oracle_tracked(p, x[0], angles, full, 45.0)
    check(np.concatenate([ya[0], yb[0]]), np.concatenate([Ya[0], Yb[0]]), y_ref, Y_ref)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from beamform_amd import capi
    torch = _torch()
    M, F = 4, 4
    x = torch.zeros((M, F * 512), dtype=torch.float32, device="cuda")
    y = torch.zeros((2, F * 512), dtype=torch.float32, device="cuda")
    trk = torch.zeros((F,), dtype=torch.int32, device="cuda")

    def code(fn, *a):
        with pytest.raises(capi.BfError) as e:
            fn(*a)
        return e.value.code

    bf = _node(make_params("das", n_mics=M))
    assert code(bf.process_device_tracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr()) == BF_EINVAL  # no angles installed
    assert code(bf.set_track_angles, np.zeros(1025)) == BF_EINVAL
    assert code(bf.set_track_angles, [0.0, float("nan")]) == BF_EINVAL
    assert code(bf.process_device_tracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr()) == BF_EINVAL  # still none
    bf.set_track_angles([10.0, 20.0])
    assert code(bf.process_device_tracked, x.data_ptr(), F, y.data_ptr(), 0) == BF_EINVAL               # null track
    bf.process_device_tracked(x.data_ptr(), F, y.data_ptr(), trk.data_ptr())
    bf.set_track_angles([])                                                                              # dropped again
    assert code(bf.process_device_tracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr()) == BF_EINVAL
    torch.cuda.synchronize()
    bf.close()
    bf = _node(make_params("das", n_mics=M), n_dirs=2)
    assert code(bf.process_device_tracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr()) == BF_EINVAL  # look-direction batch
    bf.close()
    for p, kw in ((make_params("mvdr", n_mics=M), {}), (make_params("gss", n_mics=M), {}),
                  (make_params("das", n_mics=M), dict(das_impl=capi.BF_DAS_FUSED_F32))):
        bf = _node(p, **kw)
        assert code(bf.set_track_angles, [10.0, 20.0]) == BF_ENOSYS, p["algo"]
        assert code(bf.process_device_tracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr()) == BF_ENOSYS, p["algo"]
        bf.close()


# ---- 10. the builder -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency", [0, 1, 2])
@pytest.mark.parametrize("with_map", [False, True])
def test_builder_equals_its_restatement(latency, with_map):
    from beamform_amd import capi
    torch = _torch()
    S, nb, W, A = 3, 9, 4, 5
    rng = np.random.default_rng(100 + latency)
    maps = rng.random((S, nb, A))
    peaks = np.argmax(maps, axis=2).astype(np.int32)
    min_peak = float(np.median(np.take_along_axis(maps, peaks[..., None].astype(np.int64), axis=2))) if with_map else 0.0
    md = torch.from_numpy(maps).cuda()
    for c0 in (-1, 3):
        for cut in (None, 4):
            parts = [(0, nb)] if cut is None else [(0, cut), (cut, nb)]
            carry = torch.full((S,), c0, dtype=torch.int32, device="cuda")
            c_ref = np.full(S, c0, np.int32)
            with capi.launch_trace() as tr:
                for a, b in parts:
                    pk = torch.from_numpy(np.ascontiguousarray(peaks[:, a:b])).cuda()
                    mp = md[:, a:b].contiguous()
                    trk = torch.full((S, (b - a) * W), -77, dtype=torch.int32, device="cuda")
                    capi.track_from_peaks_device(pk.data_ptr(), mp.data_ptr() if with_map else 0, A, S, b - a, W, latency, min_peak,
                                                 carry.data_ptr(), trk.data_ptr())
                    torch.cuda.synchronize()
                    t_ref, c_ref = track_ref.from_peaks(peaks[:, a:b], maps[:, a:b] if with_map else None, W, latency, min_peak, c_ref)
                    assert np.array_equal(trk.cpu().numpy(), t_ref), (c0, cut, a, b)
                    assert np.array_equal(carry.cpu().numpy(), c_ref), (c0, cut, a, b)
            assert tr.kernels == ["bf::track_from_peaks_kernel"] * len(parts), tr.kernels


def test_builder_walks_more_than_one_round_of_blocks():
    """One wavefront walks 64 blocks per round: 150 blocks, publications sparse enough that a round inherits from the one before."""
    from beamform_amd import capi
    torch = _torch()
    S, nb, W, A = 2, 150, 3, 7
    rng = np.random.default_rng(5)
    maps = rng.random((S, nb, A))
    peaks = np.argmax(maps, axis=2).astype(np.int32)
    min_peak = 0.995  # the maximum of 7 uniforms clears it in about 3 % of the blocks
    pk, md = torch.from_numpy(peaks).cuda(), torch.from_numpy(maps).cuda()  # named: they must outlive the launches that read them
    for latency in (0, 1, 70):
        carry = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        trk = torch.full((S, nb * W), -77, dtype=torch.int32, device="cuda")
        capi.track_from_peaks_device(pk.data_ptr(), md.data_ptr(), A, S, nb, W, latency, min_peak, carry.data_ptr(), trk.data_ptr())
        torch.cuda.synchronize()
        t_ref, c_ref = track_ref.from_peaks(peaks, maps, W, latency, min_peak, -1)
        assert 0 < (t_ref >= 0).sum() < t_ref.size
        assert np.array_equal(trk.cpu().numpy(), t_ref) and np.array_equal(carry.cpu().numpy(), c_ref), latency


# ---- 11. the closed loop ---------------------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_device():
    """The scene of test_doa_gpu's follow_doa test.  follow_doa_device publishes what follow_doa publishes (the maps do not depend on
    how the stream is cut), its output is the oracle's with those angles in force, and it is three enqueues: one DOA batch, one
    track_from_peaks_kernel, one tracked batch."""
    from beamform_amd import capi
    from beamform_amd.controllers import DoaTheta, follow_doa, follow_doa_device
    _torch()
    GRID = np.arange(-180.0, 180.0)
    W, M = 16, 8
    a = make_scene(M, 64, 512, SR, seed=21, theta_s=20.0, interferers=(), silent_frac=0.0)
    b = make_scene(M, 64, 512, SR, seed=22, theta_s=-60.0, interferers=(), silent_frac=0.0)
    x = np.concatenate([a, b], axis=1)
    p = make_params("das", n_mics=M, theta=0.0)
    node, doa = _node(p), capi.Doa(p, GRID, 100.0, 16000.0, W)
    _, pub_host = follow_doa(node, doa, x, W, DoaTheta(GRID))
    node.close()
    doa.close()
    node, doa = _node(p), capi.Doa(p, GRID, 100.0, 16000.0, W)
    with capi.launch_trace() as tr:
        y, published = follow_doa_device(node, doa, x, W)
    node.close()
    doa.close()
    assert published == pub_host and len(published) == 128 // W
    k = tr.kernels
    assert len(_names(k, "doa_map_kernel")) == 1 and len(_names(k, "doa_reduce_kernel")) == 1, k
    assert len(_names(k, "track_from_peaks_kernel")) == 1, k
    assert len(_names(k, "stft_bins_w64_track_kernel")) == 1 and len(_names(k, "fused_tail_track_kernel")) == 1, k
    assert len(_names(k, "istft")) == 1 and not _names(k, "das_f64_"), k
    i_doa, i_trk, i_bf = k.index(_names(k, "doa_reduce_kernel")[0]), k.index("bf::track_from_peaks_kernel"), k.index(_names(k, "stft_bins_w64_track_kernel")[0])
    assert i_doa < i_trk < i_bf, k
    # the oracle with the published angles in force one block later
    idx = {float(g): i for i, g in enumerate(GRID)}
    peaks = np.array([[idx[t] for _, t in published]], np.int32)
    track, _ = track_ref.from_peaks(peaks, None, W, 1, 0.0, -1)
    y_ref, _ = track_ref.oracle_tracked(p, x, GRID, track[0], 0.0)
    check(y, None, y_ref, None)
