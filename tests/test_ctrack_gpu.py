"""Column tracks on the GPU (bf_ctrack_*, include/bfcore.h): mvdr and lcmv with an angle per frame and per constraint column inside one
batch, against the oracle driven hop by hop with set_theta / set_interference in front of every frame whose angles change
(tests/ctrack_ref.py).  Comparison as tests/test_pipeline_gpu.py::check: equal finite masks, per-frame relative L2 on the spectrum and
relative L2 on the finite samples, both at the project's 1e-5.  The kernels are asserted from a launch trace, so no test can pass on
another path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrack_cases as cc  # noqa: E402
import ctrack_ref  # noqa: E402

from beamform_amd.params import make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF_EINVAL, BF_ENOSYS = -22, -38
REF, MIXED = 0, 1  # bf_precision


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _node(p, **kw):
    from beamform_amd import capi
    return capi.Beamformer(p, **kw)


def _z128(precision):
    return "false" if precision == MIXED else "true"


def _run_case(algo, M, K, F, n_cols, precision, dump, kernel, hop=512, layout=0):
    _torch()
    p, x, angles = cc.case(algo, M, K, F, hop)
    track = cc.mvdr_track(F, 7) if algo == "mvdr" else cc.lcmv_track(F, n_cols, 7)
    bf = _node(p, precision=precision, layout=layout)
    bf.set_ctrack_angles(angles)
    y, Y, kernels = cc.run_ctracked(bf, x[None], track[None], layout, spectrum=dump)
    bf.close()
    assert cc.names(kernels, kernel), kernels
    assert not cc.names(kernels, "mvdr_fast_kernel") and not cc.names(kernels, "mvdr_lcmv_kernel") and not cc.names(kernels, "cov2d"), kernels
    y_ref, Y_ref = cc.oracle_for((algo, M, K, F, n_cols, hop), p, x, angles, track)
    cc.check(y[0], Y[0] if dump else None, y_ref, Y_ref)


# ---- 1. mvdr: a new look angle at every frame ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dump", [True, False], ids=["dump", "nodump"])
@pytest.mark.parametrize("precision", [REF, MIXED], ids=["ref", "mixed"])
@pytest.mark.parametrize("M,F,mp", [(8, 48, 8), (3, 30, 4), (5, 24, 6)])
def test_mvdr_a_new_angle_every_frame(M, F, mp, precision, dump):
    _run_case("mvdr", M, 0, F, 1, precision, dump, f"mvdr_fast_track_kernel<{mp}, 1, {_z128(precision)}>")


# ---- 2. lcmv: every column changes at every frame ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [REF, MIXED], ids=["ref", "mixed"])
@pytest.mark.parametrize("M,K,n_cols,F,mp,kc", [(8, 2, 3, 40, 8, 3), (4, 3, 4, 20, 4, 4), (6, 1, 2, 30, 6, 2), (8, 3, 1, 40, 8, 4)])
def test_lcmv_every_column_changes_every_frame(M, K, n_cols, F, mp, kc, precision):
    _run_case("lcmv", M, K, F, n_cols, precision, True, f"mvdr_fast_track_kernel<{mp}, {kc}, {_z128(precision)}>")


# ---- 3. the group twin, and the routing past cov2d ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,M,K,F,kernel", [("mvdr", 16, 0, 26, "mvdr_lcmv_track_kernel<16, 1>"), ("lcmv", 16, 3, 26, "mvdr_lcmv_track_kernel<16, 4>"),
                                               ("lcmv", 12, 2, 24, "mvdr_lcmv_track_kernel<16, 4>")])
def test_nine_to_sixteen_microphones_run_the_group_twin(algo, M, K, F, kernel):
    _run_case(algo, M, K, F, K + 1, REF, True, kernel)


# ---- 4. the switches, each in a child process ---------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np, torch
import ctrack_cases as cc, ctrack_ref
from beamform_amd.capi import Beamformer
algo, M, K, F = %(algo)r, %(M)d, %(K)d, %(F)d
p, x, angles = cc.case(algo, M, K, F)
track = cc.mvdr_track(F, 7) if algo == "mvdr" else cc.lcmv_track(F, K + 1, 7)
bf = Beamformer(p)
bf.set_ctrack_angles(angles)
y, Y, kernels = cc.run_ctracked(bf, x[None], track[None])
bf.close()
y_ref, Y_ref, _ = ctrack_ref.oracle_ctracked(p, x, angles, track, cc.THETA0)
res = cc.errors(y[0], Y[0], y_ref, Y_ref)
res["kernels"] = kernels
print("RESULT " + json.dumps(res))
"""


@pytest.mark.parametrize("env,algo,M,K,F,kernel", [
    ({"BF_MVDR_TILE": "7"}, "mvdr", 8, 0, 40, "mvdr_fast_track_kernel<8, 1, true>"),   # lanes straddle tiles, a short last tile: where a wrong
    ({"BF_MVDR_TILE": "7"}, "lcmv", 8, 2, 40, "mvdr_fast_track_kernel<8, 3, true>"),   # per-lane frame index shows
    ({"BF_MVDR_GROUP": "1"}, "mvdr", 8, 0, 30, "mvdr_lcmv_track_kernel<8, 1>"),
    ({"BF_MVDR_GROUP": "1"}, "lcmv", 8, 2, 30, "mvdr_lcmv_track_kernel<8, 4>"),
], ids=["tile7-mvdr8", "tile7-lcmv8-k2", "group-mvdr8", "group-lcmv8-k2"])
def test_switches_act_on_tracked_batches(env, algo, M, K, F, kernel):
    code = CHILD % dict(root=ROOT, algo=algo, M=M, K=K, F=F)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(res)
    assert cc.names(res["kernels"], kernel), res["kernels"]
    assert res["finite_mask_equal"] and res["finite_frames_equal"], res
    assert res["time"] < cc.TOL_TIME and res["spectrum"] < cc.TOL_SPECTRUM, res


# ---- 5. beside the tuned shape -------------------------------------------------------------------------------------------------------------
def test_two_streams_with_different_tracks():
    _torch()
    M, K, F, S = 8, 2, 24, 2
    p, _, angles = cc.case("lcmv", M, K, F)
    x = np.stack([make_scene(M, F, 512, cc.SR, seed=5400 + s) for s in range(S)])
    track = np.stack([cc.lcmv_track(F, K + 1, 11 + 5 * s) for s in range(S)])
    assert not np.array_equal(track[0], track[1])
    bf = _node(p, n_streams=S)
    bf.set_ctrack_angles(angles)
    y, Y, kernels = cc.run_ctracked(bf, x, track)
    bf.close()
    assert cc.names(kernels, "mvdr_fast_track_kernel<8, 3, true>"), kernels
    for s in range(S):
        y_ref, Y_ref, _ = ctrack_ref.oracle_ctracked(p, x[s], angles, track[s], cc.THETA0)
        cc.check(y[s], Y[s], y_ref, Y_ref)


def test_sample_major_layout():
    _run_case("lcmv", 6, 1, 30, 2, REF, True, "mvdr_fast_track_kernel<6, 2, true>", layout=1)


@pytest.mark.parametrize("hop,F", [(128, 40), (2048, 14)])
def test_other_periods(hop, F):
    _run_case("mvdr", 4, 0, F, 1, REF, True, f"n{2 * hop}::mvdr_fast_track_kernel<4, 1, true>", hop=hop)


# ---- 6. carry and alternation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,M,K", [("mvdr", 5, 0), ("lcmv", 8, 2)])
def test_one_call_against_three_with_an_untracked_call_between(algo, M, K):
    """F frames as one tracked call and as (0, 5) tracked, (5, 6) untracked, (6, F) tracked: the history hop, the covariance history of
    the previous 10 frames (cut in the middle of its window, twice) and the overlap-add tail carry.  The untracked frame is the
    handle's own angles, which the one call says with -1."""
    _torch()
    F = 24
    p, x, angles = cc.case(algo, M, K, F)
    track = cc.mvdr_track(F, 3) if algo == "mvdr" else cc.lcmv_track(F, K + 1, 3)
    track[5] = -1
    bf = _node(p)
    bf.set_ctrack_angles(angles)
    y1, Y1, _ = cc.run_ctracked(bf, x[None], track[None])
    bf.reset()
    ys, Ys, ks = [], [], []
    for a, b, tracked in ((0, 5, True), (5, 6, False), (6, F, True)):
        y, Y, k = cc.run_ctracked(bf, x[None, :, a * 512:b * 512], track[None, a:b] if tracked else None)
        ys.append(y[0]); Ys.append(Y[0]); ks.append(k)
    bf.close()
    assert cc.names(ks[0], "_track_kernel") and not cc.names(ks[1], "_track_kernel") and cc.names(ks[2], "_track_kernel"), ks
    y_ref, Y_ref = cc.oracle_for((algo, M, K, F, "cuts"), p, x, angles, track)
    cc.check(y1[0], Y1[0], y_ref, Y_ref)
    cc.check(np.concatenate(ys), np.concatenate(Ys), y_ref, Y_ref)


# ---- 7. quirk Q3: a structural interferer change behind the install ------------------------------------------------------------------------
def test_structural_change_after_the_install_leaves_no_stale_rows():
    """lcmv with one interferer: install the angles (microphone 0's weight is 1 everywhere), append a second interferer -- the tables come
    back zeroed and row 0 is not rewritten (lcmv.cpp:50-56, 243-252) -- then a tracked batch over all three columns.  The oracle does
    the same; a table that kept the install-time row 0 would weight microphone 0 with 1 where the reference has 0."""
    _torch()
    M, F = 8, 24
    p, x, angles = cc.case("lcmv", M, 1, F)
    track = cc.lcmv_track(F, 3, 13)
    bf = _node(p)
    bf.set_ctrack_angles(angles)
    assert bf.set_interference(2, cc.OWN[2]) == 2
    assert np.all(bf.weights()[:, 0, :] == 0)
    y, Y, kernels = cc.run_ctracked(bf, x[None], track[None])
    bf.close()
    assert cc.names(kernels, "mvdr_fast_track_kernel<8, 3, true>"), kernels

    def append(node):
        assert node.set_interference(2, cc.OWN[2], threshold=1.0) == 2
        return cc.OWN[:3]
    y_ref, Y_ref, node = ctrack_ref.oracle_ctracked(p, x, angles, track, cc.THETA0, prepare=append)
    assert np.all(node.weights()[:, 0, :] == 0)
    cc.check(y[0], Y[0], y_ref, Y_ref)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from beamform_amd import capi
    torch = _torch()
    M, F = 4, 4
    x = torch.zeros((M, F * 512), dtype=torch.float32, device="cuda")
    y = torch.zeros((2, F * 512), dtype=torch.float32, device="cuda")
    trk = torch.full((F * 4,), -1, dtype=torch.int32, device="cuda")

    def code(fn, *a):
        with pytest.raises(capi.BfError) as e:
            fn(*a)
        return e.value.code

    # any other algorithm
    for p, kw in ((make_params("das", n_mics=M), {}), (make_params("gss", n_mics=M), {}), (make_params("phase", n_mics=M), {}),
                  (make_params("das", n_mics=M), dict(das_impl=capi.BF_DAS_FUSED_F32))):
        bf = _node(p, **kw)
        assert code(bf.set_ctrack_angles, [10.0, 20.0]) == BF_ENOSYS, p["algo"]
        assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 1) == BF_ENOSYS, p["algo"]
        bf.close()
    bf = _node(make_params("mvdr", n_mics=M))
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 1) == BF_EINVAL   # no angles installed
    assert code(bf.set_ctrack_angles, np.zeros(1025)) == BF_EINVAL
    assert code(bf.set_ctrack_angles, [0.0, float("nan")]) == BF_EINVAL
    assert code(bf.set_ctrack_angles, [0.0, float("inf")]) == BF_EINVAL
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 1) == BF_EINVAL   # still none
    bf.set_ctrack_angles([10.0, 20.0])
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), 0, 1) == BF_EINVAL                # null track
    assert code(bf.process_device_ctracked, 0, F, y.data_ptr(), trk.data_ptr(), 1) == BF_EINVAL              # null x
    assert code(bf.process_device_ctracked, x.data_ptr(), F, 0, trk.data_ptr(), 1) == BF_EINVAL              # null y
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 0) == BF_EINVAL   # n_cols < 1
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 2) == BF_EINVAL   # mvdr: one column
    bf.process_device_ctracked(x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 1)
    assert code(bf.set_track_angles, [10.0, 20.0]) == BF_ENOSYS                                              # bf_track_* keeps refusing
    assert code(bf.process_device_tracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr()) == BF_ENOSYS
    bf.set_ctrack_angles([])                                                                                 # dropped again
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 1) == BF_EINVAL
    torch.cuda.synchronize()
    bf.close()
    bf = _node(make_params("lcmv", n_mics=M, interf=[-75.0, 105.0]))
    bf.set_ctrack_angles([10.0, 20.0])
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 4) == BF_EINVAL   # above the column count
    bf.process_device_ctracked(x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 3)
    assert bf.set_interference(3, -170.0) == 3                                                               # the count at the time of the call
    bf.process_device_ctracked(x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 4)
    torch.cuda.synchronize()
    bf.close()
    bf = _node(make_params("mvdr", n_mics=M), n_dirs=2)                                                      # look-direction batch
    assert code(bf.set_ctrack_angles, [10.0, 20.0]) == BF_EINVAL
    assert code(bf.process_device_ctracked, x.data_ptr(), F, y.data_ptr(), trk.data_ptr(), 1) == BF_EINVAL
    bf.close()
    bf = _node(make_params("mvdr", n_mics=16, hop=4096))                                                     # 2 MiB per table
    assert code(bf.set_ctrack_angles, np.linspace(-90.0, 90.0, 300)) == BF_EINVAL                            # above 512 MiB
    bf.close()


# ---- 9. the closed loop ----------------------------------------------------------------------------------------------------------------------
def test_closed_loop_in_one_tracked_batch():
    """Two sources (20 degrees at 0.2, -60 degrees at 0.05), a Capon map per block of 8 frames, lcmv with one interferer: one DOA
    batch, one column-tracked batch.  The output is the oracle's with the track sources_track built in force."""
    from beamform_amd import capi
    from beamform_amd.controllers import DoaSources, follow_sources_tracked, sources_track
    torch = _torch()
    GRID2 = np.arange(-180.0, 180.0, 2.0)
    M, W, F = 8, 8, 64
    x = make_scene(M, F, 512, cc.SR, seed=41, theta_s=20.0, interferers=(-60.0,), sigma_s=0.2, sigma_i=0.05, silent_frac=0.0)
    p = make_params("lcmv", n_mics=M, theta=0.0, interf=[120.0])
    node = _node(p)
    doa = capi.Doa(make_params("das", n_mics=M), GRID2, 100.0, 16000.0, W)
    doa.set_method("capon")
    with capi.launch_trace() as tr:
        y, published = follow_sources_tracked(node, doa, x, W, DoaSources(GRID2, 2, 30.0))
    k = tr.kernels
    assert len(cc.names(k, "mvdr_fast_track_kernel<8, 2, true>")) == 1 and len(cc.names(k, "istft")) == 1, k
    assert not cc.names(k, "mvdr_fast_kernel"), k
    assert len(published) == F // W and all(len(i) == 1 for _, _, i in published)
    # the node is left at the last publication
    w = node.weights()
    node.close()
    # the maps again, for the track the batch ran with (they do not depend on how the stream is cut)
    xd = torch.from_numpy(x).cuda()
    maps = torch.empty((F // W, GRID2.size), dtype=torch.float64, device="cuda")
    doa.reset()
    doa.process_device(xd.data_ptr(), F, maps.data_ptr(), 0)
    torch.cuda.synchronize()
    doa.close()
    track, pub2 = sources_track(maps.cpu().numpy(), DoaSources(GRID2, 2, 30.0), W, 2)
    assert pub2 == published
    assert (track[:W] == -1).all() and (track[W:] >= 0).all()
    for t in range(F):  # the columns of one frame stay apart
        a = ctrack_ref.angles_in_force(GRID2, track[t:t + 1], [0.0, 120.0])[0]
        assert abs((a[0] - a[1] + 180.0) % 360.0 - 180.0) >= 20.0, (t, a)
    y_ref, _, ref_node = ctrack_ref.oracle_ctracked(p, x, GRID2, track, 0.0)
    cc.check(y, None, y_ref, None)
    ref_node.set_theta(published[-1][1])
    ref_node.set_interference(1, published[-1][2][0], threshold=0.0)
    assert np.abs(w - ref_node.weights()).max() < 1e-9
