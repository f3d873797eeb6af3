"""Shared by tests/test_ctrack_gpu.py and its child processes (the environment switches are read once per process): the candidate
angles, the busy tracks, one column-tracked batch on the GPU with its launch trace, and the comparison with the oracle.  Test
infrastructure only."""
import numpy as np

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene
from conftest import rel_l2

import ctrack_ref

TOL_SPECTRUM = 1e-5  # the project's own (tests/test_pipeline_gpu.py): per-frame relative L2 on the complex spectrum
TOL_TIME = 1e-5
SR = 48000.0
THETA0 = 10.0
# mvdr: five look angles
MVDR_ANGLES = [-90.0, -30.0, 0.0, 20.0, 75.0]
# lcmv: every column draws from a sector of its own, so that the columns of any one frame -- candidate or own angle, whatever the track
# says -- lie at least 20 degrees apart (near-coincident constraints have no parity claim: tools/fuzz_parity.py).  Sector c: the
# candidates COLS[c] and the column's own (create-time) angle OWN[c]
LCMV_ANGLES = [-20.0, 35.0, -60.0, -120.0, 90.0, 150.0, -160.0, -175.0, 10.0, -90.0, 120.0]
COLS = [[0, 1, 8], [2, 3, 9], [4, 5, 10], [6, 7]]
OWN = [THETA0, -75.0, 105.0, -170.0]


def _circ(a, b):
    return abs((a - b + 180.0) % 360.0 - 180.0)


for _c in range(4):
    for _d in range(_c + 1, 4):
        for _a in [LCMV_ANGLES[i] for i in COLS[_c]] + [OWN[_c]]:
            for _b in [LCMV_ANGLES[i] for i in COLS[_d]] + [OWN[_d]]:
                assert _circ(_a, _b) >= 20.0, (_a, _b)


def busy_column(F, choices, A, seed):
    """A new index at every frame drawn from `choices`, -1 and A + 2 (both: the column's own angle); every special value appears,
    frame 0 and the last frame differ from their neighbours."""
    rng = np.random.default_rng(seed)
    vals = list(choices) + [-1, A + 2]
    t = [choices[1], choices[0], choices[-1], -1, A + 2]
    while len(t) < F:
        v = vals[int(rng.integers(len(vals)))]
        if v != t[-1]:
            t.append(v)
    t = np.array(t[:F], np.int32)
    assert all(t[i] != t[i + 1] for i in range(F - 1))
    return t


def mvdr_track(F, seed):
    """[F, 1]"""
    return busy_column(F, list(range(len(MVDR_ANGLES))), len(MVDR_ANGLES), seed)[:, None]


def lcmv_track(F, n_cols, seed):
    """[F, n_cols]: every column changes at every frame"""
    return np.stack([busy_column(F, COLS[c], len(LCMV_ANGLES), seed + 31 * c) for c in range(n_cols)], axis=1)


def case(algo, M, K, F, hop=512, seed=None):
    """-> (params, x [M, F*hop], angles)"""
    p = make_params(algo, n_mics=M, hop=hop, theta=THETA0, interf=OWN[1:1 + K] if algo == "lcmv" else [])
    x = make_scene(M, F, hop, SR, seed=5000 + 100 * K + M + F if seed is None else seed)
    return p, x, (LCMV_ANGLES if algo == "lcmv" else MVDR_ANGLES)


def dev_x(x, layout):
    """x [S, M, F*H] -> the device tensor in the handle's layout."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1) if layout == 1 else x)).cuda()


def run_ctracked(bf, x, track, layout=0, spectrum=True):
    """x [S, M, F*H], track [S, F, n_cols] (None: an untracked batch) -> (y [S, F*H], Y [S, F, N] or None, kernels launched)."""
    import torch
    from beamform_amd import capi
    S, H = x.shape[0], bf.H
    F = x.shape[2] // H
    xd = dev_x(x, layout)
    yd = torch.full((S, F * H), float("nan"), dtype=torch.float32, device="cuda")
    Yd = torch.full((S, F, 2 * H, 2), float("nan"), dtype=torch.float64, device="cuda") if spectrum else None
    with capi.launch_trace() as tr:
        if track is None:
            bf.process_device(xd.data_ptr(), F, yd.data_ptr(), Yd.data_ptr() if spectrum else 0)
        else:
            track = np.ascontiguousarray(track, np.int32)
            assert track.shape[:2] == (S, F)
            td = torch.from_numpy(track).cuda()
            bf.process_device_ctracked(xd.data_ptr(), F, yd.data_ptr(), td.data_ptr(), track.shape[2], Yd.data_ptr() if spectrum else 0)
        torch.cuda.synchronize()
    Y = Yd.cpu().numpy().view(np.complex128)[..., 0] if spectrum else None
    return yd.cpu().numpy(), Y, tr.kernels


def errors(y, Y, y_ref, Y_ref):
    """tests/test_pipeline_gpu.py::check as figures: the finite masks must be equal (the frames the reference turns into NaN -- the inverse
    of a zero covariance -- are NaN on the GPU too); worst per-frame relative L2 on the spectrum, relative L2 on the finite samples."""
    res = {}
    if Y is not None:
        fin = np.isfinite(Y_ref).all(axis=1)
        res["finite_frames_equal"] = bool((np.isfinite(Y).all(axis=1) == fin).all())
        res["spectrum"] = max(rel_l2(Y[t], Y_ref[t]) for t in range(len(fin)) if fin[t]) if res["finite_frames_equal"] else float("inf")
    ok = np.isfinite(y_ref)
    res["finite_mask_equal"] = bool((np.isfinite(y) == ok).all())
    res["time"] = rel_l2(y[ok], y_ref[ok]) if res["finite_mask_equal"] else float("inf")
    return res


def check(y, Y, y_ref, Y_ref):
    res = errors(y, Y, y_ref, Y_ref)
    print(res)
    assert res["finite_mask_equal"], res
    assert res["time"] < TOL_TIME, res
    if Y is not None:
        assert res["finite_frames_equal"] and res["spectrum"] < TOL_SPECTRUM, res
    return res


def names(kernels, what):
    return [k for k in kernels if what in k]


_ORACLE = {}


def oracle_for(key, p, x, angles, track):
    """oracle_ctracked, computed once per case and shared (never written to)."""
    if key not in _ORACLE:
        y, Y, _ = ctrack_ref.oracle_ctracked(p, x, angles, track, THETA0)
        y.setflags(write=False)
        Y.setflags(write=False)
        _ORACLE[key] = (y, Y)
    return _ORACLE[key]
