"""The shapes of the lcmv beam tests (bf_config.lcmv_out_beams = R), shared by the CPU check of the permutation identity
(tests/test_lcmv_beams_cpu.py), the GPU tests (tests/test_lcmv_beams_gpu.py) and their child processes: name -> scene, parameters and
the reference's rows, each computed once per process.  Test infrastructure only.

Row r of a beam is the reference's lcmv node with `angle` and interference_angles[r-1] exchanged (W (C P) = W(C) P for a column
permutation P): oracle.OracleNode, driven with swapped angles, is the yardstick of every row; rows r >= 1 + interferers are zeros."""
import functools

import numpy as np

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene
from conftest import rel_l2
from gss_sources_ref import circle_mics

TOL_SPECTRUM = TOL_TIME = 1e-5   # tests/test_pipeline_gpu.py
THETA = 20.0
POOL = (-60.0, 90.0, 150.0, -120.0, 60.0)   # interferers, in this order


def _c(M, K, R, F, hop=512, **kw):
    return dict(M=M, K=K, R=R, F=F, hop=hop, **kw)


CASES = {
    # the lane kernel (mvdr_fast_rows_kernel), up to 8 microphones
    "l8k2": _c(8, 2, 3, 16), "l8k3": _c(8, 3, 4, 16), "l4k1": _c(4, 1, 2, 14), "l6k3": _c(6, 3, 4, 14),
    "l8k1r4": _c(8, 1, 4, 12),                  # more rows than columns
    # cov2d_rows_kernel, 9 .. 16 microphones
    "c16k3": _c(16, 3, 4, 14), "c9k1": _c(9, 1, 2, 14),
    # the group kernel: above 16 microphones, above 3 interferers, two microphones with three columns
    "g20k1": _c(20, 1, 2, 12), "g8k5": _c(8, 5, 6, 13), "g2k2": _c(2, 2, 3, 12), "g2k1": _c(2, 1, 2, 13),
    # no interferer: the twins' padding column is the identity, row 1 is zero
    "l8k0": _c(8, 0, 2, 14), "c12k0": _c(12, 0, 2, 13), "g20k0": _c(20, 0, 2, 12),
    # the other FFT sizes
    "h64": _c(4, 1, 2, 16, 64), "h256": _c(4, 1, 2, 14, 256), "h1024": _c(4, 1, 2, 13, 1024), "h2048": _c(4, 1, 2, 12, 2048),
    "h4096": _c(4, 1, 2, 12, 4096),
    # the default silent stretch: closed gates put 0.01 X_0 on every row
    "silent": _c(8, 2, 3, 20, silent=True),
    # K + 1 = M (CPU check of the identity only)
    "m4k3": _c(4, 3, 4, 13), "m5k1h64": _c(5, 1, 2, 14, 64),
    # column tracks
    "t8k2": _c(8, 2, 3, 20), "t16k1": _c(16, 1, 2, 16),
}
SEEDS = {name: 12100 + 19 * i for i, name in enumerate(CASES)}


def case_params(name, swap=0, theta=None, **over):
    """The case's parameters (theta: another look direction); swap = r >= 1: `angle` and interferer r exchanged (the reference of row r)."""
    c = CASES[name]
    theta, interf = THETA if theta is None else theta, list(POOL[:c["K"]])
    if swap:
        theta, interf[swap - 1] = interf[swap - 1], theta
    if c["M"] > 16:
        over = dict(mics=circle_mics(c["M"]), **over)
    return make_params("lcmv", n_mics=c["M"], hop=c["hop"], theta=theta, interf=interf, **over)


@functools.lru_cache(maxsize=None)
def case_scene(name, stream=0):
    c, p = CASES[name], case_params(name)
    kw = {} if c.get("silent") else {"silent_frac": 0.0}
    x = make_scene(c["M"], c["F"], hop=c["hop"], seed=SEEDS[name] + 1000 * stream, mics=p["mics"], **kw)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def row_ref(name, r, stream=0, theta=None):
    """(y [F*H] float32, Y [F, N] complex128) of row r: the oracle with angle and interf[r-1] exchanged; zeros past the columns.
    Shared, do not modify."""
    import oracle
    c = CASES[name]
    if r > c["K"]:
        y, Y = np.zeros(c["F"] * c["hop"], np.float32), np.zeros((c["F"], 2 * c["hop"]), np.complex128)
    else:
        y, Y = oracle.OracleNode(case_params(name, swap=r, theta=theta)).process(case_scene(name, stream), want_spectrum=True)
    y.setflags(write=False)
    Y.setflags(write=False)
    return y, Y


def case_ref(name, stream=0, theta=None):
    """(y [R, F*H], Y [R, F, N]) of one stream."""
    rows = [row_ref(name, r, stream, theta) for r in range(CASES[name]["R"])]
    return np.stack([y for y, _ in rows]), np.stack([Y for _, Y in rows])


def inband(p):
    from oracle import np_oracle
    f = np.abs(np_oracle.freq_vector(2 * p["hop"], p["sample_rate"]))
    return (f >= p["freq_min"]) & (f <= p["freq_max"])


# ---- the comparison --------------------------------------------------------------------------------------------------------------------
def check_time(y, y_ref, left_out=None):
    """y, y_ref [R, n]: the finite masks equal, every row within TOL_TIME on the finite samples; a zero row is exactly zero."""
    assert y.shape == y_ref.shape
    assert (np.isfinite(y) == np.isfinite(y_ref)).all()
    for r in range(y_ref.shape[0]):
        ok = np.isfinite(y_ref[r])
        if left_out is not None:
            assert (~ok).sum() <= left_out, (r, int((~ok).sum()))
        if not y_ref[r][ok].any():
            assert not y[r][ok].any(), f"row {r} is zero by definition"
        else:
            e = rel_l2(y[r][ok], y_ref[r][ok])
            print(f"row {r}: time {e:.3e}")
            assert e < TOL_TIME, (r, e)


def check_rows(p, y, Y, y_ref, Y_ref, nan_frames=(0,)):
    """Rows of one beam: y [R, F*H], Y [R, F, N] against the reference's, row by row and frame by frame.  The non-finite frames must be
    the reference's, and those only the frames named (frame 0 after a cold start)."""
    R, F, _ = Y_ref.shape
    assert Y.shape == Y_ref.shape and y.shape == y_ref.shape
    assert not Y[:, :, ~inband(p)].any(), "out of band every row is zero"
    for r in range(R):
        fin = np.isfinite(Y_ref[r]).all(axis=1)
        assert set(np.flatnonzero(~fin)) <= set(nan_frames), (r, np.flatnonzero(~fin))
        assert (np.isfinite(Y[r]).all(axis=1) == fin).all(), (r, np.flatnonzero(~np.isfinite(Y[r]).all(axis=1)))
        worst = 0.0
        for t in range(F):
            if not fin[t]:
                continue
            if not Y_ref[r, t].any():
                assert not Y[r, t].any(), f"row {r} frame {t} is zero by definition"
            else:
                worst = max(worst, rel_l2(Y[r, t], Y_ref[r, t]))
        print(f"row {r}: spectrum {worst:.3e}")
        assert worst < TOL_SPECTRUM, (r, worst)
    check_time(y, y_ref, left_out=2 * len(nan_frames) * p["hop"])


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------------
def run_dev(bf, x, F, dump=True, track=None):
    """One batch -> (y [n_out, F*H] float32, Y [n_out, F, N] complex128 or None, kernels).  The buffers start as NaN: whatever the kernels
    leave unwritten shows.  track [F, n_cols] int32: a column-tracked batch."""
    import torch
    from beamform_amd import capi
    xd = torch.from_numpy(np.array(x, order="C")).cuda()   # (a copy: the shared scenes are read-only)
    yd = torch.full((bf.n_out, F * bf.H), float("nan"), dtype=torch.float32, device="cuda")
    Yd = torch.full((bf.n_out, F, bf.N, 2), float("nan"), dtype=torch.float64, device="cuda") if dump else None
    with capi.launch_trace() as tr:
        if track is None:
            bf.process_device(xd.data_ptr(), F, yd.data_ptr(), Yd.data_ptr() if dump else 0)
        else:
            td = torch.from_numpy(np.ascontiguousarray(track, np.int32)).cuda()
            bf.process_device_ctracked(xd.data_ptr(), F, yd.data_ptr(), td.data_ptr(), track.shape[1], Yd.data_ptr() if dump else 0)
        torch.cuda.synchronize()
    return yd.cpu().numpy(), (Yd.cpu().numpy().view(np.complex128)[..., 0] if dump else None), tr.kernels


def run_case(name, cuts=None, **kw):
    """The case through a handle with R rows, as one batch or cut at `cuts` -> (y, Y, kernels of the last batch)."""
    from beamform_amd.capi import Beamformer
    c, p = CASES[name], case_params(name)
    H = c["hop"]
    bf = Beamformer(p, lcmv_out_beams=c["R"], **kw)
    cuts = [0, c["F"]] if cuts is None else [0] + list(cuts) + [c["F"]]
    ys, Ys = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y, Y, kernels = run_dev(bf, case_scene(name)[:, a * H:b * H], b - a)
        ys.append(y)
        Ys.append(Y)
    bf.close()
    return np.concatenate(ys, axis=1), np.concatenate(Ys, axis=1), kernels


def run_one_row(name, **kw):
    """The same case through an R = 1 handle -> (y [F*H], Y [F, N], kernels)."""
    from beamform_amd.capi import Beamformer
    c = CASES[name]
    bf = Beamformer(case_params(name), **kw)
    y, Y, kernels = run_dev(bf, case_scene(name), c["F"])
    bf.close()
    return y[0], Y[0], kernels


def check_case(name, y, Y, kernels, twin, one_row):
    """Every row against its reference, rows past the columns exactly zero, row 0 the R = 1 handle's bytes, whose trace names the one-row
    kernel `one_row` where this batch's names the twin `twin`."""
    c, p = CASES[name], case_params(name)
    y_ref, Y_ref = case_ref(name)
    check_rows(p, y, Y, y_ref, Y_ref)
    S = c["K"] + 1
    assert not Y[S:].any() and not y[S:].any()
    assert any(twin in k for k in kernels), kernels
    y1, Y1, k1 = run_one_row(name)
    assert any(one_row in k for k in k1) and not any("_rows_kernel" in k for k in k1), k1
    assert np.array_equal(Y[0], Y1, equal_nan=True) and np.array_equal(y[0], y1, equal_nan=True)


# ---- stream semantics: /theta and a structural interferer change between batches ---------------------------------------------------------
SEM = dict(M=8, interf=(-60.0,), R=3, F=30, cuts=(0, 5, 6, 17, 30), theta1=-140.0, new_interf=90.0, seed=12900)


def sem_params():
    return make_params("lcmv", n_mics=SEM["M"], theta=THETA, interf=SEM["interf"])


@functools.lru_cache(maxsize=None)
def sem_scene():
    x = make_scene(SEM["M"], SEM["F"], seed=SEM["seed"], silent_frac=0.0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sem_ref():
    """(y [3, F*H], Y [3, F, N]): cold start, a batch cut, /theta in front of the third piece, a second interferer in front of the fourth.
    Row r is an oracle node of its own that gets the handle's control calls with columns 0 and r exchanged: a change of the look
    direction is set_theta on row 0's node and a (non-structural, never merging) set_interference(r) on row r's; the structural change
    is the same call on every node (quirk Q3 zeroes microphone 0's entries of all columns alike).  Row 2 does not exist before the
    change -- zeros -- and starts from the history the other rows have: its node runs along from the cold start, takes the new
    interferer and then exchanges its columns 0 and 2; its time output is the overlap-add of the masked spectra."""
    import oracle
    from oracle import np_oracle
    p, x, cuts, H = sem_params(), sem_scene(), SEM["cuts"], 512
    t2, t3 = cuts[2], cuts[3]
    nodes = [oracle.OracleNode(p), oracle.OracleNode(dict(p, theta=SEM["interf"][0], interf=(THETA,))), oracle.OracleNode(p)]
    ys, Ys = [[], [], []], [[], [], []]
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if i == 2:
            nodes[0].set_theta(SEM["theta1"])
            assert nodes[1].set_interference(1, SEM["theta1"], threshold=0.0) == 1
            nodes[2].set_theta(SEM["theta1"])
        if i == 3:
            for n in nodes:
                assert n.set_interference(2, SEM["new_interf"]) == 2
            nodes[2].set_theta(SEM["new_interf"])
            assert nodes[2].set_interference(2, SEM["theta1"], threshold=0.0) == 2
        for r, n in enumerate(nodes):
            y, Y = n.process(x[:, a * H:b * H], want_spectrum=True)
            ys[r].append(y)
            Ys[r].append(Y)
    y, Y = np.stack([np.concatenate(v) for v in ys]), np.stack([np.concatenate(v) for v in Ys])
    Y[2, :t3] = 0
    y[2] = np_oracle.istft_ola(p, Y[2], p["out_amp"])
    assert t2 < t3 and np.isfinite(Y[:, 1:]).all()
    y.setflags(write=False)
    Y.setflags(write=False)
    return y, Y


# ---- column tracks -------------------------------------------------------------------------------------------------------------------------
#: candidate angles; column c draws from TRACK_COLS[c], at least 20 degrees from every other column's candidates and own angle
TRACK_ANGLES = [35.0, -20.0, -75.0, -100.0, 120.0, 165.0]


def case_track(name):
    """[F, K + 1] int32: column 0 changes at frames 7 and 14, column 1 at frames 4 and 11 (99: out of range, the column's own angle),
    column 2 at frame 9."""
    c = CASES[name]
    F = c["F"]
    t = np.full((F, 3), -1, np.int32)
    t[7:14, 0], t[14:, 0] = 0, 1
    t[:4, 1], t[4:11, 1], t[11:, 1] = 2, 99, 3
    t[9:, 2] = 4
    return np.ascontiguousarray(t[:, :c["K"] + 1])


@functools.lru_cache(maxsize=None)
def track_ref(name, r):
    """Row r of the column-tracked case: ctrack_ref.oracle_ctracked with columns 0 and r of the track and of the own angles exchanged."""
    import ctrack_ref
    p = case_params(name, swap=r)
    track = case_track(name).copy()
    track[:, [0, r]] = track[:, [r, 0]]
    y, Y, _ = ctrack_ref.oracle_ctracked(p, case_scene(name), TRACK_ANGLES, track, p["theta"])
    y.setflags(write=False)
    Y.setflags(write=False)
    return y, Y
