"""Column tracks on the host (bf_ctrack_*, include/bfcore.h): the C surface, the launch plan of a column-tracked batch
(beamform_amd/csrc/chain_plan.hpp, compiled here with g++), controllers.sources_track against controllers.follow_sources, and the oracle
helper the GPU tests compare with."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctrack_ref  # noqa: E402

from beamform_amd.params import make_params  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bf_ctrack_set_angles", "bf_process_batch_device_ctracked")
BF_EINVAL = -22


# ---- 1. surface --------------------------------------------------------------------------------------------------------------------
def test_ctrack_symbols_are_declared_listed_and_exported():
    from beamform_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "bfcore.h")).read()
    declared = set(re.findall(r"\b(bf_[a-z_0-9]+)\s*\(", header))
    for n in NAMES:
        assert n in declared and n in capi.EXPORTS and hasattr(lib, n), n
    assert hasattr(capi.Beamformer, "set_ctrack_angles") and hasattr(capi.Beamformer, "process_device_ctracked")
    from beamform_amd import controllers
    assert callable(controllers.sources_track) and callable(controllers.follow_sources_tracked)


def test_null_handle_is_refused_before_any_device_work():
    """No handle, no device: the pointers below are never read (this test runs without a GPU)."""
    from beamform_amd import capi
    lib = capi.load()
    ang = (C.c_double * 2)(10.0, 20.0)
    buf = (C.c_int32 * 16)()
    assert lib.bf_ctrack_set_angles(None, ang, 2) == BF_EINVAL
    assert lib.bf_process_batch_device_ctracked(None, C.addressof(buf), 4, C.addressof(buf), None, C.addressof(buf), 1, None) == BF_EINVAL


# ---- 2. the launch plan ------------------------------------------------------------------------------------------------------------
PLAN_SRC = r"""
#include "%s"
using namespace bf;
// mode 0: the shape written without the ctrack_cols field; 1: ctrack_cols = 0; 2: ctrack_cols = kp1
extern "C" void plan(int algo, int n_fft, int layout, int n_mics, int fused_bins, int kp1, int precision, int dump, int mvdr_group,
                     int mode, long long *o) {
    ChainShape c{algo, n_fft, layout, n_mics, 1, 1, kp1, 10, precision, dump != 0, 24, 256, 128, 3, 0, n_fft / 2 + 1, true,
                 fused_bins, true, true, mvdr_group != 0, -1, false, 1, false};
    if (mode == 1) c.ctrack_cols = 0;
    if (mode == 2) c.ctrack_cols = kp1;
    const ChainPlan p = chain_decide(c);
    const long long v[] = {p.algo, p.layout, (long long)p.front, p.z48, (long long)p.bins, p.mp, p.km, p.wps, (long long)p.rec, p.expand,
                           (long long)p.istft, (long long)p.tail, p.t0, p.t1, p.t2, p.yh32, p.mpf32, p.band_rows, p.yh_lo, p.yh_hi,
                           (long long)p.z_bytes, (long long)p.yh_bytes, (long long)p.yraw_elems, (long long)p.frames_elems, p.rows,
                           p.fused(), p.track, p.ctrack};
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = v[i];
}
"""
FIELDS = ("algo layout front z48 bins mp km wps rec expand istft tail t0 t1 t2 yh32 mpf32 band_rows yh_lo yh_hi z_bytes yh_bytes "
          "yraw_elems frames_elems rows fused track ctrack").split()
BINS_MVDR_FAST, BINS_COV2D, BINS_MVDR_LCMV = 5, 6, 7  # ChainBins::kMvdrFast, kCov2d, kMvdrLcmv


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctrack_plan")
    src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "libplan.so")
    with open(src, "w") as f:
        f.write(PLAN_SRC % os.path.join(ROOT, "beamform_amd", "csrc", "chain_plan.hpp"))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.plan.argtypes = [C.c_int] * 10 + [C.POINTER(C.c_longlong)]
    lib.plan.restype = None

    def plan(algo, N, layout, M, fused_bins, mode, kp1=1, precision=0, dump=0, mvdr_group=0):
        o = (C.c_longlong * len(FIELDS))()
        lib.plan(algo, N, layout, M, fused_bins, kp1, precision, dump, mvdr_group, mode, o)
        return dict(zip(FIELDS, o))
    return plan


def test_a_shape_without_the_field_keeps_its_plan(plan_lib):
    from beamform_amd.params import ALGO_ID
    # the rows tests/test_track_cpu.py::test_tracked_plan walks
    for name, N, M, layout, fb in itertools.product(("das", "phase", "phasempf"), (128, 1024, 2048, 8192), (2, 3, 8, 9, 16), (0, 1), (0, 1)):
        plain, off = (plan_lib(ALGO_ID[name], N, layout, M, fb, mode) for mode in (0, 1))
        assert plain == off and plain["ctrack"] == 0, (name, N, M, layout, fb)
    for name, M, kp1, N in itertools.product(("mvdr", "lcmv"), (2, 3, 8, 9, 16, 17), (1, 3, 4, 5), (256, 1024)):
        if name == "mvdr" and kp1 != 1:
            continue
        plain, off = (plan_lib(ALGO_ID[name], N, 0, M, 1, mode, kp1=kp1) for mode in (0, 1))
        assert plain == off and plain["ctrack"] == 0, (name, M, kp1, N)
        # and it is the plan the node has always had: cov2d for 9 .. 16 microphones with up to 3 interferers, the lane kernel up to 8
        # microphones wherever its columns fit, the group kernel otherwise
        want = (BINS_MVDR_LCMV if kp1 > 4 or M > 16 else BINS_COV2D if M > 8 else BINS_MVDR_FAST if (M > 2 or kp1 <= 2) else BINS_MVDR_LCMV)
        assert plain["bins"] == want, (name, M, kp1, N)


def test_column_tracked_plan(plan_lib):
    from beamform_amd.params import ALGO_ID
    for name, M, kp1, N, prec, dump, grp in itertools.product(("mvdr", "lcmv"), (2, 3, 8, 9, 16, 17), (1, 3, 4, 5), (256, 1024), (0, 1),
                                                              (0, 1), (0, 1)):
        if name == "mvdr" and kp1 != 1:
            continue
        case = (name, M, kp1, N, prec, dump, grp)
        plain, on = (plan_lib(ALGO_ID[name], N, 0, M, 1, mode, kp1=kp1, precision=prec, dump=dump, mvdr_group=grp) for mode in (0, 2))
        assert on["ctrack"] == 1 and on["track"] == 0, case
        assert on["bins"] != BINS_COV2D, case
        if plain["bins"] == BINS_COV2D:  # 9 .. 16 microphones: the group kernel's twin, as BF_MVDR_GROUP=1 picks it untracked
            grouped = plan_lib(ALGO_ID[name], N, 0, M, 1, 0, kp1=kp1, precision=prec, dump=dump, mvdr_group=1)
            assert on["bins"] == BINS_MVDR_LCMV and (on["mp"], on["km"]) == (grouped["mp"], grouped["km"]) == (16, 1 if kp1 == 1 else 4), case
            same = [k for k in FIELDS if k not in ("ctrack", "bins", "mp", "km", "wps")]
        else:
            same = [k for k in FIELDS if k != "ctrack"]
        assert {k: on[k] for k in same} == {k: plain[k] for k in same}, case
        for k in ("z_bytes", "yh_bytes", "yraw_elems", "frames_elems"):
            assert on[k] == plain[k], (case, k)
    # more than one look direction: no column track (the entry point refuses such a handle)
    # ... and the field means nothing to the other nodes
    for name in ("das", "phase", "phasempf", "gss", "mcra", "gsc"):
        for M in (4, 8, 16):
            p0, p2 = plan_lib(ALGO_ID[name], 1024, 0, M, 1, 0, kp1=3), plan_lib(ALGO_ID[name], 1024, 0, M, 1, 2, kp1=3)
            assert p0 == p2 and p2["ctrack"] == 0, (name, M)


# ---- 3. sources_track is follow_sources' schedule ------------------------------------------------------------------------------------
class _StubDoa:
    def __init__(self, maps):
        self.maps, self.b = maps, 0

    def process(self, seg):
        self.b += 1
        return self.maps[self.b - 1:self.b], None


class _StubNode:
    """Records, per frame and column, the angle in force while the frame was processed (None: the node's own)."""
    H = 2

    def __init__(self, n_cols, W):
        self.W, self.cur, self.seen = W, [None] * n_cols, []

    def process(self, seg):
        assert seg.shape[1] == self.W * self.H
        self.seen += [list(self.cur)] * self.W
        return np.zeros(seg.shape[1], np.float32)

    def set_theta(self, deg):
        self.cur[0] = deg

    def set_interference(self, idx, deg):
        assert 1 <= idx < len(self.cur)
        self.cur[idx] = deg


class _Scripted:
    """A controller that publishes what a script says, block by block (None: no publication)."""

    def __init__(self, angles, script):
        self.angles, self.script, self.b = np.asarray(angles, np.float64), script, 0

    def on_map(self, row):
        self.b += 1
        return self.script[self.b - 1]


def test_sources_track_is_follow_sources_schedule():
    from beamform_amd.controllers import DoaSources, follow_sources, sources_track
    grid = np.arange(-180.0, 180.0, 10.0)
    W, n_cols = 3, 3
    # a stretch without publication in front, a block with fewer interferers than columns, a silent block in the middle
    script = [None, None, (20.0, [-60.0, 90.0]), (30.0, [-70.0]), None, (40.0, []), (-20.0, [100.0, 150.0]), None]
    nb = len(script)
    maps = np.zeros((nb, grid.size))
    node = _StubNode(n_cols, W)
    x = np.zeros((2, nb * W * node.H), np.float32)
    _, pub_loop = follow_sources(node, _StubDoa(maps), x, W, _Scripted(grid, script))
    track, pub = sources_track(maps, _Scripted(grid, script), W, n_cols)
    assert pub == pub_loop and [b for b, _, _ in pub] == [2, 3, 5, 6]
    assert track.shape == (nb * W, n_cols) and track.dtype == np.int32
    assert (track[:3 * W] == -1).all() and (track[3 * W:, :2] >= 0).all()  # nothing published yet: the node's own angles
    for t in range(nb * W):
        for c in range(n_cols):
            want = node.seen[t][c]
            got = None if track[t, c] < 0 else float(grid[track[t, c]])
            assert got == want, (t, c)
    assert float(grid[track[4 * W, 2]]) == 90.0  # block 3 published one interferer: column 2 keeps block 2's
    # interferers beyond n_cols - 1 are dropped; latency 0 and 2 shift the schedule by a block each way
    t2, p2 = sources_track(maps, _Scripted(grid, script), W, 2)
    assert np.array_equal(t2, track[:, :2]) and p2 == pub
    t0, _ = sources_track(maps, _Scripted(grid, script), W, n_cols, latency_blocks=0)
    assert np.array_equal(t0[:-W], track[W:])
    tl2, _ = sources_track(maps, _Scripted(grid, script), W, n_cols, latency_blocks=2)
    assert np.array_equal(tl2[W:], track[:-W]) and (tl2[:W] == -1).all()
    # a real controller on random maps: the same publications as the loop, the same angles in force
    rng = np.random.default_rng(20261019)
    maps = rng.random((nb, grid.size))
    node = _StubNode(n_cols, W)
    _, pub_loop = follow_sources(node, _StubDoa(maps), x, W, DoaSources(grid, 3, 30.0, min_peak=0.985))
    track, pub = sources_track(maps, DoaSources(grid, 3, 30.0, min_peak=0.985), W, n_cols)
    assert pub == pub_loop and 0 < len(pub) < nb
    got = [[None if i < 0 else float(grid[i]) for i in row] for row in track]
    assert got == node.seen


# ---- 4. the oracle helper ------------------------------------------------------------------------------------------------------------
def test_oracle_ctracked_with_a_constant_track_is_the_steered_node():
    import oracle
    M, F = 4, 6
    x = make_scene(M, F, seed=3)
    angles = [-90.0, 20.0, 75.0, 140.0]
    # mvdr: one column
    p = make_params("mvdr", n_mics=M)
    y, Y, _ = ctrack_ref.oracle_ctracked(p, x, angles, np.full((F, 1), 2), theta0=45.0)
    node = oracle.OracleNode(dict(p, theta=45.0))
    node.set_theta(75.0)
    y_ref, Y_ref = node.process(x, want_spectrum=True)
    assert y.tobytes() == y_ref.tobytes() and Y.tobytes() == Y_ref.tobytes()
    # lcmv: both columns named, then only the look direction (the interferer stays the node's own); an index that names no angle is
    # the column's create-time angle
    p = make_params("lcmv", n_mics=M, interf=[-60.0])
    y, Y, _ = ctrack_ref.oracle_ctracked(p, x, angles, np.tile([1, 3], (F, 1)), theta0=45.0)
    node = oracle.OracleNode(dict(p, theta=45.0))
    node.set_theta(20.0)
    assert node.set_interference(1, 140.0, threshold=0.0) == 1
    y_ref, Y_ref = node.process(x, want_spectrum=True)
    assert y.tobytes() == y_ref.tobytes() and Y.tobytes() == Y_ref.tobytes()
    y, Y, _ = ctrack_ref.oracle_ctracked(p, x, angles, np.array([[-1, 7], [9, -3], [-1, -1], [4, 4], [-2, 5], [-1, 4]]), theta0=45.0)
    y_ref, Y_ref = oracle.OracleNode(dict(p, theta=45.0)).process(x, want_spectrum=True)
    fin = np.isfinite(Y_ref)
    assert (np.isfinite(Y) == fin).all() and Y[fin].tobytes() == Y_ref[fin].tobytes() and y.tobytes() == y_ref.tobytes()
    assert np.array_equal(ctrack_ref.angles_in_force(angles, np.array([[0], [5]]), [45.0, -60.0]), [[-90.0, -60.0], [45.0, -60.0]])
