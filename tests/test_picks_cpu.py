"""Multi-source picks and their column track on the host (bf_doa_pick_device, bf_ctrack_from_picks_device; include/bfcore.h): the C
surface and its argument checks, the shared arithmetic of beamform_amd/csrc/doa_pick.hpp (compiled here with g++) against numpy, and
the restatements the GPU tests compare with (tests/picks_ref.py) against controllers.pick_sources / DoaSources / sources_track."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import picks_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bf_doa_pick_device", "bf_ctrack_from_picks_device")
BF_EINVAL = -22


# ---- 1. surface ----------------------------------------------------------------------------------------------------------------------
def test_pick_symbols_are_declared_listed_and_exported():
    from beamform_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "bfcore.h")).read()
    declared = set(re.findall(r"\b(bf_[a-z_0-9]+)\s*\(", header))
    for n in NAMES:
        assert n in declared and n in capi.EXPORTS and hasattr(lib, n), n
    assert re.search(r"#define\s+BF_DOA_MAX_PICKS\s+16\b", header) and capi.BF_DOA_MAX_PICKS == 16
    assert capi.BF_DOA_MAX_PICKS == capi.BF_MAX_INTERF + 1


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_doa_pick_refuses_bad_arguments_before_any_device_work():
    """Every refusal happens on the host, in front of the launch: the pointers below are never read (this test runs without a GPU)."""
    from beamform_amd import capi
    lib = capi.load()
    buf = (C.c_double * 64)()
    ok = dict(map=C.addressof(buf), angles=C.addressof(buf), n_angles=5, n_streams=1, n_blocks=4, k=2, min_sep=10.0, rel_floor=0.5,
              picks=C.addressof(buf))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bf_doa_pick_device(a["map"], a["angles"], a["n_angles"], a["n_streams"], a["n_blocks"], a["k"], a["min_sep"],
                                      a["rel_floor"], a["picks"], None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(n_angles=0), dict(n_angles=-1), dict(n_angles=1025), dict(n_streams=0), dict(n_streams=-2), dict(k=0), dict(k=17),
           dict(min_sep=-1.0), dict(min_sep=nan), dict(min_sep=inf), dict(rel_floor=nan), dict(rel_floor=inf), dict(rel_floor=-inf),
           dict(map=None), dict(angles=None), dict(picks=None)]
    for kw in bad:
        assert call(**kw) == BF_EINVAL, kw
        assert b"bf_doa_pick_device" in lib.bf_last_error(None), kw
    assert call(n_blocks=0) == 0
    assert call(n_blocks=0, n_angles=1024, k=16, min_sep=0.0, rel_floor=-2.0) == 0   # the ends of the ranges are inside
    with pytest.raises(capi.BfError) as e:
        capi.doa_pick_device(0, C.addressof(buf), 5, 1, 4, 2, 10.0, 0.0, C.addressof(buf))
    assert e.value.code == BF_EINVAL and "bf_doa_pick_device" in str(e.value)


def test_ctrack_from_picks_refuses_bad_arguments_before_any_device_work():
    from beamform_amd import capi
    lib = capi.load()
    buf = (C.c_int32 * 64)()
    ok = dict(picks=C.addressof(buf), map=C.addressof(buf), n_angles=5, k=2, n_streams=1, n_blocks=4, W=4, latency=1, min_peak=0.5,
              n_cols=2, carry=C.addressof(buf), track=C.addressof(buf))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bf_ctrack_from_picks_device(a["picks"], a["map"], a["n_angles"], a["k"], a["n_streams"], a["n_blocks"], a["W"],
                                               a["latency"], a["min_peak"], a["n_cols"], a["carry"], a["track"], None)

    bad = [dict(n_angles=0), dict(n_angles=-3), dict(k=0), dict(k=17), dict(n_streams=0), dict(W=0), dict(latency=-1), dict(n_cols=0),
           dict(n_cols=17), dict(picks=None), dict(carry=None), dict(track=None), dict(map=None, min_peak=0.25)]
    for kw in bad:
        assert call(**kw) == BF_EINVAL, kw
        assert b"bf_ctrack_from_picks_device" in lib.bf_last_error(None), kw
    assert call(n_blocks=0) == 0 and call(n_blocks=0, map=None, min_peak=0.0, k=16, n_cols=16) == 0
    with pytest.raises(capi.BfError) as e:
        capi.ctrack_from_picks_device(0, 0, 5, 2, 1, 4, 4, 1, 0.0, 2, C.addressof(buf), C.addressof(buf))
    assert e.value.code == BF_EINVAL and "bf_ctrack_from_picks_device" in str(e.value)


# ---- 3. doa_pick.hpp against numpy -----------------------------------------------------------------------------------------------------
PICK_SRC = r"""
#include "%s"
extern "C" void sep_all(const double *a, const double *b, long n, double *out) {
    for (long i = 0; i < n; ++i) out[i] = bf::pick_sep(a[i], b[i]);
}
extern "C" void free_all(const double *a, const double *b, long n, double min_sep, int *out) {
    for (long i = 0; i < n; ++i) out[i] = bf::pick_stays_free(a[i], b[i], min_sep) ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def pick_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("doa_pick")
    src, so = os.path.join(d, "pick.cpp"), os.path.join(d, "libpick.so")
    with open(src, "w") as f:
        f.write(PICK_SRC % os.path.join(ROOT, "beamform_amd", "csrc", "doa_pick.hpp"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.sep_all.argtypes = [dp, dp, C.c_long, dp]
    lib.free_all.argtypes = [dp, dp, C.c_long, C.c_double, C.POINTER(C.c_int)]
    lib.sep_all.restype = lib.free_all.restype = None

    def sep(a, b):
        a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
        out = np.empty(a.size, np.float64)
        lib.sep_all(a.ctypes.data_as(dp), b.ctypes.data_as(dp), a.size, out.ctypes.data_as(dp))
        return out

    def stays(a, b, min_sep):
        a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
        out = np.empty(a.size, np.int32)
        lib.free_all(a.ctypes.data_as(dp), b.ctypes.data_as(dp), a.size, float(min_sep), out.ctypes.data_as(C.POINTER(C.c_int)))
        return out.astype(bool)
    return sep, stays


def _pairs():
    """Every pair of a grid that holds -180 and +180, values beyond +-360, duplicates, in no order; and pairs whose t = a - b + 180 is a
    tiny negative number, where r + 360.0 rounds to 360.0."""
    rng = np.random.default_rng(31)
    g = np.concatenate([[-180.0, 180.0, 0.0, -0.0, 360.0, -360.0, 540.0, -540.0, 719.5, -1000.25, 90.0, 90.0, -90.0, 1e-300, -1e-300],
                        np.arange(-180.0, 180.0, 7.5), rng.uniform(-800.0, 800.0, 60), np.round(rng.uniform(-180, 180, 30))])
    g = rng.permutation(g)
    a, b = [v.ravel() for v in np.meshgrid(g, g, indexing="ij")]
    u = np.spacing(180.0)  # one step of the doubles around 180: a - b = -180 - u is a number, and 360 - u is not
    ta = np.array([np.nextafter(-180.0, -np.inf), -90.0 - u, -100.0 - u, 0.0, -90.0 - 1e-13, -180.0 - 2 * u])
    tb = np.array([0.0, 90.0, 80.0, np.nextafter(180.0, np.inf), 90.0, 0.0])
    return np.concatenate([a, ta]), np.concatenate([b, tb]), a.size


def test_doa_pick_hpp_is_numpys_expression_bit_for_bit(pick_lib):
    sep, stays = pick_lib
    a, b, n_grid = _pairs()
    want = np.abs((a - b + 180.0) % 360.0 - 180.0)
    got = sep(a, b)
    assert got.tobytes() == want.tobytes()
    assert picks_ref.sep(a, b).tobytes() == want.tobytes()
    # the tiny negative differences did what they are here for: r + 360.0 rounded to 360.0, a distance of 180
    t = (a[n_grid:] - b[n_grid:]) + 180.0
    tiny = (t < 0) & (t > -1e-10)
    assert tiny.all() and tiny.size == 6
    rounds = np.fmod(t, 360.0) + 360.0 == 360.0
    assert rounds.sum() == 4 and (got[n_grid:][rounds] == 180.0).all() and (got[n_grid:][~rounds] < 180.0).all()
    assert 0.0 <= got.min() and got.max() <= 180.0
    for min_sep in (0.0, 7.5, 10.0, 180.0, 400.0):
        assert np.array_equal(stays(a, b, min_sep), want >= min_sep), min_sep


# ---- 4. picks_ref.pick is controllers.pick_sources ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 65, 130])
def test_pick_ref_is_pick_sources(A):
    from beamform_amd.controllers import pick_sources
    m = picks_ref.rows(10, A)
    assert (m[2] == m[2, 0]).all() and (m[7] == 0).all() and len(np.unique(m[1])) <= 5
    n_short = 0
    for name, grid in picks_ref.grids(A).items():
        for k, min_sep, rel_floor in picks_ref.PARAMS:
            for r in range(m.shape[0]):
                want = pick_sources(m[r], grid, k, min_sep, rel_floor)
                got = picks_ref.pick(m[r], grid, k, min_sep, rel_floor)
                assert got.dtype == np.int32 and got.shape == (k,)
                assert list(got[:len(want)]) == want and (got[len(want):] == -1).all(), (name, k, min_sep, rel_floor, r)
                n_short += len(want) < k
    assert n_short > 0  # k larger than what can be picked


# ---- 5. picks_ref.from_picks is sources_track --------------------------------------------------------------------------------------------
def test_from_picks_ref_is_sources_track():
    from beamform_amd.controllers import DoaSources, sources_track
    nb, W, A, k = 11, 3, 24, 3
    rng = np.random.default_rng(20261019)
    grid = rng.permutation(np.arange(-180.0, 180.0, 15.0))
    maps = rng.random((nb, A))
    maps[0] *= 0.01                                            # block 0 does not publish
    min_peak = float(np.median(maps.max(axis=1)))              # some blocks publish, some do not
    min_sep, rel_floor = 40.0, 0.9                             # and a publication does not always fill every column
    picks = picks_ref.pick_all(maps, grid, k, min_sep, rel_floor)
    assert (picks[:, 0] >= 0).all() and (picks[:, 1:] == -1).any() and (picks[:, 2] >= 0).any()
    ctl = DoaSources(grid, k, min_sep, rel_floor, min_peak)
    for latency in (0, 1, 2):
        for n_cols in (1, 2, 4):
            want, published = sources_track(maps, ctl, W, n_cols, latency)
            assert 0 < len(published) < nb and published[0][0] > 0
            trk, carry = picks_ref.from_picks(picks[None], maps[None], A, W, latency, min_peak, n_cols, -1)
            assert trk.shape == (1, nb * W, n_cols) and trk.dtype == np.int32
            assert np.array_equal(trk[0], want), (latency, n_cols)
            first = published[0][0] + latency                  # nothing is in force before the first publication arrives
            assert (trk[0, :first * W] == -1).all() and (trk[0, first * W:, 0] >= 0).all()
            if n_cols > k:
                assert (trk[0, :, k:] == -1).all()             # columns >= k are never updated
            # what a block nb would get: the track of one more block, whatever its map says
            more, _ = sources_track(np.concatenate([maps, maps[:1]]), ctl, W, n_cols, latency)
            assert np.array_equal(carry[0], more[-1]), (latency, n_cols)
            # a NULL map publishes every block with a valid first pick: min_peak = 0 says the same
            t0, c0 = picks_ref.from_picks(picks[None], None, A, W, latency, 0.0, n_cols, -1)
            t1, c1 = picks_ref.from_picks(picks[None], maps[None], A, W, latency, 0.0, n_cols, -1)
            assert np.array_equal(t0, t1) and np.array_equal(c0, c1)
    # Cut into two calls through carry: exact for a latency of 0 or 1 block (carry is one index per column; the header says so).
    for latency in (0, 1):
        for n_cols in (2, 4):
            one, c_one = picks_ref.from_picks(picks[None], maps[None], A, W, latency, min_peak, n_cols, -1)
            for cut in (1, 5, 10):
                a, c_a = picks_ref.from_picks(picks[None, :cut], maps[None, :cut], A, W, latency, min_peak, n_cols, -1)
                b, c_b = picks_ref.from_picks(picks[None, cut:], maps[None, cut:], A, W, latency, min_peak, n_cols, c_a)
                assert np.array_equal(np.concatenate([a, b], axis=1), one) and np.array_equal(c_b, c_one), (latency, n_cols, cut)
