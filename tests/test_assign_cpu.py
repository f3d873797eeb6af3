"""Talker identities on the host (bf_ctrack_assign_device; include/bfcore.h): the C surface and its argument checks, and the rule
three times over -- beamform_amd/csrc/doa_assign.hpp compiled here with g++, controllers.assign_sources and the restatement
tests/assign_ref.py -- on generated cases, on the properties the header states, and on a five-segment conversation whose columns the
older builder swaps."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref  # noqa: E402
import picks_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bf_ctrack_assign_device"
BF_EINVAL = -22


# ---- 1. surface and refusals ---------------------------------------------------------------------------------------------------------
def test_assign_symbol_is_declared_listed_and_exported():
    from beamform_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "bfcore.h")).read()
    declared = set(re.findall(r"\b(bf_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in capi.EXPORTS and hasattr(lib, NAME)
    assert re.search(r"#define\s+BF_ASSIGN_STATE_INTS\s+4\b", header) and capi.BF_ASSIGN_STATE_INTS == 4
    assert callable(capi.ctrack_assign_device)


def test_assign_refuses_bad_arguments_before_any_device_work():
    """Every refusal happens on the host, in front of the launch: the pointers below are never read (this test runs without a GPU)."""
    from beamform_amd import capi
    lib = capi.load()
    buf = (C.c_double * 64)()
    ptr = C.addressof(buf)
    ok = dict(picks=ptr, map=ptr, angles=ptr, n_angles=5, k=2, n_streams=1, n_blocks=4, W=4, latency=1, min_peak=0.5, gate=20.0,
              min_hits=2, max_coast=8, n_cols=2, state=ptr, track=ptr, active=ptr)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bf_ctrack_assign_device(a["picks"], a["map"], a["angles"], a["n_angles"], a["k"], a["n_streams"], a["n_blocks"], a["W"],
                                           a["latency"], a["min_peak"], a["gate"], a["min_hits"], a["max_coast"], a["n_cols"], a["state"],
                                           a["track"], a["active"], None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(n_angles=0), dict(n_angles=-1), dict(n_angles=1025), dict(k=0), dict(k=17), dict(n_streams=0), dict(n_streams=-2),
           dict(W=0), dict(latency=-1), dict(n_cols=0), dict(n_cols=17), dict(gate=nan), dict(gate=inf), dict(gate=-inf),
           dict(gate=-1.0), dict(min_hits=0), dict(min_hits=-3), dict(max_coast=-1), dict(picks=None), dict(angles=None),
           dict(state=None), dict(track=None), dict(map=None, min_peak=0.25)]
    for kw in bad:
        assert call(**kw) == BF_EINVAL, kw
        assert NAME.encode() in lib.bf_last_error(None), kw
        assert call(n_blocks=0, **kw) == BF_EINVAL, kw   # the arguments are checked first
    assert call(n_blocks=0) == 0 and call(n_blocks=0, active=None) == 0
    # both ends of every range are inside
    assert call(n_blocks=0, n_angles=1, k=1, n_cols=1, gate=0.0, min_hits=1, max_coast=0, latency=0, W=1, map=None, min_peak=0.0) == 0
    assert call(n_blocks=0, n_angles=1024, k=16, n_cols=16, gate=1e300, min_hits=2 ** 31 - 1, max_coast=2 ** 31 - 1,
                latency=2 ** 31 - 1, W=2 ** 31 - 1, n_streams=2 ** 31 - 1, map=None, min_peak=-1.0) == 0
    with pytest.raises(capi.BfError) as e:
        capi.ctrack_assign_device(0, 0, ptr, 5, 2, 1, 4, 4, 1, 0.0, 20.0, 2, 8, 2, ptr, ptr)
    assert e.value.code == BF_EINVAL and NAME in str(e.value)


# ---- 2. doa_assign.hpp, compiled on its own --------------------------------------------------------------------------------------------
ASSIGN_SRC = r"""
#include "%s"
extern "C" void assign_all(const int32_t *picks, const double *map, const double *angles, int n_angles, int k, int n_streams, long n_blocks,
                           int W, int latency, double min_peak, double gate, int min_hits, int max_coast, int n_cols, int32_t *state,
                           int32_t *track, int32_t *active) {
    for (long s = 0; s < n_streams; ++s)
        bf::assign_stream(picks + s * n_blocks * k, map ? map + s * n_blocks * n_angles : nullptr, angles, n_angles, k, n_blocks, W, latency,
                          min_peak, gate, min_hits, max_coast, n_cols, state + s * n_cols * bf::kAssignStateInts,
                          track + s * n_blocks * W * n_cols, active + s * n_blocks * n_cols);
}
"""


@pytest.fixture(scope="module")
def hpp(tmp_path_factory):
    """doa_assign.hpp behind the signature of assign_ref.assign."""
    d = tmp_path_factory.mktemp("doa_assign")
    src, so = os.path.join(d, "assign.cpp"), os.path.join(d, "libassign.so")
    with open(src, "w") as f:
        f.write(ASSIGN_SRC % os.path.join(ROOT, "beamform_amd", "csrc", "doa_assign.hpp"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.assign_all.argtypes = [ip, dp, dp, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int,
                               C.c_int, ip, ip, ip]
    lib.assign_all.restype = None

    def fn(picks, maps, angles, W, latency, min_peak, gate, min_hits, max_coast, n_cols, state):
        picks = np.ascontiguousarray(picks, np.int32)
        S, nb, k = picks.shape
        ang = np.ascontiguousarray(angles, np.float64)
        m = None if maps is None else np.ascontiguousarray(maps, np.float64)
        st = np.ascontiguousarray(np.broadcast_to(np.asarray(state, np.int32), (S, n_cols, 4))).copy()
        track = np.full((S, nb * W, n_cols), -99, np.int32)
        active = np.full((S, nb, n_cols), -99, np.int32)
        lib.assign_all(picks.ctypes.data_as(ip), None if m is None else m.ctypes.data_as(dp), ang.ctypes.data_as(dp), ang.size, k, S, nb, W,
                       latency, float(min_peak), float(gate), min_hits, max_coast, n_cols, st.ctypes.data_as(ip), track.ctypes.data_as(ip),
                       active.ctypes.data_as(ip))
        return track, active, st
    return fn


def _ctl(picks, maps, angles, W, latency, min_peak, gate, min_hits, max_coast, n_cols, state):
    from beamform_amd.controllers import assign_sources
    S = np.asarray(picks).shape[0]
    st = np.broadcast_to(np.asarray(state, np.int32), (S, n_cols, 4))
    return assign_sources(picks, maps, angles, W, latency, min_peak, gate, min_hits, max_coast, n_cols, st)


def _same(a, b, what):
    for x, y, n in zip(a, b, ("track", "active", "state")):
        assert x.dtype == np.int32 and y.dtype == np.int32 and x.shape == y.shape, (what, n)
        assert np.array_equal(x, y), (what, n)


# ---- 3. three implementations agree --------------------------------------------------------------------------------------------------
def test_three_implementations_agree(hpp):
    """Every value the sweep lists turns up, the cases do what they are for (matches, coasting, freed slots, births, dropped candidates,
    publications withheld by min_peak), and the header's C++, the controller and the restatement give the same bytes."""
    seen = {n: set() for n in ("A", "grid", "kind", "k", "n_cols", "gate", "min_hits", "max_coast", "latency", "W", "nb", "with_map")}
    n_active = n_freed = n_moved = 0
    for c in assign_ref.sweep():
        for n in seen:
            seen[n].add(c[n])
        picks, maps, angles, min_peak, state = assign_ref.case_input(c, 2)
        ref = assign_ref.run(assign_ref.assign, c, picks, maps, angles, min_peak, state)
        assert (ref[0] != -99).all() and ((ref[1] == 0) | (ref[1] == 1)).all()
        _same(assign_ref.run(hpp, c, picks, maps, angles, min_peak, state), ref, ("hpp", c))
        _same(assign_ref.run(_ctl, c, picks, maps, angles, min_peak, state), ref, ("controllers", c))
        n_active += int(ref[1].sum())
        n_freed += int(((state[..., 0] >= 0) & (state[..., 0] < c["A"]) & ~((ref[2][..., 0] >= 0) & (ref[2][..., 0] < c["A"]))).sum())
        n_moved += int((ref[0][:, 0] != ref[0][:, -1]).sum())
    assert seen["A"] == set(assign_ref.A_SET) and seen["grid"] == set(assign_ref.GRID_NAMES)
    assert seen["kind"] == set(assign_ref.KINDS) | {"slow"} and seen["with_map"] == {False, True}
    for n, s in (("k", assign_ref.K_SET), ("n_cols", assign_ref.C_SET), ("gate", assign_ref.GATE_SET), ("min_hits", assign_ref.HITS_SET),
                 ("max_coast", assign_ref.COAST_SET), ("latency", assign_ref.LAT_SET), ("W", assign_ref.W_SET), ("nb", assign_ref.NB_SET)):
        assert seen[n] == set(s), n
    assert n_active > 1000 and n_freed > 20 and n_moved > 50


def test_bad_picks_are_no_candidates(hpp):
    """Out-of-range picks (n_angles, -7, 2^31 - 1) and -1 holes: the same result as the rows with those places cut out."""
    A, k, nb = 9, 4, 30
    picks = assign_ref.pick_rows(2, nb, k, A, "bad", 3)
    assert (picks == A).any() and (picks == -7).any() and (picks == 2 ** 31 - 1).any()
    clean = np.full_like(picks, -1)
    for s in range(2):
        for b in range(nb):
            if 0 <= picks[s, b, 0] < A:  # an invalid first pick publishes nothing
                good = [p for p in picks[s, b] if 0 <= p < A]
                clean[s, b, :len(good)] = good
    angles = picks_ref.grids(A)["sorted"]
    args = (None, angles, 2, 1, 0.0, 50.0, 1, 2, 3, -1)
    _same(hpp(picks, *args), hpp(clean, *args), "bad picks")
    _same(assign_ref.assign(picks, *args), hpp(clean, *args), "bad picks, ref")


# ---- 4. stated properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latency", [0, 1])
def test_a_stream_cut_anywhere_continues_exactly(hpp, latency):
    A, k, nb, W, n_cols = 24, 3, 13, 2, 3
    picks = assign_ref.slow_rows(2, nb, k, A, 11)
    maps = assign_ref.maps_for(2, nb, A, 11)
    angles = picks_ref.grids(A)["unsorted"]
    for fn in (hpp, assign_ref.assign, _ctl):
        one = fn(picks, maps, angles, W, latency, 0.3, 20.0, 2, 2, n_cols, -1)
        assert one[1].any() and len(np.unique(one[0][0, :, 0])) > 1
        for cut in range(nb + 1):
            a = fn(picks[:, :cut], maps[:, :cut], angles, W, latency, 0.3, 20.0, 2, 2, n_cols, -1)
            b = fn(picks[:, cut:], maps[:, cut:], angles, W, latency, 0.3, 20.0, 2, 2, n_cols, a[2])
            _same((np.concatenate([a[0], b[0]], axis=1), np.concatenate([a[1], b[1]], axis=1), b[2]), one, (latency, cut))


def test_a_slot_with_idx_out_of_range_is_free_whatever_its_counters(hpp):
    A, k, nb, n_cols = 12, 2, 9, 4
    picks = assign_ref.slow_rows(1, nb, k, A, 5)
    angles = picks_ref.grids(A)["sorted"]
    base = np.full((1, n_cols, 4), -1, np.int32)
    base[0, 1] = (7, 3, 0, 7)                    # one live, confirmed slot
    base[0, :, 3] = (5, 7, -1, 2)                # and an `out` per column: it is data, not part of "free"
    want = None
    for idx in (-1, A, A + 100, -2 ** 31, 2 ** 31 - 1):
        for hits, misses in ((-1, -1), (0, 0), (2 ** 30, 2 ** 31 - 1), (-2 ** 31, 5), (2 ** 31 - 1, -2 ** 31)):
            st = base.copy()
            st[0, (0, 2, 3), 0], st[0, (0, 2, 3), 1], st[0, (0, 2, 3), 2] = idx, hits, misses
            got = [fn(picks, None, angles, 1, 1, 0.0, 70.0, 1, 1, n_cols, st) for fn in (hpp, assign_ref.assign, _ctl)]
            _same(got[0], got[1], (idx, hits, misses))
            _same(got[2], got[1], (idx, hits, misses))
            born = (got[1][2][0, :, 0] >= 0) & (got[1][2][0, :, 0] < A)
            # compare what the contract defines: track, active, and the state of every slot that is live at the end
            view = (got[1][0], got[1][1], got[1][2][0][born])
            if want is None:
                want = view
                assert born[[0, 2, 3]].any()     # a birth into a slot that came in free
            for x, y in zip(view, want):
                assert np.array_equal(x, y), (idx, hits, misses)


def test_columns_keep_their_talkers_when_the_row_order_changes(hpp):
    """k talkers pairwise more than 2 x gate apart, every one in every block, in a row order that changes from block to block: with
    min_hits = 1 every column is constant after block 0.  The older builder's columns are not -- the input does exercise the swap."""
    A, k, nb, W, gate = 36, 4, 20, 2, 10.0
    angles = picks_ref.grids(A)["unsorted"]
    talkers = np.array([int(np.flatnonzero(angles == v)[0]) for v in np.sort(angles)[[2, 9, 18, 30]]])
    d = picks_ref.sep(angles[talkers][:, None], angles[talkers][None, :])
    assert (d[~np.eye(k, dtype=bool)] > 2 * gate).all()
    rng = np.random.default_rng(77)
    picks = np.stack([talkers[rng.permutation(k)] for _ in range(nb)]).astype(np.int32)[None]
    assert len({tuple(r) for r in picks[0]}) > 5
    for fn in (hpp, assign_ref.assign, _ctl):
        track, active, state = fn(picks, None, angles, W, 0, 0.0, gate, 1, 0, k, -1)
        assert np.array_equal(track[0], np.tile(picks[0, 0], (nb * W, 1)))   # column c is the talker block 0 put there
        assert active.all() and np.array_equal(state[0, :, 0], picks[0, 0]) and (state[0, :, 1] == nb).all()
    old, _ = picks_ref.from_picks(picks, None, A, W, 0, 0.0, k, -1)
    assert all(len(np.unique(old[0, :, c])) > 1 for c in range(k))


# ---- 5. the conversation, on the restatement map ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_picks():
    import doa_capon_ref
    from beamform_amd.params import AIRA16_XY
    x = assign_ref.scene_audio()
    P, _ = doa_capon_ref.capon_map(x, AIRA16_XY[:assign_ref.SCENE_M], 512, 48000.0, assign_ref.SCENE_GRID, 100.0, 16000.0,
                                   assign_ref.SCENE_W, 1e-3)
    picks = picks_ref.pick_all(P, assign_ref.SCENE_GRID, *assign_ref.SCENE_PICK)
    picks.setflags(write=False)
    return picks


def test_scene_columns_are_talkers(hpp, scene_picks):
    g, nb, W = assign_ref.SCENE_GRID, 10, assign_ref.SCENE_W
    assert (g[assign_ref.I20], g[assign_ref.IM60], g[assign_ref.I110]) == (20.0, -60.0, 110.0)
    assert scene_picks.shape == (nb, 3)
    assert [[int(p) for p in row if p >= 0] for row in scene_picks] == assign_ref.SCENE_PICKS
    p = assign_ref.SCENE_ASSIGN
    for fn in (assign_ref.assign, hpp, _ctl):
        track, active, state = fn(scene_picks[None], None, g, W, p["latency"], 0.0, p["gate"], p["min_hits"], p["max_coast"], p["n_cols"], -1)
        assert np.array_equal(assign_ref.outs_of(track[0], state[0], W), np.array(assign_ref.SCENE_OUT))
        assert (track[0, :2 * W] == -1).all()
        assert np.array_equal(track[0, 2 * W:], np.tile([assign_ref.I20, assign_ref.IM60, -1], ((nb - 2) * W, 1)))
        assert np.array_equal(active[0], np.array(assign_ref.SCENE_ACTIVE))
    # the older builder on the same picks: column 0, the look direction, goes over to the other talker at block 3
    old, _ = picks_ref.from_picks(scene_picks[None], None, g.size, W, 1, 0.0, 3, -1)
    col0 = old[0, ::W, 0]
    assert list(col0[:4]) == [-1, assign_ref.I20, assign_ref.I20, assign_ref.IM60] and col0[7] == assign_ref.I20
    assert old[0, 9 * W, 1] == assign_ref.I110     # and the pausing talker's column is taken over


# ---- 6. sanitizers: a stand-alone program, host only -----------------------------------------------------------------------------------
SAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "%s"
// reads cases written by the test: a header of ints and doubles, then picks, angles, (map), state; writes track, active, state
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    long n_cases = 0;
    if (std::fread(&n_cases, sizeof n_cases, 1, f) != 1) return 2;
    for (long i = 0; i < n_cases; ++i) {
        long h[10];
        double g[2];
        if (std::fread(h, sizeof h, 1, f) != 1 || std::fread(g, sizeof g, 1, f) != 1) return 2;
        const long S = h[0], nb = h[1], k = h[2], A = h[3], W = h[4], lat = h[5], min_hits = h[6], max_coast = h[7], C = h[8], with_map = h[9];
        std::vector<int32_t> picks(S * nb * k), state(S * C * 4), track(S * nb * W * C), active(S * nb * C);
        std::vector<double> angles(A), map(with_map ? S * nb * A : 0);
        if (std::fread(picks.data(), 4, picks.size(), f) != picks.size() || std::fread(angles.data(), 8, A, f) != (size_t)A) return 2;
        if (with_map && std::fread(map.data(), 8, map.size(), f) != map.size()) return 2;
        if (std::fread(state.data(), 4, state.size(), f) != state.size()) return 2;
        for (long s = 0; s < S; ++s)
            bf::assign_stream(picks.data() + s * nb * k, with_map ? map.data() + s * nb * A : nullptr, angles.data(), (int)A, (int)k, nb, (int)W,
                              (int)lat, g[0], g[1], (int)min_hits, (int)max_coast, (int)C, state.data() + s * C * 4,
                              track.data() + s * nb * W * C, active.data() + s * nb * C);
        std::fwrite(track.data(), 4, track.size(), o);
        std::fwrite(active.data(), 4, active.size(), o);
        std::fwrite(state.data(), 4, state.size(), o);
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
"""


def test_assign_hpp_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """assign_block over the generated cases in a program of its own, built with -fsanitize=address,undefined and run directly:
    exact-size buffers, so a read or a write past an end, or an overflowing counter, ends the program."""
    src, exe = tmp_path / "assign_san.cpp", tmp_path / "assign_san"
    src.write_text(SAN_MAIN % os.path.join(ROOT, "beamform_amd", "csrc", "doa_assign.hpp"))
    built = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    cases = assign_ref.sweep()[::2]
    want = []
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(cases)], np.int64).tobytes())
        for c in cases:
            picks, maps, angles, min_peak, state = assign_ref.case_input(c, 2)
            f.write(np.array([2, c["nb"], c["k"], c["A"], c["W"], c["latency"], c["min_hits"], c["max_coast"], c["n_cols"],
                              int(maps is not None)], np.int64).tobytes())
            f.write(np.array([min_peak, c["gate"]], np.float64).tobytes())
            f.write(np.ascontiguousarray(picks, np.int32).tobytes() + np.ascontiguousarray(angles, np.float64).tobytes())
            if maps is not None:
                f.write(np.ascontiguousarray(maps, np.float64).tobytes())
            f.write(np.ascontiguousarray(state, np.int32).tobytes())
            want.append(b"".join(np.ascontiguousarray(v, np.int32).tobytes()
                                 for v in assign_ref.run(assign_ref.assign, c, picks, maps, angles, min_peak, state)))
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    assert (tmp_path / "out.bin").read_bytes() == b"".join(want)
