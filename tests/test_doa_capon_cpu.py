"""Capon (MVDR) direction-of-arrival maps on the host: the two new symbols and their refusals, the float64 restatement
(tests/doa_capon_ref.py) against its loop-nest twin and a closed form, the greedy source picker, the multi-source claim on
restatement maps (where the SRP-PHAT map shows the strongest source's sidelobes), and the launch plan of the three methods
(doa_decide, beamform_amd/csrc/doa.hpp), compiled here with g++."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_capon_ref  # noqa: E402
import doa_ref  # noqa: E402

from beamform_amd.params import AIRA16_XY  # noqa: E402
from beamform_amd.synth import make_scene  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 48000.0
GRID2 = np.arange(-180.0, 180.0, 2.0)
BF_EINVAL = -22


def _ang_err(a, b):
    return np.abs((np.asarray(a) - b + 180.0) % 360.0 - 180.0)


def two_source_scene(M, seed):
    """20 degrees at 0.2 plus -60 degrees at 0.05, sensor noise 0.01, 32 frames of hop 512, no silent stretch."""
    return make_scene(M, 32, 512, SR, seed=seed, theta_s=20.0, interferers=(-60.0,), sigma_s=0.2, sigma_i=0.05, silent_frac=0.0)


# ---- 1. surface ------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_listed_exported_and_null_handle_refused():
    from beamform_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "bfcore.h")).read()
    declared = set(re.findall(r"\b(bf_[a-z_0-9]+)\s*\(", header))
    for n in ("bf_doa_set_method", "bf_doa_set_loading"):
        assert n in declared and n in capi.EXPORTS and hasattr(lib, n), n
    assert re.search(r"BF_DOA_SRP_PHAT\s*=\s*0\s*,\s*BF_DOA_CAPON\s*=\s*1", header)
    assert (capi.BF_DOA_SRP_PHAT, capi.BF_DOA_CAPON) == (0, 1)
    assert lib.bf_doa_set_method(None, 1) == BF_EINVAL      # no device is touched
    assert lib.bf_doa_set_loading(None, 1e-3) == BF_EINVAL


# ---- 2. the restatement against the loop nest ------------------------------------------------------------------------------------------
def test_restatement_matches_naive_loops():
    rng = np.random.default_rng(5)
    mics = AIRA16_XY[:3]
    x = rng.standard_normal((3, 4 * 64)).astype(np.float32)
    angles = [-120.0, -90.0, 0.0, 45.0, 170.0]
    P, pk = doa_capon_ref.capon_map(x, mics, 64, SR, angles, 3000.0, 9000.0, 2)
    Pn = doa_capon_ref.capon_map_naive(x, mics, 64, SR, angles, 3000.0, 9000.0, 2)
    assert P.shape == (2, 5)
    assert np.allclose(P, Pn, rtol=1e-12, atol=1e-12)
    assert np.array_equal(pk, np.argmax(Pn, axis=1))


# ---- 3. a closed form ------------------------------------------------------------------------------------------------------------------
def test_closed_form_one_frame_on_a_steering_vector():
    """One frame X = a(theta_0): R / tau = a a^H / M, a^H R~^-1 a = M / (1 + delta / M) by Sherman-Morrison, so the map at theta_0 is
    (1 + delta / M) / (1 + delta), the bound; everywhere the map lies in (0, 1]."""
    M, N = 6, 256
    mics = AIRA16_XY[:M]
    K = doa_ref.band_bins(N, SR, 500.0, 12000.0)
    angles = np.arange(-180.0, 180.0, 7.5)
    a = doa_ref.weights(mics, angles, N, SR, K)  # [D, M, K]
    d0 = 11
    for delta in (1e-3, 1e-2, 1.0):
        P = doa_capon_ref.capon_from_spectra(a[d0][None], a, 1, delta)
        assert P.shape == (1, len(angles))
        assert abs(P[0, d0] - (1 + delta / M) / (1 + delta)) <= 1e-12
        assert np.all(P > 0) and np.all(P <= 1.0)
        assert np.argmax(P[0]) == d0


# ---- 4. the picker ---------------------------------------------------------------------------------------------------------------------
def test_pick_sources_and_doa_sources():
    from beamform_amd.controllers import DoaSources, pick_sources
    ang = np.arange(-180.0, 180.0, 10.0)  # 36 angles
    row = np.zeros(36)
    row[[3, 20]] = 1.0                    # a tie: the lowest index first
    row[21] = 0.9                         # within 15 degrees of index 20: suppressed
    row[30] = 0.5
    assert pick_sources(row, ang, 3, 15.0) == [3, 20, 30]
    assert pick_sources(row, ang, 1, 15.0) == [3]
    assert pick_sources(row, ang, 3, 5.0) == [3, 20, 21]         # a smaller separation lets the neighbour through
    # circular separation across +-180: -180 and 170 are 10 degrees apart
    row = np.zeros(36)
    row[0], row[35], row[18] = 1.0, 0.8, 0.3
    assert pick_sources(row, ang, 2, 15.0) == [0, 18]
    assert pick_sources(row, ang, 2, 10.0) == [0, 35]            # a distance equal to min_sep is not "below" it
    # rel_floor: picks stop below rel_floor x the row's maximum
    assert pick_sources(row, ang, 3, 15.0, rel_floor=0.5) == [0]
    assert pick_sources(row, ang, 3, 15.0, rel_floor=0.3) == [0, 18]
    # k larger than the number of separable peaks: every angle ends up picked or suppressed
    flat = np.ones(36)
    assert pick_sources(flat, ang, 99, 90.0) == [0, 9, 18, 27]
    assert pick_sources(flat, ang, 99, 1000.0) == [0]
    assert pick_sources(row, ang, 0, 15.0) == []
    c = DoaSources(ang, 2, 15.0)
    assert c.on_map(row) == (-180.0, [0.0])
    assert DoaSources(ang, 3, 15.0, rel_floor=0.5).on_map(row) == (-180.0, [])
    assert DoaSources(ang, 2, 15.0, min_peak=1.5).on_map(row) is None
    assert DoaSources(ang, 2, 15.0, min_peak=1.0).on_map(row) == (-180.0, [0.0])  # not below min_peak: published


# ---- 5. the multi-source claim, on restatement maps --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_maps():
    out = {}
    for M in (8, 4):
        for seed in (40, 41):
            x = two_source_scene(M, seed)
            out[M, seed] = doa_capon_ref.srp_and_capon(x, AIRA16_XY[:M], 512, SR, GRID2, 100.0, 16000.0, 16)
    return out


def test_capon_map_finds_both_sources_where_srp_phat_does_not(scene_maps):
    from beamform_amd.controllers import pick_sources
    for (M, seed), (Ps, Pc) in scene_maps.items():
        assert Pc.shape == (2, 180) and np.all(Pc > 0) and np.all(Pc <= 1.0)
        for b in range(2):
            got = GRID2[pick_sources(Pc[b], GRID2, 2, 15.0)]
            for src in (20.0, -60.0):
                assert np.min(_ang_err(got, src)) <= 5.0, (M, seed, b, got)
    Ps, _ = scene_maps[8, 41]
    second = [GRID2[pick_sources(Ps[b], GRID2, 2, 15.0)[1]] for b in range(2)]
    assert all(_ang_err(s, -60.0) > 5.0 for s in second), second   # the strongest source's sidelobe outranks the weaker source


# ---- 6. the launch decisions -------------------------------------------------------------------------------------------------------------
PLAN_SRC = r"""
#define BF_DOA_PLAN_ONLY
#include "%s"
using namespace bf;
extern "C" void plan(int method, int M, int S, int nfft, int D, int nK, int W, long long F, long long *o) {
    const DoaPlan p = doa_decide(DoaShape{M, S, nfft, D, nK, W, (long)F}, method);
    const long long v[] = {p.method, (long long)p.path, p.mp, p.seg_bins, p.segments, p.ws_elems, p.chunk_blocks, p.chunk_frames,
                           p.grid_x, p.grid_y, p.grid_z, (long long)p.z_bytes, (long long)p.flags_bytes, (long long)p.part_bytes,
                           p.epart_offset, (long long)p.ws_bytes, (long long)p.table_bytes};
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = v[i];
}
"""
FIELDS = ("method path mp seg_bins segments ws_elems chunk_blocks chunk_frames grid_x grid_y grid_z z_bytes flags_bytes part_bytes "
          "epart_offset ws_bytes table_bytes").split()
SRP_PHAT, CAPON, MUSIC = 0, 1, 2


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("doa_plan")
    src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "libplan.so")
    with open(src, "w") as f:
        f.write(PLAN_SRC % os.path.join(ROOT, "beamform_amd", "csrc", "doa.hpp"))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.plan.argtypes = [C.c_int] * 7 + [C.c_longlong, C.POINTER(C.c_longlong)]
    lib.plan.restype = None

    def run(method, M, S, nfft, D, nK, W, F):
        o = (C.c_longlong * len(FIELDS))()
        lib.plan(method, M, S, nfft, D, nK, W, F, o)
        return dict(zip(FIELDS, o))
    return run


def test_launch_plan(plan):
    budget = 256 << 20
    for M in range(2, 33):
        for S, nfft, D, nK, W, F in ((1, 1024, 72, 339, 16, 65536), (3, 1024, 360, 509, 8, 32), (1, 256, 1, 37, 1, 1 << 20),
                                     (1, 4096, 8, 64, 4, 4), (2, 8192, 1024, 65, 1, 3), (1, 128, 72, 128, 5000, 10000)):
            NP = (M + 1) // 2
            # Capon and MUSIC: the work space per problem and the partial-sum columns differ, nothing else
            for method, ws_elems, cols in ((CAPON, M * (M + 1) // 2 + M, D), (MUSIC, M * (M + 1) // 2 + M + M * M, D + M)):
                p = plan(method, M, S, nfft, D, nK, W, F)
                case = (method, M, S, nfft, D, nK, W, F)
                assert p["method"] == method, case
                # the path by the microphone count alone
                assert p["path"] == (0 if M <= 8 else 1), case
                assert p["mp"] == (2 * NP if M <= 8 else 0), case
                assert p["ws_elems"] == (0 if M <= 8 else ws_elems), case
                # the segments by |K| alone: 64 bins each
                G = -(-nK // 64)
                assert (p["seg_bins"], p["segments"]) == (64, G), case
                # a chunk: whole blocks within the budget, at least one, at most the batch
                per_block = W * S * NP * nfft * 16 + G * S * cols * 8 + p["ws_elems"] * S * G * 64 * 16
                nb = max(1, min(budget // per_block, F // W))
                assert p["chunk_blocks"] == nb and p["chunk_frames"] == nb * W, case
                assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (G * nb, S, 1), case
                assert p["z_bytes"] == nb * W * S * NP * nfft * 16, case
                assert p["flags_bytes"] == 0, case
                assert p["part_bytes"] == G * S * nb * cols * 8, case
                assert p["ws_bytes"] == p["ws_elems"] * S * nb * G * 64 * 16, case
                assert p["table_bytes"] == D * M * nK * 16, case
                if nb > 1:
                    assert p["z_bytes"] + p["part_bytes"] + p["ws_bytes"] <= budget, case
                # MUSIC's eigenvalue sums lie behind the chunk's angle rows, and part_bytes covers both regions
                assert p["epart_offset"] == (G * S * nb * D if method == MUSIC else 0), case
                if method == MUSIC:
                    assert p["part_bytes"] == (p["epart_offset"] + G * S * nb * M) * 8, case
            # SRP-PHAT: frames within the budget, rounded down to whole blocks, at least one block, at most the batch
            p = plan(SRP_PHAT, M, S, nfft, D, nK, W, F)
            case = (SRP_PHAT, M, S, nfft, D, nK, W, F)
            G48 = -(-nK // 48)
            assert (p["method"], p["path"], p["ws_elems"], p["ws_bytes"], p["epart_offset"]) == (SRP_PHAT, 2, 0, 0, 0), case
            assert p["mp"] == (M if M in (2, 4, 8, 16) else 0), case
            assert (p["seg_bins"], p["segments"]) == (48, G48), case
            per_frame = S * (NP * nfft * 16 + G48 * D * 8 + 8)
            CF = budget // per_frame
            CF = min(max(CF - CF % W, W), F)
            assert p["chunk_frames"] == CF and p["chunk_blocks"] * W == CF, case
            assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (-(-CF // 64) * -(-D // 32), G48, S), case
            assert p["z_bytes"] == S * CF * NP * nfft * 16, case
            assert p["flags_bytes"] == S * (CF + 1) * 2 * 4, case
            assert p["part_bytes"] == G48 * S * CF * D * 8, case
            assert p["table_bytes"] == D * M * nK * 16, case
            if CF > W:
                assert CF * per_frame <= budget, case
    # the segment count does not move with anything but the method and |K|
    for method in (SRP_PHAT, CAPON, MUSIC):  # 130 bins: three segments of 48 as of 64
        assert {plan(method, M, S, 1024, D, 130, W, 64 * W)["segments"]
                for M in (2, 8, 9, 32) for S in (1, 4) for D in (1, 360) for W in (1, 16)} == {3}
    assert [plan(CAPON, 8, 1, 1024, 72, nK, 16, 64)["segments"] for nK in (1, 63, 64, 65, 128, 129, 511)] == [1, 1, 1, 2, 2, 3, 8]
    assert [plan(MUSIC, 8, 1, 1024, 72, nK, 16, 64)["segments"] for nK in (1, 63, 64, 65, 128, 129, 511)] == [1, 1, 1, 2, 2, 3, 8]
    assert [plan(SRP_PHAT, 8, 1, 1024, 72, nK, 16, 64)["segments"] for nK in (1, 47, 48, 49, 96, 97, 511)] == [1, 1, 1, 2, 2, 3, 11]
