"""The launch geometry of the chain (csrc/chain_geom.hpp: band_plan, chain_geom and the item formulas of the kernels) on the CPU, through
tests/host_emul's emul_band_plan / emul_chain_geom / emul_chain_cover:
  A. field for field equal to the arithmetic the launchers carried before it moved (tests/chain_geom_ref.py), on seeded random shapes;
  B. invariants of every partition on the same shapes: exact cover, run-length shapes, limits, mvdr_fast_kernel inside its workspace,
     the fused front inside its workspaces, rows read against rows written."""
import ctypes as C

import numpy as np
import pytest

import chain_geom_ref as ref
from chain_plan_util import ALGO, CHAIN_SWITCHES, NODES, PLAN

SHAPE = ("algo", "n_fft", "layout", "n_mics", "n_streams", "n_dirs", "kp1", "past_windows", "precision", "dump", "n_frames", "n_cus",
         "gsc_filter_size", "smooth_size", "band_yh_lo", "band_yh_hi", "aligned16") + tuple(CHAIN_SWITCHES) + (
         "gss_rows", "track", "ctrack_cols", "gss_postfilter", "lcmv_rows", "mvdr_tile")                       # ChainShape's order
BAND = ("skip_lo", "skip_hi", "yh_lo", "yh_hi", "q_lo", "n_main", "n_extra", "extra_q0", "extra_q1", "solve0", "nb", "ok")
PLAN_X = PLAN + ("rows", "track", "ctrack", "postfilter", "post_rp", "_0", "_1")
GEOM = ("ok", "run_len", "stft_blocks", "fpr", "rps", "total", "rpb", "fused_grid", "tail_blocks", "ew_blocks", "lane_blocks", "rec_blocks",
        "expand_blocks", "tile", "tps", "gx", "gy", "cov2d_grid", "fp_q_lo", "fp_n_main", "fp_n_extra", "fp_extra_q0", "fp_extra_q1",
        "fp_solve0", "fp_nb", "fp_tile", "fp_tiles", "fp_wps", "fast_grid", "fast_km", "wpc", "zero", "gss_grid", "per_run",
        "runs_per_stream", "istft_grid", "ola_grid", "smooth_grid", "smooth4_grid", "state_grid", "lds_serial", "lds_par", "nlms_grid")
# emul_chain_cover's out[], stage by stage.  `ok`: 1 = the items of every stream, in index order, tile its frames without gap or overlap (and
# the stage's own structure holds: see below), 0 = they do not, -1 = nothing to walk (no such stage, a generic kernel, an invalid geometry).
# `items`: indices walked; `dropped`: those of them the kernel's own guard drops.
#   front   fused fronts: rounds, block by block (a block without a round clears ok).  stft / stft_small / stft_wave2048: runs, the pairs of a
#           run checked against each other, counted once per run.  Never dropped.
#   bins    mvdr_lcmv_kernel: blockIdx.x = (stream, tile); never dropped.
#           cov2d_kernel: items = ALL blocks of the grid, dropped = blocks whose unit lies behind the last one; every live unit must meet its
#           problem groups once each and in order.
#           mvdr_fast_kernel: lanes of the FIRST and the LAST stream only (fast_streams = 1 or 2 says how many were walked), dropped = the dead
#           lanes behind their last (tile, problem); every live lane is checked against (tile, slot) = divmod(id, nb), the tiles of slot 0
#           must tile the stream.  The wavefronts of the streams in between: lanes 0 and 63, stream and prefetch bound only.
#           fast_hi = the highest frame index any visited lane prefetches, dead lanes included (-1: another kernel).
#   istft   istft32_kernel / istft_w64_kernel: every chunk / run slot of the grid (8 / 4 per block), dropped = those behind the last stream;
#           the w64 walk counts frame PAIRS.  istft_small_kernel / istft_split_kernel: streams x ceil(frames / L) runs, never dropped.
COVER = ("front_ok", "front_items", "front_dropped", "bins_ok", "bins_items", "bins_dropped", "fast_hi", "istft_ok", "istft_items",
         "istft_dropped", "fast_streams", "_")
SR = 48000.0
N_SHAPES = 2400


def _longs(names, d):
    return (C.c_long * len(names))(*[int(d[k]) for k in names])


def band_plan(lib, N, fmin, fmax, algo, sr=SR):
    out = (C.c_long * len(BAND))()
    lib.emul_band_plan.restype = None
    lib.emul_band_plan.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.emul_band_plan(N, sr, fmin, fmax, algo, out)
    return dict(zip(BAND, out))


def chain_geom(lib, shape, band):
    out = (C.c_long * (len(PLAN_X) + len(GEOM)))()
    lib.emul_chain_geom.restype = None
    lib.emul_chain_geom.argtypes = [C.c_void_p] * 3
    lib.emul_chain_geom(_longs(SHAPE, shape), _longs(BAND, band), out)
    v = list(out)
    return dict(zip(PLAN_X, v[:len(PLAN_X)])), dict(zip(GEOM, v[len(PLAN_X):]))


def chain_cover(lib, shape, band):
    out = (C.c_long * len(COVER))()
    lib.emul_chain_cover.restype = None
    lib.emul_chain_cover.argtypes = [C.c_void_p] * 3
    lib.emul_chain_cover(_longs(SHAPE, shape), _longs(BAND, band), out)
    return dict(zip(COVER, out))


def _log_int(rng, hi):
    """1 .. hi, log-uniform: small and large values alike, and the walks stay quick."""
    return int(min(hi, max(1, round(float(np.exp(rng.uniform(0.0, np.log(hi + 0.5))))))))


def random_shapes():
    """Seeded: all eight nodes, every hop 64 ... 4096, 1-32 microphones (gsc <= 16), 1-16 columns, both precisions, dump on / off, 1-300
    streams, 1-304 CUs, 1-70 000 frames, random bands (empty ones, ones that reach the Nyquist problems), lcmv_rows / gss_rows above 1,
    tracked and column-tracked batches, forced tiles 0, 1, 5, 7, 512, every switch of the chain off its default now and then."""
    rng = np.random.default_rng(2031)
    shapes = []
    for i in range(N_SHAPES):
        algo = NODES[i % 8]
        a = ALGO[algo]
        hop = int(2 ** rng.integers(6, 13))
        N = 2 * hop
        # the tuned microphone counts (<= 8: the lane kernels, the fused fronts) as often as the rest
        M = int(rng.integers(1, 9)) if rng.integers(0, 2) else int(rng.integers(1, 17 if algo == "gsc" else 33))
        kp1 = int(rng.integers(1, 17) if rng.integers(0, 2) else rng.integers(1, 5)) if algo in ("lcmv", "gss") else 1
        dirs = int(rng.integers(2, 5)) if algo != "gsc" and rng.integers(0, 4) == 0 else 1
        S = _log_int(rng, 300) if rng.integers(0, 4) else int(rng.integers(1, 301))
        F = _log_int(rng, 70000)
        if i % 97 == 0:
            F = int(rng.integers(60000, 70001))
        # the band: [fmin, fmax] inside the spectrum, from 0 Hz (problems 0 and N/2), up to Nyquist and beyond (problems N/2-1, N/2+1), empty
        kind = int(rng.integers(0, 6))
        fmin = 0.0 if kind == 0 else float(rng.uniform(0.0, SR / 2))
        fmax = {0: float(rng.uniform(fmin, SR / 2)), 1: SR / 2, 2: 30000.0, 3: fmin - 1.0}.get(kind, float(rng.uniform(fmin, SR / 2)))
        if kind == 5:
            fmin, fmax = 0.0, SR / 2
        rows = int(rng.integers(2, 17)) if rng.integers(0, 3) == 0 else 1
        tracked = dirs == 1 and rng.integers(0, 4) == 0
        sw = dict(CHAIN_SWITCHES)
        if rng.integers(0, 3) == 0:
            sw.update(fused_bins=int(rng.integers(0, 2)), stft_small=int(rng.integers(0, 2)), stft_split=int(rng.integers(0, 2)),
                      mvdr_group=int(rng.integers(0, 2)), gss_group=int(rng.integers(-1, 2)), gsc_serial=int(rng.integers(0, 2)))
        shapes.append((dict(algo=a, n_fft=N, layout=int(rng.integers(0, 2)), n_mics=M, n_streams=S, n_dirs=dirs, kp1=kp1,
                            past_windows=int(rng.integers(1, 65)), precision=int(rng.integers(0, 2)), dump=int(rng.integers(0, 2)),
                            n_frames=F, n_cus=int(rng.integers(1, 305)), gsc_filter_size=int(rng.integers(1, 257)),
                            smooth_size=int(rng.integers(1, 65)), aligned16=int(rng.integers(0, 4) != 0), **sw,
                            gss_rows=rows if algo == "gss" else 1, track=int(tracked and algo in ("das", "phase", "phasempf")),
                            ctrack_cols=int(rng.integers(1, kp1 + 1)) if tracked and algo in ("mvdr", "lcmv") else 0,
                            gss_postfilter=int(algo == "gss" and rng.integers(0, 2)), lcmv_rows=rows if algo == "lcmv" else 1,
                            mvdr_tile=int(rng.choice([0, 0, 0, 1, 5, 7, 512]))), fmin, fmax))
    return shapes


@pytest.fixture(scope="module")
def batches(emul_lib):
    """Every random shape with its band, plan, geometry and walk (C++) and the reference's band and geometry (Python): computed once."""
    out = []
    for shape, fmin, fmax in random_shapes():
        b = band_plan(emul_lib, shape["n_fft"], fmin, fmax, shape["algo"])
        shape = dict(shape, band_yh_lo=b["yh_lo"], band_yh_hi=b["yh_hi"])
        p, g = chain_geom(emul_lib, shape, b)
        rb = ref.band(shape["n_fft"], SR, fmin, fmax, shape["algo"])
        out.append(dict(shape=shape, band=b, plan=p, geom=g, cover=chain_cover(emul_lib, shape, b), ref_band=rb, ref=ref.geom(shape, p, rb),
                        fmin=fmin, fmax=fmax))
    return out


@pytest.fixture(scope="module")
def valid(batches):
    """The shapes whose geometry fits the kernels' integers and the grid limits: all but the largest spectrum dumps of many rows."""
    return [t for t in batches if t["ref"][0]]


def _ctx(t):
    return {k: t[k] for k in ("shape", "fmin", "fmax", "band", "plan", "geom")}


# ---- A. equal to the parent's arithmetic ---------------------------------------------------------------------------------------------------

def test_one_band_scan_gives_what_the_three_scans_gave(batches):
    kinds = set()
    for t in batches:
        band_node = t["shape"]["algo"] in (ref.MVDR, ref.LCMV, ref.GSS)
        names = BAND if band_node else BAND[:4]          # FastPlan's part means nothing outside mvdr / lcmv / gss
        assert {k: t["band"][k] for k in names} == {k: t["ref_band"][k] for k in names}, _ctx(t)
        b = t["band"]
        if band_node:
            N = t["shape"]["n_fft"]
            kinds.add(("empty" if b["nb"] == 1 else "main") + ("+extra%d" % b["n_extra"]) + ("+0Hz" if b["extra_q0"] == N // 2 else ""))
    assert {"empty+extra0", "main+extra0", "main+extra1", "main+extra2+0Hz"} <= kinds, kinds


def test_geometry_is_the_launchers_arithmetic_on_random_shapes(batches):
    assert len(batches) >= 2000
    seen = {k: set() for k in ("front", "bins", "istft", "tail", "zero", "mvdr_tile")}
    n_unfit = 0
    for t in batches:
        fits, want = t["ref"]
        g, p = t["geom"], t["plan"]
        assert g["ok"] == int(fits), (_ctx(t), want)
        if not fits:          # (the largest dumps of many rows: expand_spectrum_kernel's grid.x; the limits have their own test below)
            assert all(v == 0 for v in g.values()), _ctx(t)
            n_unfit += 1
            continue
        assert {k: g[k] for k in GEOM[1:]} == {k: want.get(k, 0) for k in GEOM[1:]}, (_ctx(t), want)
        for k in ("front", "bins", "istft", "tail"):
            seen[k].add(p[k])
        if p["bins"] == ref.B_MVDR_FAST:
            seen["zero"].add(g["zero"])
            seen["mvdr_tile"].add(t["shape"]["mvdr_tile"])
    assert seen["front"] == set(range(7)) and seen["bins"] == set(range(10)) and seen["istft"] == set(range(6)), seen
    assert seen["tail"] == set(range(6)) and seen["zero"] == set(range(3)) and seen["mvdr_tile"] == {0, 1, 5, 7, 512}, seen
    assert len(batches) - n_unfit >= 2000


def test_headline_mvdr_shape_is_the_one_the_kernel_file_describes(emul_lib):
    """cov_kernels.hip: "65 536 frames, 340 problems: 1 020 wavefronts of 342 frames = one round" (8 microphones, make_params' band,
    256 CUs, one wavefront per SIMD: 1 024 slots).  One round of 342 + 12 frames costs less than two of 171 + 12, which is what the
    comment named before it was pinned here; the launchers' arithmetic (chain_geom_ref.py) has always chosen the former."""
    from beamform_amd.params import make_params
    pr = make_params("mvdr", n_mics=8)
    b = band_plan(emul_lib, 1024, pr["freq_min"], pr["freq_max"], ref.MVDR, pr["sample_rate"])
    shape = dict(algo=ref.MVDR, n_fft=1024, layout=0, n_mics=8, n_streams=1, n_dirs=1, kp1=1, past_windows=pr["past_windows"], precision=0,
                 dump=0, n_frames=65536, n_cus=256, gsc_filter_size=128, smooth_size=3, band_yh_lo=b["yh_lo"], band_yh_hi=b["yh_hi"],
                 aligned16=1, **CHAIN_SWITCHES, gss_rows=1, track=0, ctrack_cols=0, gss_postfilter=0, lcmv_rows=1, mvdr_tile=0)
    p, g = chain_geom(emul_lib, shape, b)
    assert p["bins"] == ref.B_MVDR_FAST and g["ok"] == 1
    assert (g["fp_nb"], g["fp_tile"], g["fp_tiles"], g["fp_wps"], g["fast_grid"], g["wpc"]) == (340, 342, 192, 1020, 1020, 4), g
    assert -(-g["fast_grid"] // (256 * g["wpc"])) == 1          # one round over the 4 x CUs slots
    fits, want = ref.geom(shape, p, ref.band(1024, pr["sample_rate"], pr["freq_min"], pr["freq_max"], ref.MVDR))
    assert fits and {k: g[k] for k in GEOM[1:]} == {k: want.get(k, 0) for k in GEOM[1:]}, (g, want)


# ---- B. invariants ---------------------------------------------------------------------------------------------------------------------------

def test_every_partition_covers_every_stream_and_frame_exactly_once(valid):
    """emul_chain_cover walks the items of every partition in index order through the header's formulas (chain_stft_item, chain_run_item,
    chain_w64_item: (stream, pair) units, chain_cov2d_block, chain_fast_lane) and checks that a stream's items tile its frames without gap
    or overlap.  No item is empty, except where the kernel's own guard drops it:
      istft32_kernel / istft_w64_kernel   chunks / runs behind the last stream's: the grid is whole blocks of 8 / 4 (`s < a.n_streams`)
      cov2d_kernel                        blocks of the units behind the last one: units come in eights (`unit >= tiles_per_stream * n_streams`)
      mvdr_fast_kernel                    the lanes behind a stream's last (tile, problem) pair (`live`)
    The generic kernels take one (stream, frame[, pair]) per item by division alone: nothing to walk."""
    walked = {k: 0 for k in ("front", "bins", "istft")}
    for t in valid:
        c, g, p, s = t["cover"], t["geom"], t["plan"], t["shape"]
        So = s["n_streams"] * (s["n_mics"] if s["algo"] == ref.GSC else s["n_dirs"])
        Si, NQ = So * p["rows"], s["n_fft"] // 2 + 2
        for k in walked:
            assert c[k + "_ok"] in (1, -1), (k, c, _ctx(t))
            walked[k] += c[k + "_ok"] == 1
        assert (c["front_ok"] == -1) == (p["front"] == ref.K_STFT_GENERIC), (c, _ctx(t))
        assert (c["bins_ok"] == 1) == (p["bins"] in (ref.B_MVDR_FAST, ref.B_COV2D, ref.B_MVDR_LCMV)), (c, _ctx(t))
        assert (c["istft_ok"] == 1) == (p["istft"] in (ref.I_W64, ref.I_F32, ref.I_SMALL, ref.I_SPLIT)), (c, _ctx(t))
        if c["front_ok"] == 1:
            assert c["front_dropped"] == 0, (c, _ctx(t))
        if p["bins"] == ref.B_MVDR_LCMV:
            assert c["bins_dropped"] == 0 and g["gy"] * (256 // p["mp"]) >= NQ, (c, _ctx(t))
        elif p["bins"] == ref.B_COV2D:
            n_grp = (NQ + 15) // 16
            assert c["bins_dropped"] == g["cov2d_grid"] - g["tps"] * So * n_grp and c["bins_dropped"] < 8 * n_grp, (c, _ctx(t))
        elif p["bins"] == ref.B_MVDR_FAST:
            assert c["bins_dropped"] == c["fast_streams"] * (64 * g["fp_wps"] - g["fp_tiles"] * g["fp_nb"]), (c, _ctx(t))
            assert 0 <= 64 * g["fp_wps"] - g["fp_tiles"] * g["fp_nb"] < 64, (c, _ctx(t))
        if p["istft"] == ref.I_F32:
            assert c["istft_dropped"] == 8 * g["istft_grid"] - g["runs_per_stream"] * Si < 8, (c, _ctx(t))
        elif p["istft"] == ref.I_W64:
            assert c["istft_dropped"] == 4 * g["istft_grid"] - g["runs_per_stream"] * Si < 4, (c, _ctx(t))
        elif c["istft_ok"] == 1:
            assert c["istft_dropped"] == 0 and 8 * g["istft_grid"] >= c["istft_items"], (c, _ctx(t))
    assert min(walked.values()) > 100, walked


def test_run_lengths_have_the_shape_their_kernels_need(valid):
    for t in valid:
        g, p, N = t["geom"], t["plan"], t["shape"]["n_fft"]
        if p["front"] == ref.K_STFT_SMALL:          # whole groups of 1024 / N frames
            assert g["run_len"] >= 1024 // N and g["run_len"] % (1024 // N) == 0, _ctx(t)
        if not p["fused"]:
            assert 1 <= g["run_len"] <= 256, _ctx(t)
        if p["istft"] == ref.I_SMALL:               # whole groups, at least four: a run recomputes one
            assert g["per_run"] % (1024 // N) == 0 and g["per_run"] >= 4 * (1024 // N), _ctx(t)
        if p["istft"] == ref.I_SPLIT:               # at least 8 frames: a run recomputes one
            assert g["per_run"] >= 8, _ctx(t)
        if p["bins"] == ref.B_MVDR_FAST:
            assert 1 <= g["fp_tile"] <= min(512, t["shape"]["n_frames"]), _ctx(t)


def test_grids_and_narrowed_values_stay_inside_their_limits(valid):
    grids = ("stft_blocks", "fused_grid", "tail_blocks", "ew_blocks", "lane_blocks", "rec_blocks", "expand_blocks", "gx", "cov2d_grid", "fast_grid",
             "gss_grid", "istft_grid", "ola_grid", "smooth_grid", "smooth4_grid", "state_grid", "nlms_grid")
    ints = ("run_len", "fpr", "tile", "tps", "fp_tile", "fp_tiles", "fp_wps", "per_run", "runs_per_stream")
    for t in valid:
        g, (_, want) = t["geom"], t["ref"]
        for k in grids:
            assert (1 <= g[k] <= ref.GX_MAX) if k in want else g[k] == 0, (k, _ctx(t))          # a grid the batch launches is >= 1
        assert 0 <= g["gy"] <= ref.GY_MAX and all(0 <= g[k] <= ref.INT_MAX for k in ints), _ctx(t)
        assert g["fp_tiles"] * g["fp_nb"] + 63 <= ref.INT_MAX, _ctx(t)


def _direct(emul_lib, algo, N, M, S, F, fmin=100.0, fmax=16000.0, **over):
    b = band_plan(emul_lib, N, fmin, fmax, algo)
    shape = dict(algo=algo, n_fft=N, layout=0, n_mics=M, n_streams=S, n_dirs=1, kp1=1, past_windows=10, precision=0, dump=0, n_frames=F,
                 n_cus=256, gsc_filter_size=128, smooth_size=3, band_yh_lo=b["yh_lo"], band_yh_hi=b["yh_hi"], aligned16=1, **CHAIN_SWITCHES,
                 gss_rows=1, track=0, ctrack_cols=0, gss_postfilter=0, lcmv_rows=1, mvdr_tile=0)
    shape.update(over)
    p, g = chain_geom(emul_lib, shape, b)
    return shape, b, p, g, ref.geom(shape, p, ref.band(N, SR, fmin, fmax, algo))


@pytest.mark.parametrize("what", ["fast_lanes", "ew_grid", "group_units", "w64_runs"])
def test_a_batch_outside_the_limits_is_invalid_and_nothing_else(emul_lib, what):
    """Shapes built at the limits: the last one that fits is the launchers' arithmetic, the first one that does not is invalid -- ok = 0 and
    every other field 0, so that nothing can be launched from it."""
    nb = 340          # make_params' band at N = 1024
    inside, outside = {
        # mvdr_fast_kernel's fp.tiles * fp.nb (+ 63: its id0 + lane) is an int: a forced tile of one frame, frame counts near 2^31 / nb
        "fast_lanes": (dict(algo=ref.MVDR, N=1024, M=8, S=1, F=(2**31 - 64) // nb, mvdr_tile=1),
                       dict(algo=ref.MVDR, N=1024, M=8, S=1, F=(2**31 - 64) // nb + 1, mvdr_tile=1)),
        # pointwise_bins_kernel: a thread per (stream, frame, problem), grid.x <= 2^31 - 1
        "ew_grid": (dict(algo=ref.PHASE, N=8192, M=16, S=300, F=440000), dict(algo=ref.PHASE, N=8192, M=16, S=300, F=450000)),
        # the group kernel's tiles_per_stream * n_streams is an int (and its grid.x)
        "group_units": (dict(algo=ref.MVDR, N=256, M=8, S=300, F=64 * ((2**31 - 1) // 300), mvdr_group=1),
                        dict(algo=ref.MVDR, N=256, M=8, S=300, F=64 * ((2**31 - 1) // 300 + 1), mvdr_group=1)),
        # istft_w64_kernel: one CU, many streams -- a stream is one run of all its pairs, pairs_per_run is an int
        "w64_runs": (dict(algo=ref.MCRA, N=1024, M=1, S=40, F=2 * (2**31 - 1), n_cus=1), dict(algo=ref.MCRA, N=1024, M=1, S=40, F=2 * 2**31, n_cus=1)),
    }[what]
    shape, _, p, g, (fits, want) = _direct(emul_lib, **inside)
    assert fits and g["ok"] == 1 and {k: g[k] for k in GEOM[1:]} == {k: want.get(k, 0) for k in GEOM[1:]}, (shape, p, g, want)
    shape, _, p, g, (fits, _) = _direct(emul_lib, **outside)
    assert not fits and all(v == 0 for v in g.values()), (shape, p, g)


def _fast_bytes_needed(shape, plan, hi):
    """Bytes of Z up to and including frame `hi` of the LAST input stream, history in front: ((S - 1) (P + F) + P + hi + 1) frames."""
    S, P, F, M, N = shape["n_streams"], shape["past_windows"], shape["n_frames"], shape["n_mics"], shape["n_fft"]
    return ((S - 1) * (P + F) + P + hi + 1) * ((M + 1) // 2) * N * (12 if plan["z48"] else 16)


def test_mvdr_fast_prefetch_stays_inside_its_workspace(valid, emul_lib):
    """Every lane of mvdr_fast_kernel prefetches frames tA0 + dt .. tA0 + dt + n_it - 1 of its stream (chain_fast_lane), its own tile being
    shorter or not: the highest of them, behind the history and the streams in front, must lie inside z_bytes -- the batch plus 512 frames
    of slack.  Also with forced tiles beyond the slack, which come back as 512."""
    n = 0
    for t in valid:
        if t["plan"]["bins"] == ref.B_MVDR_FAST:
            hi, F = t["cover"]["fast_hi"], t["shape"]["n_frames"]
            assert F - 1 <= hi < F + 512 and _fast_bytes_needed(t["shape"], t["plan"], hi) <= t["plan"]["z_bytes"], _ctx(t)
            n += 1
    assert n > 100
    for forced in (513, 600, 100000):
        for F in (1, 511, 512, 513, 700, 1025, 70000):
            for S, mixed in ((1, 0), (3, 1)):
                shape, b, p, g, (fits, want) = _direct(emul_lib, algo=ref.MVDR, N=1024, M=8, S=S, F=F, mvdr_tile=forced, precision=mixed)
                assert p["bins"] == ref.B_MVDR_FAST and fits and g["ok"] == 1 and g["fp_tile"] == min(512, F) == want["fp_tile"], (shape, g)
                c = chain_cover(emul_lib, shape, b)
                assert c["bins_ok"] == 1 and F - 1 <= c["fast_hi"] < F + 512, (shape, g, c)
                assert _fast_bytes_needed(shape, p, c["fast_hi"]) <= p["z_bytes"], (shape, g, c)


def test_fused_front_stays_inside_its_workspaces(valid):
    n = 0
    for t in valid:
        s, p = t["shape"], t["plan"]
        if p["fused"]:          # xtail = Z: [stream][frame][2][MP] complex doubles
            assert s["n_streams"] * s["n_frames"] * 2 * p["mp"] * 16 <= p["z_bytes"], _ctx(t)
            n += 1
        if s["algo"] == ref.PHASEMPF:          # aux: a double per (stream, frame, row slot) behind the f64x2 rows
            So, YS = s["n_streams"] * s["n_dirs"], s["n_fft"] // 2 + 4
            assert So * s["n_frames"] * YS * (16 + 8) <= p["yh_bytes"], _ctx(t)
    assert n > 100


def test_rows_the_backward_transform_reads_are_written_or_zeroed(valid):
    """mvdr / lcmv through mvdr_fast_kernel: the backward transform (and the spectrum dump) reads problem 0 and yh_lo .. yh_hi -- every
    problem unless the rows are band-limited.  The kernel writes the problems its FastPlan enumerates; what lies between must be covered by
    the zero-fill the geometry names, and where it names none the two sets are equal."""
    kinds = set()
    for t in valid:
        g, p = t["geom"], t["plan"]
        if p["bins"] != ref.B_MVDR_FAST:
            continue
        read = {0} | set(range(p["yh_lo"], p["yh_hi"] + 1))
        extra = [g["fp_extra_q0"], g["fp_extra_q1"]][:g["fp_n_extra"]]
        written = {0} | set(range(g["fp_q_lo"], g["fp_q_lo"] + g["fp_n_main"])) | set(extra)
        assert len(written) == g["fp_nb"] and max(written) < t["shape"]["n_fft"] // 2 + 2, _ctx(t)
        if g["zero"] == ref.Z_NONE:
            assert read == written, _ctx(t)
        else:          # the fill covers every row of the batch, in the format the backward transform reads
            assert written <= read and (g["zero"] == ref.Z_F32) == bool(p["yh32"]), _ctx(t)
        kinds.add((g["zero"], bool(p["band_rows"]), bool(p["yh32"])))
    assert {(ref.Z_NONE, True, False), (ref.Z_NONE, True, True), (ref.Z_NONE, False, True), (ref.Z_F64, False, False),
            (ref.Z_F32, False, True)} <= kinds, kinds
