"""The cases of tests/param_cases.py are worth running (no GPU), shown on the oracle alone: every parameter a case is named for moves
the oracle's output by at least 1e-3 -- 100 times the parity bar -- when it alone goes back to its launch value, and so does swapping
the two values of a twin pair; the oracle's two restatements (C++ and numpy, different FFTs) agree on the case to 1e-9, so no
thresholded decision of the case sits on a rounding tie; the output is finite where the existing tests expect it and busy enough;
and chain_decide names the kernels the table names.

`python tests/test_params_cpu.py [case ...]` prints the measured figures that param_cases.py quotes."""
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import param_cases as pc
from chain_plan_util import chain_kernels, params_plan
from conftest import rel_l2

N_CUS = 256
SENS = 1e-3           # 100 times the parity bar of 1e-5 (the margin of tests/gsc_cases.py)
O2O = 1e-9
# one representative per oracle run: the two precisions and the tile lengths of a shape share scene, parameters and therefore figures
REPS = {}
for _c in pc.CASES:
    REPS.setdefault(pc.oracle_key(_c), _c.name)
IDS = list(REPS.values())
ALL = [c.name for c in pc.CASES]


def launch_value(c, key):
    return pc.make_params(c.algo, n_mics=c.M, interf=c.interf)[key]


def distance(a, b):
    """Relative L2 between two outputs [rows, T] over the samples both leave finite (mvdr / lcmv: the window still filling)."""
    ok = np.isfinite(a) & np.isfinite(b)
    assert ok.mean() > 0.3      # (three frames behind a non-finite first one: the last hop alone)
    return 0.0 if np.array_equal(a[ok], b[ok]) else rel_l2(a[ok], b[ok])


def inband(p):
    from oracle import np_oracle
    f = np.abs(np_oracle.freq_vector(2 * p["hop"], p["sample_rate"]))
    band = np.ones(len(f), bool) if p["algo"] in ("phasempf", "mcra") else (f >= p["freq_min"]) & (f <= p["freq_max"])
    band[0] = False
    return band


@functools.lru_cache(maxsize=None)
def measured(name):
    """Every oracle-side figure of a case (stream 0), computed once."""
    from oracle import np_oracle
    c = pc.BY_NAME[name]
    p = pc.params(c)
    y, Y = pc.reference(c)
    sens = {k: distance(pc.reference(c, **{k: launch_value(c, k)})[0], y) for k in c.named}
    swaps = {}
    for a, b in pc.TWINS:
        if a in c.named and b in c.named and c.over[a] != c.over[b]:
            swaps[f"{a}<->{b}"] = distance(pc.reference(c, **{a: c.over[b], b: c.over[a]})[0], y)
    # the numpy restatement, wherever it implements what the case runs: the plain node, and row 0 of the unfiltered gss rows
    o2o = None
    e = c.extra
    if not (e.get("track") or e.get("dirs") or e.get("pf")):
        if e.get("rows"):
            import oracle
            y2, Y2 = oracle.OracleNode(p).process(pc.scene(c)[0], want_spectrum=True)
            y1, Y1 = y[0], Y[0]
        else:
            y2, Y2 = np_oracle.process(p, pc.scene(c)[0])
            y1, Y1 = y[0], (None if Y is None else Y[0])
        if Y1 is None:
            assert np.array_equal(np.isfinite(y1), np.isfinite(y2))
            o2o = distance(y1[None], y2[None])
        else:
            fin = np.isfinite(Y1).all(axis=1)
            assert np.array_equal(fin, np.isfinite(Y2).all(axis=1)), "the restatements disagree on which frames are finite"
            o2o = max([rel_l2(Y1[t], Y2[t]) for t in range(c.F) if fin[t] and np.abs(Y1[t]).max() > 0] + [0.0])
    busy = None
    if Y is not None and (c.algo in ("phasempf", "mcra") or e.get("pf")) and not p["out_only_noise"]:
        a = np.abs(Y[0][:, inband(p)])
        floor = p["noise_floor"] if c.algo != "mcra" else 0.0
        busy = float(((a > 0) & (np.abs(a - floor) > 1e-9 * max(floor, 1e-30))).mean())
    fin_frames = None if Y is None else np.isfinite(Y).all(axis=2).all(axis=0)
    return dict(sens=sens, swaps=swaps, o2o=o2o, busy=busy, finite=bool(np.isfinite(y).all()), fin_frames=fin_frames,
                finite_share=float(np.isfinite(y).mean()))


def fmt(name):
    m = measured(name)
    parts = [f"{k} {v:.1e}" for k, v in {**m["sens"], **m["swaps"]}.items()]
    parts += [f"o2o {m['o2o']:.0e}"] if m["o2o"] is not None else []
    parts += [f"busy {m['busy']:.2f}"] if m["busy"] is not None else []
    return f"{name}: " + " ".join(parts)


@pytest.mark.parametrize("name", IDS)
def test_every_named_key_moves_the_oracle(name):
    m = measured(name)
    print(fmt(name))
    c = pc.BY_NAME[name]
    assert set(m["sens"]) == set(c.named)
    for k, d in {**m["sens"], **m["swaps"]}.items():
        assert d >= SENS, (name, k, d)


def test_the_recursion_cases_swap_every_twin():
    """The cases named for the whole recursion set carry all three twin pairs (mcra's node has no mpf_alphaS: two)."""
    for c in pc.CASES:
        if set(pc.MPF) <= set(c.named) or set(pc.GPF) <= set(c.named):
            assert len(measured(REPS[pc.oracle_key(c)])["swaps"]) == 3, c.name
        if c.algo == "mcra":
            assert len(measured(REPS[pc.oracle_key(c)])["swaps"]) == 2, c.name


@pytest.mark.parametrize("name", IDS)
def test_no_near_ties(name):
    m = measured(name)
    if m["o2o"] is None:
        c = pc.BY_NAME[name]
        assert c.extra.get("track") or c.extra.get("dirs") or c.extra.get("pf")   # driven hop by hop / filtered: one statement only
        return
    assert m["o2o"] <= O2O, (name, m["o2o"])


@pytest.mark.parametrize("name", IDS)
def test_output_is_not_degenerate(name):
    c = pc.BY_NAME[name]
    m = measured(name)
    if c.algo in ("mvdr", "lcmv"):
        # what tests/test_hops_gpu.py's check() tolerates: frames the oracle itself leaves non-finite (the inverse of the empty or
        # rank-deficient covariance of the first frames), matched frame by frame on the device; most of the batch must be finite
        assert m["fin_frames"][1:].any(), "no finite frame to compare"
        if c.F > 3:
            assert m["fin_frames"].mean() >= 0.5, m["fin_frames"]
    else:
        assert m["finite"]
    if m["busy"] is not None:
        assert m["busy"] >= 0.10, m["busy"]


def twin_of(k):
    """The kernels chain_decide does not name itself: the launcher swaps in the track / all-rows twin of the planned kernel
    (chain_plan.hpp: ChainPlan::track, ctrack, rows), and the post-filter and das have plans of their own."""
    if "das_" in k or "gss_postfilter_kernel" in k:
        return None
    return (k.replace("stft_bins_w64_track_kernel", "stft_bins_w64_kernel").replace("_track_kernel", "_kernel")
            .replace("gss_kernel_all<", "gss_kernel<").replace("gss_lane_kernel_all<", "gss_lane_kernel<"))


@pytest.mark.parametrize("name", ALL)
def test_plan_names_the_kernels_of_the_table(emul_lib, name):
    c = pc.BY_NAME[name]
    assert set(c.env) <= {"BF_MVDR_GROUP", "BF_GSS_GROUP", "BF_MVDR_TILE"}
    if c.algo == "das":
        assert all("das_" in k for k in c.kernels)     # das in double / fused fp32: no chain (tests/test_das_f64_plan_gpu.py, test_das_gpu.py)
        return
    sw = {}
    if "BF_MVDR_GROUP" in c.env:
        sw["mvdr_group"] = int(c.env["BF_MVDR_GROUP"])
    if "BF_GSS_GROUP" in c.env:
        sw["gss_group"] = int(c.env["BF_GSS_GROUP"])
    if c.extra.get("offset"):
        sw["aligned16"] = False
    d = params_plan(emul_lib, pc.params(c), c.F, N_CUS, layout=c.layout, streams=c.streams, dirs=c.extra.get("dirs", 1),
                    mixed=c.precision == pc.MIXED, **sw)
    plan = chain_kernels(d, 2 * c.hop)
    for k in c.kernels:
        t = twin_of(k)
        assert t is None or t in plan, (k, plan)


def test_the_table_covers_what_it_set_out_to():
    """Every smoothing instantiation, every window length on every covariance kernel, both precisions."""
    ks = {k.split("::")[-1] for c in pc.CASES for k in c.kernels}
    for sz in (1, 2, 4, 5, 6, 8):
        assert f"smooth4_kernel<{sz}>" in ks
    assert "smooth_kernel" in ks
    for P in (1, 2, 3, 11, 64):
        for z in ("true", "false"):
            for k in (f"mvdr_fast_kernel<8, 1, {z}>", f"mvdr_fast_kernel<4, 2, {z}>", f"mvdr_fast_kernel<8, 3, {z}>", f"mvdr_fast_kernel<6, 1, {z}>",
                      f"cov2d_kernel<1, 3, {z}>", f"cov2d_kernel<4, 2, {z}>", f"mvdr_fast_track_kernel<8, 1, {z}>"):
                assert any(c.over.get("past_windows") == P and any(k in n for n in c.kernels) for c in pc.CASES), (P, k)
    for c in pc.CASES:
        assert len(c.env) <= 2 and c.F * c.hop <= 8192 or c.streams == 64


if __name__ == "__main__":
    for name in sys.argv[1:] or IDS:
        print(fmt(name), flush=True)
