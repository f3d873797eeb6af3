"""The gsc cases of tests/gsc_cases.py are worth running (no GPU): their plans are the kernels the table names, every NLMS instantiation
chain_decide can select is named by a case, the oracle's two restatements agree on every case ten times tighter than the bar the device
is held to, and the cancelling path is busy enough in every case that a wrong filter update cannot hide under that bar.

`python tests/test_gsc_cpu.py [case ...]` prints the measured figures that gsc_cases.py quotes."""
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gsc_cases as gc
from chain_plan_util import chain_kernels, chain_plan, dispatch_rows, params_plan
from conftest import rel_l2

N_CUS = 256           # the plan of a gsc batch does not depend on it
IDS = [c.name for c in gc.CASES]


def nlms_recursion(p, a):
    """oracle/np_oracle.py gsc_process from the aligned signals a [M, T] on, statement for statement, with counters:
    -> (out, upper beamformer, lop per sample, dict of counts, filters at the end)."""
    f32 = np.float32
    M, fs = p["n_mics"], p["gsc_filter_size"]
    T = a.shape[1]
    bm = np.zeros((max(M - 1, 0), fs), f32); flt = np.zeros_like(bm); lo = np.zeros(fs, f32)
    out, upper, lops = np.zeros(T, f32), np.zeros(T, f32), np.zeros(T, f32)
    n = dict(open=0, steps=0, b2=0, nonfinite=0)
    ratios = []
    mu0, mu_max = p["gsc_mu0"], p["gsc_mu_max"]
    with np.errstate(all="ignore"):
        for j in range(T):
            das = f32(0.0)
            for m in range(M):
                das = f32(das + a[m, j])
            o = f32(das / f32(M))
            upper[j] = o
            if M > 1:
                bm[:, :-1] = bm[:, 1:]
                bm[:, -1] = a[1:, j] - a[:-1, j]
                bo = np.cumsum(flt * bm, axis=1, dtype=f32)[:, -1]
                for i in range(M - 1):
                    o = f32(o - bo[i])
            lo[:-1] = lo[1:]; lo[-1] = o
            lop = f32(np.sqrt(f32(np.cumsum(lo * lo, dtype=f32)[-1] / f32(fs))))
            out[j] = o
            lops[j] = lop
            if lop < p["gsc_vad_threshold"] or not p["gsc_use_vad"]:
                n["open"] += 1
                for i in range(M - 1):
                    bp = f32(np.sqrt(f32(np.cumsum(bm[i] * bm[i], dtype=f32)[-1] / f32(fs))))
                    r = np.float64(mu0) * np.float64(bp) / np.float64(lop)
                    ratios.append(r)
                    n["steps"] += 1
                    if r < mu_max:
                        mu = f32(np.float64(mu0) / np.float64(lop))
                    else:
                        mu = f32(np.float64(mu0) / np.float64(bp))
                        n["b2"] += 1
                    if not np.isfinite(mu):
                        mu = f32(0.0)
                        n["nonfinite"] += 1
                    upd = flt[i] + f32(mu * o) * bm[i]
                    flt[i] = np.where(np.isnan(upd), f32(0.0), upd)
    n["ratios"] = np.asarray(ratios)
    return out, upper, lops, n, flt


@functools.lru_cache(maxsize=None)
def measured(name):
    """Every oracle-side figure of a case, computed once: both restatements and the instrumented recursion, per stream."""
    import oracle
    from oracle import np_oracle
    c = gc.BY_NAME[name]
    p = gc.params(c)
    xs = gc.scene(c)
    res = []
    for x in xs:
        y_cpp = oracle.OracleNode(p).process(x)[0]
        y_np = np_oracle.gsc_process(p, x)
        X = np_oracle.stft(p, x)
        w = np_oracle.steering(p, p["theta"])
        a = np.stack([np_oracle.istft_ola(p, np.conj(w[m]) * X[:, m, :]) for m in range(c.M)])
        y_in, upper, lops, n, flt = nlms_recursion(p, a)
        assert np.array_equal(y_in, y_np, equal_nan=True), "the instrumented copy is not np_oracle's recursion any more"
        T = len(y_cpp)
        res.append(dict(y_cpp=y_cpp, y_np=y_np, upper=upper, lops=lops, ratios=n["ratios"],
                        d=0.0 if np.array_equal(y_cpp, upper) else rel_l2(y_cpp, upper), o2o=0.0 if np.array_equal(y_np, y_cpp) else rel_l2(y_np, y_cpp),
                        open=n["open"] / T, b2=n["b2"] / max(n["steps"], 1), nf=n["nonfinite"] / max(n["steps"], 1),
                        tap=float(np.abs(flt).max()) if flt.size else 0.0))
    return res


def nlms_name(lib, M, fs, serial):
    d = chain_plan(lib, algo=7, n_fft=1024, n_mics=M, n_frames=4, n_cus=N_CUS, gsc_filter_size=fs, gsc_serial=serial)
    return chain_kernels(d, 1024)[-1].split("::")[1]


@pytest.mark.parametrize("name", IDS)
def test_plan_yields_the_kernels_of_the_table(emul_lib, name):
    c = gc.BY_NAME[name]
    assert set(c.env) <= {"BF_GSC_SERIAL"}
    d = params_plan(emul_lib, gc.params(c), c.F, N_CUS, layout=c.layout, streams=c.streams, gsc_serial=int(c.env.get("BF_GSC_SERIAL", "0")))
    assert chain_kernels(d, 2 * c.hop) == c.kernels


def test_every_selectable_nlms_instantiation_is_named_by_a_case(emul_lib):
    """chain_decide over M = 1 .. 16, filter sizes 1 .. 256, BF_GSC_SERIAL off / on: 27 instantiations, each launched by a named case;
    the wider deals of the 2- and 4-wavefront kernel that launch_gsc_nlms also instantiates are never selected."""
    sweep = {nlms_name(emul_lib, M, fs, serial) for M in range(1, 17) for fs in range(1, 257) for serial in (0, 1)}
    named = {c.kernels[-1].split("::")[1] for c in gc.CASES}
    assert sweep <= named, sorted(sweep - named)
    assert len(sweep) == 27, sorted(sweep)
    for kp in (1, 2, 4):
        for nw, nbl in ((4, 2), (4, 4), (2, 2), (2, 4), (2, 8)):
            assert f"gsc_nlms_mw_kernel<{nw}, {nbl}, {kp}>" not in sweep


def test_every_gsc_period_of_the_dispatch_table_has_a_case():
    rows = [r for r in dispatch_rows() if r[0].split(",")[0].strip() == "gsc" and not r[6].startswith("(refused")]
    assert {int(r[1]) for r in rows} == {64, 128, 256, 512, 1024, 2048, 4096}
    for r in rows:
        hit = [c for c in gc.CASES if c.hop == int(r[1]) and c.M == int(r[3]) and c.over["gsc_filter_size"] == 128 and not c.env
               and c.layout == gc.PLANAR]
        assert hit and all(" + ".join(c.kernels) == r[6] for c in hit), r


@pytest.mark.parametrize("name", IDS)
def test_oracle_agrees_with_itself(name):
    """The two restatements take the aligned signals through different FFTs, as the device does.  1e-6 -- a tenth of the device's bar --
    shows that no branch flips and diverges inside the case.  (Measured: the same bytes in every case of the table -- the transforms'
    1e-16 vanishes in the float32 rounding of the aligned signals.)"""
    for m in measured(name):
        assert np.array_equal(np.isfinite(m["y_np"]), np.isfinite(m["y_cpp"])) and np.isfinite(m["y_cpp"]).all()
        assert m["o2o"] < 1e-6, m["o2o"]


@pytest.mark.parametrize("name", IDS)
def test_the_canceller_is_working(name):
    """The output is at least 1e-3 (100 times the parity bar) away from the upper beamformer alone.  One microphone has no blocking
    branch: there the output IS the upper beamformer."""
    c = gc.BY_NAME[name]
    for m in measured(name):
        if c.M == 1:
            assert np.array_equal(m["y_np"], m["upper"])
            continue
        assert m["d"] >= 1e-3, m["d"]
        assert m["tap"] > 0.0 and m["open"] > 0.0


def test_the_dedicated_cases_take_the_rarer_branch():
    for name in gc.VAD_CASES:
        m = measured(name)[0]
        assert 0.2 <= m["open"] <= 0.8, (name, m["open"])
    for name in gc.BRANCH2_CASES:
        m = measured(name)[0]
        assert 0.1 <= m["b2"] <= 0.9, (name, m["b2"])
    m = measured(gc.ZEROS_CASE)[0]
    assert m["nf"] >= 0.1, m["nf"]                      # 0 / 0 and x / 0 step sizes, zeroed
    assert np.isfinite(m["y_cpp"]).all()


if __name__ == "__main__":
    import json
    out = {}
    for name in sys.argv[1:] or IDS:
        m = measured(name)[0]
        out[name] = {k: float(m[k]) for k in ("d", "o2o", "open", "b2", "nf", "tap")}
        q = np.quantile(m["lops"], [0.2, 0.35, 0.5, 0.65, 0.8])
        r = np.quantile(m["ratios"][np.isfinite(m["ratios"])], [0.1, 0.5, 0.9]) if len(m["ratios"]) else []
        print(name, json.dumps(out[name]), "lop quantiles", [float(f"{v:.4g}") for v in q], "mu0*bp/lop quantiles", [float(f"{v:.4g}") for v in r], flush=True)
    print("JSON " + json.dumps(out))
