"""das_f64_pair_kernel / das_f64_ring_kernel with the delay-structured gains (geometry.hpp das_sep_gains_w64_f64): against the oracle at
the tolerance of the other das-in-double tests (tests/test_fused_bins_gpu.py: relative L2 below 1e-6), and against the CPU restatement of
the new accumulation (tests/host_emul_sep) at 4 x the CPU's own figure for new form against table form (das_sep_util.SEP_VS_TABLE_BOUND)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from beamform_amd.params import make_params
from beamform_amd.synth import make_scene
from conftest import rel_l2
from das_sep_util import GEOMETRIES, SEP_VS_TABLE_BOUND, load_sep_lib, sep_das

pytestmark = pytest.mark.gpu
TOL = 1e-6   # tests/test_fused_bins_gpu.py, das in double against the oracle
HERE = os.path.dirname(os.path.abspath(__file__))


def _params(geo, M, theta):
    mics = GEOMETRIES[geo]
    M = M if mics is None else len(mics)
    return make_params("das", n_mics=M, theta=theta, **({} if mics is None else {"mics": mics}))


def _run(p, x, n_streams=1, **kw):
    from beamform_amd.capi import BF_DAS_F64, Beamformer, launch_trace
    bf = Beamformer(p, n_streams=n_streams, das_impl=BF_DAS_F64, **kw)
    with launch_trace() as tr:
        y = bf.process(x)
    return np.asarray(y).reshape(n_streams, -1), tr.kernels, bf


def _margins(u):
    """u complex [pairs][1024], what the kernel casts to float (frame t real, t + 1 imaginary).  For every (frame, sample): how far the
    value is from the nearest point where one of the two float casts of the epilogue -- (float)u, then (float)((double)f h[n]) -- rounds
    the other way, relative to the pair's largest magnitude.  A sample closer to such a point than the allowed deviation may come out as
    the neighbouring float; no other sample may."""
    n = np.arange(1024)
    h = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / 1024))

    def dist(v):   # distance of the doubles v from the two rounding boundaries around (float)v
        f = v.astype(np.float32)
        lo, hi = np.nextafter(f, np.float32(-np.inf)).astype(np.float64), np.nextafter(f, np.float32(np.inf)).astype(np.float64)
        f = f.astype(np.float64)
        return np.minimum(np.abs(v - 0.5 * (f + lo)), np.abs(v - 0.5 * (f + hi)))

    peak = np.abs(u).max(axis=1, keepdims=True)
    v = np.stack([u.real, u.imag], axis=1)                       # [pairs][2][1024]
    d1 = dist(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.where(h > 0, dist(v.astype(np.float32).astype(np.float64) * h) / h, np.inf)
    return (np.minimum(d1, d2) / peak[:, None, :]).reshape(-1, 1024)   # [frame][1024]


def _check_against_restatement(y, p, theta, x):
    """y float32 [F * 512] of the kernel against the CPU restatement of the new form: the same float wherever the restatement's double is
    further than 4 x SEP_VS_TABLE_BOUND (of the pair's peak) from a rounding boundary of either contribution to the hop."""
    lib = load_sep_lib()
    yc, u, _ = sep_das(lib, p, theta, x, 1, want_u=True)
    F = y.size // 512
    m = _margins(u)[:F]
    head, tail = m[:, :512], np.vstack([np.full((1, 512), np.inf), m[:-1, 512:]])   # hop t = first half of frame t + second half of frame t - 1
    slack = np.minimum(head, tail).reshape(-1)
    diff = y != yc
    dev = float(np.abs(y.astype(np.float64) - yc).max() / np.abs(yc).max())
    print(f"kernel against the restated new form: {int(diff.sum())} of {y.size} floats differ, largest deviation {dev:.3e} of the peak; "
          f"smallest slack of a sample {float(slack.min()):.3e}")
    assert np.all(slack[diff] <= 4 * SEP_VS_TABLE_BOUND), (int(diff.sum()), float(slack[diff].max()))
    assert np.abs(y.astype(np.float64) - yc).max() <= 2.0 ** -22 * np.abs(yc).max()   # and then by one float step of the sums, no more


@pytest.mark.parametrize("geo,M,theta", [("aira16-first-8 (1 = 7)", 8, 20.0), ("aira16-first-8 (1 = 7)", 3, 60.0), ("aira16-first-8 (1 = 7)", 2, -50.0),
                                         ("2 = 3 and 5 = 6", 8, 35.0), ("all distinct", 8, 35.0)])
def test_planar_against_the_oracle_and_the_restated_new_form(geo, M, theta):
    """1, 2, 3 and 17 frames (17: more pairs than wavefronts, so pairs are drawn from the work word): 2, 3 and 8 microphones, the
    merged-pair and the distinct-rows geometry."""
    import oracle
    p = _params(geo, M, theta)
    M = p["n_mics"]
    for F in (1, 2, 3, 17):
        x = make_scene(M, F, seed=4100 + 10 * M + F, mics=p["mics"])
        y, kernels, _ = _run(p, x)
        assert any("das_f64_pair_kernel" in k for k in kernels), kernels
        y_ref, _ = oracle.OracleNode(p).process(x)
        err = rel_l2(y[0], y_ref)
        print(f"F = {F}: relative L2 against the oracle {err:.3e}")
        assert err < TOL, (F, err)
        _check_against_restatement(y[0], p, theta, x)


def test_two_streams():
    import oracle
    p = _params("aira16-first-8 (1 = 7)", 8, -15.0)
    xs = np.stack([make_scene(8, 17, seed=4300 + s) for s in range(2)])
    y, kernels, _ = _run(p, xs, n_streams=2)
    assert any("das_f64_pair_kernel" in k for k in kernels), kernels
    for s in range(2):
        assert rel_l2(y[s], oracle.OracleNode(p).process(xs[s])[0]) < TOL, s
        _check_against_restatement(y[s], p, -15.0, xs[s])


def test_resteer_between_batches_rebuilds_the_tables_and_keeps_the_state():
    import oracle
    p = _params("aira16-first-8 (1 = 7)", 8, 35.0)
    x = make_scene(8, 16, seed=4400)
    node = oracle.OracleNode(p)
    y1, kernels, bf = _run(p, np.ascontiguousarray(x[:, :7 * 512]))
    assert any("das_f64_pair_kernel" in k for k in kernels), kernels
    r1 = node.process(np.ascontiguousarray(x[:, :7 * 512]))[0]
    bf.set_theta(-70.0)
    node.set_theta(-70.0)
    y2 = np.asarray(bf.process(np.ascontiguousarray(x[:, 7 * 512:]))).reshape(-1)
    r2 = node.process(np.ascontiguousarray(x[:, 7 * 512:]))[0]
    assert rel_l2(y1[0], r1) < TOL and rel_l2(y2, r2) < TOL
    assert rel_l2(np.concatenate([y1[0], y2]), np.concatenate([r1, r2])) < TOL


def _forty_frames():
    p = _params("aira16-first-8 (1 = 7)", 8, 20.0)
    x = make_scene(8, 40, seed=4500)
    return p, x, _run(p, x)[0][0]


def test_forty_frames_in_chunks_of_four_and_two_pairs():
    """BF_DAS_F64_SCHED=4,2 (read once per process: a child): several chunks and chunk edges in a small batch -- against the oracle, and
    the same bytes as the default plan (a chunk plan never changes which frames share a transform)."""
    import oracle
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_das_sep_gpu as t; "
            "print('RESULT ' + json.dumps(t._forty_frames()[2].view('uint32').tolist()))" % (os.path.dirname(HERE), HERE))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BF_DAS_F64_SCHED="4,2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    yc = np.array(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]), np.uint32).view(np.float32)
    p, x, y = _forty_frames()
    assert rel_l2(yc, oracle.OracleNode(p).process(x)[0]) < TOL
    assert np.array_equal(yc, y)
    _check_against_restatement(yc, p, 20.0, x)


def test_sample_major_input_at_8_microphones_matches_planar_bit_for_bit():
    from beamform_amd.capi import BF_INTERLEAVED
    p = _params("aira16-first-8 (1 = 7)", 8, 20.0)
    x = make_scene(8, 17, seed=4600)
    y, _, _ = _run(p, x)
    yi, kernels, _ = _run(p, np.ascontiguousarray(x.T), layout=BF_INTERLEAVED)
    assert any("das_f64_ring_kernel" in k for k in kernels), kernels
    assert np.array_equal(yi, y)
