"""gsc on the GPU against the oracle at every JACK period, filter sizes 1 .. 256 and every NLMS instantiation the launch plan can select
(the cases and what makes them worth running: tests/gsc_cases.py, tests/test_gsc_cpu.py).  Every case also asserts with the launch trace
that the instantiation it is named for is the one that ran.  BF_GSC_SERIAL is read once per process: the cases that set it share one
fresh child process."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gsc_cases as gc
from conftest import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5   # test_gsc_matches_oracle's bar: relative L2 and largest error relative to the largest output sample

IN_PROCESS = [c.name for c in gc.CASES if not c.env]
SERIAL = [c.name for c in gc.CASES if c.env]
assert all(gc.BY_NAME[n].env == gc.SERIAL for n in SERIAL)


def _layout(c, x):
    """planar [S][M][T] -> what a handle of the case's layout reads."""
    return np.ascontiguousarray(np.swapaxes(x, -1, -2)) if c.layout == gc.INTERLEAVED else np.ascontiguousarray(x)


def oracle_of(c, x):
    import oracle
    p = gc.params(c)
    return np.stack([oracle.OracleNode(p).process(x[s])[0] for s in range(c.streams)])


def run_batch(c, x):
    """One batch through the C ABI -> (y [S][T], the kernels it launched)."""
    from beamform_amd.capi import launch_trace
    from conftest import Beamformer
    bf = Beamformer(gc.params(c), n_streams=c.streams, layout=c.layout)
    with launch_trace() as tr:
        y = np.atleast_2d(bf.process(_layout(c, x)))
    bf.close()
    return y, [k.replace("bf::", "") for k in tr.kernels]


def measure(name):
    """The figures the assertions need, as plain JSON values (the serial cases are measured in a child process)."""
    c = gc.BY_NAME[name]
    x = gc.scene(c)
    y_ref = oracle_of(c, x)
    y, kernels = run_batch(c, x)
    fin = bool(np.isfinite(y).all())
    same = bool(np.array_equal(np.isfinite(y), np.isfinite(y_ref)))
    ok = np.isfinite(y) & np.isfinite(y_ref)
    return dict(finite=fin, same_finite_pattern=same, ref_finite=bool(np.isfinite(y_ref).all()), kernels=kernels,
                rel=rel_l2(y[ok], y_ref[ok]), maxabs=float(np.abs(y[ok].astype(np.float64) - y_ref[ok]).max() / np.abs(y_ref[ok]).max()))


@functools.lru_cache(maxsize=None)
def measured(name):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return measure(name)


CHILD = r"""
import sys, json
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import test_gsc_gpu as t
print("RESULT " + json.dumps({n: t.measure(n) for n in sys.argv[1:]}))
"""


@pytest.fixture(scope="module")
def serial_results():
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)] + SERIAL, env=dict(os.environ, **gc.SERIAL), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def check(name, m):
    c = gc.BY_NAME[name]
    print(f"{name}: rel_l2 {m['rel']:.3e} max abs / max|y_ref| {m['maxabs']:.3e} {m['kernels'][-1]}")
    assert m["ref_finite"] and m["finite"] and m["same_finite_pattern"], m
    assert m["rel"] < TOL, m
    assert m["maxabs"] < 1e-5, m
    for k in c.kernels:   # the case ran the instantiation it is named for
        assert k in m["kernels"], (k, m["kernels"])


@pytest.mark.parametrize("name", IN_PROCESS)
def test_gsc_case_matches_oracle(name):
    check(name, measured(name))


@pytest.mark.parametrize("name", SERIAL)
def test_gsc_serial_case_matches_oracle(name, serial_results):
    check(name, serial_results[name])


@pytest.mark.parametrize("default,serial", [("m8-fs129", "fs129-m8-serial"), ("m16-fs255", "m16-fs255-serial")])
def test_default_and_serial_kernel_on_the_same_input(default, serial, serial_results):
    """Both meet the oracle on their own; they sum in different orders and need not agree bit for bit."""
    d, s = gc.BY_NAME[default], gc.BY_NAME[serial]
    assert (d.M, d.hop, d.F, d.over, d.seed) == (s.M, s.hop, s.F, s.over, s.seed)
    assert "gsc_nlms_mw_kernel" in d.kernels[-1] and "gsc_nlms_kernel" in s.kernels[-1]
    check(default, measured(default))
    check(serial, serial_results[serial])


def test_two_launches_give_the_same_bytes():
    """gsc_nlms_mw_kernel<8, 2, 4>: wavefronts run ahead of one another between the barriers and hand their sums over through the two
    halves of s_bo / s_pw -- a race would show as a difference between two launches."""
    c = gc.BY_NAME["fs256-m10"]
    assert c.kernels[-1].endswith("gsc_nlms_mw_kernel<8, 2, 4>")
    x = gc.scene(c)
    (y1, k1), (y2, k2) = run_batch(c, x), run_batch(c, x)
    assert c.kernels[-1] in k1 and k1 == k2
    assert y1.tobytes() == y2.tobytes()


def test_filter_longer_than_the_callback_one_callback_at_a_time():
    """hop 64 with 256 taps: the rings and the output window span four callbacks.  bf_process_hop per callback, the single batch and the
    oracle agree."""
    import oracle
    from conftest import Beamformer
    c = gc.BY_NAME["hop64-m5-fs256"]
    x = gc.scene(c)[0]
    y_ref = oracle_of(c, x[None])[0]
    bf = Beamformer(gc.params(c))
    y = np.concatenate([bf.process_hop(x[:, t * c.hop:(t + 1) * c.hop]) for t in range(c.F)])
    yb = run_batch(c, x[None])[0][0]
    bf.close()
    print(f"per callback vs oracle {rel_l2(y, y_ref):.3e}, vs the single batch {rel_l2(y, yb):.3e}, same bytes: {y.tobytes() == yb.tobytes()}")
    assert np.isfinite(y).all()
    assert rel_l2(y, y_ref) < TOL and np.abs(y - y_ref).max() < 1e-5 * np.abs(y_ref).max()
    assert rel_l2(y, yb) < TOL and np.abs(y - yb).max() < 1e-5 * np.abs(yb).max()


def test_state_carries_across_cuts_a_checkpoint_theta_and_streams():
    """hop 128, 200 taps, two streams: batches of 1, 1, 3, 1 and the rest; a checkpoint into a fresh handle after the second cut, a new look
    direction after the third."""
    import oracle
    from conftest import Beamformer
    c = gc.BY_NAME["carry-m3-fs200-s2"]
    p, S, H = gc.params(c), c.streams, c.hop
    xs = gc.scene(c)
    nodes = [oracle.OracleNode(p) for _ in range(S)]
    bf = Beamformer(p, n_streams=S)
    cuts = [0, 1, 2, 5, 6, c.F]
    ys, refs = [], []
    for n, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if n == 2:  # checkpoint into a fresh handle
            blob = bf.get_state()
            bf.close()
            bf = Beamformer(p, n_streams=S)
            bf.set_state(blob)
        if n == 3:
            bf.set_theta(-50.0)
            for nd in nodes:
                nd.set_theta(-50.0)
        seg = np.ascontiguousarray(xs[:, :, a * H:b * H])
        ys.append(np.atleast_2d(bf.process(seg)))
        refs.append(np.stack([nodes[s].process(seg[s])[0] for s in range(S)]))
    bf.close()
    y, r = np.concatenate(ys, axis=1), np.concatenate(refs, axis=1)
    assert np.isfinite(y).all()
    for s in range(S):
        print(f"stream {s}: rel_l2 {rel_l2(y[s], r[s]):.3e}")
        assert rel_l2(y[s], r[s]) < TOL and np.abs(y[s] - r[s]).max() < 1e-5 * np.abs(r[s]).max()
    # the uncut batch of the same streams (before the look direction moves) is the table's case
    check(c.name, measured(c.name))
