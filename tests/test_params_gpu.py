"""Every node parameter off its launch value on the GPU, against the oracle (the cases and what makes them worth running:
tests/param_cases.py, tests/test_params_cpu.py).  Every case goes through the C ABI twice -- without a spectrum dump (the launch the
table names; the launch trace is held to it) and with one -- and meets the project's bar: relative L2 below 1e-5 on every frame's
spectrum and on the time signal, with the oracle's own finite pattern (tests/test_hops_gpu.py's check); where a node has no spectrum
dump of its own (gsc) or emits rows (gss), the largest error relative to the largest output sample as well (tests/test_gsc_gpu.py's
check).  Switches are read once per process: the cases of one environment share one fresh child process."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import param_cases as pc
from conftest import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5

IN_PROCESS = [c.name for c in pc.CASES if not c.env]
BY_ENV = {pc.env_id(e): [c.name for c in pc.CASES if c.env == e] for e in pc.ENVS}
CHILD_CASES = [(eid, n) for eid, names in BY_ENV.items() for n in names]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def node(c, **kw):
    from beamform_amd import capi
    e = c.extra
    if c.algo == "das":
        kw["das_impl"] = capi.BF_DAS_FUSED_F32 if e.get("f32") else capi.BF_DAS_F64
    if e.get("rows"):
        kw["gss_out_sources"] = e["rows"]
    if e.get("pf"):
        kw["gss_postfilter"] = 1
    bf = capi.Beamformer(pc.params(c), n_streams=c.streams, layout=c.layout, precision=c.precision, n_dirs=e.get("dirs", 1), **kw)
    if e.get("dirs"):
        bf.set_thetas(pc.DIR_ANGLES[:e["dirs"]])
    if e.get("track"):
        if c.algo == "mvdr":
            import ctrack_cases as cc
            bf.set_ctrack_angles(cc.MVDR_ANGLES)
        else:
            bf.set_track_angles(pc.DIR_ANGLES)
    return bf


def _layout(c, x):
    """planar [S][M][T] -> what a handle of the case's layout reads."""
    return np.ascontiguousarray(np.swapaxes(x, -1, -2)) if c.layout == pc.INTERLEAVED else np.ascontiguousarray(x)


def run_dev(c, x, dump):
    """One batch through bf_process_batch_device (or its tracked twins) on a fresh handle -> (y [streams, rows, T],
    Y [streams, rows, F, N] or None, the kernels it launched).  The output buffers start as NaN."""
    from beamform_amd.capi import launch_trace
    torch = _torch()
    bf = node(c)
    F, H, S = x.shape[-1] // c.hop, c.hop, c.streams
    xd = torch.from_numpy(_layout(c, x)).cuda()
    off = 1 if c.extra.get("offset") else 0        # one float in: 4-byte aligned, not 16
    ybuf = torch.full((bf.n_out * F * H + off,), float("nan"), dtype=torch.float32, device="cuda")
    yptr = ybuf.data_ptr() + 4 * off
    assert not off or (yptr % 16 == 4 and ybuf.data_ptr() % 16 == 0)
    Yd = torch.full((bf.n_out, F, 2 * H, 2), float("nan"), dtype=torch.float64, device="cuda") if dump else None
    Yptr = Yd.data_ptr() if dump else 0
    with launch_trace() as tr:
        if c.extra.get("track"):
            t = pc.track_of(c)
            td = torch.from_numpy(np.array(np.broadcast_to(t, (S,) + t.shape), np.int32)).cuda()    # the same track on every stream
            if c.algo == "mvdr":
                bf.process_device_ctracked(xd.data_ptr(), F, yptr, td.data_ptr(), 1, Yptr)
            else:
                bf.process_device_tracked(xd.data_ptr(), F, yptr, td.data_ptr(), Yptr)
        else:
            bf.process_device(xd.data_ptr(), F, yptr, Yptr)
        torch.cuda.synchronize()
    y = ybuf[off:].cpu().numpy().reshape(S, bf.n_out // S, F * H)
    Y = Yd.cpu().numpy().view(np.complex128)[..., 0].reshape(S, bf.n_out // S, F, 2 * H) if dump else None
    bf.close()
    return y, Y, [k.replace("bf::", "") for k in tr.kernels]


def run_pieces(c, x):
    """The same streams through one handle in the batches of c.cuts (host interface), one callback at a time (per_hop), with the state
    saved and restored into a fresh handle after `checkpoint` frames -> y [streams, rows, T]."""
    H, S = c.hop, c.streams
    cuts = list(range(c.F + 1)) if c.extra.get("per_hop") else list(c.cuts)
    bf = node(c)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a and a == c.extra.get("checkpoint"):
            blob = bf.get_state()
            bf.close()
            bf = node(c)
            bf.set_state(blob)
        seg = x[:, :, a * H:b * H]
        if c.extra.get("per_hop"):
            assert S == 1 and c.layout == pc.PLANAR
            parts.append(np.asarray(bf.process_hop(seg[0])).reshape(1, -1, H))
        else:
            parts.append(np.asarray(bf.process(_layout(c, seg))).reshape(S, -1, (b - a) * H))
    bf.close()
    return np.concatenate(parts, axis=2)


def compare(y, Y, y_ref, Y_ref):
    """Rows of one stream against the oracle's -> the figures check() asserts on.  pattern: the same frames / samples are finite;
    zeros: what the oracle leaves exactly zero (a row beyond the source count) is exactly zero; spec: worst per-frame relative L2 over
    the finite, non-zero frames; time: relative L2 over the finite samples of a row; maxabs: largest error over largest sample."""
    r = dict(pattern=True, zeros=True, spec=0.0, time=0.0, maxabs=0.0)
    for row in range(y_ref.shape[0]):
        if Y is not None and Y_ref is not None:
            fin = np.isfinite(Y_ref[row]).all(axis=1)
            r["pattern"] &= bool((np.isfinite(Y[row]).all(axis=1) == fin).all())
            for t in np.flatnonzero(fin):
                if not np.isfinite(Y[row, t]).all():
                    continue
                if not Y_ref[row, t].any():
                    r["zeros"] &= not Y[row, t].any()
                else:
                    r["spec"] = max(r["spec"], rel_l2(Y[row, t], Y_ref[row, t]))
        ok = np.isfinite(y_ref[row])
        r["pattern"] &= bool((np.isfinite(y[row]) == ok).all())
        ok &= np.isfinite(y[row])
        if not y_ref[row][ok].any():
            r["zeros"] &= not y[row][ok].any()
        else:
            r["time"] = max(r["time"], rel_l2(y[row][ok], y_ref[row][ok]))
            r["maxabs"] = max(r["maxabs"], float(np.abs(y[row][ok].astype(np.float64) - y_ref[row][ok]).max() / np.abs(y_ref[row][ok]).max()))
    return r


def _worst(rs):
    return dict(pattern=all(r["pattern"] for r in rs), zeros=all(r["zeros"] for r in rs), spec=max(r["spec"] for r in rs),
                time=max(r["time"] for r in rs), maxabs=max(r["maxabs"] for r in rs))


_REFS = {}


def reference(c, s):
    """Shared by the cases of one oracle run (the two precisions, the tile lengths); never written to."""
    key = (pc.oracle_key(c), s)
    if key not in _REFS:
        _REFS[key] = pc.reference(c, s)
    return _REFS[key]


def measure(name):
    """The figures the assertions need, as plain JSON values (cases with an environment are measured in a child process)."""
    c = pc.BY_NAME[name]
    x = pc.scene(c)
    streams = pc.compared_streams(c)
    refs = {s: reference(c, s) for s in streams}
    y, _, kernels = run_dev(c, x, dump=False)
    out = dict(kernels=kernels, nodump=_worst([compare(y[s], None, refs[s][0], None) for s in streams]))
    if c.algo != "gsc" and not c.extra.get("f32"):   # (gsc has no spectrum; the fp32 das opt-in dumps the Hermitian part only)
        yd, Yd, _ = run_dev(c, x, dump=True)
        out["dump"] = _worst([compare(yd[s], Yd[s], *refs[s]) for s in streams])
    if c.cuts or c.extra.get("per_hop"):
        yp = run_pieces(c, x)
        out["pieces"] = _worst([compare(yp[s], None, refs[s][0], None) for s in streams])
        out["pieces_vs_batch"] = _worst([compare(yp[s], None, y[s], None) for s in streams])
        out["pieces_same_bytes"] = bool(yp.tobytes() == y.tobytes())
    return out


@functools.lru_cache(maxsize=None)
def measured(name):
    from beamform_amd.capi import BfError
    _torch()
    try:
        return measure(name)
    except BfError as e:      # a HIP error behind the C ABI: nothing more is started on this device
        pytest.exit(f"{name}: {e}", returncode=3)


CHILD = r"""
import sys, json
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import test_params_gpu as t
print("RESULT " + json.dumps({n: t.measure(n) for n in sys.argv[1:]}))
"""


@functools.lru_cache(maxsize=None)
def child_results(eid):
    """One fresh child process per environment, started once (never by replacing this program), one at a time."""
    env = next(e for e in pc.ENVS if pc.env_id(e) == eid)
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)] + BY_ENV[eid], env=dict(os.environ, **env), capture_output=True,
                         text=True, timeout=600)
    if out.returncode != 0 and ("BfError" in out.stderr or out.returncode < 0):   # a HIP error or a signal: nothing more is started
        pytest.exit(f"child {eid}: exit {out.returncode}: {out.stderr[-2000:]}", returncode=3)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def check(name, m):
    c = pc.BY_NAME[name]
    peak = c.algo == "gsc" or bool(c.extra.get("rows"))      # no spectrum of its own / rows: tests/test_gsc_gpu.py's bar on the time signal
    worst = max([m[k][f] for k in ("nodump", "dump", "pieces", "pieces_vs_batch") if k in m for f in ("spec", "time")])
    print(f"{name}: worst relative L2 {worst:.3e}  " + "  ".join(
        f"{k}: spectrum {m[k]['spec']:.2e} time {m[k]['time']:.2e} max abs / peak {m[k]['maxabs']:.2e}" for k in ("nodump", "dump", "pieces", "pieces_vs_batch")
        if k in m) + (f"  pieces == batch bit for bit: {m['pieces_same_bytes']}" if "pieces" in m else ""))
    for k in c.kernels:   # the case ran what it is named for
        assert any(k in t for t in m["kernels"]), (k, m["kernels"])
    for k in ("nodump", "dump", "pieces", "pieces_vs_batch"):
        if k not in m:
            continue
        assert m[k]["pattern"] and m[k]["zeros"], (k, m[k])
        assert m[k]["spec"] < TOL and m[k]["time"] < TOL, (k, m[k])
        if peak:
            assert m[k]["maxabs"] < 1e-5, (k, m[k])
    assert (c.cuts is None and not c.extra.get("per_hop")) or "pieces" in m


@pytest.mark.parametrize("name", IN_PROCESS)
def test_case_matches_oracle(name):
    check(name, measured(name))


@pytest.mark.parametrize("eid,name", CHILD_CASES, ids=[n for _, n in CHILD_CASES])
def test_switched_case_matches_oracle(eid, name):
    check(name, child_results(eid)[name])


def test_a_handful_of_children():
    assert len(BY_ENV) <= 6 and sum(len(v) for v in BY_ENV.values()) == len(CHILD_CASES)
