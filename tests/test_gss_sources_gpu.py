"""gss with every separated source (bf_config.gss_out_sources = R): the rows of each beam through the C ABI against the numpy
reference tests/gss_sources_ref.py (tied to the oracles and bounded in rounding by tests/test_gss_sources_cpu.py).  Every row is
judged on its own at the suite's 1e-5 per-frame relative L2; what the definition makes zero must be exactly zero."""
import numpy as np
import pytest

from beamform_amd.capi import BF_INTERLEAVED, BF_PRECISION_MIXED, BfError, launch_trace
from beamform_amd.synth import make_scene
from conftest import rel_l2
from gss_sources_cases import (CASES, SEEDS, SEM, case_params, case_ref, case_scene, case_streams, sem_params, sem_ref, sem_scene)

pytestmark = pytest.mark.gpu

TOL_SPECTRUM = TOL_TIME = 1e-5   # tests/test_pipeline_gpu.py


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _bf(p, **kw):
    from beamform_amd.capi import Beamformer
    return Beamformer(p, **kw)


def run_dev(bf, x, F, dump=True):
    """One batch through bf_process_batch_device -> (y [n_out, F*H] float32, Y [n_out, F, N] complex128 or None).  The buffers start
    as NaN: whatever the kernels leave unwritten shows."""
    torch = _torch()
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((bf.n_out, F * bf.H), float("nan"), dtype=torch.float32, device="cuda")
    Yd = torch.full((bf.n_out, F, bf.N, 2), float("nan"), dtype=torch.float64, device="cuda") if dump else None
    bf.process_device(xd.data_ptr(), F, yd.data_ptr(), Yd.data_ptr() if dump else 0)
    torch.cuda.synchronize()
    return yd.cpu().numpy(), (Yd.cpu().numpy().view(np.complex128)[..., 0] if dump else None)


def inband(p):
    from oracle import np_oracle
    f = np.abs(np_oracle.freq_vector(2 * p["hop"], p["sample_rate"]))
    return (f >= p["freq_min"]) & (f <= p["freq_max"])


def check_time(y, y_ref):
    """y, y_ref [R, F*H]"""
    assert (np.isfinite(y) == np.isfinite(y_ref)).all()
    for r in range(y_ref.shape[0]):
        ok = np.isfinite(y_ref[r])
        if not y_ref[r][ok].any():
            assert not y[r][ok].any(), f"row {r} is zero by definition"
        else:
            e = rel_l2(y[r][ok], y_ref[r][ok])
            assert e < TOL_TIME, (r, e)


def check_rows(p, y, Y, y_ref, Y_ref):
    """Rows of one beam: y [R, F*H], Y [R, F, N] against the reference's; non-finite frames must match as tests/test_pipeline_gpu.py's
    check() asks."""
    R, F, _ = Y_ref.shape
    assert Y.shape == Y_ref.shape and y.shape == y_ref.shape
    assert not Y[:, :, ~inband(p)].any(), "out of band every row is zero"
    for r in range(R):
        fin = np.isfinite(Y_ref[r]).all(axis=1)
        assert (np.isfinite(Y[r]).all(axis=1) == fin).all()
        for t in range(F):
            if not fin[t]:
                continue
            if not Y_ref[r, t].any():
                assert not Y[r, t].any(), f"row {r} frame {t} is zero by definition"
            else:
                e = rel_l2(Y[r, t], Y_ref[r, t])
                assert e < TOL_SPECTRUM, (r, t, e)
    check_time(y, y_ref)


def _one_stream_case(name, **kw):
    c, p = CASES[name], case_params(name)
    bf = _bf(p, gss_out_sources=c["R"], **kw)
    with launch_trace() as tr:
        y, Y = run_dev(bf, case_scene(name), c["F"])
    bf.close()
    return c, p, y, Y, tr.kernels


@pytest.mark.parametrize("name", ["g8", "g4", "g16", "g20"])
def test_group_kernel_rows(name):
    """gss_kernel_all at hop 512, one stream: 8 / 4 / 16 microphones on DPP sums, 20 on the LDS walk; spectrum dump and time output per
    row; row 0 is the R = 1 node's output bit for bit (the same sums in the same order)."""
    c, p, y, Y, kernels = _one_stream_case(name)
    assert any("gss_kernel_all<" in k for k in kernels) and not any("gss_lane" in k for k in kernels), kernels
    y_ref, Y_ref = case_ref(name)
    check_rows(p, y, Y, y_ref, Y_ref)
    S = len(c["interf"]) + 1
    assert not Y[S:].any() and not y[S:].any()
    one = _bf(p)
    y1, Y1 = run_dev(one, case_scene(name), c["F"])
    one.close()
    assert np.array_equal(Y[0], Y1[0]) and np.array_equal(y[0], y1[0])


def test_more_rows_than_sources():
    """R = 4 over two sources: rows 2 and 3 are exact zeros in the spectrum and in time."""
    c, p, y, Y, _ = _one_stream_case("r4s2")
    check_rows(p, y, Y, *case_ref("r4s2"))
    assert not Y[2:].any() and not y[2:].any()


@pytest.mark.parametrize("name", ["l8", "l7", "l6"])
def test_lane_kernel_rows(name):
    """gss_lane_kernel_all: one lane per (beam, problem) once the lanes fill the chip; two uneven batches, streams 0, 1, 31 and the
    last against the reference, every row."""
    c, p = CASES[name], case_params(name)
    n, F, H, R = c["streams"], c["F"], p["hop"], c["R"]
    keep = case_streams(name)
    xs = np.stack([case_scene(name, s) if s in keep else make_scene(c["M"], F, hop=H, seed=SEEDS[name] + 1000 * s, silent_frac=0.0)
                   for s in range(n)])
    bf = _bf(p, n_streams=n, gss_out_sources=R)
    ys, Ys = [], []
    for a, b in ((0, 3), (3, F)):
        with launch_trace() as tr:
            y, Y = run_dev(bf, xs[:, :, a * H:b * H], b - a)
        assert any("gss_lane_kernel" in k for k in tr.kernels) and not any("gss_kernel" in k for k in tr.kernels), tr.kernels
        ys.append(y)
        Ys.append(Y)
    bf.close()
    y, Y = np.concatenate(ys, axis=1), np.concatenate(Ys, axis=1)
    assert np.isfinite(y).all() and np.isfinite(Y).all()
    for s in keep:
        y_ref, Y_ref = case_ref(name, s)
        check_rows(p, y[s * R:(s + 1) * R], Y[s * R:(s + 1) * R], y_ref, Y_ref)


@pytest.mark.parametrize("name", ["h64", "h256", "h1024", "h2048", "h4096"])
def test_other_fft_sizes(name):
    c, p, y, Y, _ = _one_stream_case(name)
    check_rows(p, y, Y, *case_ref(name))


def _sem_controls(bf, i):
    if i == 2:
        bf.set_theta(SEM["theta1"])
    if i == 3:
        assert bf.set_interference(2, SEM["new_interf"]) == 2


def _sem_pieces():
    cuts, H = SEM["cuts"], 512
    x = sem_scene()
    return [(b - a, np.ascontiguousarray(x[:, a * H:b * H])) for a, b in zip(cuts[:-1], cuts[1:])]


def test_stream_semantics_across_batches():
    """Batch cuts, /theta in front of the third piece, a second interferer in front of the fourth: row 2 is silent before it and live
    after it, every row restarts from W = C^H with the rest, and the tails of all rows carry across the cuts."""
    bf = _bf(sem_params(), gss_out_sources=SEM["R"])
    ys, Ys = [], []
    for i, (n, x) in enumerate(_sem_pieces()):
        _sem_controls(bf, i)
        y, Y = run_dev(bf, x, n)
        ys.append(y)
        Ys.append(Y)
    bf.close()
    y, Y = np.concatenate(ys, axis=1), np.concatenate(Ys, axis=1)
    y_ref, Y_ref = sem_ref()
    check_rows(sem_params(), y, Y, y_ref, Y_ref)
    t3 = SEM["cuts"][3]
    assert not Y[2, :t3].any() and Y[2, t3:].any() and not y[2, :t3 * 512].any()


def test_stream_semantics_with_two_look_directions():
    """n_dirs = 2: output stream (dir * R + r); bf_set_theta moves direction 0 only, the interferer change restarts both."""
    bf = _bf(sem_params(), n_dirs=2, gss_out_sources=SEM["R"])
    ys = []
    for i, (n, x) in enumerate(_sem_pieces()):
        _sem_controls(bf, i)
        y = bf.process(x)
        assert y.shape == (2, SEM["R"], n * 512)
        ys.append(y)
    bf.close()
    y = np.concatenate(ys, axis=2)
    check_time(y[0], sem_ref(None, True)[0])
    check_time(y[1], sem_ref(None, False)[0])


def test_stream_semantics_hop_by_hop():
    """bf_process_hop: out = [R][nframes] per callback."""
    bf = _bf(sem_params(), gss_out_sources=SEM["R"])
    x, cuts, out = sem_scene(), SEM["cuts"], []
    for t in range(SEM["F"]):
        if t in cuts[1:-1]:
            _sem_controls(bf, cuts.index(t))
        o = bf.process_hop(x[:, t * 512:(t + 1) * 512])
        assert o.shape == (SEM["R"], 512)
        out.append(o)
    bf.close()
    check_time(np.concatenate(out, axis=1), sem_ref()[0])


#: bf_state_size of a one-row gss handle with 4 microphones, one interferer, hop 512, one stream -- the parent commit's value
#: (header 32 + control 656 + carried hop 8192 + one tail 2048 + demixing matrices 1024 * 16 * 4 * 16)
STATE_BYTES_R1 = 1059504


def test_checkpoint_with_rows():
    from beamform_amd.params import make_params
    _torch()
    M, F, R = 4, 16, 3
    p = make_params("gss", n_mics=M, theta=10.0, interf=(-60.0,))
    x = make_scene(M, 2 * F, seed=2)
    a = _bf(p, gss_out_sources=R)
    a.process(np.ascontiguousarray(x[:, : F * 512]))
    blob = a.get_state()
    ya2 = a.process(np.ascontiguousarray(x[:, F * 512:]))
    b = _bf(p, gss_out_sources=R)
    b.process(np.ascontiguousarray(x[:, : 3 * 512]))  # scramble b's state first
    b.set_state(blob)
    yb2 = b.process(np.ascontiguousarray(x[:, F * 512:]))
    assert ya2.shape == (R, F * 512) and np.array_equal(ya2, yb2, equal_nan=True)
    one = _bf(p)
    one.process(np.ascontiguousarray(x[:, : F * 512]))
    blob1 = one.get_state()
    assert len(blob1) == STATE_BYTES_R1 and len(blob) == STATE_BYTES_R1 + (R - 1) * 512 * 4
    with pytest.raises(BfError):
        b.set_state(blob1)
    with pytest.raises(BfError):
        b.set_state(blob1 + bytes(len(blob) - len(blob1)))     # long enough: the header tells the row counts apart
    with pytest.raises(BfError):
        one.set_state(blob)
    one.set_state(blob1)
    for h in (a, b, one):
        h.close()


def test_interleaved_input_and_mixed_precision():
    """[sample][mic] input reads the same samples; BF_PRECISION_MIXED changes nothing in front of gss's backward transform and is
    judged on the time output."""
    c, p = CASES["small"], case_params("small")
    y_ref, Y_ref = case_ref("small")
    bf = _bf(p, layout=BF_INTERLEAVED, gss_out_sources=c["R"])
    y, Y = run_dev(bf, case_scene("small").T, c["F"])
    bf.close()
    check_rows(p, y, Y, y_ref, Y_ref)
    bf = _bf(p, precision=BF_PRECISION_MIXED, gss_out_sources=c["R"])
    y, _ = run_dev(bf, case_scene("small"), c["F"], dump=False)
    bf.close()
    check_time(y, y_ref)


def test_stream_rms_counts_every_row():
    torch = _torch()
    c, p = CASES["small"], case_params("small")
    n, F, R = 2, c["F"], c["R"]
    xs = np.stack([case_scene("small"), case_scene("small", 1)])
    bf = _bf(p, n_streams=n, n_dirs=2, gss_out_sources=R)
    xd = torch.from_numpy(xs).cuda()
    yd = torch.empty((n * 2 * R, F * 512), dtype=torch.float32, device="cuda")
    bf.process_device(xd.data_ptr(), F, yd.data_ptr())
    rms = bf.stream_rms(yd.data_ptr(), F)
    y = yd.cpu().numpy().astype(np.float64)
    bf.close()
    assert rms.shape == (n, 2, R)
    want = np.sqrt((y ** 2).mean(axis=1)).reshape(n, 2, R)
    assert np.allclose(rms, want, rtol=1e-12, atol=0) and (want > 0).all()
    check_time(y[:R].astype(np.float32), case_ref("small")[0])
